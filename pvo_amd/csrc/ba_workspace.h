// ---------------------------------------------------------------------------
// workspace: constants, fixed-point sums, the plan and the carved workspace every stage reads
// ---------------------------------------------------------------------------
#pragma once
#include "common.h"

namespace {

constexpr float kMinDepth = 0.25f;

// The reduced pose system is accumulated in 64-bit FIXED POINT (units of 2^-28): integer atomics commute, so the sums - and
// with them poses and depths - are bitwise reproducible from run to run, and identical whether the edges sit on one GPU or
// are sharded over several (fp64 atomics, used before, made the last bits order dependent).  Every addend is an fp32
// partial sum (|v| <~ 1e8 at most: w J^2 over a chunk of pixels), so 2^-28 = 3.7e-9 absolute resolution is far below its
// own rounding error, and |sum| < 2^35 leaves 7 bits of headroom.  Non-finite or out-of-range addends raise meta[4]; the
// solve then takes the reference's failure path (zero update, droid_kernels.cu:1186-1189).
constexpr double kFix = 268435456.0, kInvFix = 1.0 / 268435456.0;
__device__ __forceinline__ void fix_add(long long* sys, long long idx, double v, int* meta) {
  if (!(fabs(v) < 3.0e10)) { meta[4] = 1; return; }
#ifdef PVO_BA_NO_ATOMICS                 // (timing experiment only - tools/ba_kernel_timeline.py PROBE_DEFS: the sums are lost)
  if (idx >= 0) return;
#endif
  atomicAdd(reinterpret_cast<unsigned long long*>(sys + idx), static_cast<unsigned long long>(__double2ll_rn(v * kFix)));
}
constexpr int kDealEdges = 2;           // edges (consecutive in the plan's by-source order) per chunk-sum workgroup of the Schur kernel
constexpr int kPPT = 2;                 // pixels per thread in assemble (1: 432 workgroups, measured slower - profiles/r03_ba_ablation.txt)
constexpr int kChunkA = 256 * kPPT;     // pixels per assemble workgroup
constexpr int kMaxSep = 12;                                      // separator poses of the partitioned solve (beyond: not partitioned)
constexpr int kXchgDoubles = 2 + 36 * kMaxSep * kMaxSep + 12 * kMaxSep;


// tools/ba_kernel_timeline.py builds this file with -DPVO_BA_PROBE=3: every workgroup of the assembly / Schur / back-substitution
// kernels stamps the constant-rate clock (10 ns) at its phases: g_ba_wg_probe[(kernel * 4096 + workgroup) * 8 + slot]
#if defined(PVO_BA_PROBE) && PVO_BA_PROBE == 3
__device__ unsigned long long* g_ba_wg_probe = nullptr;
#define BA_WG_PROBE(kern, slot)                                                                                         \
  do {                                                                                                                  \
    if (g_ba_wg_probe && threadIdx.x == 0 && blockIdx.z == 0) {                                                         \
      const unsigned wg_ = blockIdx.y * gridDim.x + blockIdx.x;                                                         \
      if (wg_ < 4096u) g_ba_wg_probe[((kern) * 4096u + wg_) * 8u + (slot)] = wall_clock64();                            \
    }                                                                                                                   \
  } while (0)
#else
#define BA_WG_PROBE(kern, slot)
#endif

struct Plan {            // int region of the workspace
  int* kidx;             // [F]   frame -> depth index, -1 if none
  int* kx;               // [F]   depth index -> frame
  int* eptr;             // [F+1] CSR over depth index -> edges (ascending edge id)
  int* eidx;             // [E]
  int* meta;             // [16]  0:K 1:status(non-SPD) 2:eta mismatch 3:row table overflow 4:non-finite / out-of-range system entry
                         //       5,6: the sensor-depth prior's map (low / high word of a const float*, 0 = none) 7: its alpha (float bits)
                         //       8: the stereo baseline (float bits, 0 = none: an edge (i, i) is an identity edge)
  int* env;              // [P]   numeric envelope of a system for the envelope solve (ba_env_kernel; INT_MAX between solves)
};

struct Ws {
  Plan plan;
  float *Eii, *Eij;      // [E][6][HW]
  float *Cii, *bz;       // [E][HW]
  float *Ei;             // [P][6][HW]
  float *Q, *w;          // [F'][HW]   (F' = min(F, P+E) rows)
  float *dx;             // [P][6]
  float *part;           // [E][assembly chunks][90]: per-chunk sums of an edge's pose blocks and gradients (depth BA)
  long long* sys;        // [(6P)^2 + 6P] fixed point
  double* chol;          // [(6P)^2 + 6P] scratch for the global-memory factorisation
  double* xchg;          // partitioned pose solve: [2 doubles = 4 ints: flags, split | separator terms | separator solution] (kXchgDoubles)
  double* ldiag;         // blocked multi-workgroup solve (big dense-ish systems): factored diagonal blocks [n / 48 + 1][48 x 48 + 48]
  double* xvec;          // ... and its solution [6P]
  float* Mrg;            // [E][6][HW]: the summed Eij rows of edges that share source AND target frame (Schur kernel), at the first one's index
  // dense windows (P <= kDenseMaxPoses), two-stage Schur sums: per (depth frame, 256-pixel chunk) the tile-pair sums of the chunk,
  // the frame's row -> system-entry table and its tile count (0 = this frame went the atomic way).  All three are indexed by the
  // frame's staging SLOT (schur_stage_slot: by frame identity), not by its row in the call's plan
  float* spart;          // [kSchurStageFrames(P)][ceil(HW/256)][kSchurStagePairs][256]
  short* srow;           // [kSchurStageFrames(P)][128]
  int* sT;               // [kSchurStageFrames(P)]
  size_t bytes;
};
constexpr int kSchurStagePairs = 36;     // tile pairs of up to 8 row tiles
constexpr int kSchurStageFront = 8;      // source frames right in front of the window that have a staging slot beside the window's own
__host__ __device__ __forceinline__ int schur_stage_frames(int P) { return (P > 0 && P <= 29) ? P + kSchurStageFront : 0; }
// The staging slot of a depth frame, by the frame's IDENTITY: the window's frames [t0, t1) and the kSchurStageFront frames in front
// of them, slot = frame - (t0 - kSchurStageFront); -1 = no slot, the frame's chunks go to the system one by one.  Whether a frame's
// chunk sums are rounded to fixed point once or chunk by chunk changes the words of `sys`, so the choice must not read anything a
// rank of an edge-sharded run sees differently (the row of the frame in this call's plan, the number of depth frames, the eta layout).
__host__ __device__ __forceinline__ int schur_stage_slot(int frame, int t0, int P) {
  const int slot = frame - t0 + kSchurStageFront;
  return (slot >= 0 && slot < schur_stage_frames(P)) ? slot : -1;
}

__host__ size_t align_up(size_t x) { return (x + 255) & ~static_cast<size_t>(255); }
// the host's bound on the depth frames K = |unique([t0, t1) U ii)| of a call: rows of Q / w, and of every grid over depth frames
__host__ int depth_rows_bound(int nframes, int P, int E) { return (nframes < P + E) ? nframes : (P + E); }

__host__ Ws carve(void* base, int E, int P, int F, int HW) {
  Ws w{};
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += align_up(bytes); return r; };
  const int Kmax = depth_rows_bound(F, P, E);
  const size_t n6 = static_cast<size_t>(6) * (P > 0 ? P : 0);
  w.plan.kidx = reinterpret_cast<int*>(take(sizeof(int) * (F + 1)));
  w.plan.kx = reinterpret_cast<int*>(take(sizeof(int) * (F + 1)));
  w.plan.eptr = reinterpret_cast<int*>(take(sizeof(int) * (F + 2)));
  w.plan.eidx = reinterpret_cast<int*>(take(sizeof(int) * (E + 1)));
  w.plan.meta = reinterpret_cast<int*>(take(sizeof(int) * 16));
  w.plan.env = reinterpret_cast<int*>(take(sizeof(int) * ((P > 0 ? P : 0) + 1)));
  w.Eii = reinterpret_cast<float*>(take(sizeof(float) * static_cast<size_t>(E) * 6 * HW));
  w.Eij = reinterpret_cast<float*>(take(sizeof(float) * static_cast<size_t>(E) * 6 * HW));
  w.Cii = reinterpret_cast<float*>(take(sizeof(float) * static_cast<size_t>(E) * HW));
  w.bz = reinterpret_cast<float*>(take(sizeof(float) * static_cast<size_t>(E) * HW));
  w.Ei = reinterpret_cast<float*>(take(sizeof(float) * static_cast<size_t>(P > 0 ? P : 0) * 6 * HW));
  w.Q = reinterpret_cast<float*>(take(sizeof(float) * static_cast<size_t>(Kmax) * HW));
  w.w = reinterpret_cast<float*>(take(sizeof(float) * static_cast<size_t>(Kmax) * HW));
  w.dx = reinterpret_cast<float*>(take(sizeof(float) * (n6 + 8)));
  w.part = reinterpret_cast<float*>(take(sizeof(float) * static_cast<size_t>(E) * ((HW + kChunkA - 1) / kChunkA) * 90 + 16));
  w.sys = reinterpret_cast<long long*>(take(sizeof(double) * (n6 * n6 + n6 + 8)));
  // (both at every size: a packed envelope message - pvo_ba_finish_packed - is factorised from the compact image whatever P is)
  w.chol = reinterpret_cast<double*>(take(sizeof(double) * (n6 * n6 + n6 + 27 * (n6 / 6) + 32)));
  w.xchg = reinterpret_cast<double*>(take(sizeof(double) * kXchgDoubles));
  w.ldiag = reinterpret_cast<double*>(take(sizeof(double) * (n6 / 48 + 2) * (48 * 48 + 48)));
  w.xvec = reinterpret_cast<double*>(take(sizeof(double) * (n6 + 8)));
  w.Mrg = reinterpret_cast<float*>(take(sizeof(float) * static_cast<size_t>(E) * 6 * HW));
  {
    const size_t ks = static_cast<size_t>(schur_stage_frames(P));
    w.spart = reinterpret_cast<float*>(take(sizeof(float) * ks * ((HW + 255) / 256) * kSchurStagePairs * 256));
    w.srow = reinterpret_cast<short*>(take(sizeof(short) * ks * 128));
    w.sT = reinterpret_cast<int*>(take(sizeof(int) * (ks + 1)));
  }
  w.bytes = off;
  return w;
}

// ---------------------------------------------------------------------------
// the sensor-depth prior (pvo_ba_depth_prior): part of the plan's device-side state, read once per workgroup by the depth phase
// ---------------------------------------------------------------------------
struct DepthPrior { const float* sens; float alpha; };     // sens: [F][HW] measured inverse depth, 0 = no measurement; nullptr = none

__device__ __forceinline__ void store_prior(int* meta, const float* sens, float alpha) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(sens);
  meta[5] = static_cast<int>(a & 0xffffffffull);
  meta[6] = static_cast<int>(a >> 32);
  meta[7] = sens ? __float_as_int(alpha) : 0;
}
__device__ __forceinline__ DepthPrior load_prior(const int* meta) {
  const unsigned long long a = (static_cast<unsigned long long>(static_cast<unsigned>(meta[6])) << 32) | static_cast<unsigned>(meta[5]);
  DepthPrior pr;
  pr.sens = reinterpret_cast<const float*>(a);
  pr.alpha = __int_as_float(meta[7]);
  return pr;
}
__global__ void ba_prior_kernel(int* meta, const float* sens, float alpha) { store_prior(meta, sens, alpha); }

// the stereo baseline (pvo_ba_stereo): with b > 0 an edge (i, i) is the fixed left -> right transform of the rig.  Read once per
// workgroup by the assembly.
__global__ void ba_stereo_kernel(int* meta, float baseline) { meta[8] = __float_as_int(baseline); }

// ---------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ba_plan_kernel(
    const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, Plan pl,
    int E, int F, int t0, int t1, int K_eta, int motion_only, const float* sens, float alpha, float baseline) {
  __shared__ int seg[257];
  const int tid = threadIdx.x;
  for (int b = tid; b < t1 - t0; b += 256) pl.env[b] = 0x7fffffff;
  // presence bitmap
  for (int f = tid; f < F; f += 256) pl.kidx[f] = (f >= t0 && f < t1) ? 1 : 0;
  __syncthreads();
  for (int e = tid; e < E; e += 256) {
    const long long f = ii[e];
    if (f >= 0 && f < F) pl.kidx[f] = 1;   // benign race: everyone writes 1
  }
  __syncthreads();
  // exclusive scan of the bitmap, one contiguous segment per thread
  const int per = (F + 255) / 256;
  const int lo = min(tid * per, F), hi = min(lo + per, F);
  int cnt = 0;
  for (int f = lo; f < hi; ++f) cnt += pl.kidx[f];
  seg[tid + 1] = cnt;
  if (tid == 0) seg[0] = 0;
  __syncthreads();
  if (tid == 0) for (int i = 1; i <= 256; ++i) seg[i] += seg[i - 1];
  __syncthreads();
  int run = seg[tid];
  for (int f = lo; f < hi; ++f) {
    if (pl.kidx[f]) { pl.kx[run] = f; pl.kidx[f] = run; ++run; } else pl.kidx[f] = -1;
  }
  const int K = seg[256];
  __syncthreads();
  // CSR of edges by depth index (= source frame), ascending edge id inside a row
  for (int k = tid; k < K; k += 256) {
    const int f = pl.kx[k];
    int c = 0;
    for (int e = 0; e < E; ++e) c += (ii[e] == f) ? 1 : 0;
    pl.eptr[k + 1] = c;
  }
  if (tid == 0) pl.eptr[0] = 0;
  __syncthreads();
  if (tid == 0) for (int k = 1; k <= K; ++k) pl.eptr[k] += pl.eptr[k - 1];
  __syncthreads();
  for (int k = tid; k < K; k += 256) {
    const int f = pl.kx[k];
    int o = pl.eptr[k];
    for (int e = 0; e < E; ++e) if (ii[e] == f) pl.eidx[o++] = e;
  }
  if (tid == 0) {
    pl.meta[0] = K;
    pl.meta[1] = 0;
    pl.meta[3] = 0;
    pl.meta[4] = 0;
    // eta must have one row per depth frame (or one row, broadcast).  Anything else is a caller error the host cannot see
    // without a synchronisation (K is found here): flagged, and the step becomes a NO-OP - the Schur grid is sized by the caller's
    // row count, so depth frames beyond it would keep stale Q / w; the solve reports failure (dx = 0, poses untouched) and the
    // back-substitution leaves every depth map alone (status_out[0] = 1, [2] = 1).
    pl.meta[2] = (!motion_only && K_eta != K && K_eta != 1) ? 1 : 0;
    store_prior(pl.meta, sens, alpha);      // (pvo_ba_plan: none - a fresh plan runs the arithmetic without the term)
    pl.meta[8] = __float_as_int(baseline);  // (pvo_ba_plan: 0 - no stereo edges)
  }
}

}  // namespace
