// ---------------------------------------------------------------------------
// schur: depth elimination for one (pixel chunk, depth frame)
// ---------------------------------------------------------------------------
#pragma once
#include "ba_workspace.h"
#include "ba_assemble.h"

namespace {

// Row r of depth frame k: r == -1 is the window-pose row (Ei[k], pose kx[k]-t0),
// r >= 0 is outgoing edge eidx[eptr[k]+r] (Eij, pose jj-t0).
struct RowRef { const float* base; int pose; };

__device__ __forceinline__ RowRef row_of(int r, int k, const Plan& pl, const float* Ei, const float* Eij,
                                         const int64_t* jj, int HW, int t0, int P) {
  RowRef R;
  if (r < 0) {
    const int p = pl.kx[k] - t0;
    R.pose = (p >= 0 && p < P) ? p : -1;
    R.base = Ei + static_cast<long long>(p >= 0 && p < P ? p : 0) * 6 * HW;
  } else {
    const int e = pl.eidx[pl.eptr[k] + r];
    const int p = static_cast<int>(jj[e]) - t0;
    R.pose = (p >= 0 && p < P) ? p : -1;
    R.base = Eij + static_cast<long long>(e) * 6 * HW;
  }
  return R;
}

// ---- depth: C, w, Q and the window-pose rows Ei for one (pixel, depth frame) ----------
// (accum_cuda x3 + the Q expression of ba_cuda, droid_kernels.cu:1374-1378).  Runs as the first phase of the Schur
// kernel: every workgroup prepares Q, w and Ei for exactly the pixels it is about to reduce.
__device__ __forceinline__ void depth_pixel(const Plan& pl, int k, int x, const float* __restrict__ eta, int K_eta,
                                            const float* __restrict__ Eii, const float* __restrict__ Cii, const float* __restrict__ bz,
                                            float* __restrict__ Ei, float* __restrict__ Q, float* __restrict__ w, int HW, int t0, int P,
                                            const int* __restrict__ edges, int deg, int pself,
                                            const DepthPrior& pr, const float* __restrict__ disps) {
  // `edges` = this depth frame's out-edges in LDS (round 4): read from the plan in global memory inside this loop, every
  // iteration was two dependent round trips (eidx[o], then the rows of edge e) - 6 x 2 of them in front of the first product
  const bool self_in = pself >= 0 && pself < P;
  float C = 0.0f, ww = 0.0f, ei[6] = {0, 0, 0, 0, 0, 0};
  // (six edges' 48 loads in flight: a frame of a real window has ~18 out-edges and this loop was a third of the kernel at unroll 2)
#pragma unroll 6
  for (int o = 0; o < deg; ++o) {
    const int e = edges[o];
    C += Cii[static_cast<long long>(e) * HW + x];
    ww += bz[static_cast<long long>(e) * HW + x];
    if (self_in) {
#pragma unroll
      for (int n = 0; n < 6; ++n) ei[n] += Eii[(static_cast<long long>(e) * 6 + n) * HW + x];
    }
  }
  // K_eta == 1 broadcasts; a row-count mismatch is flagged in meta[2] and clamped here
  const float et = eta[static_cast<long long>(k < K_eta ? k : K_eta - 1) * HW + x];
  // The sensor-depth prior (upstream DROID-SLAM's RGB-D term): where the frame has a measurement s > 0, alpha takes eta's place in C
  // and alpha (d - s) leaves w.  SELECTS, not blends: no map, or no measurement at this pixel, is C + et and ww - 0.0f - the bits
  // of the arithmetic without the term.  Only for a frame with out-edges in THIS call (deg > 0): an edge-sharded rank plans every
  // window frame, and one it does not own has C = w = 0 here and must keep dz = 0, or the ranks would each apply the term.
  float cp = et, wp = 0.0f;
  if (pr.sens != nullptr && deg > 0) {
    const long long fx = static_cast<long long>(pself + t0) * HW + x;      // (pself + t0 = the frame, kx[k])
    const float s = pr.sens[fx];
    if (s > 0.0f) { cp = pr.alpha; wp = pr.alpha * (disps[fx] - s); }
  }
  Q[static_cast<long long>(k) * HW + x] = 1.0f / (C + cp);           // droid_kernels.cu:1376
  w[static_cast<long long>(k) * HW + x] = ww - wp;
  if (self_in) {
#pragma unroll
    for (int n = 0; n < 6; ++n) Ei[(static_cast<long long>(pself) * 6 + n) * HW + x] = ei[n];
  }
}

// For depth frame k, M stacks the 6-row blocks that couple it to window poses: Ei[k] (its own
// pose) and Eij[e] for every outgoing edge whose target pose is free, plus one extra row w_k,
// so that the rhs correction M (Q w) falls out of the same product.  One workgroup owns
// (512 pixels, k); each wave reduces its 128 pixels with v_mfma_f32_16x16x4_f32 — exact fp32
// FMA chains, K = pixels — one 16x16 tile pair at a time (row tiles re-read from L2, which
// keeps any graph degree in one code path).  Wave partials meet in LDS and leave as fp64
// atomics on the dense pose system: S is SUBTRACTED (A - S, v - E Q w; :1382).  Up to 4 row
// tiles (10 free neighbours) all tile pairs accumulate in one pass; beyond that one pair at a time.
// The reference enumerates (a,b,k) triples on the host and launches one 256-thread block per
// triple with 36 LDS tree reductions each (schur_block :1201-1290, EEt6x6 :980-1035).
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kSchurPix = 256;           // pixels per workgroup (a quarter per wave); 512: 48 workgroups at S-B, 19.9 us; 256: 96, 18.1 us
constexpr int kMaxRows = 1024;           // rows of M the LDS row table can describe
constexpr int kFastTiles = 4;            // up to 4 row tiles (63 rows + w) accumulate in one pass

// Row pointers pass through an LDS table: typed as GLOBAL-address-space pointers, so that what is loaded through them is a
// global_load (a plain `const float*` read back from LDS is a generic pointer and every access a flat_load: 112 of them in
// this kernel, each counting against both vmcnt and lgkmcnt)
typedef const float __attribute__((address_space(1))) gfloat;

// The LDS row table says, per row of M, where the row lives - a source array and a row index in it, packed into one int - and which
// entry of the pose system its sums go to (a short).  6 KB for kMaxRows rows instead of the 12 KB that pointers + ints took: with the
// 40 KB of `red` the workgroup stays under a third of the CU's 160 KB (three workgroups per CU instead of two; a frontend window
// with its inactive edges launches 550-700 of them).
constexpr int kRowEij = 0, kRowMrg = 1, kRowEi = 2, kRowW = 3;
__device__ __forceinline__ int row_code(int src, long long row) { return (src << 28) | static_cast<int>(row); }
struct RowTab {
  const int* code;           // LDS: (source << 28) | row index, -1 = padding
  const short* out;          // LDS: 6 * pose + comp for an M row, -2 for the w row, -1 padding
  const float* base[4];      // Eij, Mrg, Ei, w
  int HW;
  __device__ __forceinline__ gfloat* ptr(int r) const {
    const int c = code[r];
    if (c < 0) return nullptr;
    const int src = c >> 28;
    const float* b = src == kRowEij ? base[0] : (src == kRowMrg ? base[1] : (src == kRowEi ? base[2] : base[3]));
    return (gfloat*)(b + static_cast<long long>(c & 0x0fffffff) * HW);
  }
};

template <bool VEC4>
__device__ __forceinline__ f32x4 load4(gfloat* __restrict__ row, int p, int HW) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (row == nullptr) return v;
  if (VEC4) {
    if (p + 3 < HW) return *reinterpret_cast<const f32x4 __attribute__((address_space(1)))*>(row + p);
  }
  if (p < HW) v.x = row[p];
  if (p + 1 < HW) v.y = row[p + 1];
  if (p + 2 < HW) v.z = row[p + 2];
  if (p + 3 < HW) v.w = row[p + 3];
  return v;
}

// scatter one reduced 16x16 tile (ti,tj) of -S into the pose system
template <typename V>
__device__ __forceinline__ void scatter_tile(V v, int reg, int l, int ti, int tj, const short* rowout,
                                             long long* __restrict__ sys, int n6, int* meta) {
  // D[i][j]: i = 4*(lane>>4)+reg (row in tile ti), j = lane&15 (row in tile tj)
  const int oi = rowout[ti * 16 + 4 * (l >> 4) + reg];
  const int oj = rowout[tj * 16 + (l & 15)];
  if (oi < 0) return;
  const double val = -static_cast<double>(v);
  if (oj >= 0) {
    // lower block triangle only (see pose_block_scatter): entry (oi, oj) if its block row is not above its block column, and
    // the mirrored entry of an off-diagonal tile pair under the same rule - inside a diagonal 6 x 6 block both are kept
    const int bi = oi / 6, bj = oj / 6;
    if (bi >= bj) fix_add(sys, static_cast<long long>(oi) * n6 + oj, val, meta);
    if (ti != tj && bj >= bi) fix_add(sys, static_cast<long long>(oj) * n6 + oi, val, meta);   // mirrored tile
  } else if (oj == -2) {
    fix_add(sys, static_cast<long long>(n6) * n6 + oi, val, meta);                 // rhs: - E (Q w)
  }
}

// all T(T+1)/2 tile pairs in ONE pass over the pixels (rows read once, accumulators static)
template <int T, bool VEC4, int PIX>
__device__ __forceinline__ void schur_pass(const RowTab& rt,
                                           gfloat* __restrict__ qrow, float* red /*[4][NT*4][64]*/,
                                           long long* __restrict__ sys, int HW, int n6, int pix_base, int* meta) {
  constexpr int NT = T * (T + 1) / 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int idx = lane & 15, kq = lane >> 4;
  gfloat* rows[T];
#pragma unroll
  for (int t = 0; t < T; ++t) rows[t] = rt.ptr(t * 16 + idx);
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int s = 0; s < PIX / 64; ++s) {
    const int p = pix_base + s * 16 + 4 * kq;
    const f32x4 q = load4<VEC4>(qrow, p, HW);
    f32x4 b[T], a[T];
#pragma unroll
    for (int t = 0; t < T; ++t) { b[t] = load4<VEC4>(rows[t], p, HW); a[t] = b[t] * q; }
    int n = 0;
#pragma unroll
    for (int ti = 0; ti < T; ++ti)
#pragma unroll
      for (int tj = ti; tj < T; ++tj) {
        // K index of step c = pixel p + c of lane group kq (the same pixel for A and B)
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ti].x, b[tj].x, acc[n], 0, 0, 0);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ti].y, b[tj].y, acc[n], 0, 0, 0);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ti].z, b[tj].z, acc[n], 0, 0, 0);
        acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ti].w, b[tj].w, acc[n], 0, 0, 0);
        ++n;
      }
  }
  BA_WG_PROBE(1, 5);                     // products done (wave 0)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    float* r = red + (static_cast<size_t>(wave) * NT + t) * 256;
    r[lane] = acc[t].x; r[64 + lane] = acc[t].y; r[128 + lane] = acc[t].z; r[192 + lane] = acc[t].w;
  }
  __syncthreads();
  BA_WG_PROBE(1, 6);                     // all four waves' products in LDS
  int n = 0;
#pragma unroll
  for (int ti = 0; ti < T; ++ti)
#pragma unroll
    for (int tj = ti; tj < T; ++tj) {
      const float* r0 = red + static_cast<size_t>(n) * 256 + tid;
      const float v = (r0[0] + r0[static_cast<size_t>(NT) * 256]) +
                      (r0[static_cast<size_t>(2 * NT) * 256] + r0[static_cast<size_t>(3 * NT) * 256]);
      scatter_tile(v, tid >> 6, tid & 63, ti, tj, rt.out, sys, n6, meta);
      ++n;
    }
}

// Row tile ti against the CNT row tiles tj0 .. tj0 + CNT - 1 (tj0 >= ti) in one pass over the pixels: what a depth frame with more
// than kFastTiles row tiles (> 9 free neighbours: a frontend window with its inactive edges, found by the full-sequence run of
// bench.py - the replayed S-B / S-A windows have no inactive edges and never came here) used to do one tile PAIR at a time, two
// workgroup barriers per pair: 15 to 36 rounds, 118 us per launch.  Per pair the SAME chain of MFMAs in the same order and the
// same (w0 + w1) + (w2 + w3) reduction as every other path: bit-identical sums.
template <int CNT, bool VEC4, int PIX>
__device__ __forceinline__ void schur_rowpass(const RowTab& rt, gfloat* __restrict__ qrow, float* red,
                                              long long* __restrict__ sys, int HW, int n6, int pix_base, int* meta, int ti, int tj0) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int idx = lane & 15, kq = lane >> 4;
  gfloat* __restrict__ ra = rt.ptr(ti * 16 + idx);
  gfloat* rb[CNT];
#pragma unroll
  for (int t = 0; t < CNT; ++t) rb[t] = rt.ptr((tj0 + t) * 16 + idx);
  f32x4 acc[CNT];
#pragma unroll
  for (int t = 0; t < CNT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int s = 0; s < PIX / 64; ++s) {
    const int p = pix_base + s * 16 + 4 * kq;
    const f32x4 q = load4<VEC4>(qrow, p, HW);
    const f32x4 a0 = load4<VEC4>(ra, p, HW);
    const f32x4 a = a0 * q;
    f32x4 b[CNT];
#pragma unroll
    for (int t = 0; t < CNT; ++t) b[t] = load4<VEC4>(rb[t], p, HW);
#pragma unroll
    for (int t = 0; t < CNT; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[t].x, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[t].y, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[t].z, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[t].w, acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < CNT; ++t) {
    float* r = red + (static_cast<size_t>(wave) * CNT + t) * 256;
    r[lane] = acc[t].x; r[64 + lane] = acc[t].y; r[128 + lane] = acc[t].z; r[192 + lane] = acc[t].w;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < CNT; ++t) {
    const float* r0 = red + static_cast<size_t>(t) * 256 + tid;
    const float v = (r0[0] + r0[static_cast<size_t>(CNT) * 256]) + (r0[static_cast<size_t>(2 * CNT) * 256] + r0[static_cast<size_t>(3 * CNT) * 256]);
    scatter_tile(v, tid >> 6, tid & 63, ti, tj0 + t, rt.out, sys, n6, meta);
  }
  __syncthreads();                        // `red` is rewritten by the next pass
}

// schur_rowpass with the depth frame's rows STAGED IN LDS (round 6: dense frontend windows).  Streaming from global memory, every row
// tile is read once per row pass it takes part in: 26 frames x 6 chunks with 7 row tiles re-read 1.1 MB of a (frame, chunk)'s 211 KB
// of rows - 170 MB per launch, the whole of its 75 us (tools/ba_kernel_timeline.py at NF=26 RAD=8 HT=30 WD=101: tile pairs 38-52 us
// per workgroup against ~3 us of MFMA).  Staged once per (frame, 256-pixel chunk) the pairs read LDS.  Same operands, same chain of
// MFMAs in the same order, same (w0 + w1) + (w2 + w3) reduction: bit-identical to the streaming form at the same chunk size.
constexpr int kLdsRowPad = 4;            // floats between rows: 16-byte alignment of every row, rows 8 apart share a bank group (2-way)
template <int CNT, int PIX>
__device__ __forceinline__ void schur_rowpass_lds(const float* L, const float* Lq, int nrows, const short* rowout, float* red,
                                                  long long* __restrict__ sys, int n6, int* meta, int ti, int tj0,
                                                  float* __restrict__ part_out, int pair0) {
  constexpr int pitch = PIX + kLdsRowPad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int idx = lane & 15, kq = lane >> 4;
  const int ra_row = ti * 16 + idx;
  const float* ra = L + static_cast<size_t>(ra_row < nrows ? ra_row : 0) * pitch;
  const bool oka = ra_row < nrows;
  const float* rb[CNT];
  bool okb[CNT];
#pragma unroll
  for (int t = 0; t < CNT; ++t) {
    const int r = (tj0 + t) * 16 + idx;
    okb[t] = r < nrows;
    rb[t] = L + static_cast<size_t>(okb[t] ? r : 0) * pitch;
  }
  f32x4 acc[CNT];
#pragma unroll
  for (int t = 0; t < CNT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int s = 0; s < PIX / 64; ++s) {
    const int p = wave * (PIX / 4) + s * 16 + 4 * kq;                    // (inside the chunk)
    const f32x4 q = *reinterpret_cast<const f32x4*>(Lq + p);
    const f32x4 a0 = oka ? *reinterpret_cast<const f32x4*>(ra + p) : zero;
    const f32x4 a = a0 * q;
    f32x4 b[CNT];
#pragma unroll
    for (int t = 0; t < CNT; ++t) b[t] = okb[t] ? *reinterpret_cast<const f32x4*>(rb[t] + p) : zero;
#pragma unroll
    for (int t = 0; t < CNT; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[t].x, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[t].y, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[t].z, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[t].w, acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < CNT; ++t) {
    float* r = red + (static_cast<size_t>(wave) * CNT + t) * 256;
    r[lane] = acc[t].x; r[64 + lane] = acc[t].y; r[128 + lane] = acc[t].z; r[192 + lane] = acc[t].w;
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < CNT; ++t) {
    const float* r0 = red + static_cast<size_t>(t) * 256 + tid;
    const float v = (r0[0] + r0[static_cast<size_t>(CNT) * 256]) + (r0[static_cast<size_t>(2 * CNT) * 256] + r0[static_cast<size_t>(3 * CNT) * 256]);
    // two-stage sums (dense windows): the chunk's tile-pair sum goes to the workspace, ba_schur_reduce_kernel adds a frame's chunks and
    // issues ONE fixed-point atomic per entry and frame - with one per chunk the 3.3 M memory-side atomics of a window's launch were
    // half of its 93 us (tools/ba_kernel_timeline.py with PROBE_DEFS=-DPVO_BA_NO_ATOMICS)
    if (part_out) part_out[static_cast<size_t>(pair0 + t) * 256 + tid] = v;
    else scatter_tile(v, tid >> 6, tid & 63, ti, tj0 + t, rowout, sys, n6, meta);
  }
  __syncthreads();                        // `red` is rewritten by the next pass
}

template <bool VEC4, int PIX>
__device__ __forceinline__ void ba_schur_body(
    const Plan& pl, const int64_t* __restrict__ jj, const float* __restrict__ eta, int K_eta,
    const float* __restrict__ Eii, const float* __restrict__ Cii, const float* __restrict__ bz,
    float* __restrict__ Ei, const float* __restrict__ Eij,
    float* __restrict__ Q, float* __restrict__ w, long long* __restrict__ sys,
    int HW, int t0, int P, const float* __restrict__ part, const int64_t* __restrict__ ii, int E, int chunksA, int deal_rows,
    float* __restrict__ Mrg, int depth_done, int lds_floats, float* __restrict__ spart, short* __restrict__ srow, int* __restrict__ sT,
    const float* __restrict__ disps) {
  __shared__ int rowcode[kMaxRows];       // see RowTab
  __shared__ short rowout[kMaxRows];
  __shared__ int nrows_s;
  __shared__ float red[4 * (kFastTiles * (kFastTiles + 1) / 2) * 256];   // 40 KB
  // the assembly's chunk sums, per edge, are added up and scattered by workgroups of their OWN: the last `deal_rows` rows of the
  // grid (at most two edges each).  Dealt over the depth frames' workgroups, as in round 3, the 36 of 96 that had an edge at S-B
  // started their own work 3.5 us late - and the kernel ends with its slowest workgroup (profiles/r04_ba_kernel_timeline.txt).
  // gridDim.z slices: the row-tile passes of a depth frame with MANY neighbours (more than kFastTiles row tiles: a frontend window
  // with its inactive edges) are dealt over the slices, ti = z, z + gridDim.z, ...; everything else is slice 0's and the other
  // slices leave at once.  Every slice that stays runs the depth phase itself (identical values to identical addresses - the
  // rows a slice reads are the ones it wrote) and every tile pair is still summed by ONE workgroup in the fixed order.
  const int zi = blockIdx.z, Z = gridDim.z;
  if (static_cast<int>(blockIdx.y) >= static_cast<int>(gridDim.y) - deal_rows) {
    if (zi != 0) return;
    if (part && threadIdx.x < 90) {
      // kDealEdges edges per workgroup, CONSECUTIVE in the plan's by-source order: an edge's (ii, ii) block and vi entries land on
      // the same addresses as its neighbours' (same source frame), so their fixed-point addends are summed in a register and
      // leave as one atomic when the address changes - integer sums: the system is bit for bit what one atomic per edge gave.
      // (A real window's 342 edges were 30 780 memory-side atomics, up to ~33 deep on a diagonal entry: half of the launch's
      // 105 us, bench.py `sequence`; two edges a workgroup apart in the edge list shared nothing.)
      const int t = threadIdx.x;
      const int wgi = (blockIdx.y - (gridDim.y - deal_rows)) * gridDim.x + blockIdx.x;
      // (the plan lists only edges whose source frame lies in [0, F): eidx[eptr[K] ..) is not initialised - bound by the plan's count)
      const int Epl = pl.eptr[pl.meta[0]];
      const int p0 = wgi * kDealEdges, p1 = (p0 + kDealEdges < Epl) ? p0 + kDealEdges : Epl;
      long long pend_idx[2] = {-1, -1}, pend_acc[2] = {0, 0};
      for (int pos = p0; pos < p1; ++pos) {
        const int e = pl.eidx[pos];
        double val = 0.0;
        for (int c = 0; c < chunksA; ++c) val += static_cast<double>(part[(static_cast<long long>(e) * chunksA + c) * 90 + t]);
        if (!(fabs(val) < 3.0e10)) { pl.meta[4] = 1; continue; }       // (fix_add's range check)
        const long long q = __double2ll_rn(val * kFix);
        long long idx[2];
        pose_block_targets(t, static_cast<int>(ii[e]) - t0, static_cast<int>(jj[e]) - t0, P, idx);
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
          if (idx[sl] < 0) continue;
          if (idx[sl] == pend_idx[sl]) { pend_acc[sl] += q; continue; }
          if (pend_idx[sl] >= 0) atomicAdd(reinterpret_cast<unsigned long long*>(sys + pend_idx[sl]), static_cast<unsigned long long>(pend_acc[sl]));
          pend_idx[sl] = idx[sl]; pend_acc[sl] = q;
        }
      }
#pragma unroll
      for (int sl = 0; sl < 2; ++sl)
        if (pend_idx[sl] >= 0) atomicAdd(reinterpret_cast<unsigned long long*>(sys + pend_idx[sl]), static_cast<unsigned long long>(pend_acc[sl]));
    }
    return;
  }
  const int k = blockIdx.y;
  BA_WG_PROBE(1, 0);
  if (k >= pl.meta[0]) return;
  BA_WG_PROBE(1, 1);                     // chunk sums of the assembly added, meta read
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n6 = 6 * P;
  // this depth frame's out-edges and their target poses, fetched ONCE and in parallel into LDS: eptr -> eidx -> jj is a chain
  // of three dependent loads that the depth phase and the row table used to walk per edge (12 + 12 serial round trips at S-B)
  __shared__ int s_edge[256], s_pose[256];
  __shared__ int s_lead[64], s_merged[64], any_merged_s;      // (the ballot path below: at most 64 out-edges)
  const int e0 = pl.eptr[k], deg_all = pl.eptr[k + 1] - e0;
  const int pself = pl.kx[k] - t0;
  const bool in_lds = deg_all <= 256;
  if (zi > 0 && 6 * deg_all + 7 <= 16 * kFastTiles) return;      // at most kFastTiles row tiles whatever the poses: slice 0 alone
  if (in_lds && tid < deg_all) {
    const int e = pl.eidx[e0 + tid];
    s_edge[tid] = e;
    s_pose[tid] = static_cast<int>(jj[e]) - t0;
  }
  __syncthreads();
  BA_WG_PROBE(1, 2);                     // edge list in LDS
  // The depth phase needs the edge list only.  Slice 0 issues it BEFORE wave 0 builds the row table, so the table's ~1 us of LDS
  // work hides behind the depth phase's loads (as up to round 4); ONE barrier behind both publishes table and rows together.
  // (S-B's launch: 18.2 us with the table in front and a 64-step follower scan, 17.3 now, 16.2 with round 4's kernel -
  // profiles/r05_schur_sweep.txt, block 6.)
  auto depth_phase = [&]() {
    const DepthPrior pr = load_prior(pl.meta);      // (uniform: one read per workgroup, and none when ba_depth_kernel ran in front)
#pragma unroll
    for (int h = 0; h < PIX / 256; ++h) {
      const int x = blockIdx.x * PIX + h * 256 + tid;
      if (x < HW) depth_pixel(pl, k, x, eta, K_eta, Eii, Cii, bz, Ei, Q, w, HW, t0, P, in_lds ? s_edge : pl.eidx + e0, deg_all, pself, pr, disps);
    }
  };
  // (every slice that gets here may have to stay - more than kFastTiles row tiles unless targets merge or are fixed - and then needs
  // the rows: it issues the depth phase in front of the table like slice 0 instead of behind it; a slice that leaves after all has
  // written the same values to the same addresses as slice 0.)
  // depth_done: ba_depth_kernel ran in front of this launch (windows on 512-pixel chunks, round 6): at a real frontend window every
  // one of the four slices re-read the frame's 16-18 edges x 8 rows here - 164 MB per launch instead of 41, and 20 us at the head of
  // every workgroup (tools/ba_kernel_timeline.py, NF=26 RAD=8 HT=30 WD=101)
  if (!depth_done) depth_phase();
  if (in_lds && deg_all <= 64) {
    // row table by wave 0, one lane per out-edge: the position of an edge's six rows = the number of free target poses before it
    // (ballot + popcount) - the same order as the sequential walk below, which took 1.9 us of this kernel at S-B
    // Round 5: edges of this frame that share their TARGET pose (a frontend window keeps every aged-out edge as an inactive one,
    // factor_graph.py:281-289: the same frame pair several times - 18 out-edges to ~7 distinct poses) contribute row blocks that
    // only ever meet as their SUM: S gets (sum_e E_e) Q (sum_e E_e)^T for that pose.  The first edge of each target (the "leader",
    // in edge order) stands for the group; a leader with followers reads the group's summed rows from `Mrg` (written below by
    // this workgroup for its own pixels, in edge order), one without reads its own Eij rows as before.  Rows 6 x 18 + 7 -> 6 x 7 + 7:
    // four row tiles, the one-pass path.  Frames without repeated targets take exactly the path they took (bit-identical).
    if (tid < 64) {
      const bool free_pose = tid < deg_all && s_pose[tid] >= 0 && s_pose[tid] < P;      // fixed target pose: drops out (:1125, :1227)
      int lead = tid;
      if (free_pose) {
        const int p = s_pose[tid];
        for (int u = 0; u < tid; ++u) if (s_pose[u] == p) { lead = u; break; }
      }
      s_lead[tid] = free_pose ? lead : -1;
      const bool is_lead = free_pose && lead == tid;
      const unsigned long long mask = __ballot(is_lead);
      // followers per leader: a leader has some iff another lane names it
      const int named = (free_pose && lead != tid) ? lead : -1;
      unsigned long long has_f = 0ull;
      for (int u = 1; u < deg_all; ++u) {          // (lane 0 leads itself; uniform bound: deg_all is the workgroup's)
        const int lu = __shfl(named, u);
        if (lu >= 0) has_f |= 1ull << lu;
      }
      const bool self = pself >= 0 && pself < P;
      const int base = self ? 6 : 0;
      const bool merged = is_lead && ((has_f >> tid) & 1ull);
      s_merged[tid] = merged ? 1 : 0;
      if (is_lead) {
        const int r = base + 6 * __popcll(mask & ((1ull << tid) - 1ull));
        const int e = s_edge[tid], p = s_pose[tid];
        const int src = merged ? kRowMrg : kRowEij;
#pragma unroll
        for (int n = 0; n < 6; ++n) { rowcode[r + n] = row_code(src, static_cast<long long>(e) * 6 + n); rowout[r + n] = static_cast<short>(6 * p + n); }
      }
      if (tid == 0) {
        if (self) {
#pragma unroll
          for (int n = 0; n < 6; ++n) { rowcode[n] = row_code(kRowEi, static_cast<long long>(pself) * 6 + n); rowout[n] = static_cast<short>(6 * pself + n); }
        }
        int r = base + 6 * __popcll(mask);
        if (r > 0) { rowcode[r] = row_code(kRowW, k); rowout[r] = -2; ++r; }
        const int padded = (r + 15) & ~15;
        for (int q = r; q < padded; ++q) { rowcode[q] = -1; rowout[q] = -1; }
        nrows_s = r;
        any_merged_s = has_f != 0ull ? 1 : 0;
      }
    }
  } else if (tid == 0) {                  // any degree: sequential
    any_merged_s = 0;
    int r = 0;
    if (pself >= 0 && pself < P) {
      for (int n = 0; n < 6; ++n) { rowcode[r] = row_code(kRowEi, static_cast<long long>(pself) * 6 + n); rowout[r] = static_cast<short>(6 * pself + n); ++r; }
    }
    for (int o = 0; o < deg_all; ++o) {
      const int e = in_lds ? s_edge[o] : pl.eidx[e0 + o];
      const int p = in_lds ? s_pose[o] : static_cast<int>(jj[e]) - t0;
      if (p < 0 || p >= P) continue;      // fixed target pose: drops out (:1125, :1227)
      if (r + 7 > kMaxRows) { pl.meta[3] = 1; break; }   // > 169 free neighbours of one frame: flagged
      for (int n = 0; n < 6; ++n) { rowcode[r] = row_code(kRowEij, static_cast<long long>(e) * 6 + n); rowout[r] = static_cast<short>(6 * p + n); ++r; }
    }
    if (r > 0) { rowcode[r] = row_code(kRowW, k); rowout[r] = -2; ++r; }
    const int padded = (r + 15) & ~15;
    for (int q = r; q < padded; ++q) { rowcode[q] = -1; rowout[q] = -1; }
    nrows_s = r;
  }
  // Slice 0 has issued its depth phase in front of the table (above); the other slices need the tile count first - most of them
  // leave here - and run the depth phase now.
  if (zi > 0) {
    __syncthreads();
    if (((nrows_s + 15) >> 4) <= kFastTiles) return;               // (uniform: nrows_s is the workgroup's)
  }
  BA_WG_PROBE(1, 3);                     // row table built, depth phase issued
  __syncthreads();
  const int nrows = nrows_s;
  const int T = (nrows + 15) >> 4;
  if (in_lds && deg_all <= 64 && any_merged_s) {        // the summed rows of every target group with more than one edge, this workgroup's pixels
#pragma unroll
    for (int h = 0; h < PIX / 256; ++h) {
      const int x = blockIdx.x * PIX + h * 256 + tid;
      if (x >= HW) continue;
      for (int L = 0; L < deg_all; ++L) {
        if (!s_merged[L]) continue;                       // (uniform over the workgroup)
        float m[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int t = L; t < deg_all; ++t) {
          if (s_lead[t] != L) continue;
          const int e = s_edge[t];
#pragma unroll
          for (int n = 0; n < 6; ++n) m[n] += Eij[(static_cast<long long>(e) * 6 + n) * HW + x];
        }
        const int el = s_edge[L];
#pragma unroll
        for (int n = 0; n < 6; ++n) Mrg[(static_cast<long long>(el) * 6 + n) * HW + x] = m[n];
      }
    }
    __syncthreads();                      // (uniform: any_merged_s is the workgroup's)
  }
  BA_WG_PROBE(1, 4);                     // depth rows (and merged rows) stored
  const bool lds_path = lds_floats > 0 && T > kFastTiles && static_cast<long long>(nrows) * (PIX + kLdsRowPad) + PIX <= lds_floats;
  const int slot = schur_stage_slot(pl.kx[k], t0, P);        // (by frame identity: the same on every rank, whatever row k the frame has here)
  const bool staged = lds_path && spart != nullptr && slot >= 0 && T * (T + 1) / 2 <= kSchurStagePairs;
  if (sT != nullptr && slot >= 0 && blockIdx.x == 0 && zi == 0) {          // what ba_schur_reduce_kernel needs to know about this frame
    if (tid == 0) sT[slot] = staged ? T : 0;
    if (staged && tid < 16 * T) srow[slot * 128 + tid] = rowout[tid];
  }
  if (nrows == 0) return;

  gfloat* __restrict__ qrow = (gfloat*)(Q + static_cast<long long>(k) * HW);
  const RowTab rt = {rowcode, rowout, {Eij, Mrg, Ei, w}, HW};
  const int pix_base = blockIdx.x * PIX + wave * (PIX / 4);

  switch (T) {
    case 1: schur_pass<1, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta); BA_WG_PROBE(1, 7); return;
    case 2: schur_pass<2, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta); BA_WG_PROBE(1, 7); return;
    case 3: schur_pass<3, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta); BA_WG_PROBE(1, 7); return;
    case 4: schur_pass<4, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta); BA_WG_PROBE(1, 7); return;
    default: break;
  }
  // any degree: one ROW TILE against up to eight others per pass (row tiles re-read from L2 once per pass)
  constexpr int kPassTiles = 8;           // 8 x 4 x 256 floats of `red` = 32 KB
  if (lds_path) {
    // (round 6) the frame's rows of this chunk + Q, once into LDS (dynamic segment; the host asks for it only on 256-pixel chunks of
    // a dense window and launches ONE slice then); a frame whose rows do not fit streams them as before, a few lines down
    extern __shared__ __attribute__((aligned(16))) float dyn_rows[];
    constexpr int pitch = PIX + kLdsRowPad;
    float* Lq = dyn_rows + static_cast<size_t>(nrows) * pitch;
    const int x0 = blockIdx.x * PIX;
    // (eight rows' loads in flight per wave before the first store: one row at a time the staging was 26 serial round trips to HBM
    // per wave - 50 of the workgroup's 60 us)
    static_assert(PIX == 256 || PIX == 512 || PIX == 1024, "chunk");
    for (int r0 = wave; r0 < nrows; r0 += 32) {
      f32x4 v[8][PIX / 256];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = r0 + 4 * u;
        gfloat* src = rt.ptr(r < nrows ? r : r0);
#pragma unroll
        for (int c = 0; c < PIX / 256; ++c) v[u][c] = load4<VEC4>(src, x0 + c * 256 + lane * 4, HW);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int r = r0 + 4 * u;
        if (r < nrows) {
#pragma unroll
          for (int c = 0; c < PIX / 256; ++c)
            *reinterpret_cast<f32x4*>(dyn_rows + static_cast<size_t>(r) * pitch + c * 256 + lane * 4) = v[u][c];
        }
      }
    }
    if (wave == 0) {
#pragma unroll
      for (int c = 0; c < PIX / 256; ++c) {
        const int px = c * 256 + lane * 4;
        *reinterpret_cast<f32x4*>(Lq + px) = load4<VEC4>(qrow, x0 + px, HW);
      }
    }
    __syncthreads();
    BA_WG_PROBE(1, 5);                   // (LDS form: rows staged)
    float* part_out = staged ? spart + (static_cast<size_t>(slot) * gridDim.x + blockIdx.x) * kSchurStagePairs * 256 : nullptr;
    for (int ti = 0; ti < T; ++ti) {
      if (ti == 1) BA_WG_PROBE(1, 6);    // (LDS form: first row pass - the longest: T tile pairs - done)
      const int ph = ti % (2 * Z);
      if ((ph < Z ? ph : 2 * Z - 1 - ph) != zi) continue;
      for (int tj0 = ti; tj0 < T; tj0 += kPassTiles) {
        const int cnt = (T - tj0 < kPassTiles) ? T - tj0 : kPassTiles;
        const int pair0 = ti * T - ti * (ti - 1) / 2 + (tj0 - ti);      // index of pair (ti, tj0) among the T (T + 1) / 2
        switch (cnt) {
          case 1: schur_rowpass_lds<1, PIX>(dyn_rows, Lq, nrows, rowout, red, sys, n6, pl.meta, ti, tj0, part_out, pair0); break;
          case 2: schur_rowpass_lds<2, PIX>(dyn_rows, Lq, nrows, rowout, red, sys, n6, pl.meta, ti, tj0, part_out, pair0); break;
          case 3: schur_rowpass_lds<3, PIX>(dyn_rows, Lq, nrows, rowout, red, sys, n6, pl.meta, ti, tj0, part_out, pair0); break;
          case 4: schur_rowpass_lds<4, PIX>(dyn_rows, Lq, nrows, rowout, red, sys, n6, pl.meta, ti, tj0, part_out, pair0); break;
          case 5: schur_rowpass_lds<5, PIX>(dyn_rows, Lq, nrows, rowout, red, sys, n6, pl.meta, ti, tj0, part_out, pair0); break;
          case 6: schur_rowpass_lds<6, PIX>(dyn_rows, Lq, nrows, rowout, red, sys, n6, pl.meta, ti, tj0, part_out, pair0); break;
          case 7: schur_rowpass_lds<7, PIX>(dyn_rows, Lq, nrows, rowout, red, sys, n6, pl.meta, ti, tj0, part_out, pair0); break;
          default: schur_rowpass_lds<8, PIX>(dyn_rows, Lq, nrows, rowout, red, sys, n6, pl.meta, ti, tj0, part_out, pair0); break;
        }
      }
    }
    BA_WG_PROBE(1, 7);
    return;
  }
  // row tile ti costs T - ti tile pairs: the slices take them in a SNAKE (0 1 2 3 3 2 1 0 0 1 ...), so that every slice gets the same
  // number of pairs (T = 7, four slices: 7 | 6 + 1 | 5 + 2 | 4 + 3; dealt ti = z, z + 4, .. slice 0 had 10 and slice 3 had 4, and the
  // launch ends with its slowest slice).  Every pair is still one workgroup's chain in the same order: bit-identical.
  for (int ti = 0; ti < T; ++ti) {
    const int ph = ti % (2 * Z);
    if ((ph < Z ? ph : 2 * Z - 1 - ph) != zi) continue;
    for (int tj0 = ti; tj0 < T; tj0 += kPassTiles) {
      const int cnt = (T - tj0 < kPassTiles) ? T - tj0 : kPassTiles;
      switch (cnt) {
        case 1: schur_rowpass<1, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta, ti, tj0); break;
        case 2: schur_rowpass<2, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta, ti, tj0); break;
        case 3: schur_rowpass<3, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta, ti, tj0); break;
        case 4: schur_rowpass<4, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta, ti, tj0); break;
        case 5: schur_rowpass<5, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta, ti, tj0); break;
        case 6: schur_rowpass<6, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta, ti, tj0); break;
        case 7: schur_rowpass<7, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta, ti, tj0); break;
        default: schur_rowpass<8, VEC4, PIX>(rt, qrow, red, sys, HW, n6, pix_base, pl.meta, ti, tj0); break;
      }
    }
  }
  BA_WG_PROBE(1, 7);
}

template <bool VEC4, int PIX>
__global__ __launch_bounds__(256) void ba_schur_mfma_kernel(
    Plan pl, const int64_t* __restrict__ jj, const float* __restrict__ eta, int K_eta,
    const float* __restrict__ Eii, const float* __restrict__ Cii, const float* __restrict__ bz,
    float* __restrict__ Ei, const float* __restrict__ Eij,
    float* __restrict__ Q, float* __restrict__ w, long long* __restrict__ sys,
    int HW, int t0, int P, const float* __restrict__ part, const int64_t* __restrict__ ii, int E, int chunksA, int deal_rows,
    float* __restrict__ Mrg, int depth_done, int lds_floats, float* __restrict__ spart, short* __restrict__ srow, int* __restrict__ sT,
    const float* __restrict__ disps) {
  ba_schur_body<VEC4, PIX>(pl, jj, eta, K_eta, Eii, Cii, bz, Ei, Eij, Q, w, sys, HW, t0, P, part, ii, E, chunksA, deal_rows, Mrg, depth_done, lds_floats,
                           spart, srow, sT, disps);
}

// second stage of the dense-window Schur sums: tile pair p of depth frame k = the sum over the frame's chunks (fixed order, fp64: the
// addends are fp32) -> one fixed-point atomic per entry.  Integer sums across frames as before: bitwise reproducible, and an
// edge-sharded run gets the whole graph's bits (a frame's edges, hence its chunks, live on one rank, and whether a frame is staged
// is decided by its identity: schur_stage_slot).
__global__ __launch_bounds__(256) void ba_schur_reduce_kernel(Plan pl, const float* __restrict__ spart, const short* __restrict__ srow,
                                                              const int* __restrict__ sT, long long* __restrict__ sys, int gx, int n6, int t0) {
  const int k = blockIdx.y, p = blockIdx.x, tid = threadIdx.x;
  if (k >= pl.meta[0]) return;
  const int slot = schur_stage_slot(pl.kx[k], t0, n6 / 6);
  if (slot < 0) return;
  const int T = sT[slot];
  if (T == 0 || p >= T * (T + 1) / 2) return;
  __shared__ short rowout[128];
  if (tid < 128) rowout[tid] = tid < 16 * T ? srow[slot * 128 + tid] : static_cast<short>(-1);
  __syncthreads();
  int ti = 0, base = 0;
  while (base + (T - ti) <= p) { base += T - ti; ++ti; }
  const int tj = ti + (p - base);
  double v = 0.0;
  const float* sp = spart + (static_cast<size_t>(slot) * gx * kSchurStagePairs + p) * 256 + tid;
  const size_t step = static_cast<size_t>(kSchurStagePairs) * 256;
  for (int x0 = 0; x0 < gx; x0 += 8) {                     // (eight chunks' loads in flight; the additions keep the chunk order)
    float a[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) a[u] = sp[static_cast<size_t>(x0 + u < gx ? x0 + u : x0) * step];
#pragma unroll
    for (int u = 0; u < 8; ++u) if (x0 + u < gx) v += static_cast<double>(a[u]);
  }
  scatter_tile(v, tid >> 6, tid & 63, ti, tj, rowout, sys, n6, pl.meta);
}

// the depth phase of the Schur kernel as a launch of its own (one thread per pixel and depth frame): C, w, Q and the frame's own pose
// rows Ei, in exactly the order depth_pixel states - the values are bit for bit what the fused form writes.  Used in front of the
// 512- / 1024-pixel Schur grids (windows beyond ~15 poses), where the Schur kernel's z-slices would each repeat it.
__global__ __launch_bounds__(256) void ba_depth_kernel(
    Plan pl, const float* __restrict__ eta, int K_eta, const float* __restrict__ Eii, const float* __restrict__ Cii,
    const float* __restrict__ bz, float* __restrict__ Ei, float* __restrict__ Q, float* __restrict__ w, int HW, int t0, int P,
    const float* __restrict__ disps) {
  const int k = blockIdx.y;
  if (k >= pl.meta[0]) return;
  const DepthPrior pr = load_prior(pl.meta);
  __shared__ int s_edge[256];
  const int tid = threadIdx.x;
  const int e0 = pl.eptr[k], deg_all = pl.eptr[k + 1] - e0;
  const int pself = pl.kx[k] - t0;
  const bool in_lds = deg_all <= 256;
  if (in_lds && tid < deg_all) s_edge[tid] = pl.eidx[e0 + tid];
  __syncthreads();
  const int x = blockIdx.x * 256 + tid;
  if (x < HW) depth_pixel(pl, k, x, eta, K_eta, Eii, Cii, bz, Ei, Q, w, HW, t0, P, in_lds ? s_edge : pl.eidx + e0, deg_all, pself, pr, disps);
}

}  // namespace
