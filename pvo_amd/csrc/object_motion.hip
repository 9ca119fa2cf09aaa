// object_motion.hip — per-instance rigid motion from the graph's full flow: per job (an edge i -> j and a label of frame i) the transform
// A in SE(3) that takes the segment's back-projected points from camera i at time i to camera j at time j, so that they project onto
// the targets (a PnP problem: six unknowns, two rows per pixel).  Contract: include/pvo_hip.h (pvo_object_motion); yardstick:
// tests/object_motion_reference.py.  The launch shape, the butterfly and the slab layout are tsdf_track.hip's, restated here so that
// the tracker's translation unit keeps its bytes.
//
//   (a) motion_jobs_kernel     one thread per job: the edge and its frames checked, the start (given, or G_j G_i^-1) copied to rel, the
//                              sixteen job floats (R row-major, t, frame i, frame j, edge; frame i = -1: nothing is dereferenced)
//   (b) motion_pixels_kernel   job-major: grid (groups of four 8 x 8 tiles, jobs), a 64-lane wave on a tile.  A wave reads its 64 labels
//                              first; with no member it hands in a zero slab without touching disps, target or weight.  Otherwise r, J
//                              and the pixel's 32 accumulands (H 21, b 6, E, count, the camera-i point 3), reduced in a FIXED order: the
//                              halving butterfly inside the wave, the four waves through LDS, one 128-byte slab per workgroup
//   (c) motion_solve_kernel    one workgroup per job: the slabs summed in fixed order in fp64, the info row, damping, a 6 x 6 fp64
//                              Cholesky, the step, the retraction (se3.h), the next job floats; after the last evaluation the motion
//                              in the world frame and the centroid
//
// 2 iters + 3 launches: (a), then (b)(c) per evaluation.  No atomics, no allocation, no host synchronisation; no device loop's trip count
// depends on data.
#include "se3.h"

namespace {

constexpr int kBlock = 256;           // four waves side by side: 32 x 8 pixels
constexpr int kTile = 8;
constexpr int kSlab = 32;             // floats per workgroup and job: H 0..20, b 21..26, E 27, count 28, sum of Xi 29..31
constexpr int kSolveBlock = 256;      // eight groups of 32 threads walk a job's slabs
constexpr int kJobFloats = 16;        // R 0..8, t 9..11, frame i [12], frame j [13], edge [14] (as int bits), [15] unused
constexpr size_t kAlign = 256;

inline size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }
inline bool finite_f(float v) { return v - v == 0.0f; }

// R of the quaternion as stored (no normalisation), every multiply-add one fma; then t
__device__ __forceinline__ void job_constants(const Pose A, float* __restrict__ o) {
  const float x = A.q.x, y = A.q.y, z = A.q.z, w = A.q.w;
  o[0] = fmaf(-2.0f, fmaf(y, y, z * z), 1.0f); o[1] = 2.0f * fmaf(x, y, -(z * w));          o[2] = 2.0f * fmaf(x, z, y * w);
  o[3] = 2.0f * fmaf(x, y, z * w);             o[4] = fmaf(-2.0f, fmaf(x, x, z * z), 1.0f); o[5] = 2.0f * fmaf(y, z, -(x * w));
  o[6] = 2.0f * fmaf(x, z, -(y * w));          o[7] = 2.0f * fmaf(y, z, x * w);             o[8] = fmaf(-2.0f, fmaf(x, x, y * y), 1.0f);
  o[9] = A.t.x; o[10] = A.t.y; o[11] = A.t.z;
}

__device__ __forceinline__ void store_pose(float* p, const Pose T) {
  const float v[7] = {T.t.x, T.t.y, T.t.z, T.q.x, T.q.y, T.q.z, T.q.w};
#pragma unroll
  for (int k = 0; k < 7; ++k) p[k] = v[k];
}

// A B and A^-1 B from se3.h's quaternion product and rotation; the quaternions are stored as the products come
__device__ __forceinline__ Pose pose_mul(const Pose A, const Pose B) {
  Pose C;
  C.q = qmul(A.q, B.q);
  const Vec3 r = rotate(A.q, B.t);
  C.t = {r.x + A.t.x, r.y + A.t.y, r.z + A.t.z};
  return C;
}
__device__ __forceinline__ Pose pose_inv_mul(const Pose A, const Pose B) {
  const Quat qi = qconj(A.q);
  Pose C;
  C.q = qmul(qi, B.q);
  C.t = rotate(qi, {B.t.x - A.t.x, B.t.y - A.t.y, B.t.z - A.t.z});
  return C;
}

struct Jobs {
  const float* poses; const int64_t* ii; const int64_t* jj; const int64_t* job_edge; const float* start;
  float* rel; float* jc;
  int N, E, nframes;
};

__global__ __launch_bounds__(64) void motion_jobs_kernel(const Jobs in) {
  const int n = blockIdx.x * 64 + threadIdx.x;
  if (n >= in.N) return;
  float* o = in.jc + static_cast<long long>(kJobFloats) * n;
  const long long e = in.job_edge[n];
  long long fi = -1, fj = -1;
  if (e >= 0 && e < in.E) { fi = in.ii[e]; fj = in.jj[e]; }
  const bool known = fi >= 0 && fi < in.nframes && fj >= 0 && fj < in.nframes;
  Pose A;
  A.t = {0.0f, 0.0f, 0.0f};
  A.q = {0.0f, 0.0f, 0.0f, 1.0f};
  if (in.start) A = load_pose(in.start + 7ll * n);                     // (read before rel, which may be the same array, is written)
  else if (known) A = rel_pose(load_pose(in.poses + 7 * fi), load_pose(in.poses + 7 * fj));
  store_pose(in.rel + 7ll * n, A);
  job_constants(A, o);
  o[12] = __int_as_float(known ? static_cast<int>(fi) : -1);
  o[13] = __int_as_float(known ? static_cast<int>(fj) : -1);
  o[14] = __int_as_float(known ? static_cast<int>(e) : -1);
  o[15] = 0.0f;
}

// one step of the halving butterfly: lanes l and l ^ MASK share 2 HALF values; the lane with the bit keeps the upper HALF, the other the
// lower HALF, and each adds what its partner hands over.  The value a lane ends with is fixed by its lane number alone.
template <int HALF>
__device__ __forceinline__ void butterfly(float (&a)[kSlab], int lane, int mask) {
  const bool up = (lane & mask) != 0;
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const float send = up ? a[i] : a[i + HALF], keep = up ? a[i + HALF] : a[i];
    a[i] = keep + __shfl_xor(send, mask);
  }
}

struct Pixels {
  const float* jc; const float* intrinsics; const float* disps; const int32_t* labels; const int32_t* job_label;
  const float* target; const float* weight;
  int N, ht, wd, across;              // across: workgroups per row of tiles
  float z_min, huber;
  float* slabs; float* residual; float* jac;
};

__global__ __launch_bounds__(kBlock) void motion_pixels_kernel(const Pixels in) {
  __shared__ float part[kBlock / 64][kSlab];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bx = static_cast<int>(blockIdx.x) % in.across, by = static_cast<int>(blockIdx.x) / in.across;
  const int ui = (bx * (kBlock / 64) + wave) * kTile + (lane & 7), vi = by * kTile + (lane >> 3);
  const bool inside = ui < in.wd && vi < in.ht;
  const float fx = in.intrinsics[0], fy = in.intrinsics[1], cx = in.intrinsics[2], cy = in.intrinsics[3];
  const long long HW = static_cast<long long>(in.ht) * in.wd;
  const long long pix = static_cast<long long>(vi) * in.wd + ui;
  const long long nb = gridDim.x, blk = blockIdx.x;
  for (int n = blockIdx.y; n < in.N; n += gridDim.y) {
    const float* __restrict__ c = in.jc + static_cast<long long>(kJobFloats) * n;        // wave-uniform
    const int fi = __float_as_int(c[12]), e = __float_as_int(c[14]);
    bool member = false;
    if (inside && fi >= 0) member = in.labels[fi * HW + pix] == in.job_label[n];
    float a[kSlab];
#pragma unroll
    for (int k = 0; k < kSlab; ++k) a[k] = 0.0f;
    float r[2] = {0.0f, 0.0f}, J[2][6] = {{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}};
    bool votes = false;
    const bool any = __ballot(member) != 0ull;                                            // wave-uniform
    if (member) {
      const float d = in.disps[fi * HW + pix];
      const float w = in.weight ? in.weight[e * HW + pix] : 1.0f;
      const float tu = in.target[2 * (e * HW + pix)], tv = in.target[2 * (e * HW + pix) + 1];
      if (d > 0.0f && d - d == 0.0f && w > 0.0f && w - w == 0.0f) {
        const float z = 1.0f / d;
        const float rx = (static_cast<float>(ui) - cx) / fx, ry = (static_cast<float>(vi) - cy) / fy;
        const float X[3] = {z * rx, z * ry, z};
        float Y[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) Y[i] = fmaf(c[3 * i], X[0], fmaf(c[3 * i + 1], X[1], fmaf(c[3 * i + 2], X[2], c[9 + i])));
        votes = Y[2] > in.z_min && tu - tu == 0.0f && tv - tv == 0.0f;
        if (votes) {
          const float iz = 1.0f / Y[2];
          const float qx = Y[0] * iz, qy = Y[1] * iz;
          r[0] = fmaf(fx, qx, cx) - tu;
          r[1] = fmaf(fy, qy, cy) - tv;
          const float ax = fx * iz, ay = fy * iz;
          const float mx = -(ax * qx), my = -(ay * qy);
          J[0][0] = ax; J[0][2] = mx;
          J[0][3] = mx * Y[1];
          J[0][4] = fmaf(ax, Y[2], -(mx * Y[0]));
          J[0][5] = -(ax * Y[1]);
          J[1][1] = ay; J[1][2] = my;
          J[1][3] = fmaf(my, Y[1], -(ay * Y[2]));
          J[1][4] = -(my * Y[0]);
          J[1][5] = ay * Y[0];
          const float mag = sqrtf(fmaf(r[0], r[0], r[1] * r[1]));
          const bool quad = in.huber == 0.0f || mag <= in.huber;
          const float k = quad ? 1.0f : in.huber / mag;
          const float rho = quad ? mag * mag : in.huber * fmaf(2.0f, mag, -in.huber);
          const float wk = w * k;
          int t = 0;
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            const float wu = wk * J[0][i], wv = wk * J[1][i];
#pragma unroll
            for (int j = i; j < 6; ++j) a[t++] = fmaf(wu, J[0][j], wv * J[1][j]);
            a[21 + i] = fmaf(wu, r[0], wv * r[1]);
          }
          a[27] = w * rho;
          a[28] = 1.0f;
          a[29] = X[0]; a[30] = X[1]; a[31] = X[2];
        }
      }
    }
    if (inside) {
      if (in.residual) {
        float* o = in.residual + 2 * (n * HW + pix);
        o[0] = votes ? r[0] : __builtin_nanf("");
        o[1] = votes ? r[1] : __builtin_nanf("");
      }
      if (in.jac) {
        float* o = in.jac + 12 * (n * HW + pix);
#pragma unroll
        for (int i = 0; i < 12; ++i) o[i] = votes ? J[i / 6][i % 6] : 0.0f;
      }
    }
    if (any) {                                                          // (a wave without a member: its 32 sums are +0 as they stand)
      butterfly<16>(a, lane, 32);
      butterfly<8>(a, lane, 16);
      butterfly<4>(a, lane, 8);
      butterfly<2>(a, lane, 4);
      butterfly<1>(a, lane, 2);
      a[0] = a[0] + __shfl_xor(a[0], 1);                                // value (lane >> 1) of the wave
    }
    if (!(lane & 1)) part[wave][lane >> 1] = a[0];
    __syncthreads();
    if (threadIdx.x < kSlab) {
      const int t = threadIdx.x;
      in.slabs[(n * nb + blk) * kSlab + t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
    }
    __syncthreads();
  }
}

struct Solve {
  const float* slabs; const float* poses; float* jc; float* rel; float* motion; float* info; double* system; float* centroid;
  int nb, rows, row, last, min_count;
  float lm, ep;
};

__global__ __launch_bounds__(kSolveBlock) void motion_solve_kernel(const Solve in) {
  __shared__ double part[kSolveBlock / kSlab][kSlab];
  __shared__ double sum[kSlab];
  const int s = blockIdx.x, t = threadIdx.x & (kSlab - 1), grp = threadIdx.x / kSlab;
  const float* __restrict__ slab = in.slabs + static_cast<long long>(s) * in.nb * kSlab;
  double acc = 0.0;
  for (int k = grp; k < in.nb; k += kSolveBlock / kSlab) acc += static_cast<double>(slab[static_cast<long long>(k) * kSlab + t]);
  part[grp][t] = acc;
  __syncthreads();
  if (threadIdx.x < kSlab) {
    double v = part[0][t];
#pragma unroll
    for (int g = 1; g < kSolveBlock / kSlab; ++g) v += part[g][t];
    sum[t] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float* jc = in.jc + static_cast<long long>(kJobFloats) * s;
  float* row = in.info + (static_cast<long long>(s) * in.rows + in.row) * 4;
  double* sys = in.system && in.last ? in.system + 27ll * s : nullptr;
  float* cen = in.centroid && in.last ? in.centroid + 3ll * s : nullptr;
  const int fi = __float_as_int(jc[12]), fj = __float_as_int(jc[13]);
  if (fi < 0) {                           // no such edge or frame: rel holds the start, nothing else is known
    row[0] = 0.0f; row[1] = 0.0f; row[2] = 0.0f; row[3] = 4.0f;
    if (sys) for (int k = 0; k < 27; ++k) sys[k] = 0.0;
    if (cen) { cen[0] = 0.0f; cen[1] = 0.0f; cen[2] = 0.0f; }
    if (in.last) {
      float* m = in.motion + 7ll * s;
      m[0] = 0.0f; m[1] = 0.0f; m[2] = 0.0f; m[3] = 0.0f; m[4] = 0.0f; m[5] = 0.0f; m[6] = 1.0f;
    }
    return;
  }
  if (sys) for (int k = 0; k < 27; ++k) sys[k] = sum[k];
  double A[6][6], rhs[6];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int j = i; j < 6; ++j) { A[i][j] = sum[k]; A[j][i] = sum[k]; ++k; }
      rhs[i] = -sum[21 + i];
    }
  }
  const double lm = static_cast<double>(in.lm), ep = static_cast<double>(in.ep);
#pragma unroll
  for (int i = 0; i < 6; ++i) A[i][i] = A[i][i] + (lm * A[i][i] + ep);
  // Cholesky A = L L^T in place (lower), every pivot tested; then L y = -b, L^T xi = y
  bool good = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double dgl = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) dgl -= A[j][k] * A[j][k];
    good = good && dgl > 0.0 && dgl - dgl == 0.0;
    const double l = sqrt(dgl);
    A[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= A[i][k] * A[j][k];
      A[i][j] = v / l;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = rhs[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= A[i][k] * rhs[k];
    rhs[i] = v / A[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = rhs[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v -= A[k][i] * rhs[k];
    rhs[i] = v / A[i][i];
  }
  float xi[6], big = 0.0f;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    xi[i] = static_cast<float>(rhs[i]);
    good = good && xi[i] - xi[i] == 0.0f;
    big = fmaxf(big, fabsf(xi[i]));
  }
  const bool few = !(sum[28] >= static_cast<double>(in.min_count));
  const int status = few ? 1 : (good ? 0 : 2);
  const bool step = status == 0 && !in.last;
  row[0] = static_cast<float>(sum[27]); row[1] = static_cast<float>(sum[28]); row[2] = step ? big : 0.0f; row[3] = static_cast<float>(status);
  float* ps = in.rel + 7ll * s;
  if (step) {
    const Pose T = retract(xi, load_pose(ps));
    store_pose(ps, T);
    job_constants(T, jc);
  }
  if (!in.last) return;
  const Pose Gi = load_pose(in.poses + 7ll * fi), Gj = load_pose(in.poses + 7ll * fj);
  store_pose(in.motion + 7ll * s, pose_inv_mul(Gj, pose_mul(load_pose(ps), Gi)));          // G_j^-1 (A G_i)
  if (cen) {
    Vec3 m = {0.0f, 0.0f, 0.0f};
    if (sum[28] > 0.0) {
      const Vec3 mean = {static_cast<float>(sum[29] / sum[28]), static_cast<float>(sum[30] / sum[28]), static_cast<float>(sum[31] / sum[28])};
      m = rotate(qconj(Gi.q), {mean.x - Gi.t.x, mean.y - Gi.t.y, mean.z - Gi.t.z});
    }
    cen[0] = m.x; cen[1] = m.y; cen[2] = m.z;
  }
}

inline int blocks_of(int ht, int wd) {
  const int across = kTile * (kBlock / 64);
  return ((wd + across - 1) / across) * ((ht + kTile - 1) / kTile);
}

inline size_t workspace_bytes(int N, int ht, int wd) {
  if (N <= 0 || ht <= 0 || wd <= 0 || static_cast<long long>(ht) * wd >= (1ll << 31)) return 0;
  return aligned(sizeof(float) * kJobFloats * static_cast<size_t>(N)) +
         aligned(sizeof(float) * kSlab * static_cast<size_t>(N) * static_cast<size_t>(blocks_of(ht, wd)));
}

}  // namespace

#define PVO_REQ(c) do { if (!(c)) return PVO_EINVAL; } while (0)

extern "C" size_t pvo_object_motion_args_size(void) { return sizeof(pvo_object_motion_args); }
extern "C" size_t pvo_object_motion_workspace_bytes(int N, int ht, int wd) { return workspace_bytes(N, ht, wd); }

extern "C" int pvo_object_motion(const pvo_object_motion_args* a, void* workspace, size_t workspace_bytes_given, void* stream) {
  PVO_REQ(a);
  PVO_REQ(a->N >= 0 && a->E >= 0 && a->nframes >= 0 && a->ht >= 0 && a->wd >= 0 && static_cast<long long>(a->ht) * a->wd < (1ll << 31));
  PVO_REQ(a->iters >= 0 && a->iters <= PVO_OBJECT_MOTION_MAX_ITERS && a->z_min > 0.0f && finite_f(a->z_min) && a->huber >= 0.0f &&
          finite_f(a->huber) && a->lm >= 0.0f && finite_f(a->lm) && a->ep >= 0.0f && finite_f(a->ep) && a->min_count >= 1);
  if (a->N == 0 || static_cast<long long>(a->ht) * a->wd == 0) return PVO_OK;      // no job or no pixel
  PVO_REQ(a->intrinsics && a->job_edge && a->job_label && a->rel && a->motion && a->info);
  PVO_REQ(a->nframes == 0 || (a->poses && a->disps && a->labels));
  PVO_REQ(a->E == 0 || (a->ii && a->jj && a->target));
  PVO_REQ(static_cast<long long>(a->N) * blocks_of(a->ht, a->wd) < (1ll << 31));
  if (!workspace || workspace_bytes_given < workspace_bytes(a->N, a->ht, a->wd)) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  hipStream_t s = pvo_stream(stream);
  float* jc = static_cast<float*>(workspace);
  float* slabs = reinterpret_cast<float*>(static_cast<char*>(workspace) + aligned(sizeof(float) * kJobFloats * static_cast<size_t>(a->N)));
  const Jobs jobs = {a->poses, a->ii, a->jj, a->job_edge, a->start, a->rel, jc, a->N, a->E, a->nframes};
  hipLaunchKernelGGL(motion_jobs_kernel, dim3((a->N + 63) / 64), dim3(64), 0, s, jobs);
  PVO_CHECK_LAUNCH();
  const int across = (a->wd + kTile * (kBlock / 64) - 1) / (kTile * (kBlock / 64)), nb = blocks_of(a->ht, a->wd);
  const dim3 grid(nb, a->N < 65535 ? a->N : 65535);
  for (int e = 0; e <= a->iters; ++e) {
    const bool last = e == a->iters;
    const Pixels px = {jc, a->intrinsics, a->disps, a->labels, a->job_label, a->target, a->weight, a->N, a->ht, a->wd, across,
                       a->z_min, a->huber, slabs, last ? a->residual : nullptr, last ? a->jac : nullptr};
    hipLaunchKernelGGL(motion_pixels_kernel, grid, dim3(kBlock), 0, s, px);
    PVO_CHECK_LAUNCH();
    const Solve sv = {slabs, a->poses, jc, a->rel, a->motion, a->info, a->system, a->centroid, nb, a->iters + 1, e, last ? 1 : 0,
                      a->min_count, a->lm, a->ep};
    hipLaunchKernelGGL(motion_solve_kernel, dim3(a->N), dim3(kSolveBlock), 0, s, sv);
    PVO_CHECK_LAUNCH();
  }
  return PVO_OK;
}
