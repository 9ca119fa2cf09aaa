// tsdf_track.hip — frame-to-model tracking: refine a camera pose against the fused TSDF by minimising the signed distance at the
// frame's back-projected pixels (direct SDF tracking, Bylow et al. 2013).  Contracts: include/pvo_hip.h (pvo_tsdf_track,
// pvo_tsdf_sparse_track); yardstick: tests/tsdf_track_reference.py.
//
//   (a) track_views_kernel    one thread per slot: the start pose copied to poses_out, the sixteen view floats of tsdf_ray.h from it
//                             (the FRAME id in [12], -1 for an id outside [0, nframes))
//   (b) track_pixels_kernel   one thread per pixel, the render's block shape (a 64-lane wave on an 8 x 8 tile, four waves side by side):
//                             ONE trilinear sample at the pixel's own depth, its gradient, J, and the pixel's 29 accumulands
//                             (H's upper triangle 21, b 6, E, count).  They are reduced in a FIXED order: inside the wave by a halving
//                             butterfly (32 shuffles: at every step a lane keeps half of its values and hands the other half over),
//                             across the four waves through LDS, and written as one 128-byte slab per workgroup
//   (c) track_solve_kernel    one workgroup per slot: the slot's slabs summed in fixed order in fp64, the info row, damping, a 6 x 6
//                             fp64 Cholesky, the step, the retraction (se3.h), the pose and the view floats of the next evaluation
//
// 2 iters + 3 launches: (a), then (b)(c) per evaluation.  No atomics, no allocation, no host synchronisation; no device loop's trip count
// depends on data.  The slab sum and the solve are NOT folded into the next (b)'s prologue: see DESIGN.md (frame-to-model tracking).
#include "tsdf_volume.h"

namespace {

using namespace tsdf_volume;         // aligned, finite_f, volume_ok, world_ok, kB

constexpr int kBlock = 256;           // four waves side by side: 32 x 8 pixels
constexpr int kTile = 8;
constexpr int kSlab = 32;             // floats per workgroup and slot: H 0..20, b 21..26, E 27, count 28, 29..31 zero
constexpr int kSolveBlock = 256;      // eight groups of 32 threads walk a slot's slabs

// a volume that has no cell (a dense dimension < 2, no brick): nothing is valid and nothing is dereferenced
struct EmptyVolume {
  const float* tsdf; const float* wsum;
  int n[3];
  float min_weight;
  __device__ __forceinline__ int corners(const int (&)[3], int (&)[8]) const { return 2; }
};

struct Frames { const float* vc; const float* intrinsics; const float* disps; const float* weight; int N, ht, wd; float band, huber; };
struct PixelOut { float* slabs; float* residual; float* jac; };

__global__ __launch_bounds__(64) void track_views_kernel(const float* poses, float* poses_out, const int64_t* __restrict__ ix,
                                                         float* __restrict__ vc, int N, int nframes, const Vol vol) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= N) return;
  float p[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) p[k] = poses[7ll * s + k];
#pragma unroll
  for (int k = 0; k < 7; ++k) poses_out[7ll * s + k] = p[k];
  float* o = vc + static_cast<long long>(kViewFloats) * s;
  const long long f = ix[s];
  if (f < 0 || f >= nframes) {            // never dereferenced
    o[12] = __int_as_float(-1);
    return;
  }
  ray_view_constants(p, 0, vol, o);
  o[12] = __int_as_float(static_cast<int>(f));
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

template <class V>
__global__ __launch_bounds__(kBlock) void track_pixels_kernel(V vol, const Frames in, const PixelOut out) {
  __shared__ float part[kBlock / 64][kSlab];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ui = (blockIdx.x * (kBlock / 64) + wave) * kTile + (lane & 7), vi = blockIdx.y * kTile + (lane >> 3);
  const bool inside = ui < in.wd && vi < in.ht;
  const Intr K = load_intr(in.intrinsics);
  const long long HW = static_cast<long long>(in.ht) * in.wd;
  const long long pix = static_cast<long long>(vi) * in.wd + ui;
  const long long nb = static_cast<long long>(gridDim.x) * gridDim.y, blk = static_cast<long long>(blockIdx.y) * gridDim.x + blockIdx.x;
  for (int b = blockIdx.z; b < in.N; b += gridDim.z) {
    const float* __restrict__ c = in.vc + static_cast<long long>(kViewFloats) * b;        // wave-uniform
    const int f = __float_as_int(c[12]);
    float a[kSlab];
#pragma unroll
    for (int k = 0; k < kSlab; ++k) a[k] = 0.0f;
    float S = 0.0f, J[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool votes = false;
    if (inside && f >= 0) {
      const float d = in.disps[f * HW + pix];
      const float w = in.weight ? in.weight[f * HW + pix] : 1.0f;
      if (d > 0.0f && d - d == 0.0f && w > 0.0f && w - w == 0.0f) {
        const float z = 1.0f / d;
        const Ray r = ray_of_pixel(c, K, ui, vi);
        int cell[3], at[8];
        float fr[3];
        bool valid = ray_point_cell(r, z, vol.n, cell, fr);
        if (valid) valid = vol.corners(cell, at) == 0;
        if (valid) valid = vol.wsum[at[0]] >= vol.min_weight;       // corner 0's weight before the other fifteen values
        if (valid) {
#pragma unroll
          for (int j = 1; j < 8; ++j) valid = valid && vol.wsum[at[j]] >= vol.min_weight;
        }
        if (valid) {
          float s[8], g[3];
#pragma unroll
          for (int j = 0; j < 8; ++j) s[j] = vol.tsdf[at[j]];
          S = ray_trilinear(s, fr);
          const float mag = fabsf(S);
          votes = mag < in.band;
          if (votes) {
            ray_gradient(s, fr, g);
            const float rx = (static_cast<float>(ui) - K.cx) / K.fx, ry = (static_cast<float>(vi) - K.cy) / K.fy;
            const float X[3] = {z * rx, z * ry, z};
            float gc[3];                                              // R grad / voxel = M^T grad
#pragma unroll
            for (int i = 0; i < 3; ++i) gc[i] = fmaf(c[i], g[0], fmaf(c[3 + i], g[1], c[6 + i] * g[2]));
            J[0] = -gc[0]; J[1] = -gc[1]; J[2] = -gc[2];
            J[3] = -fmaf(X[1], gc[2], -(X[2] * gc[1]));
            J[4] = -fmaf(X[2], gc[0], -(X[0] * gc[2]));
            J[5] = -fmaf(X[0], gc[1], -(X[1] * gc[0]));
            const bool quad = in.huber == 0.0f || mag <= in.huber;
            const float k = quad ? 1.0f : in.huber / mag;
            const float rho = quad ? S * S : in.huber * fmaf(2.0f, mag, -in.huber);
            const float wk = w * k;
            int t = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
              const float wj = wk * J[i];
#pragma unroll
              for (int j = i; j < 6; ++j) a[t++] = wj * J[j];
              a[21 + i] = wj * S;
            }
            a[27] = w * rho;
            a[28] = 1.0f;
          }
        }
      }
    }
    if (inside) {
      if (out.residual) out.residual[b * HW + pix] = votes ? S : __builtin_nanf("");
      if (out.jac) {
        float* o = out.jac + 6 * (b * HW + pix);
#pragma unroll
        for (int i = 0; i < 6; ++i) o[i] = votes ? J[i] : 0.0f;
      }
    }
    butterfly<16>(a, lane, 32);
    butterfly<8>(a, lane, 16);
    butterfly<4>(a, lane, 8);
    butterfly<2>(a, lane, 4);
    butterfly<1>(a, lane, 2);
    const float total = a[0] + __shfl_xor(a[0], 1);                   // value (lane >> 1) of the wave
    if (!(lane & 1)) part[wave][lane >> 1] = total;
    __syncthreads();
    if (threadIdx.x < kSlab) {
      const int t = threadIdx.x;
      out.slabs[(b * nb + blk) * kSlab + t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
    }
    __syncthreads();
  }
}

struct Solve {
  const float* slabs; float* vc; float* poses_out; float* info; double* system;
  int nb, rows, row, last, min_count;
  float lm, ep;
  Vol vol;
};

__global__ __launch_bounds__(kSolveBlock) void track_solve_kernel(const Solve in) {
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
  float* vc = in.vc + static_cast<long long>(kViewFloats) * s;
  float* row = in.info + (static_cast<long long>(s) * in.rows + in.row) * 4;
  double* sys = in.system && in.last ? in.system + 27ll * s : nullptr;
  const int f = __float_as_int(vc[12]);
  if (f < 0) {                            // an id outside [0, nframes): the pose was copied, nothing else is known
    row[0] = 0.0f; row[1] = 0.0f; row[2] = 0.0f; row[3] = 4.0f;
    if (sys) for (int k = 0; k < 27; ++k) sys[k] = 0.0;
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
  if (!step) return;                      // the pose and its view floats stay
  float* ps = in.poses_out + 7ll * s;
  const Pose T = retract(xi, load_pose(ps));
  const float p[7] = {T.t.x, T.t.y, T.t.z, T.q.x, T.q.y, T.q.z, T.q.w};
#pragma unroll
  for (int k = 0; k < 7; ++k) ps[k] = p[k];
  ray_view_constants(p, 0, in.vol, vc);
  vc[12] = __int_as_float(f);
}

// what the two calls share behind their volume
struct Common {
  const float* poses; const float* disps; const float* intrinsics; const int64_t* ix; const float* weight;
  int N, nframes, ht, wd, iters, min_count;
  float band, huber, lm, ep, voxel, min_weight;
  const float* origin;
  float* poses_out; float* info; double* system; float* residual; float* jac;
};

inline int blocks_of(int ht, int wd) {
  const int across = kTile * (kBlock / 64);
  return ((wd + across - 1) / across) * ((ht + kTile - 1) / kTile);
}

inline size_t workspace_bytes(int N, int ht, int wd) {
  if (N <= 0 || ht <= 0 || wd <= 0 || static_cast<long long>(ht) * wd >= (1ll << 31)) return 0;
  return aligned(sizeof(float) * kViewFloats * static_cast<size_t>(N)) +
         aligned(sizeof(float) * kSlab * static_cast<size_t>(N) * static_cast<size_t>(blocks_of(ht, wd)));
}

inline bool track_ok(const Common& c) {
  return c.N >= 0 && c.nframes >= 0 && c.ht >= 0 && c.wd >= 0 && static_cast<long long>(c.ht) * c.wd < (1ll << 31) &&
         c.ht <= kTile * 65535 &&           // (one row of workgroups per eight rows of pixels, gridDim.y <= 65535)
         c.voxel > 0.0f && finite_f(c.voxel) && c.min_weight == c.min_weight &&
         finite_f(c.origin[0]) && finite_f(c.origin[1]) && finite_f(c.origin[2]) &&
         c.iters >= 0 && c.iters <= PVO_TSDF_TRACK_MAX_ITERS && c.band > 0.0f && c.band <= 1.0f && c.huber >= 0.0f && finite_f(c.huber) &&
         c.lm >= 0.0f && finite_f(c.lm) && c.ep >= 0.0f && finite_f(c.ep) && c.min_count >= 1;
}

template <class V>
int launch(const V& vol, const Common& c, void* workspace, hipStream_t s) {
  float* vc = static_cast<float*>(workspace);
  float* slabs = reinterpret_cast<float*>(static_cast<char*>(workspace) + aligned(sizeof(float) * kViewFloats * static_cast<size_t>(c.N)));
  const Vol o = {c.origin[0], c.origin[1], c.origin[2], c.voxel};
  const int across = kTile * (kBlock / 64);
  const dim3 grid((c.wd + across - 1) / across, (c.ht + kTile - 1) / kTile, c.N < 65535 ? c.N : 65535);
  hipLaunchKernelGGL(track_views_kernel, dim3((c.N + 63) / 64), dim3(64), 0, s, c.poses, c.poses_out, c.ix, vc, c.N, c.nframes, o);
  PVO_CHECK_LAUNCH();
  const Frames in = {vc, c.intrinsics, c.disps, c.weight, c.N, c.ht, c.wd, c.band, c.huber};
  for (int e = 0; e <= c.iters; ++e) {
    const bool last = e == c.iters;
    const PixelOut out = {slabs, last ? c.residual : nullptr, last ? c.jac : nullptr};
    hipLaunchKernelGGL(track_pixels_kernel<V>, grid, dim3(kBlock), 0, s, vol, in, out);
    PVO_CHECK_LAUNCH();
    const Solve sv = {slabs, vc, c.poses_out, c.info, c.system, static_cast<int>(grid.x * grid.y), c.iters + 1, e, last ? 1 : 0, c.min_count,
                      c.lm, c.ep, o};
    hipLaunchKernelGGL(track_solve_kernel, dim3(c.N), dim3(kSolveBlock), 0, s, sv);
    PVO_CHECK_LAUNCH();
  }
  return PVO_OK;
}

}  // namespace

extern "C" size_t pvo_tsdf_track_args_size(void) { return sizeof(pvo_tsdf_track_args); }
extern "C" size_t pvo_tsdf_sparse_track_args_size(void) { return sizeof(pvo_tsdf_sparse_track_args); }

extern "C" size_t pvo_tsdf_track_workspace_bytes(int N, int ht, int wd) { return workspace_bytes(N, ht, wd); }
extern "C" size_t pvo_tsdf_sparse_track_workspace_bytes(int N, int ht, int wd) { return workspace_bytes(N, ht, wd); }

// the checks both calls make after their volume's limits; PVO_OK + *go = false: nothing to do
static int track_common(const Common& c, const void* workspace, size_t workspace_bytes_given, bool* go) {
  *go = false;
  PVO_REQ(track_ok(c));
  if (c.N == 0 || static_cast<long long>(c.ht) * c.wd == 0) return PVO_OK;      // no pixel
  PVO_REQ(c.poses && c.poses_out && c.info && c.disps && c.intrinsics && c.ix);
  PVO_REQ(static_cast<long long>(c.N) * blocks_of(c.ht, c.wd) < (1ll << 31));
  if (!workspace || workspace_bytes_given < workspace_bytes(c.N, c.ht, c.wd)) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  *go = true;
  return PVO_OK;
}

extern "C" int pvo_tsdf_track(const pvo_tsdf_track_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  PVO_REQ(volume_ok(a->nz, a->ny, a->nx));
  const Common c = {a->poses, a->disps, a->intrinsics, a->ix, a->weight, a->N, a->nframes, a->ht, a->wd, a->iters, a->min_count,
                    a->band, a->huber, a->lm, a->ep, a->voxel, a->min_weight, a->origin, a->poses_out, a->info, a->system, a->residual, a->jac};
  bool go;
  const int r = track_common(c, workspace, workspace_bytes, &go);
  if (!go) return r;
  hipStream_t s = pvo_stream(stream);
  if (a->nz < 2 || a->ny < 2 || a->nx < 2) {                                     // no cell
    const EmptyVolume none = {nullptr, nullptr, {2, 2, 2}, a->min_weight};
    return launch(none, c, workspace, s);
  }
  PVO_REQ(a->tsdf && a->wsum);
  const DenseVolume vol = {a->tsdf, a->wsum, nullptr, nullptr, {a->nx, a->ny, a->nz}, a->min_weight};
  return launch(vol, c, workspace, s);
}

extern "C" int pvo_tsdf_sparse_track(const pvo_tsdf_sparse_track_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  PVO_REQ(world_ok(a->gz, a->gy, a->gx, a->cap));
  const Common c = {a->poses, a->disps, a->intrinsics, a->ix, a->weight, a->N, a->nframes, a->ht, a->wd, a->iters, a->min_count,
                    a->band, a->huber, a->lm, a->ep, a->voxel, a->min_weight, a->origin, a->poses_out, a->info, a->system, a->residual, a->jac};
  bool go;
  const int r = track_common(c, workspace, workspace_bytes, &go);
  if (!go) return r;
  hipStream_t s = pvo_stream(stream);
  if (a->cap == 0 || static_cast<long long>(a->gz) * a->gy * a->gx == 0) {       // no brick
    const EmptyVolume none = {nullptr, nullptr, {2, 2, 2}, a->min_weight};
    return launch(none, c, workspace, s);
  }
  PVO_REQ(a->tsdf && a->wsum && a->grid);
  const BrickVolume vol = {a->tsdf, a->wsum, nullptr, nullptr, {kB * a->gx, kB * a->gy, kB * a->gz}, a->min_weight,
                           a->grid, a->gy, a->gx, a->cap, {-1, -1, -1}, -1};
  return launch(vol, c, workspace, s);
}
