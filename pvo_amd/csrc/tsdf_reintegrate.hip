// tsdf_reintegrate.hip — a live volume: keyframes whose pose or depth moved are taken out of the running average as they were fused and
// put back as they are now, in ONE pass over the volume (BundleFusion's re-integration).  Contracts: include/pvo_hip.h
// (pvo_tsdf_reintegrate, pvo_tsdf_sparse_reintegrate); yardstick: tests/tsdf_reintegrate_reference.py.
//
//   dense   (a) reintegrate_frames_kernel   one thread per slot of BOTH sets: the slot constants of tsdf.hip (tsdf_frame_constants), the
//                                           REMOVE table from poses_old / ix_old in front of the ADD table from poses / ix
//           (b) tsdf_reintegrate_kernel     one thread per voxel, x fastest: the REMOVE slots in order (tsdf_unfuse_frame), then the ADD
//                                           slots in order (tsdf_fuse_frame); the volume is read and written once whatever N_old + N is
//   bricks  (a) sparse_frames_kernel        (tsdf_brick_cull.h, the brick integration's) once per set that has slots: constants, zfar
//           (b) sparse_reintegrate_kernel   one workgroup per brick: per set, chunks of 512 slots culled by brick_sees_frame against THAT
//                                           set's constants and zfar, survivors compacted in slot order, then the dense kernel's functions
//
// No atomics: a voxel is one thread's sequential loop, so the same operands give the same bytes.  The slot constants are wave-uniform
// loads and a wave without a hit branches over the gathers, as in tsdf_integrate_kernel.
#include "tsdf_brick_cull.h"
#include "tsdf_volume.h"

namespace {

constexpr int kB = PVO_TSDF_BRICK;
constexpr int kBrick = kB * kB * kB;
constexpr int kBlock = 256;
static_assert(kB == 8 && kBrick == 512, "the index arithmetic below shifts by 3 and 6");

struct FrameSet { const float* poses; const int64_t* ix; int N; };

// slots [0, old.N): the REMOVE set, slots [old.N, old.N + add.N): the ADD set
__global__ __launch_bounds__(64) void reintegrate_frames_kernel(const FrameSet old, const FrameSet add, float* __restrict__ fc, int nframes,
                                                                const Vol vol) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= old.N + add.N) return;
  const bool first = b < old.N;
  const float* __restrict__ poses = first ? old.poses : add.poses;
  const long long f = first ? old.ix[b] : add.ix[b - old.N];
  float* o = fc + static_cast<long long>(kFrameFloats) * b;
  if (f < 0 || f >= nframes) {            // never dereferenced
    o[12] = __int_as_float(-1);
    return;
  }
  tsdf_frame_constants(poses, f, vol, o);
}

template <bool RGB>
__global__ __launch_bounds__(kBlock) void tsdf_reintegrate_kernel(float* __restrict__ tsdf, float* __restrict__ wsum, float* __restrict__ rgb,
                                                                 const float* __restrict__ fc, const float* __restrict__ intrinsics,
                                                                 const Fuse in_old, const Fuse in, int N_old, int N, int nz, int ny, int nx,
                                                                 float w_floor) {
  const long long total = static_cast<long long>(nz) * ny * nx;
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  const bool live = i < total;
  const int x = static_cast<int>(i % nx), y = static_cast<int>((i / nx) % ny), z = static_cast<int>(i / (static_cast<long long>(nx) * ny));
  const float xf = static_cast<float>(x), yf = static_cast<float>(y), zf = static_cast<float>(z);
  const Intr K = load_intr(intrinsics);
  const long long HW = static_cast<long long>(in.ht) * in.wd;
  const long long plane = static_cast<long long>(in.IH) * in.IW;
  Voxel a = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, false, 0, 0.0f};
  if (live) {
    a.T = tsdf[i]; a.W = wsum[i];
    if (RGB) { a.cr = rgb[3 * i]; a.cg = rgb[3 * i + 1]; a.cb = rgb[3 * i + 2]; }
  }
  for (int b = 0; b < N_old; ++b) {
    const float* __restrict__ c = fc + static_cast<long long>(kFrameFloats) * b;      // wave-uniform
    const int f = __float_as_int(c[12]);
    if (f < 0) continue;
    tsdf_unfuse_frame<RGB>(a, c, f, xf, yf, zf, live, K, in_old, HW, plane, w_floor);
  }
  for (int b = N_old; b < N_old + N; ++b) {
    const float* __restrict__ c = fc + static_cast<long long>(kFrameFloats) * b;      // wave-uniform
    const int f = __float_as_int(c[12]);
    if (f < 0) continue;
    tsdf_fuse_frame<RGB>(a, c, f, xf, yf, zf, live, K, in, HW, plane);
  }
  if (a.touched) {                        // (only a live voxel can be)
    tsdf[i] = a.T; wsum[i] = a.W;
    if (RGB) { rgb[3 * i] = a.cr; rgb[3 * i + 1] = a.cg; rgb[3 * i + 2] = a.cb; }
  }
}

// the slots [0, N) of the table fc against the brick, 512 at a time; the survivors, in slot order, applied to the voxel by `apply`
template <typename Apply>
__device__ __forceinline__ int brick_cull_and_apply(const float* __restrict__ fc, int N, float ccx, float ccy, float ccz, float msum,
                                                    float voxel, const Intr K, const Fuse in, int* list, int* wave_n, Apply apply) {
  const int tid = threadIdx.x;
  int survivors = 0;
  for (int c0 = 0; c0 < N; c0 += kBrick) {
    const int b = c0 + tid;
    const bool keep = b < N && brick_sees_frame(fc + static_cast<long long>(kFrameFloats) * b, ccx, ccy, ccz, msum, voxel, K, in);
    const unsigned long long m = __ballot(keep);
    if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(m);
    __syncthreads();
    int pos = lanes_below(m), n = 0;
#pragma unroll
    for (int w = 0; w < kBrick / 64; ++w) {
      if (w < (tid >> 6)) pos += wave_n[w];
      n += wave_n[w];
    }
    if (keep) list[pos] = b;
    survivors += n;
    __syncthreads();
    for (int k = 0; k < n; ++k) {
      const int s = __builtin_amdgcn_readfirstlane(list[k]);
      const float* __restrict__ c = fc + static_cast<long long>(kFrameFloats) * s;    // wave-uniform
      apply(c, __float_as_int(c[12]));
    }
    __syncthreads();                      // list and wave_n are rewritten by the next chunk
  }
  return survivors;
}

template <bool RGB>
__global__ __launch_bounds__(kBrick) void sparse_reintegrate_kernel(float* __restrict__ tsdf, float* __restrict__ wsum, float* __restrict__ rgb,
                                                                   const int32_t* __restrict__ coord, const int32_t* __restrict__ bricks,
                                                                   int cap, const float* __restrict__ fc_old, const float* __restrict__ fc,
                                                                   const float* __restrict__ intrinsics, const Fuse in_old, const Fuse in,
                                                                   int N_old, int N, float voxel, float w_floor, int32_t* __restrict__ kept) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  if (slot >= min(bricks[0], cap)) return;              // (the whole workgroup)
  const int bz = coord[3 * slot], by = coord[3 * slot + 1], bx = coord[3 * slot + 2];
  const int x = kB * bx + (tid & 7), y = kB * by + ((tid >> 3) & 7), z = kB * bz + (tid >> 6);
  const float xf = static_cast<float>(x), yf = static_cast<float>(y), zf = static_cast<float>(z);
  const float ccx = static_cast<float>(kB * bx) + 3.5f, ccy = static_cast<float>(kB * by) + 3.5f, ccz = static_cast<float>(kB * bz) + 3.5f;
  const float msum = voxel * static_cast<float>(kB * (bx + by + bz) + 21);
  const Intr K = load_intr(intrinsics);
  const long long HW = static_cast<long long>(in.ht) * in.wd;
  const long long plane = static_cast<long long>(in.IH) * in.IW;
  const long long i = static_cast<long long>(slot) * kBrick + tid;
  Voxel a = {tsdf[i], wsum[i], 0.0f, 0.0f, 0.0f, false, 0, 0.0f};
  if (RGB) { a.cr = rgb[3 * i]; a.cg = rgb[3 * i + 1]; a.cb = rgb[3 * i + 2]; }
  __shared__ int list[kBrick];
  __shared__ int wave_n[kBrick / 64];
  int survivors = brick_cull_and_apply(fc_old, N_old, ccx, ccy, ccz, msum, voxel, K, in_old, list, wave_n, [&](const float* c, int f) {
    tsdf_unfuse_frame<RGB>(a, c, f, xf, yf, zf, true, K, in_old, HW, plane, w_floor);
  });
  survivors += brick_cull_and_apply(fc, N, ccx, ccy, ccz, msum, voxel, K, in, list, wave_n, [&](const float* c, int f) {
    tsdf_fuse_frame<RGB>(a, c, f, xf, yf, zf, true, K, in, HW, plane);
  });
  if (kept && tid == 0) kept[slot] = survivors;
  if (a.touched) {
    tsdf[i] = a.T; wsum[i] = a.W;
    if (RGB) { rgb[3 * i] = a.cr; rgb[3 * i + 1] = a.cg; rgb[3 * i + 2] = a.cb; }
  }
}

using tsdf_volume::aligned;
using tsdf_volume::finite_f;

inline size_t table_bytes(int N) { return N <= 0 ? 0 : aligned(sizeof(float) * kFrameFloats * static_cast<size_t>(N)); }

// what the two calls share: the scalars, the two frame sets, the colour arguments.  PVO_OK = in order
template <typename Args>
int check_common(const Args* a) {
  if (!(a->N >= 0 && a->N_old >= 0 && a->nframes >= 0 && a->ht >= 0 && a->wd >= 0 && static_cast<long long>(a->ht) * a->wd < (1ll << 31)))
    return PVO_EINVAL;
  if (static_cast<long long>(a->N) + a->N_old >= (1ll << 31)) return PVO_EINVAL;
  if (!(a->voxel > 0.0f && finite_f(a->voxel) && a->trunc > 0.0f && finite_f(a->trunc))) return PVO_EINVAL;
  if (!(a->z_near >= 0.0f && finite_f(a->z_near) && a->w_max >= 0.0f && finite_f(a->w_max))) return PVO_EINVAL;
  if (!(a->w_floor >= 0.0f && finite_f(a->w_floor))) return PVO_EINVAL;
  if (!(finite_f(a->origin[0]) && finite_f(a->origin[1]) && finite_f(a->origin[2]))) return PVO_EINVAL;
  return PVO_OK;
}

template <typename Args>
int check_operands(const Args* a) {
  if (!(a->tsdf && a->wsum && a->intrinsics)) return PVO_EINVAL;
  if (a->N_old > 0 && !(a->poses_old && a->disps_old && a->ix_old)) return PVO_EINVAL;
  if (a->N > 0 && !(a->poses && a->disps && a->ix)) return PVO_EINVAL;
  if (a->rgb && !a->images) return PVO_EINVAL;           // a colour volume needs the images
  if (a->images) {
    if (!(a->img_stride >= 1 && a->img_offset >= 0 && a->IH > 0 && a->IW > 0)) return PVO_EINVAL;
    if (!(static_cast<long long>(a->img_stride) * (a->ht - 1) + a->img_offset < a->IH)) return PVO_EINVAL;
    if (!(static_cast<long long>(a->img_stride) * (a->wd - 1) + a->img_offset < a->IW)) return PVO_EINVAL;
  }
  return PVO_OK;
}

template <typename Args>
void fuse_operands(const Args* a, Fuse& in_old, Fuse& in) {
  in_old = {a->disps_old, a->weight_old, a->images, a->ht, a->wd, a->IH, a->IW, a->img_stride, a->img_offset, a->trunc, a->z_near, a->w_max};
  in = {a->disps, a->weight, a->images, a->ht, a->wd, a->IH, a->IW, a->img_stride, a->img_offset, a->trunc, a->z_near, a->w_max};
}

}  // namespace

#define PVO_REQ(c) do { if (!(c)) return PVO_EINVAL; } while (0)

extern "C" size_t pvo_tsdf_reintegrate_args_size(void) { return sizeof(pvo_tsdf_reintegrate_args); }
extern "C" size_t pvo_tsdf_sparse_reintegrate_args_size(void) { return sizeof(pvo_tsdf_sparse_reintegrate_args); }

extern "C" size_t pvo_tsdf_reintegrate_workspace_bytes(int N_old, int N) {
  const long long n = static_cast<long long>(N_old > 0 ? N_old : 0) + (N > 0 ? N : 0);
  return n <= 0 || n >= (1ll << 31) ? 0 : aligned(sizeof(float) * kFrameFloats * static_cast<size_t>(n));
}

extern "C" size_t pvo_tsdf_sparse_reintegrate_workspace_bytes(int N_old, int N) { return table_bytes(N_old) + table_bytes(N); }

extern "C" int pvo_tsdf_reintegrate(const pvo_tsdf_reintegrate_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  PVO_REQ(tsdf_volume::volume_ok(a->nz, a->ny, a->nx));
  if (const int e = check_common(a)) return e;
  const long long total = static_cast<long long>(a->nz) * a->ny * a->nx;
  if (total == 0 || a->N_old + a->N == 0 || a->ht * a->wd == 0) return PVO_OK;      // nothing to do
  if (const int e = check_operands(a)) return e;
  if (!workspace || workspace_bytes < pvo_tsdf_reintegrate_workspace_bytes(a->N_old, a->N)) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  hipStream_t s = pvo_stream(stream);
  float* fc = static_cast<float*>(workspace);
  const Vol vol = {a->origin[0], a->origin[1], a->origin[2], a->voxel};
  const FrameSet old = {a->poses_old, a->ix_old, a->N_old}, add = {a->poses, a->ix, a->N};
  hipLaunchKernelGGL(reintegrate_frames_kernel, dim3((a->N_old + a->N + 63) / 64), dim3(64), 0, s, old, add, fc, a->nframes, vol);
  PVO_CHECK_LAUNCH();
  Fuse in_old, in;
  fuse_operands(a, in_old, in);
  const dim3 grid(static_cast<unsigned>((total + kBlock - 1) / kBlock));
  if (a->rgb)
    hipLaunchKernelGGL(tsdf_reintegrate_kernel<true>, grid, dim3(kBlock), 0, s, a->tsdf, a->wsum, a->rgb, fc, a->intrinsics, in_old, in,
                       a->N_old, a->N, a->nz, a->ny, a->nx, a->w_floor);
  else
    hipLaunchKernelGGL(tsdf_reintegrate_kernel<false>, grid, dim3(kBlock), 0, s, a->tsdf, a->wsum, a->rgb, fc, a->intrinsics, in_old, in,
                       a->N_old, a->N, a->nz, a->ny, a->nx, a->w_floor);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

extern "C" int pvo_tsdf_sparse_reintegrate(const pvo_tsdf_sparse_reintegrate_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  PVO_REQ(tsdf_volume::world_ok(a->gz, a->gy, a->gx, a->cap));
  if (const int e = check_common(a)) return e;
  if (a->cap == 0 || a->N_old + a->N == 0 || a->ht * a->wd == 0) return PVO_OK;     // nothing to do
  PVO_REQ(a->coord && a->bricks);
  if (const int e = check_operands(a)) return e;
  if (!workspace || workspace_bytes < pvo_tsdf_sparse_reintegrate_workspace_bytes(a->N_old, a->N)) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  hipStream_t s = pvo_stream(stream);
  float* fc_old = static_cast<float*>(workspace);
  float* fc = reinterpret_cast<float*>(static_cast<char*>(workspace) + table_bytes(a->N_old));
  const Vol vol = {a->origin[0], a->origin[1], a->origin[2], a->voxel};
  const long long HW = static_cast<long long>(a->ht) * a->wd;
  if (a->N_old > 0) {
    hipLaunchKernelGGL(sparse_frames_kernel, dim3(a->N_old), dim3(kCullBlock), 0, s, a->poses_old, a->ix_old, a->disps_old, a->weight_old,
                       fc_old, a->nframes, HW, vol);
    PVO_CHECK_LAUNCH();
  }
  if (a->N > 0) {
    hipLaunchKernelGGL(sparse_frames_kernel, dim3(a->N), dim3(kCullBlock), 0, s, a->poses, a->ix, a->disps, a->weight, fc, a->nframes, HW, vol);
    PVO_CHECK_LAUNCH();
  }
  Fuse in_old, in;
  fuse_operands(a, in_old, in);
  if (a->rgb)
    hipLaunchKernelGGL(sparse_reintegrate_kernel<true>, dim3(a->cap), dim3(kBrick), 0, s, a->tsdf, a->wsum, a->rgb, a->coord, a->bricks, a->cap,
                       fc_old, fc, a->intrinsics, in_old, in, a->N_old, a->N, a->voxel, a->w_floor, a->kept);
  else
    hipLaunchKernelGGL(sparse_reintegrate_kernel<false>, dim3(a->cap), dim3(kBrick), 0, s, a->tsdf, a->wsum, a->rgb, a->coord, a->bricks, a->cap,
                       fc_old, fc, a->intrinsics, in_old, in, a->N_old, a->N, a->voxel, a->w_floor, a->kept);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}
