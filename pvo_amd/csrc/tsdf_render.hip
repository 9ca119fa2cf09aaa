// tsdf_render.hip — the fused volume seen from a camera: per view and pixel the depth, normal, colour and segment id of the first
// zero crossing of the TSDF along the pixel's ray.  Contracts: include/pvo_hip.h (pvo_tsdf_render, pvo_tsdf_sparse_render); yardstick:
// tests/tsdf_render_reference.py.
//
//   (a) render_views_kernel    one thread per slot of ix: M = R^T / voxel, p0 = (-R^T t - origin) / voxel and the view id, -1 for an
//                              id outside [0, nviews): sixteen floats per slot in the workspace
//   (b) render_pixels_kernel   one thread per pixel, a 64-lane wave on an 8 x 8 tile of the image (neighbouring rays walk neighbouring
//                              cells, so a wave's gathers fall into few cache lines); the walk itself is ray_pixel of tsdf_ray.h,
//                              instantiated for the dense volume and for the brick volume, which differ only in where a cell's
//                              corners are stored and in the jump over bricks that do not exist
//
// No atomics, no allocation, no host synchronisation; every pixel of every slot is written by exactly one thread.
#include "tsdf_volume.h"

namespace {

using namespace tsdf_volume;         // aligned, finite_f, volume_ok, world_ok, kB

constexpr int kBlock = 256;           // four waves side by side: 32 x 8 pixels
constexpr int kTile = 8;

__global__ __launch_bounds__(64) void render_views_kernel(const float* __restrict__ poses, const int64_t* __restrict__ ix,
                                                          float* __restrict__ vc, int N, int nviews, const Vol vol) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= N) return;
  float* o = vc + static_cast<long long>(kViewFloats) * b;
  const long long f = ix[b];
  if (f < 0 || f >= nviews) {             // never dereferenced
    o[12] = __int_as_float(-1);
    return;
  }
  ray_view_constants(poses, f, vol, o);
}

struct Views { const float* vc; const float* intrinsics; int N, ht, wd, klo, khi; float dz; };

template <class V>
__global__ __launch_bounds__(kBlock) void render_pixels_kernel(V vol, const Views in, const RenderOut out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ui = (blockIdx.x * (kBlock / 64) + wave) * kTile + (lane & 7), vi = blockIdx.y * kTile + (lane >> 3);
  if (ui >= in.wd || vi >= in.ht) return;
  const Intr K = load_intr(in.intrinsics);
  const long long HW = static_cast<long long>(in.ht) * in.wd;
  for (int b = blockIdx.z; b < in.N; b += gridDim.z) {
    const float* __restrict__ c = in.vc + static_cast<long long>(kViewFloats) * b;        // wave-uniform
    const bool live = __float_as_int(c[12]) >= 0;
    Ray r = {{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    if (live) r = ray_of_pixel(c, K, ui, vi);
    ray_pixel(vol, r, live, in.dz, in.klo, in.khi, out, b * HW + static_cast<long long>(vi) * in.wd + ui);
  }
}

// what the two calls share behind their volume: the views, the marching range and the outputs
struct Common {
  const float* poses; const float* intrinsics; const int64_t* ix;
  int N, nviews, ht, wd;
  float z_near, z_far, dz, voxel, min_weight;
  const float* origin;
  const void* label_volume;
  float* depth; float* normal; uint8_t* rgba; int32_t* label; int32_t* visited;
};

inline bool march_ok(const Common& c) {
  return c.N >= 0 && c.nviews >= 0 && c.ht >= 0 && c.wd >= 0 && static_cast<long long>(c.ht) * c.wd < (1ll << 31) &&
         c.voxel > 0.0f && finite_f(c.voxel) && c.min_weight == c.min_weight &&
         finite_f(c.origin[0]) && finite_f(c.origin[1]) && finite_f(c.origin[2]) &&
         finite_f(c.z_near) && finite_f(c.z_far) && finite_f(c.dz) && c.dz > 0.0f && c.z_near >= 0.0f && c.z_far > c.z_near &&
         (c.z_far - c.z_near) / c.dz <= 65536.0f && c.z_far / c.dz < 4194304.0f &&
         !(reinterpret_cast<uintptr_t>(c.rgba) & 3) && (!c.label || c.label_volume);
}

// every output of every slot as a miss: all four are zero bytes
int fill_misses(const Common& c, hipStream_t s) {
  const size_t px = static_cast<size_t>(c.N) * c.ht * c.wd;
  hipError_t e = hipMemsetAsync(c.depth, 0, 4 * px, s);
  if (e == hipSuccess && c.normal) e = hipMemsetAsync(c.normal, 0, 12 * px, s);
  if (e == hipSuccess && c.rgba) e = hipMemsetAsync(c.rgba, 0, 4 * px, s);
  if (e == hipSuccess && c.label) e = hipMemsetAsync(c.label, 0, 4 * px, s);
  if (e == hipSuccess && c.visited) e = hipMemsetAsync(c.visited, 0, 8 * px, s);
  if (e != hipSuccess) { pvo_note_hip_error(static_cast<int>(e)); return PVO_ELAUNCH; }
  return PVO_OK;
}

template <class V>
int launch(const V& vol, const Common& c, void* workspace, hipStream_t s) {
  float* vc = static_cast<float*>(workspace);
  const Vol o = {c.origin[0], c.origin[1], c.origin[2], c.voxel};
  hipLaunchKernelGGL(render_views_kernel, dim3((c.N + 63) / 64), dim3(64), 0, s, c.poses, c.ix, vc, c.N, c.nviews, o);
  PVO_CHECK_LAUNCH();
  const Views in = {vc, c.intrinsics, c.N, c.ht, c.wd, static_cast<int>(ceilf(c.z_near / c.dz)), static_cast<int>(floorf(c.z_far / c.dz)), c.dz};
  const RenderOut out = {c.depth, c.normal, c.rgba, c.label, c.visited};
  const int across = kTile * (kBlock / 64);
  const dim3 grid((c.wd + across - 1) / across, (c.ht + kTile - 1) / kTile, c.N < 65535 ? c.N : 65535);
  if (grid.y > 65535u) return PVO_EINVAL;               // (ht > 524280: no image)
  hipLaunchKernelGGL(render_pixels_kernel<V>, grid, dim3(kBlock), 0, s, vol, in, out);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

}  // namespace

extern "C" size_t pvo_tsdf_render_args_size(void) { return sizeof(pvo_tsdf_render_args); }
extern "C" size_t pvo_tsdf_sparse_render_args_size(void) { return sizeof(pvo_tsdf_sparse_render_args); }

extern "C" size_t pvo_tsdf_render_workspace_bytes(int N) {
  return N <= 0 ? 0 : aligned(sizeof(float) * kViewFloats * static_cast<size_t>(N));
}
extern "C" size_t pvo_tsdf_sparse_render_workspace_bytes(int N) { return pvo_tsdf_render_workspace_bytes(N); }

extern "C" int pvo_tsdf_render(const pvo_tsdf_render_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  PVO_REQ(volume_ok(a->nz, a->ny, a->nx));
  const Common c = {a->poses, a->intrinsics, a->ix, a->N, a->nviews, a->ht, a->wd, a->z_near, a->z_far, a->dz, a->voxel, a->min_weight,
                    a->origin, a->label, a->depth, a->normal, a->rgba, a->out_label, a->visited};
  PVO_REQ(march_ok(c));
  if (a->N == 0 || a->ht * a->wd == 0) return PVO_OK;                     // no pixel
  PVO_REQ(a->depth);
  hipStream_t s = pvo_stream(stream);
  if (a->nz < 2 || a->ny < 2 || a->nx < 2) return fill_misses(c, s);      // no cell
  PVO_REQ(a->poses && a->intrinsics && a->ix && a->tsdf && a->wsum);
  if (!workspace || workspace_bytes < pvo_tsdf_render_workspace_bytes(a->N)) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  const DenseVolume vol = {a->tsdf, a->wsum, a->rgb, a->label, {a->nx, a->ny, a->nz}, a->min_weight};
  return launch(vol, c, workspace, s);
}

extern "C" int pvo_tsdf_sparse_render(const pvo_tsdf_sparse_render_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  PVO_REQ(world_ok(a->gz, a->gy, a->gx, a->cap));
  const Common c = {a->poses, a->intrinsics, a->ix, a->N, a->nviews, a->ht, a->wd, a->z_near, a->z_far, a->dz, a->voxel, a->min_weight,
                    a->origin, a->label, a->depth, a->normal, a->rgba, a->out_label, a->visited};
  PVO_REQ(march_ok(c));
  if (a->N == 0 || a->ht * a->wd == 0) return PVO_OK;                     // no pixel
  PVO_REQ(a->depth);
  hipStream_t s = pvo_stream(stream);
  if (a->cap == 0 || static_cast<long long>(a->gz) * a->gy * a->gx == 0) return fill_misses(c, s);      // no brick
  PVO_REQ(a->poses && a->intrinsics && a->ix && a->tsdf && a->wsum && a->grid);
  if (!workspace || workspace_bytes < pvo_tsdf_sparse_render_workspace_bytes(a->N)) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  const BrickVolume vol = {a->tsdf, a->wsum, a->rgb, a->label, {kB * a->gx, kB * a->gy, kB * a->gz}, a->min_weight,
                           a->grid, a->gy, a->gx, a->cap, {-1, -1, -1}, -1};
  return launch(vol, c, workspace, s);
}
