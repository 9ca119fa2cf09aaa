// tsdf_reintegrate.hip — a live volume: keyframes whose pose or depth moved are taken out of the running average as they were fused and
// put back as they are now, in ONE pass over the volume (BundleFusion's re-integration).  Contracts: include/pvo_hip.h
// (pvo_tsdf_reintegrate, pvo_tsdf_sparse_reintegrate); yardstick: tests/tsdf_reintegrate_reference.py.
//
//   dense   (a) tsdf_frames_kernel                   (tsdf_dense_walk.h) one thread per slot of BOTH sets: the REMOVE table from poses_old /
//                                                    ix_old in front of the ADD table from poses / ix
//           (b) tsdf_reintegrate_kernel<DenseWalk>   (tsdf_fuse.h) one thread per voxel, x fastest: the REMOVE slots in order
//                                                    (tsdf_unfuse_frame), then the ADD slots in order (tsdf_fuse_frame); the volume is
//                                                    read and written once whatever N_old + N is
//   bricks  (a) sparse_frames_kernel                 (tsdf_brick_cull.h, the brick integration's) once per set that has slots
//           (b) tsdf_reintegrate_kernel<BrickWalk>   one workgroup per brick: per set, chunks of 512 slots culled by brick_sees_frame
//                                                    against THAT set's constants and zfar, survivors compacted in slot order, then
//                                                    the dense walk's functions
//
// No atomics: a voxel is one thread's sequential loop, so the same operands give the same bytes.  Every __global__ function launched
// here is a template of those headers, instantiated with the walker of the volume.
#include "tsdf_brick_cull.h"
#include "tsdf_dense_walk.h"

using namespace tsdf_volume;

namespace {

// what the two calls state beyond a fusion's scalars: the REMOVE set's size and the weight floor
template <typename Args>
bool reintegrate_scalars_ok(const Args* a) {
  return fuse_scalars_ok(a) && a->N_old >= 0 && static_cast<long long>(a->N) + a->N_old < (1ll << 31) && a->w_floor >= 0.0f &&
         finite_f(a->w_floor);
}

template <typename Args>
bool reintegrate_operands_ok(const Args* a) {
  return a->tsdf && a->wsum && a->intrinsics && (a->N_old <= 0 || (a->poses_old && a->disps_old && a->ix_old)) &&
         (a->N <= 0 || (a->poses && a->disps && a->ix)) && images_ok(a);
}

}  // namespace

extern "C" size_t pvo_tsdf_reintegrate_args_size(void) { return sizeof(pvo_tsdf_reintegrate_args); }
extern "C" size_t pvo_tsdf_sparse_reintegrate_args_size(void) { return sizeof(pvo_tsdf_sparse_reintegrate_args); }

extern "C" size_t pvo_tsdf_reintegrate_workspace_bytes(int N_old, int N) {
  const long long n = static_cast<long long>(N_old > 0 ? N_old : 0) + (N > 0 ? N : 0);
  return n >= (1ll << 31) ? 0 : table_bytes(n);
}

extern "C" size_t pvo_tsdf_sparse_reintegrate_workspace_bytes(int N_old, int N) { return table_bytes(N_old) + table_bytes(N); }

extern "C" int pvo_tsdf_reintegrate(const pvo_tsdf_reintegrate_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  PVO_REQ(volume_ok(a->nz, a->ny, a->nx));
  PVO_REQ(reintegrate_scalars_ok(a));
  const long long total = static_cast<long long>(a->nz) * a->ny * a->nx;
  if (total == 0 || a->N_old + a->N == 0 || a->ht * a->wd == 0) return PVO_OK;      // nothing to do
  PVO_REQ(reintegrate_operands_ok(a));
  if (!workspace || workspace_bytes < pvo_tsdf_reintegrate_workspace_bytes(a->N_old, a->N)) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  hipStream_t s = pvo_stream(stream);
  float* fc = static_cast<float*>(workspace);
  const Vol vol = {a->origin[0], a->origin[1], a->origin[2], a->voxel};
  hipLaunchKernelGGL(tsdf_frames_kernel, dim3((a->N_old + a->N + 63) / 64), dim3(64), 0, s, FrameSet{a->poses_old, a->ix_old, a->N_old},
                     FrameSet{a->poses, a->ix, a->N}, fc, a->nframes, vol);
  PVO_CHECK_LAUNCH();
  const Fuse in_old = fuse_operands(a, a->disps_old, a->weight_old), in = fuse_operands(a, a->disps, a->weight);
  const DenseWalk w = {a->nz, a->ny, a->nx};
  const dim3 grid(static_cast<unsigned>((total + DenseWalk::kThreads - 1) / DenseWalk::kThreads));
  pick_rgb_lab(a->rgb != nullptr, false, [&](auto RGB, auto) {
    hipLaunchKernelGGL((tsdf_reintegrate_kernel<DenseWalk, decltype(RGB)::value>), grid, dim3(DenseWalk::kThreads), 0, s, w, a->tsdf, a->wsum,
                       a->rgb, fc, fc + static_cast<long long>(kFrameFloats) * a->N_old, a->intrinsics, in_old, in, a->N_old, a->N, a->w_floor);
  });
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

extern "C" int pvo_tsdf_sparse_reintegrate(const pvo_tsdf_sparse_reintegrate_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  PVO_REQ(world_ok(a->gz, a->gy, a->gx, a->cap));
  PVO_REQ(reintegrate_scalars_ok(a));
  if (a->cap == 0 || a->N_old + a->N == 0 || a->ht * a->wd == 0) return PVO_OK;     // nothing to do
  PVO_REQ(a->coord && a->bricks);
  PVO_REQ(reintegrate_operands_ok(a));
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
  const Fuse in_old = fuse_operands(a, a->disps_old, a->weight_old), in = fuse_operands(a, a->disps, a->weight);
  const BrickWalk w = {a->coord, a->bricks, a->cap, a->voxel, a->kept};
  pick_rgb_lab(a->rgb != nullptr, false, [&](auto RGB, auto) {
    hipLaunchKernelGGL((tsdf_reintegrate_kernel<BrickWalk, decltype(RGB)::value>), dim3(a->cap), dim3(BrickWalk::kThreads), 0, s, w, a->tsdf,
                       a->wsum, a->rgb, fc_old, fc, a->intrinsics, in_old, in, a->N_old, a->N, a->w_floor);
  });
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}
