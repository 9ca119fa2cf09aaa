// tsdf.hip — dense surface reconstruction: keyframe depth maps fused into a truncated signed distance volume, and a triangle mesh
// extracted from it by naive surface nets.  Contracts: include/pvo_hip.h (pvo_tsdf_integrate, pvo_tsdf_mesh); yardstick:
// tests/tsdf_reference.py.
//
//   integrate  (a) tsdf_frames_kernel                 (tsdf_dense_walk.h) one thread per slot of ix, the first set empty: sixteen floats per
//                                                     slot in the workspace
//              (b) tsdf_integrate_kernel<DenseWalk>   (tsdf_fuse.h) one thread per voxel, x fastest, the frame loop inside
//   mesh       classify / scan / vertices / faces of tsdf_mesh.h over DenseCells: one thread per cell, 256 per workgroup
//
// No atomics anywhere: every output index is a function of the classification bits alone, and a voxel's running average is one
// thread's sequential loop - the same operands give the same bytes.  Every __global__ function launched here is a template of those
// headers, which the brick volume (tsdf_sparse.hip) instantiates with its own walker and addresser.
//
// Panoptic (pvo_tsdf_integrate_panoptic, pvo_tsdf_mesh_panoptic): the same launches with the LAB instantiations of (b) and of the
// vertex kernel - the label vote inside the voxel's frame loop, the vertex's label beside its position.
#include "tsdf_mesh.h"
#include "tsdf_dense_walk.h"

using namespace tsdf_volume;

namespace {

inline MeshLayout dense_mesh_layout(int nz, int ny, int nx, long long& cells, long long& blocks) {
  cells = static_cast<long long>(nz - 1) * (ny - 1) * (nx - 1);
  blocks = (cells + DenseCells::kThreads - 1) / DenseCells::kThreads;
  return mesh_layout(static_cast<size_t>(blocks), static_cast<size_t>(cells));
}

}  // namespace

extern "C" size_t pvo_tsdf_integrate_args_size(void) { return sizeof(pvo_tsdf_integrate_args); }
extern "C" size_t pvo_tsdf_mesh_args_size(void) { return sizeof(pvo_tsdf_mesh_args); }
extern "C" size_t pvo_tsdf_panoptic_args_size(void) { return sizeof(pvo_tsdf_panoptic_args); }
extern "C" size_t pvo_tsdf_mesh_labels_args_size(void) { return sizeof(pvo_tsdf_mesh_labels_args); }

extern "C" size_t pvo_tsdf_integrate_workspace_bytes(int N) { return table_bytes(N); }

extern "C" size_t pvo_tsdf_mesh_workspace_bytes(int nz, int ny, int nx) {
  if (nz < 2 || ny < 2 || nx < 2 || !volume_ok(nz, ny, nx)) return 0;
  long long cells, blocks;
  return dense_mesh_layout(nz, ny, nx, cells, blocks).total;
}

namespace {

// pvo_tsdf_integrate (p == NULL) and pvo_tsdf_integrate_panoptic: one validation, one launch sequence
int integrate_impl(const pvo_tsdf_integrate_args* a, const pvo_tsdf_panoptic_args* p, bool panoptic, void* workspace, size_t workspace_bytes,
                   void* stream) {
  PVO_REQ(a);
  if (panoptic) PVO_REQ(panoptic_ok(p, a));
  PVO_REQ(volume_ok(a->nz, a->ny, a->nx));
  PVO_REQ(fuse_scalars_ok(a));
  const long long total = static_cast<long long>(a->nz) * a->ny * a->nx;
  if (total == 0 || a->N == 0 || a->ht * a->wd == 0) return PVO_OK;       // nothing to fuse
  PVO_REQ(a->tsdf && a->wsum && a->poses && a->disps && a->intrinsics && a->ix);
  PVO_REQ(images_ok(a));
  if (!workspace || workspace_bytes < table_bytes(a->N)) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  hipStream_t s = pvo_stream(stream);
  float* fc = static_cast<float*>(workspace);
  const Vol vol = {a->origin[0], a->origin[1], a->origin[2], a->voxel};
  hipLaunchKernelGGL(tsdf_frames_kernel, dim3((a->N + 63) / 64), dim3(64), 0, s, FrameSet{nullptr, nullptr, 0},
                     FrameSet{a->poses, a->ix, a->N}, fc, a->nframes, vol);
  PVO_CHECK_LAUNCH();
  const Fuse in = fuse_operands(a, a->disps, a->weight);
  const DenseWalk w = {a->nz, a->ny, a->nx};
  const dim3 grid(static_cast<unsigned>((total + DenseWalk::kThreads - 1) / DenseWalk::kThreads));
  pick_rgb_lab(a->rgb != nullptr, panoptic, [&](auto RGB, auto LAB) {
    hipLaunchKernelGGL((tsdf_integrate_kernel<DenseWalk, decltype(RGB)::value, decltype(LAB)::value>), grid, dim3(DenseWalk::kThreads), 0, s, w, a->tsdf, a->wsum,
                       a->rgb, fc, a->intrinsics, in, a->N, vote_volumes<decltype(LAB)::value>(p));
  });
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

}  // namespace

extern "C" int pvo_tsdf_integrate(const pvo_tsdf_integrate_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  return integrate_impl(a, nullptr, false, workspace, workspace_bytes, stream);
}

extern "C" int pvo_tsdf_integrate_panoptic(const pvo_tsdf_integrate_args* a, const pvo_tsdf_panoptic_args* p, void* workspace,
                                           size_t workspace_bytes, void* stream) {
  return integrate_impl(a, p, true, workspace, workspace_bytes, stream);
}

namespace {

// pvo_tsdf_mesh (p == NULL) and pvo_tsdf_mesh_panoptic
int mesh_impl(const pvo_tsdf_mesh_args* a, const pvo_tsdf_mesh_labels_args* p, bool panoptic, void* workspace, size_t workspace_bytes,
              void* stream) {
  PVO_REQ(a);
  if (panoptic) PVO_REQ(mesh_labels_ok(p, a));
  PVO_REQ(volume_ok(a->nz, a->ny, a->nx));
  PVO_REQ(mesh_scalars_ok(a));
  hipStream_t s = pvo_stream(stream);
  if (a->nz < 2 || a->ny < 2 || a->nx < 2) return mesh_no_cell(a->counts, s);
  PVO_REQ(a->tsdf && a->wsum);
  PVO_REQ(mesh_outputs_ok(a));
  long long cells, blocks;
  const MeshLayout L = dense_mesh_layout(a->nz, a->ny, a->nx, cells, blocks);
  if (!workspace || workspace_bytes < L.total) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 7));
  const DenseCells g = {{a->tsdf, a->wsum, a->rgb, a->origin[0], a->origin[1], a->origin[2], a->voxel, a->min_weight}, a->nz, a->ny, a->nx, cells};
  const MeshOut out = {a->verts, a->normals, a->rgba, a->faces, a->vcap, a->fcap};
  return mesh_launch(g, static_cast<int>(blocks), L, workspace, out, a->counts, panoptic ? p : nullptr, s);
}

}  // namespace

extern "C" int pvo_tsdf_mesh(const pvo_tsdf_mesh_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  return mesh_impl(a, nullptr, false, workspace, workspace_bytes, stream);
}

extern "C" int pvo_tsdf_mesh_panoptic(const pvo_tsdf_mesh_args* a, const pvo_tsdf_mesh_labels_args* p, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return mesh_impl(a, p, true, workspace, workspace_bytes, stream);
}
