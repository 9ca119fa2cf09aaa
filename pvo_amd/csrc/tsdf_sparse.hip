// tsdf_sparse.hip — the brick volume: 8 x 8 x 8 blocks of voxels near observed surfaces, reached through a dense indirection grid.
// Contracts: include/pvo_hip.h (pvo_tsdf_sparse_allocate / _integrate / _mesh); yardsticks: the dense kernels of tsdf.hip, with which
// this file shares its arithmetic (tsdf_fuse.h), and tests/tsdf_sparse_reference.py.
//
//   allocate   (a) marks cleared             hipMemsetAsync of one byte per brick of the grid
//              (b) alloc_frames_kernel       one thread per slot of ix: R, t and the frame id
//              (c) alloc_mark_kernel         one thread per (slot, pixel): S samples along the ray, a same-value byte store per brick
//              (d) alloc_count_kernel        per 256 grid entries: bricks held, bricks new (marked and not held)
//              (e) alloc_scan_kernel         one workgroup: the bricks held, exclusive scan of the new ones behind them, bricks[0]
//              (f) alloc_assign_kernel       grid and coord of the new bricks whose slot is below cap
//   integrate  (a) sparse_frames_kernel      (tsdf_brick_cull.h) one workgroup per slot: the dense call's constants, zfar = max 1/d, the
//                                            cull's scalars
//              (b) tsdf_integrate_kernel<BrickWalk>  (tsdf_fuse.h) one workgroup per brick, one thread per voxel: cull per chunk of
//                                            512 slots, survivors compacted in slot order, then the dense walk's per-(voxel, frame) function
//   mesh       classify / scan / vertices / faces of tsdf_mesh.h over BrickCells: one workgroup per brick, neighbours through the grid
//   panoptic   (pvo_tsdf_sparse_integrate_panoptic / _mesh_panoptic) the LAB instantiations of the integrate and the vertex kernel in
//              the same launches, as in tsdf.hip
//
// No atomics anywhere: marks are same-value stores, every index is a function of flags alone, a voxel is one thread's sequential loop.
#include "tsdf_mesh.h"
#include "tsdf_brick_cull.h"

using namespace tsdf_volume;

namespace {

constexpr int kBlock = 256;

// ------------------------------------------------------------------------------------------------------------ allocate

struct World { int gz, gy, gx; float ox, oy, oz, voxel; };

__global__ __launch_bounds__(64) void alloc_frames_kernel(const float* __restrict__ poses, const int64_t* __restrict__ ix,
                                                          float* __restrict__ fc, int N, int nframes) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= N) return;
  float* o = fc + static_cast<long long>(kFrameFloats) * b;
  const long long f = ix[b];
  if (f < 0 || f >= nframes) {            // never dereferenced
    o[12] = __int_as_float(-1);
    return;
  }
  const Pose G = load_pose(poses + 7 * f);
  const Quat q = G.q;
  o[0] = 1.0f - 2.0f * (q.y * q.y + q.z * q.z); o[1] = 2.0f * (q.x * q.y - q.z * q.w); o[2] = 2.0f * (q.x * q.z + q.y * q.w);
  o[3] = 2.0f * (q.x * q.y + q.z * q.w); o[4] = 1.0f - 2.0f * (q.x * q.x + q.z * q.z); o[5] = 2.0f * (q.y * q.z - q.x * q.w);
  o[6] = 2.0f * (q.x * q.z - q.y * q.w); o[7] = 2.0f * (q.y * q.z + q.x * q.w); o[8] = 1.0f - 2.0f * (q.x * q.x + q.y * q.y);
  o[9] = G.t.x; o[10] = G.t.y; o[11] = G.t.z;
  o[12] = __int_as_float(static_cast<int>(f));
}

struct Mark {
  const float* disps; const float* weight;
  int ht, wd, S;
  float trunc, z_near, margin;
};

__global__ __launch_bounds__(kBlock) void alloc_mark_kernel(const float* __restrict__ fc, const float* __restrict__ intrinsics, const Mark in,
                                                           const World g, int N, uint8_t* __restrict__ marks) {
  const long long HW = static_cast<long long>(in.ht) * in.wd;
  const long long k = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
  if (k >= HW) return;
  const int vi = static_cast<int>(k / in.wd), ui = static_cast<int>(k - static_cast<long long>(vi) * in.wd);
  const Intr K = load_intr(intrinsics);
  const float rx = (static_cast<float>(ui) - K.cx) / K.fx, ry = (static_cast<float>(vi) - K.cy) / K.fy;
  const float lim[3] = {static_cast<float>(kB * g.gx), static_cast<float>(kB * g.gy), static_cast<float>(kB * g.gz)};
  const int dim[3] = {g.gx, g.gy, g.gz};
  for (int b = blockIdx.y; b < N; b += gridDim.y) {
    const float* __restrict__ c = fc + static_cast<long long>(kFrameFloats) * b;      // wave-uniform
    const int f = __float_as_int(c[12]);
    if (f < 0) continue;
    const float d = in.disps[f * HW + k];
    const float w = in.weight ? in.weight[f * HW + k] : 1.0f;
    if (!(d > 0.0f && d < __builtin_inff() && w > 0.0f && w < __builtin_inff())) continue;
    const float z = 1.0f / d;
    const float lo = fmaxf(in.z_near, z - in.trunc), hi = z + in.trunc;
    if (!(hi >= lo)) continue;
    for (int s = 0; s < in.S; ++s) {
      const float zk = lo + (hi - lo) * (static_cast<float>(s) / static_cast<float>(in.S - 1));
      const float ax = rx * zk - c[9], ay = ry * zk - c[10], az = zk - c[11];
      // X = R^T (Xc - t), then voxels from the origin
      const float p[3] = {((c[0] * ax + c[3] * ay + c[6] * az) - g.ox) / g.voxel, ((c[1] * ax + c[4] * ay + c[7] * az) - g.oy) / g.voxel,
                          ((c[2] * ax + c[5] * ay + c[8] * az) - g.oz) / g.voxel};
      bool inside = true;
      int blo[3], bhi[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const float h = p[e] + 0.5f;
        inside = inside && h >= 0.0f && h < lim[e];                                  // (NaN fails)
        // floor((c + 0.5) / 8) of the two corner coordinates, -1 where outside the grid; |.| < 2^22 inside the test
        const float l = floorf((h - in.margin) * 0.125f), u = floorf((h + in.margin) * 0.125f);
        blo[e] = (l >= 0.0f && l < static_cast<float>(dim[e])) ? static_cast<int>(l) : -1;
        bhi[e] = (u >= 0.0f && u < static_cast<float>(dim[e])) ? static_cast<int>(u) : -1;
      }
      if (!inside) continue;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int bx = (j & 1) ? bhi[0] : blo[0], by = (j & 2) ? bhi[1] : blo[1], bz = (j & 4) ? bhi[2] : blo[2];
        if (bx < 0 || by < 0 || bz < 0) continue;
        if (((j & 1) && bhi[0] == blo[0]) || ((j & 2) && bhi[1] == blo[1]) || ((j & 4) && bhi[2] == blo[2])) continue;   // stored already
        marks[(static_cast<long long>(bz) * g.gy + by) * g.gx + bx] = 1;
      }
    }
  }
}

__global__ __launch_bounds__(kBlock) void alloc_count_kernel(const int32_t* __restrict__ grid, const uint8_t* __restrict__ marks, long long G,
                                                            int* __restrict__ acount, int* __restrict__ ncount) {
  const int tid = threadIdx.x;
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + tid;
  bool held = false, fresh = false;
  if (i < G) {
    held = grid[i] >= 0;
    fresh = !held && marks[i] != 0;
  }
  const unsigned long long mh = __ballot(held), mf = __ballot(fresh);
  __shared__ int wave_h[kBlock / 64], wave_f[kBlock / 64];
  if ((tid & 63) == 0) { wave_h[tid >> 6] = __popcll(mh); wave_f[tid >> 6] = __popcll(mf); }
  __syncthreads();
  if (tid == 0) {
    acount[blockIdx.x] = (wave_h[0] + wave_h[1]) + (wave_h[2] + wave_h[3]);
    ncount[blockIdx.x] = (wave_f[0] + wave_f[1]) + (wave_f[2] + wave_f[3]);
  }
}

// nbase[i] = bricks held + the new bricks of the workgroups before i (scan.h); bricks[0] = held + new, not clamped by cap
__global__ __launch_bounds__(kScanThreads) void alloc_scan_kernel(const int* __restrict__ acount, const int* __restrict__ ncount,
                                                                  int* __restrict__ nbase, int32_t* __restrict__ bricks, int M) {
  const int* const cnt[2] = {acount, ncount};
  int run[2], total[2];
  const ScanChunk c = scan_counts(cnt, M, run, total);
  int next = total[0] + run[1];           // behind the bricks held
  for (int i = c.lo; i < c.hi; ++i) { nbase[i] = next; next += ncount[i]; }
  if (threadIdx.x == 0) bricks[0] = total[0] + total[1];
}

__global__ __launch_bounds__(kBlock) void alloc_assign_kernel(int32_t* __restrict__ grid, const uint8_t* __restrict__ marks, long long G,
                                                             const int* __restrict__ nbase, int32_t* __restrict__ coord, int cap,
                                                             int gy, int gx) {
  const int tid = threadIdx.x;
  const long long i = static_cast<long long>(blockIdx.x) * kBlock + tid;
  const bool fresh = i < G && grid[i] < 0 && marks[i] != 0;
  const unsigned long long m = __ballot(fresh);
  __shared__ int wave_n[kBlock / 64];
  if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(m);
  __syncthreads();
  if (!fresh) return;
  int slot = nbase[blockIdx.x] + lanes_below(m);
  for (int w = 0; w < (tid >> 6); ++w) slot += wave_n[w];
  if (slot >= cap) return;                // written nowhere: the caller sees bricks[0] > cap
  grid[i] = slot;
  coord[3 * slot] = static_cast<int32_t>(i / (static_cast<long long>(gx) * gy));
  coord[3 * slot + 1] = static_cast<int32_t>((i / gx) % gy);
  coord[3 * slot + 2] = static_cast<int32_t>(i % gx);
}

// ------------------------------------------------------------------------------------------------------------ host

struct AllocLayout { size_t marks, acount, ncount, nbase, frames, total; long long G, blocks; };
inline AllocLayout alloc_layout(int gz, int gy, int gx, int N) {
  AllocLayout L;
  L.G = static_cast<long long>(gz) * gy * gx;
  L.blocks = (L.G + kBlock - 1) / kBlock;
  const size_t per = aligned(sizeof(int) * L.blocks);
  L.marks = 0;
  L.acount = aligned(L.G); L.ncount = L.acount + per; L.nbase = L.ncount + per;
  L.frames = L.nbase + per;
  L.total = L.frames + table_bytes(N);
  return L;
}

inline MeshLayout brick_mesh_layout(int cap) {
  return mesh_layout(static_cast<size_t>(cap), static_cast<size_t>(cap) * kBrick);
}

}  // namespace

extern "C" size_t pvo_tsdf_sparse_allocate_args_size(void) { return sizeof(pvo_tsdf_sparse_allocate_args); }
extern "C" size_t pvo_tsdf_sparse_integrate_args_size(void) { return sizeof(pvo_tsdf_sparse_integrate_args); }
extern "C" size_t pvo_tsdf_sparse_mesh_args_size(void) { return sizeof(pvo_tsdf_sparse_mesh_args); }

extern "C" size_t pvo_tsdf_sparse_allocate_workspace_bytes(int gz, int gy, int gx, int N) {
  if (!world_ok(gz, gy, gx, 0) || static_cast<long long>(gz) * gy * gx == 0 || N <= 0) return 0;
  return alloc_layout(gz, gy, gx, N).total;
}

extern "C" size_t pvo_tsdf_sparse_integrate_workspace_bytes(int N) { return table_bytes(N); }

extern "C" size_t pvo_tsdf_sparse_mesh_workspace_bytes(int cap) {
  if (cap <= 0 || !world_ok(0, 0, 0, cap)) return 0;
  return brick_mesh_layout(cap).total;
}

extern "C" int pvo_tsdf_sparse_allocate(const pvo_tsdf_sparse_allocate_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  PVO_REQ(world_ok(a->gz, a->gy, a->gx, a->cap));
  PVO_REQ(a->N >= 0 && a->nframes >= 0 && a->ht >= 0 && a->wd >= 0 && static_cast<long long>(a->ht) * a->wd < (1ll << 31));
  PVO_REQ(a->voxel > 0.0f && finite_f(a->voxel) && a->trunc > 0.0f && finite_f(a->trunc) && a->trunc / a->voxel <= 4096.0f);
  PVO_REQ(a->z_near >= 0.0f && finite_f(a->z_near) && a->margin >= 0.0f && a->margin <= static_cast<float>(kB));
  PVO_REQ(origin_ok(a));
  const AllocLayout L = alloc_layout(a->gz, a->gy, a->gx, a->N);
  if (L.G == 0 || a->N == 0 || a->ht * a->wd == 0) return PVO_OK;         // nothing to mark
  PVO_REQ(a->grid && a->bricks && a->poses && a->disps && a->intrinsics && a->ix);
  PVO_REQ(a->cap == 0 || a->coord);
  if (!workspace || workspace_bytes < L.total) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  hipStream_t s = pvo_stream(stream);
  char* ws = static_cast<char*>(workspace);
  uint8_t* marks = reinterpret_cast<uint8_t*>(ws + L.marks);
  int* acount = reinterpret_cast<int*>(ws + L.acount);
  int* ncount = reinterpret_cast<int*>(ws + L.ncount);
  int* nbase = reinterpret_cast<int*>(ws + L.nbase);
  float* fc = reinterpret_cast<float*>(ws + L.frames);
  const hipError_t e = hipMemsetAsync(marks, 0, static_cast<size_t>(L.G), s);
  if (e != hipSuccess) { pvo_note_hip_error(static_cast<int>(e)); return PVO_ELAUNCH; }
  hipLaunchKernelGGL(alloc_frames_kernel, dim3((a->N + 63) / 64), dim3(64), 0, s, a->poses, a->ix, fc, a->N, a->nframes);
  PVO_CHECK_LAUNCH();
  const Mark in = {a->disps, a->weight, a->ht, a->wd, static_cast<int>(ceilf(a->trunc / a->voxel)) + 1, a->trunc, a->z_near, a->margin};
  const World g = {a->gz, a->gy, a->gx, a->origin[0], a->origin[1], a->origin[2], a->voxel};
  const long long HW = static_cast<long long>(a->ht) * a->wd;
  hipLaunchKernelGGL(alloc_mark_kernel, dim3(static_cast<unsigned>((HW + kBlock - 1) / kBlock), a->N < 65535 ? a->N : 65535), dim3(kBlock),
                     0, s, fc, a->intrinsics, in, g, a->N, marks);
  PVO_CHECK_LAUNCH();
  const dim3 blocks(static_cast<unsigned>(L.blocks));
  hipLaunchKernelGGL(alloc_count_kernel, blocks, dim3(kBlock), 0, s, a->grid, marks, L.G, acount, ncount);
  PVO_CHECK_LAUNCH();
  hipLaunchKernelGGL(alloc_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, acount, ncount, nbase, a->bricks, static_cast<int>(L.blocks));
  PVO_CHECK_LAUNCH();
  hipLaunchKernelGGL(alloc_assign_kernel, blocks, dim3(kBlock), 0, s, a->grid, marks, L.G, nbase, a->coord, a->cap, a->gy, a->gx);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

namespace {

// pvo_tsdf_sparse_integrate (p == NULL) and pvo_tsdf_sparse_integrate_panoptic: one validation, one launch sequence
int sparse_integrate_impl(const pvo_tsdf_sparse_integrate_args* a, const pvo_tsdf_panoptic_args* p, bool panoptic, void* workspace,
                          size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  if (panoptic) PVO_REQ(panoptic_ok(p, a));
  PVO_REQ(world_ok(a->gz, a->gy, a->gx, a->cap));
  PVO_REQ(fuse_scalars_ok(a));
  if (a->cap == 0 || a->N == 0 || a->ht * a->wd == 0) return PVO_OK;      // nothing to fuse
  PVO_REQ(a->tsdf && a->wsum && a->coord && a->bricks && a->poses && a->disps && a->intrinsics && a->ix);
  PVO_REQ(images_ok(a));
  if (!workspace || workspace_bytes < table_bytes(a->N)) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  hipStream_t s = pvo_stream(stream);
  float* fc = static_cast<float*>(workspace);
  const Vol vol = {a->origin[0], a->origin[1], a->origin[2], a->voxel};
  hipLaunchKernelGGL(sparse_frames_kernel, dim3(a->N), dim3(kCullBlock), 0, s, a->poses, a->ix, a->disps, a->weight, fc, a->nframes,
                     static_cast<long long>(a->ht) * a->wd, vol);
  PVO_CHECK_LAUNCH();
  const Fuse in = fuse_operands(a, a->disps, a->weight);
  const BrickWalk w = {a->coord, a->bricks, a->cap, a->voxel, a->kept};
  pick_rgb_lab(a->rgb != nullptr, panoptic, [&](auto RGB, auto LAB) {
    hipLaunchKernelGGL((tsdf_integrate_kernel<BrickWalk, decltype(RGB)::value, decltype(LAB)::value>), dim3(a->cap), dim3(BrickWalk::kThreads),
                       0, s, w, a->tsdf, a->wsum, a->rgb, fc, a->intrinsics, in, a->N, vote_volumes<decltype(LAB)::value>(p));
  });
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

}  // namespace

extern "C" int pvo_tsdf_sparse_integrate(const pvo_tsdf_sparse_integrate_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  return sparse_integrate_impl(a, nullptr, false, workspace, workspace_bytes, stream);
}

extern "C" int pvo_tsdf_sparse_integrate_panoptic(const pvo_tsdf_sparse_integrate_args* a, const pvo_tsdf_panoptic_args* p, void* workspace,
                                                  size_t workspace_bytes, void* stream) {
  return sparse_integrate_impl(a, p, true, workspace, workspace_bytes, stream);
}

namespace {

// pvo_tsdf_sparse_mesh (p == NULL) and pvo_tsdf_sparse_mesh_panoptic
int sparse_mesh_impl(const pvo_tsdf_sparse_mesh_args* a, const pvo_tsdf_mesh_labels_args* p, bool panoptic, void* workspace,
                     size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  if (panoptic) PVO_REQ(mesh_labels_ok(p, a));
  PVO_REQ(world_ok(a->gz, a->gy, a->gx, a->cap));
  PVO_REQ(mesh_scalars_ok(a) && a->bricks);
  hipStream_t s = pvo_stream(stream);
  if (a->cap == 0 || static_cast<long long>(a->gz) * a->gy * a->gx == 0) return mesh_no_cell(a->counts, s);      // no brick
  PVO_REQ(a->grid && a->coord && a->tsdf && a->wsum);
  PVO_REQ(mesh_outputs_ok(a));
  const MeshLayout L = brick_mesh_layout(a->cap);
  if (!workspace || workspace_bytes < L.total) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 7));
  const BrickCells g = {{a->tsdf, a->wsum, a->rgb, a->origin[0], a->origin[1], a->origin[2], a->voxel, a->min_weight},
                        a->grid, a->coord, a->bricks, a->gz, a->gy, a->gx, a->cap};
  const MeshOut out = {a->verts, a->normals, a->rgba, a->faces, a->vcap, a->fcap};
  return mesh_launch(g, a->cap, L, workspace, out, a->counts, panoptic ? p : nullptr, s);
}

}  // namespace

extern "C" int pvo_tsdf_sparse_mesh(const pvo_tsdf_sparse_mesh_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  return sparse_mesh_impl(a, nullptr, false, workspace, workspace_bytes, stream);
}

extern "C" int pvo_tsdf_sparse_mesh_panoptic(const pvo_tsdf_sparse_mesh_args* a, const pvo_tsdf_mesh_labels_args* p, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  return sparse_mesh_impl(a, p, true, workspace, workspace_bytes, stream);
}
