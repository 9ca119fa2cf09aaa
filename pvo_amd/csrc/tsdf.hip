// tsdf.hip — dense surface reconstruction: keyframe depth maps fused into a truncated signed distance volume, and a triangle mesh
// extracted from it by naive surface nets.  Contracts: include/pvo_hip.h (pvo_tsdf_integrate, pvo_tsdf_mesh); yardstick:
// tests/tsdf_reference.py.
//
//   integrate  (a) tsdf_frames_kernel     one thread per slot of ix: the frame's twelve pre-multiplied constants  voxel * R  and
//                                         R origin + t  (so that Xc = A (x, y, z) + b for the INTEGER voxel index) and its frame id,
//                                         -1 for an id outside [0, nframes): sixteen floats per slot in the workspace
//              (b) tsdf_integrate_kernel  one thread per voxel, x fastest; the frame loop runs inside, so the volume is read and
//                                         written once per call whatever N is.  The slot's constants are wave-uniform loads; a wave none
//                                         of whose voxels projects into a frame skips its gathers.
//   mesh       (a) mesh_classify_kernel   one thread per cell: active bit, the three quad bits, per-workgroup counts
//              (b) mesh_scan_kernel       one workgroup: exclusive scans of both counts in index order, the two totals
//              (c) mesh_verts_kernel      vertex of every active cell (and cell -> vertex index in the workspace)
//              (d) mesh_faces_kernel      two triangles per quad
//
// No atomics anywhere: every output index is a function of the classification bits alone, and a voxel's running average is one
// thread's sequential loop - the same operands give the same bytes.  The slot constants, the update of a voxel by one frame and the
// vertex of a cell are the inline functions of tsdf_fuse.h, which the brick volume (tsdf_sparse.hip) calls as well.
//
// Panoptic (pvo_tsdf_integrate_panoptic, pvo_tsdf_mesh_panoptic): the same launches with the LAB instantiations of (b) and (c) - the
// label vote inside the voxel's frame loop, the vertex's label beside its position.  What they need beyond the plain kernels' arguments
// is the kernels' last argument, empty without LAB, so the plain instantiations keep their code.
#include "tsdf_fuse.h"

namespace {

constexpr int kBlock = 256;
constexpr int kScanThreads = 1024;

// ------------------------------------------------------------------------------------------------------------ integrate

__global__ __launch_bounds__(64) void tsdf_frames_kernel(const float* __restrict__ poses, const int64_t* __restrict__ ix,
                                                         float* __restrict__ fc, int N, int nframes, const Vol vol) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= N) return;
  float* o = fc + static_cast<long long>(kFrameFloats) * b;
  const long long f = ix[b];
  if (f < 0 || f >= nframes) {            // never dereferenced
    o[12] = __int_as_float(-1);
    return;
  }
  tsdf_frame_constants(poses, f, vol, o);
}

// LAB: with the label vote on the caller's label / lconf volumes (pvo_tsdf_integrate_panoptic)
template <bool RGB, bool LAB>
__global__ __launch_bounds__(kBlock) void tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ wsum, float* __restrict__ rgb,
                                                               const float* __restrict__ fc, const float* __restrict__ intrinsics,
                                                               const Fuse in, int N, int nz, int ny, int nx, const VoteVolumes<LAB> pan) {
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
    if constexpr (LAB) { a.L = pan.label[i]; a.lc = pan.lconf[i]; }
  }
  for (int b = 0; b < N; ++b) {
    const float* __restrict__ c = fc + static_cast<long long>(kFrameFloats) * b;      // wave-uniform
    const int f = __float_as_int(c[12]);
    if (f < 0) continue;
    if constexpr (LAB) tsdf_fuse_frame<RGB, true>(a, c, f, xf, yf, zf, live, K, in, HW, plane, pan.maps);
    else tsdf_fuse_frame<RGB>(a, c, f, xf, yf, zf, live, K, in, HW, plane);
  }
  if (a.touched) {
    tsdf[i] = a.T; wsum[i] = a.W;
    if (RGB) { rgb[3 * i] = a.cr; rgb[3 * i + 1] = a.cg; rgb[3 * i + 2] = a.cb; }
    if constexpr (LAB) { pan.label[i] = a.L; pan.lconf[i] = a.lc; }
  }
}

// ------------------------------------------------------------------------------------------------------------ mesh

struct Grid {
  const float* tsdf; const float* wsum; const float* rgb;
  int nz, ny, nx;
  float ox, oy, oz, voxel, min_weight;
};

__device__ __forceinline__ void cell_coords(long long k, const Grid g, int& cz, int& cy, int& cx) {
  const int mx = g.nx - 1, my = g.ny - 1;
  cx = static_cast<int>(k % mx); cy = static_cast<int>((k / mx) % my); cz = static_cast<int>(k / (static_cast<long long>(mx) * my));
}

__device__ __forceinline__ long long voxel_index(const Grid g, int z, int y, int x) {
  return (static_cast<long long>(z) * g.ny + y) * g.nx + x;
}

// all eight corners of the cell at (cz, cy, cx) valid; the caller keeps the cell's indices in [0, dim - 1)
__device__ __forceinline__ bool cell_valid(const Grid g, int cz, int cy, int cx) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 8; ++j) ok = ok && g.wsum[voxel_index(g, cz + (j >> 2), cy + ((j >> 1) & 1), cx + (j & 1))] >= g.min_weight;
  return ok;
}

__global__ __launch_bounds__(kBlock) void mesh_classify_kernel(const Grid g, long long cells, uint8_t* __restrict__ flags,
                                                              int* __restrict__ vcount, int* __restrict__ qcount) {
  const int tid = threadIdx.x;
  const long long k = static_cast<long long>(blockIdx.x) * kBlock + tid;
  int flag = 0;
  if (k < cells) {                        // (no early return: every wave reaches the ballots and the barrier)
    int cz, cy, cx;
    cell_coords(k, g, cz, cy, cx);
    bool valid = true;
    int inside = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long v = voxel_index(g, cz + (j >> 2), cy + ((j >> 1) & 1), cx + (j & 1));
      valid = valid && g.wsum[v] >= g.min_weight;
      inside |= (g.tsdf[v] < 0.0f ? 1 : 0) << j;
    }
    if (valid && inside != 0 && inside != 255) {
      flag = kActive | ((inside & 1) ? kInsideA : 0);
      const int c[3] = {cx, cy, cz};
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, cc = (a + 2) % 3;
        if ((((inside >> (1 << a)) ^ inside) & 1) == 0 || c[b] < 1 || c[cc] < 1) continue;
        // the three other cells around the edge share it, so they are not all on one side: active = all corners valid
        int eb[3] = {0, 0, 0}, ec[3] = {0, 0, 0};
        eb[b] = 1; ec[cc] = 1;
        if (cell_valid(g, cz - eb[2], cy - eb[1], cx - eb[0]) && cell_valid(g, cz - eb[2] - ec[2], cy - eb[1] - ec[1], cx - eb[0] - ec[0]) &&
            cell_valid(g, cz - ec[2], cy - ec[1], cx - ec[0]))
          flag |= 2 << a;
      }
    }
    flags[k] = static_cast<uint8_t>(flag);
  }
  const unsigned long long ma = __ballot(flag & kActive);
  const int quads = __popcll(__ballot(flag & 2)) + __popcll(__ballot(flag & 4)) + __popcll(__ballot(flag & 8));
  __shared__ int wave_v[kBlock / 64], wave_q[kBlock / 64];
  if ((tid & 63) == 0) { wave_v[tid >> 6] = __popcll(ma); wave_q[tid >> 6] = quads; }
  __syncthreads();
  if (tid == 0) {
    vcount[blockIdx.x] = (wave_v[0] + wave_v[1]) + (wave_v[2] + wave_v[3]);
    qcount[blockIdx.x] = (wave_q[0] + wave_q[1]) + (wave_q[2] + wave_q[3]);
  }
}

// exclusive scans of vcount and qcount [M] in index order (thread t owns a contiguous chunk, map_points.hip's scan);
// counts = (vertices, faces = 2 * quads), not clamped by any capacity
__global__ __launch_bounds__(kScanThreads) void mesh_scan_kernel(const int* __restrict__ vcount, const int* __restrict__ qcount,
                                                                 int* __restrict__ vbase, int* __restrict__ qbase,
                                                                 int32_t* __restrict__ counts, int M) {
  const int tid = threadIdx.x;
  const int chunk = (M + kScanThreads - 1) / kScanThreads;
  const int lo = static_cast<int>(min(static_cast<long long>(tid) * chunk, static_cast<long long>(M))), hi = min(lo + chunk, M);
  __shared__ int buf[2][kScanThreads];
  for (int pass = 0; pass < 2; ++pass) {
    const int* __restrict__ cnt = pass ? qcount : vcount;
    int* __restrict__ base = pass ? qbase : vbase;
    int s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    int cur = 0;
    buf[0][tid] = s;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < kScanThreads; off <<= 1) {      // Hillis-Steele, inclusive
      buf[cur ^ 1][tid] = buf[cur][tid] + (tid >= off ? buf[cur][tid - off] : 0);
      cur ^= 1;
      __syncthreads();
    }
    int run = buf[cur][tid] - s;
    for (int i = lo; i < hi; ++i) { base[i] = run; run += cnt[i]; }
    if (tid == kScanThreads - 1) counts[pass] = pass ? 2 * buf[cur][tid] : buf[cur][tid];
    __syncthreads();                                        // buf is reused by the second pass
  }
}

// LAB: the vertex's label into vlabel as well (pvo_tsdf_mesh_panoptic)
template <bool LAB>
__global__ __launch_bounds__(kBlock) void mesh_verts_kernel(const Grid g, long long cells, const uint8_t* __restrict__ flags,
                                                           const int* __restrict__ vbase, int32_t* __restrict__ vidx, const MeshOut out,
                                                           const VertexLabels<LAB> lab) {
  const int tid = threadIdx.x;
  const long long k = static_cast<long long>(blockIdx.x) * kBlock + tid;
  const bool active = k < cells && (flags[k] & kActive);
  const unsigned long long m = __ballot(active);
  __shared__ int wave_n[kBlock / 64];
  if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(m);
  __syncthreads();
  if (!active) return;
  int idx = vbase[blockIdx.x] + lanes_below(m);
  for (int w = 0; w < (tid >> 6); ++w) idx += wave_n[w];
  vidx[k] = idx;                          // (also beyond the capacity: the faces name the vertex by its index)
  if (idx >= out.vcap) return;            // written nowhere; the caller sees counts[0] > vcap
  int cz, cy, cx;
  cell_coords(k, g, cz, cy, cx);
  float s[8];
  long long at[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    at[j] = voxel_index(g, cz + (j >> 2), cy + ((j >> 1) & 1), cx + (j & 1));
    s[j] = g.tsdf[at[j]];
  }
  surface_net_vertex(s, g.rgb, at, cx, cy, cz, g.ox, g.oy, g.oz, g.voxel, out, idx);
  if constexpr (LAB) lab.vlabel[idx] = surface_net_label(s, lab.label, at);
}

__global__ __launch_bounds__(kBlock) void mesh_faces_kernel(const Grid g, long long cells, const uint8_t* __restrict__ flags,
                                                           const int* __restrict__ qbase, const int32_t* __restrict__ vidx, const MeshOut out) {
  const int tid = threadIdx.x;
  const long long k = static_cast<long long>(blockIdx.x) * kBlock + tid;
  const int flag = k < cells ? flags[k] : 0;
  // quads are numbered cell by cell, inside a cell by axis: the quads of the lower lanes, whatever their axis, come first
  const unsigned long long mx = __ballot(flag & 2), my = __ballot(flag & 4), mz = __ballot(flag & 8);
  __shared__ int wave_n[kBlock / 64];
  if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(mx) + __popcll(my) + __popcll(mz);
  __syncthreads();
  if (!(flag & 14)) return;
  int q = qbase[blockIdx.x] + lanes_below(mx) + lanes_below(my) + lanes_below(mz);
  for (int w = 0; w < (tid >> 6); ++w) q += wave_n[w];
  const long long mxc = g.nx - 1, mxy = mxc * (g.ny - 1);
  const long long step[3] = {1, mxc, mxy};              // cell index strides along x, y, z
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(flag & (2 << a))) continue;
    const long long sb = step[(a + 1) % 3], sc = step[(a + 2) % 3];
    const int q0 = vidx[k], q1 = vidx[k - sb], q2 = vidx[k - sb - sc], q3 = vidx[k - sc];
    const bool fwd = (flag & kInsideA) != 0;            // corner 0 inside; otherwise its neighbour is: reversed winding
    const int f0 = 2 * q, f1 = 2 * q + 1;
    if (f0 < out.fcap) {
      int32_t* o = out.faces + 3ll * f0;
      o[0] = q0; o[1] = fwd ? q1 : q2; o[2] = fwd ? q2 : q1;
    }
    if (f1 < out.fcap) {
      int32_t* o = out.faces + 3ll * f1;
      o[0] = q0; o[1] = fwd ? q2 : q3; o[2] = fwd ? q3 : q2;
    }
    ++q;
  }
}

constexpr size_t kAlign = 256;
inline size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }

struct MeshLayout { size_t vcount, qcount, vbase, qbase, vidx, flags, total; long long cells, blocks; };
inline MeshLayout mesh_layout(int nz, int ny, int nx) {
  MeshLayout L;
  L.cells = static_cast<long long>(nz - 1) * (ny - 1) * (nx - 1);
  L.blocks = (L.cells + kBlock - 1) / kBlock;
  const size_t per = aligned(sizeof(int) * L.blocks);
  L.vcount = 0; L.qcount = per; L.vbase = 2 * per; L.qbase = 3 * per;
  L.vidx = 4 * per;
  L.flags = L.vidx + aligned(sizeof(int32_t) * L.cells);
  L.total = L.flags + aligned(L.cells);
  return L;
}

inline bool volume_ok(int nz, int ny, int nx) {
  return nz >= 0 && ny >= 0 && nx >= 0 && static_cast<long long>(nz) * ny < (1ll << 31) && static_cast<long long>(nz) * ny * nx < (1ll << 31);
}
inline bool finite_f(float v) { return v - v == 0.0f; }

}  // namespace

#define PVO_REQ(c) do { if (!(c)) return PVO_EINVAL; } while (0)

extern "C" size_t pvo_tsdf_integrate_args_size(void) { return sizeof(pvo_tsdf_integrate_args); }
extern "C" size_t pvo_tsdf_mesh_args_size(void) { return sizeof(pvo_tsdf_mesh_args); }
extern "C" size_t pvo_tsdf_panoptic_args_size(void) { return sizeof(pvo_tsdf_panoptic_args); }
extern "C" size_t pvo_tsdf_mesh_labels_args_size(void) { return sizeof(pvo_tsdf_mesh_labels_args); }

extern "C" size_t pvo_tsdf_integrate_workspace_bytes(int N) {
  return N <= 0 ? 0 : aligned(sizeof(float) * kFrameFloats * static_cast<size_t>(N));
}

extern "C" size_t pvo_tsdf_mesh_workspace_bytes(int nz, int ny, int nx) {
  if (nz < 2 || ny < 2 || nx < 2 || !volume_ok(nz, ny, nx)) return 0;
  return mesh_layout(nz, ny, nx).total;
}

namespace {

// pvo_tsdf_integrate (p == NULL) and pvo_tsdf_integrate_panoptic: one validation, one launch sequence
int integrate_impl(const pvo_tsdf_integrate_args* a, const pvo_tsdf_panoptic_args* p, bool panoptic, void* workspace, size_t workspace_bytes,
                   void* stream) {
  PVO_REQ(a);
  if (panoptic) {
    PVO_REQ(p && p->label && p->lconf && p->labels && p->label_div >= 1);
    PVO_REQ(static_cast<long long>(p->lh) * p->label_div >= a->ht && static_cast<long long>(p->lw) * p->label_div >= a->wd);
  }
  PVO_REQ(volume_ok(a->nz, a->ny, a->nx));
  PVO_REQ(a->N >= 0 && a->nframes >= 0 && a->ht >= 0 && a->wd >= 0 && static_cast<long long>(a->ht) * a->wd < (1ll << 31));
  PVO_REQ(a->voxel > 0.0f && finite_f(a->voxel) && a->trunc > 0.0f && finite_f(a->trunc));
  PVO_REQ(a->z_near >= 0.0f && finite_f(a->z_near) && a->w_max >= 0.0f && finite_f(a->w_max));
  PVO_REQ(finite_f(a->origin[0]) && finite_f(a->origin[1]) && finite_f(a->origin[2]));
  const long long total = static_cast<long long>(a->nz) * a->ny * a->nx;
  if (total == 0 || a->N == 0 || a->ht * a->wd == 0) return PVO_OK;       // nothing to fuse
  PVO_REQ(a->tsdf && a->wsum && a->poses && a->disps && a->intrinsics && a->ix);
  PVO_REQ(!a->rgb || a->images);                 // a colour volume needs the images
  if (a->images) {
    PVO_REQ(a->img_stride >= 1 && a->img_offset >= 0 && a->IH > 0 && a->IW > 0);
    PVO_REQ(static_cast<long long>(a->img_stride) * (a->ht - 1) + a->img_offset < a->IH);
    PVO_REQ(static_cast<long long>(a->img_stride) * (a->wd - 1) + a->img_offset < a->IW);
  }
  if (!workspace || workspace_bytes < pvo_tsdf_integrate_workspace_bytes(a->N)) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  hipStream_t s = pvo_stream(stream);
  float* fc = static_cast<float*>(workspace);
  const Vol vol = {a->origin[0], a->origin[1], a->origin[2], a->voxel};
  hipLaunchKernelGGL(tsdf_frames_kernel, dim3((a->N + 63) / 64), dim3(64), 0, s, a->poses, a->ix, fc, a->N, a->nframes, vol);
  PVO_CHECK_LAUNCH();
  const Fuse in = {a->disps, a->weight, a->images, a->ht, a->wd, a->IH, a->IW, a->img_stride, a->img_offset, a->trunc, a->z_near, a->w_max};
  const dim3 grid(static_cast<unsigned>((total + kBlock - 1) / kBlock));
  if (panoptic) {
    const VoteVolumes<true> pan = {p->label, p->lconf, {p->labels, p->lh, p->lw, p->label_div}};
    if (a->rgb)
      hipLaunchKernelGGL((tsdf_integrate_kernel<true, true>), grid, dim3(kBlock), 0, s, a->tsdf, a->wsum, a->rgb, fc, a->intrinsics, in, a->N,
                         a->nz, a->ny, a->nx, pan);
    else
      hipLaunchKernelGGL((tsdf_integrate_kernel<false, true>), grid, dim3(kBlock), 0, s, a->tsdf, a->wsum, a->rgb, fc, a->intrinsics, in, a->N,
                         a->nz, a->ny, a->nx, pan);
  } else if (a->rgb)
    hipLaunchKernelGGL((tsdf_integrate_kernel<true, false>), grid, dim3(kBlock), 0, s, a->tsdf, a->wsum, a->rgb, fc, a->intrinsics, in, a->N,
                       a->nz, a->ny, a->nx, VoteVolumes<false>{});
  else
    hipLaunchKernelGGL((tsdf_integrate_kernel<false, false>), grid, dim3(kBlock), 0, s, a->tsdf, a->wsum, a->rgb, fc, a->intrinsics, in, a->N,
                       a->nz, a->ny, a->nx, VoteVolumes<false>{});
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
  if (panoptic) PVO_REQ(p && p->label && (a->vcap == 0 || p->vlabel));
  PVO_REQ(volume_ok(a->nz, a->ny, a->nx));
  PVO_REQ(a->voxel > 0.0f && finite_f(a->voxel) && a->min_weight == a->min_weight);
  PVO_REQ(finite_f(a->origin[0]) && finite_f(a->origin[1]) && finite_f(a->origin[2]));
  PVO_REQ(a->vcap >= 0 && a->fcap >= 0 && a->counts);
  PVO_REQ(!((reinterpret_cast<uintptr_t>(a->rgba) & 3)));
  hipStream_t s = pvo_stream(stream);
  if (a->nz < 2 || a->ny < 2 || a->nx < 2) {     // no cell: the counts alone
    const hipError_t e = hipMemsetAsync(a->counts, 0, 2 * sizeof(int32_t), s);
    if (e != hipSuccess) { pvo_note_hip_error(static_cast<int>(e)); return PVO_ELAUNCH; }
    return PVO_OK;
  }
  PVO_REQ(a->tsdf && a->wsum);
  PVO_REQ((a->vcap == 0 || a->verts) && (a->fcap == 0 || a->faces));
  const MeshLayout L = mesh_layout(a->nz, a->ny, a->nx);
  if (!workspace || workspace_bytes < L.total) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 7));
  char* ws = static_cast<char*>(workspace);
  int* vcount = reinterpret_cast<int*>(ws + L.vcount);
  int* qcount = reinterpret_cast<int*>(ws + L.qcount);
  int* vbase = reinterpret_cast<int*>(ws + L.vbase);
  int* qbase = reinterpret_cast<int*>(ws + L.qbase);
  int32_t* vidx = reinterpret_cast<int32_t*>(ws + L.vidx);
  uint8_t* flags = reinterpret_cast<uint8_t*>(ws + L.flags);
  const Grid g = {a->tsdf, a->wsum, a->rgb, a->nz, a->ny, a->nx, a->origin[0], a->origin[1], a->origin[2], a->voxel, a->min_weight};
  const MeshOut out = {a->verts, a->normals, a->rgba, a->faces, a->vcap, a->fcap};
  const dim3 grid(static_cast<unsigned>(L.blocks));
  hipLaunchKernelGGL(mesh_classify_kernel, grid, dim3(kBlock), 0, s, g, L.cells, flags, vcount, qcount);
  PVO_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, vcount, qcount, vbase, qbase, a->counts, static_cast<int>(L.blocks));
  PVO_CHECK_LAUNCH();
  if (panoptic)
    hipLaunchKernelGGL(mesh_verts_kernel<true>, grid, dim3(kBlock), 0, s, g, L.cells, flags, vbase, vidx, out,
                       VertexLabels<true>{p->label, p->vlabel});
  else
    hipLaunchKernelGGL(mesh_verts_kernel<false>, grid, dim3(kBlock), 0, s, g, L.cells, flags, vbase, vidx, out, VertexLabels<false>{});
  PVO_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_faces_kernel, grid, dim3(kBlock), 0, s, g, L.cells, flags, qbase, vidx, out);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

}  // namespace

extern "C" int pvo_tsdf_mesh(const pvo_tsdf_mesh_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  return mesh_impl(a, nullptr, false, workspace, workspace_bytes, stream);
}

extern "C" int pvo_tsdf_mesh_panoptic(const pvo_tsdf_mesh_args* a, const pvo_tsdf_mesh_labels_args* p, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return mesh_impl(a, p, true, workspace, workspace_bytes, stream);
}
