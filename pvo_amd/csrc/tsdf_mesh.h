// tsdf_mesh.h — naive surface nets, ONE body for the dense volume (tsdf.hip) and the brick volume (tsdf_sparse.hip).  The active-cell
// rule, the three quad bits, the numbering of vertices and quads by ballots, the winding and the capacity protocol stand here once; a
// volume is seen through a cell addresser (DenseCells, BrickCells) that only says where a corner or a neighbouring cell is stored, so
// a sparse vertex has the bytes of the dense vertex of that cell.
//
//   (a) mesh_classify_kernel<A>  one thread per cell: active bit, the three quad bits, per-workgroup counts
//   (b) mesh_scan_kernel         one workgroup: exclusive scans of both counts in workgroup order (scan.h), the two totals
//   (c) mesh_verts_kernel<A,LAB> vertex of every active cell (and cell -> vertex index in the workspace); LAB: its label as well
//   (d) mesh_faces_kernel<A>     two triangles per quad
//
// An addresser A is the kernels' first argument and answers, for the thread's cell c (an A::Cell):
//   enter(c)                  false = the WHOLE workgroup has no cell (and takes part in no barrier); else c.has = this thread has a
//                             cell, c.k = its index into flags / vidx.  The count slot of a workgroup is blockIdx.x.
//   locate(c)                 c.g = the cell's global integer coordinates (x, y, z) - called only where a cell needs them
//   corner(c, j)              pool index of corner j = 4 dz + 2 dy + dx of a located cell; exists(v) = that corner is stored
//   neighbour(c, dz, dy, dx)  flags / vidx index of the cell at that offset (each 0 or -1), which the caller knows to be active
//   neighbour_valid(c, ...)   all eight corners of that cell stored with wsum >= min_weight
// Vertices come out in the order of (workgroup, thread): raster order of cells for DenseCells, (slot, raster order inside the brick)
// for BrickCells.
#pragma once
#include "scan.h"
#include "tsdf_fuse.h"
#include "tsdf_host.h"

namespace {

// flag byte of a cell: bit 0 active, bits 1-3 a quad around the edge corner 0 -> corner 0 + e_a (a = x, y, z), bit 4 corner 0 inside
constexpr int kActive = 1, kInsideA = 16;

struct MeshOut { float* verts; float* normals; uint8_t* rgba; int32_t* faces; int vcap, fcap; };

template <bool LAB> struct VertexLabels {};
template <> struct VertexLabels<true> { const int32_t* label; int32_t* vlabel; };            // label: shaped like tsdf; vlabel [vcap]

// vertex idx (< out.vcap) of the cell with the INTEGER index (cx, cy, cz) and corner values s[j] (j = 4 dz + 2 dy + dx); corner j's
// colour is rgb[3 * at[j] ..] (rgb may be NULL): position, normal and colour as include/pvo_hip.h pvo_tsdf_mesh states them
__device__ __forceinline__ void surface_net_vertex(const float (&s)[8], const float* __restrict__ rgb, const long long (&at)[8], int cx,
                                                   int cy, int cz, float ox, float oy, float oz, float voxel, const MeshOut out, int idx) {
  // mean of the crossings of the sign-changing edges, in cell coordinates; edges in the order x (from corners 0, 2, 4, 6),
  // y (0, 1, 4, 5), z (0, 1, 2, 3)
  float p[3] = {0.0f, 0.0f, 0.0f};
  int n = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j & (1 << a)) continue;
      const float sa = s[j], sb = s[j | (1 << a)];
      if ((sa < 0.0f) == (sb < 0.0f)) continue;
      const float t = sa / (sa - sb);     // opposite sides: |sa - sb| = |sa| + |sb| > 0
#pragma unroll
      for (int e = 0; e < 3; ++e) p[e] += (e == a) ? t : static_cast<float>((j >> e) & 1);
      ++n;
    }
  }
  const float nf = static_cast<float>(n);
  float* o = out.verts + 3ll * idx;
  o[0] = ox + voxel * (static_cast<float>(cx) + p[0] / nf);
  o[1] = oy + voxel * (static_cast<float>(cy) + p[1] / nf);
  o[2] = oz + voxel * (static_cast<float>(cz) + p[2] / nf);
  if (out.normals) {                      // central gradient of the eight corners, toward increasing tsdf
    const float gx = ((s[1] - s[0]) + (s[3] - s[2])) + ((s[5] - s[4]) + (s[7] - s[6]));
    const float gy = ((s[2] - s[0]) + (s[3] - s[1])) + ((s[6] - s[4]) + (s[7] - s[5]));
    const float gz = ((s[4] - s[0]) + (s[5] - s[1])) + ((s[6] - s[2]) + (s[7] - s[3]));
    const float len = sqrtf(gx * gx + gy * gy + gz * gz);
    float* q = out.normals + 3ll * idx;
    const bool zero = !(len > 0.0f);
    q[0] = zero ? 0.0f : gx / len; q[1] = zero ? 0.0f : gy / len; q[2] = zero ? 0.0f : gz / len;
  }
  if (out.rgba) {
    uchar4 c = make_uchar4(0, 0, 0, 255);
    if (rgb) {
      float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int e = 0; e < 3; ++e) acc[e] += rgb[3 * at[j] + e];
      }
      // mean + 0.5, floored, clamped to [0, 255] (NaN -> 0)
      c.x = static_cast<uint8_t>(min(255, max(0, pvo_floor_to_int(acc[0] * 0.125f + 0.5f))));
      c.y = static_cast<uint8_t>(min(255, max(0, pvo_floor_to_int(acc[1] * 0.125f + 0.5f))));
      c.z = static_cast<uint8_t>(min(255, max(0, pvo_floor_to_int(acc[2] * 0.125f + 0.5f))));
    }
    reinterpret_cast<uchar4*>(out.rgba)[idx] = c;
  }
}

// ------------------------------------------------------------------------------------------------------------ addressers

// what both addressers hold: the volume's arrays and its placement
struct MeshVolume {
  const float* tsdf; const float* wsum; const float* rgb;
  float ox, oy, oz, voxel, min_weight;
};

// raster cells of a dense [nz,ny,nx] volume, x fastest, 256 per workgroup
struct DenseCells {
  static constexpr int kThreads = 256;
  MeshVolume v;
  int nz, ny, nx;
  long long cells;                        // (nz - 1) (ny - 1) (nx - 1)
  struct Cell { long long k; bool has; int g[3]; };

  __device__ __forceinline__ bool enter(Cell& c) const {
    c.k = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
    c.has = c.k < cells;
    return true;
  }
  __device__ __forceinline__ void locate(Cell& c) const {
    const int mx = nx - 1, my = ny - 1;
    c.g[0] = static_cast<int>(c.k % mx); c.g[1] = static_cast<int>((c.k / mx) % my);
    c.g[2] = static_cast<int>(c.k / (static_cast<long long>(mx) * my));
  }
  static __device__ __forceinline__ bool exists(long long) { return true; }
  __device__ __forceinline__ long long voxel_index(int z, int y, int x) const { return (static_cast<long long>(z) * ny + y) * nx + x; }
  __device__ __forceinline__ long long corner(const Cell& c, int j) const {
    return voxel_index(c.g[2] + (j >> 2), c.g[1] + ((j >> 1) & 1), c.g[0] + (j & 1));
  }
  __device__ __forceinline__ long long neighbour(const Cell& c, int dz, int dy, int dx) const {
    const long long mx = nx - 1;
    return c.k + (dz * (ny - 1) + dy) * mx + dx;
  }
  // (the caller keeps the neighbour's indices in [0, dim - 1))
  __device__ __forceinline__ bool neighbour_valid(const Cell& c, int dz, int dy, int dx) const {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      ok = ok && v.wsum[voxel_index(c.g[2] + dz + (j >> 2), c.g[1] + dy + ((j >> 1) & 1), c.g[0] + dx + (j & 1))] >= v.min_weight;
    return ok;
  }
};

// the 512 cells whose corner 0 lies in one brick, one brick in use per workgroup; the slots of the 27 bricks around it in LDS
struct BrickCells {
  static constexpr int kThreads = 512;
  MeshVolume v;
  const int32_t* grid; const int32_t* coord; const int32_t* bricks;
  int gz, gy, gx, cap;
  struct Cell { long long k; bool has; int b[3], g[3]; int lx, ly, lz; const int* nb; };

  // the slots of the 3 x 3 x 3 bricks around brick (bz,by,bx) into nb (LDS), -1 outside the grid; ends with a barrier
  __device__ __forceinline__ void load_neighbours(int bz, int by, int bx, int* nb) const {
    const int tid = threadIdx.x;
    if (tid < 27) {
      const int z = bz + tid / 9 - 1, y = by + (tid / 3) % 3 - 1, x = bx + tid % 3 - 1;
      const bool in = z >= 0 && z < gz && y >= 0 && y < gy && x >= 0 && x < gx;
      const int s = in ? grid[(static_cast<long long>(z) * gy + y) * gx + x] : -1;
      nb[tid] = s < cap ? s : -1;         // (a slot the pool does not have is no brick)
    }
    __syncthreads();
  }
  // pool index of the voxel at local (lz,ly,lx), each in [-1, 8], of the brick whose neighbours are nb; -1 in a brick that does not exist
  static __device__ __forceinline__ long long voxel_at(const int* nb, int lz, int ly, int lx) {
    const int s = nb[((lz >> 3) + 1) * 9 + ((ly >> 3) + 1) * 3 + ((lx >> 3) + 1)];
    return s < 0 ? -1 : static_cast<long long>(s) * 512 + (((lz & 7) << 6) | ((ly & 7) << 3) | (lx & 7));
  }

  __device__ __forceinline__ bool enter(Cell& c) const {
    const int slot = blockIdx.x, tid = threadIdx.x;
    if (slot >= min(bricks[0], cap)) return false;      // a slot not in use has no cell
    __shared__ int nb[27];
    const int bz = coord[3 * slot], by = coord[3 * slot + 1], bx = coord[3 * slot + 2];
    load_neighbours(bz, by, bx, nb);
    c.nb = nb;
    c.k = static_cast<long long>(slot) * kThreads + tid;
    c.has = true;
    c.b[0] = bx; c.b[1] = by; c.b[2] = bz;
    return true;
  }
  // (the local coordinates are formed HERE, in the block that uses them: the compiler's per-block value ranges then see 0 .. 7)
  __device__ __forceinline__ void locate(Cell& c) const {
    const int tid = threadIdx.x;
    c.lx = tid & 7; c.ly = (tid >> 3) & 7; c.lz = tid >> 6;
    c.g[0] = 8 * c.b[0] + c.lx; c.g[1] = 8 * c.b[1] + c.ly; c.g[2] = 8 * c.b[2] + c.lz;
  }
  static __device__ __forceinline__ bool exists(long long v) { return v >= 0; }
  __device__ __forceinline__ long long corner(const Cell& c, int j) const {
    return voxel_at(c.nb, c.lz + (j >> 2), c.ly + ((j >> 1) & 1), c.lx + (j & 1));
  }
  // (an active cell's brick exists)
  __device__ __forceinline__ long long neighbour(const Cell& c, int dz, int dy, int dx) const {
    return voxel_at(c.nb, c.lz + dz, c.ly + dy, c.lx + dx);
  }
  __device__ __forceinline__ bool neighbour_valid(const Cell& c, int dz, int dy, int dx) const {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long at = voxel_at(c.nb, c.lz + dz + (j >> 2), c.ly + dy + ((j >> 1) & 1), c.lx + dx + (j & 1));
      ok = ok && at >= 0 && v.wsum[at >= 0 ? at : 0] >= v.min_weight;
    }
    return ok;
  }
};

// ------------------------------------------------------------------------------------------------------------ kernels

template <typename A>
__global__ __launch_bounds__(A::kThreads) void mesh_classify_kernel(const A g, uint8_t* __restrict__ flags, int* __restrict__ vcount,
                                                                   int* __restrict__ qcount) {
  const int tid = threadIdx.x;
  typename A::Cell c;
  if (!g.enter(c)) {                      // (the whole workgroup)
    if (tid == 0) { vcount[blockIdx.x] = 0; qcount[blockIdx.x] = 0; }
    return;
  }
  int flag = 0;
  if (c.has) {                            // (no early return: every wave reaches the ballots and the barrier)
    g.locate(c);
    bool valid = true;
    int inside = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long at = g.corner(c, j);
      const bool stored = A::exists(at);
      valid = valid && stored && g.v.wsum[stored ? at : 0] >= g.v.min_weight;
      inside |= (g.v.tsdf[stored ? at : 0] < 0.0f ? 1 : 0) << j;
    }
    if (valid && inside != 0 && inside != 255) {
      flag = kActive | ((inside & 1) ? kInsideA : 0);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, cc = (a + 2) % 3;
        if ((((inside >> (1 << a)) ^ inside) & 1) == 0 || c.g[b] < 1 || c.g[cc] < 1) continue;
        // the three other cells around the edge share it, so they are not all on one side: active = all corners valid
        int eb[3] = {0, 0, 0}, ec[3] = {0, 0, 0};
        eb[b] = 1; ec[cc] = 1;
        if (g.neighbour_valid(c, -eb[2], -eb[1], -eb[0]) && g.neighbour_valid(c, -eb[2] - ec[2], -eb[1] - ec[1], -eb[0] - ec[0]) &&
            g.neighbour_valid(c, -ec[2], -ec[1], -ec[0]))
          flag |= 2 << a;
      }
    }
    flags[c.k] = static_cast<uint8_t>(flag);
  }
  const unsigned long long ma = __ballot(flag & kActive);
  const int quads = __popcll(__ballot(flag & 2)) + __popcll(__ballot(flag & 4)) + __popcll(__ballot(flag & 8));
  __shared__ int wave_v[A::kThreads / 64], wave_q[A::kThreads / 64];
  if ((tid & 63) == 0) { wave_v[tid >> 6] = __popcll(ma); wave_q[tid >> 6] = quads; }
  __syncthreads();
  if (tid == 0) {
    int nv = 0, nq = 0;
#pragma unroll
    for (int w = 0; w < A::kThreads / 64; ++w) { nv += wave_v[w]; nq += wave_q[w]; }
    vcount[blockIdx.x] = nv; qcount[blockIdx.x] = nq;
  }
}

// exclusive scans of vcount and qcount [M] in workgroup order; counts = (vertices, faces = 2 * quads), not clamped by any capacity
__global__ __launch_bounds__(kScanThreads) void mesh_scan_kernel(const int* __restrict__ vcount, const int* __restrict__ qcount,
                                                                 int* __restrict__ vbase, int* __restrict__ qbase,
                                                                 int32_t* __restrict__ counts, int M) {
  const int* const cnt[2] = {vcount, qcount};
  int run[2], total[2];
  const ScanChunk c = scan_counts(cnt, M, run, total);
  for (int i = c.lo; i < c.hi; ++i) { vbase[i] = run[0]; run[0] += vcount[i]; qbase[i] = run[1]; run[1] += qcount[i]; }
  if (threadIdx.x == 0) { counts[0] = total[0]; counts[1] = 2 * total[1]; }
}

// LAB: the vertex's label into vlabel as well (pvo_tsdf_mesh_panoptic, pvo_tsdf_sparse_mesh_panoptic)
template <typename A, bool LAB>
__global__ __launch_bounds__(A::kThreads) void mesh_verts_kernel(const A g, const uint8_t* __restrict__ flags, const int* __restrict__ vbase,
                                                                int32_t* __restrict__ vidx, const MeshOut out, const VertexLabels<LAB> lab) {
  const int tid = threadIdx.x;
  typename A::Cell c;
  if (!g.enter(c)) return;                // (the whole workgroup)
  const bool active = c.has && (flags[c.k] & kActive);
  const unsigned long long m = __ballot(active);
  __shared__ int wave_n[A::kThreads / 64];
  if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(m);
  __syncthreads();
  if (!active) return;
  int idx = vbase[blockIdx.x] + lanes_below(m);
  for (int w = 0; w < (tid >> 6); ++w) idx += wave_n[w];
  vidx[c.k] = idx;                        // (also beyond the capacity: the faces name the vertex by its index)
  if (idx >= out.vcap) return;            // written nowhere; the caller sees counts[0] > vcap
  g.locate(c);
  float s[8];
  long long at[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    at[j] = g.corner(c, j);               // (an active cell: all eight exist)
    s[j] = g.v.tsdf[at[j]];
  }
  surface_net_vertex(s, g.v.rgb, at, c.g[0], c.g[1], c.g[2], g.v.ox, g.v.oy, g.v.oz, g.v.voxel, out, idx);
  if constexpr (LAB) lab.vlabel[idx] = surface_net_label(s, lab.label, at);
}

template <typename A>
__global__ __launch_bounds__(A::kThreads) void mesh_faces_kernel(const A g, const uint8_t* __restrict__ flags, const int* __restrict__ qbase,
                                                                const int32_t* __restrict__ vidx, const MeshOut out) {
  const int tid = threadIdx.x;
  typename A::Cell c;
  if (!g.enter(c)) return;                // (the whole workgroup)
  const int flag = c.has ? flags[c.k] : 0;
  // quads are numbered cell by cell, inside a cell by axis: the quads of the lower lanes, whatever their axis, come first
  const unsigned long long mx = __ballot(flag & 2), my = __ballot(flag & 4), mz = __ballot(flag & 8);
  __shared__ int wave_n[A::kThreads / 64];
  if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(mx) + __popcll(my) + __popcll(mz);
  __syncthreads();
  if (!(flag & 14)) return;
  int q = qbase[blockIdx.x] + lanes_below(mx) + lanes_below(my) + lanes_below(mz);
  for (int w = 0; w < (tid >> 6); ++w) q += wave_n[w];
  g.locate(c);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(flag & (2 << a))) continue;
    int eb[3] = {0, 0, 0}, ec[3] = {0, 0, 0};
    eb[(a + 1) % 3] = 1; ec[(a + 2) % 3] = 1;
    // (a quad's four cells are active: they exist)
    const int q0 = vidx[c.k], q1 = vidx[g.neighbour(c, -eb[2], -eb[1], -eb[0])],
              q2 = vidx[g.neighbour(c, -eb[2] - ec[2], -eb[1] - ec[1], -eb[0] - ec[0])], q3 = vidx[g.neighbour(c, -ec[2], -ec[1], -ec[0])];
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

// ------------------------------------------------------------------------------------------------------------ host

// the workspace of a mesh call: per workgroup the two counts and their two bases, per cell the vertex index and the flag byte
struct MeshLayout { size_t vcount, qcount, vbase, qbase, vidx, flags, total; };
inline MeshLayout mesh_layout(size_t groups, size_t cells) {
  using tsdf_volume::aligned;
  MeshLayout L;
  const size_t per = aligned(sizeof(int) * groups);
  L.vcount = 0; L.qcount = per; L.vbase = 2 * per; L.qbase = 3 * per;
  L.vidx = 4 * per;
  L.flags = L.vidx + aligned(sizeof(int32_t) * cells);
  L.total = L.flags + aligned(cells);
  return L;
}

// the four launches over `groups` workgroups of the addresser's cells; p != NULL: the panoptic call
template <typename A>
int mesh_launch(const A g, int groups, const MeshLayout L, void* workspace, const MeshOut out, int32_t* counts,
                const pvo_tsdf_mesh_labels_args* p, hipStream_t s) {
  char* ws = static_cast<char*>(workspace);
  int* vcount = reinterpret_cast<int*>(ws + L.vcount);
  int* qcount = reinterpret_cast<int*>(ws + L.qcount);
  int* vbase = reinterpret_cast<int*>(ws + L.vbase);
  int* qbase = reinterpret_cast<int*>(ws + L.qbase);
  int32_t* vidx = reinterpret_cast<int32_t*>(ws + L.vidx);
  uint8_t* flags = reinterpret_cast<uint8_t*>(ws + L.flags);
  const dim3 grid(static_cast<unsigned>(groups)), block(A::kThreads);
  hipLaunchKernelGGL(mesh_classify_kernel<A>, grid, block, 0, s, g, flags, vcount, qcount);
  PVO_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, vcount, qcount, vbase, qbase, counts, groups);
  PVO_CHECK_LAUNCH();
  if (p)
    hipLaunchKernelGGL((mesh_verts_kernel<A, true>), grid, block, 0, s, g, flags, vbase, vidx, out, VertexLabels<true>{p->label, p->vlabel});
  else
    hipLaunchKernelGGL((mesh_verts_kernel<A, false>), grid, block, 0, s, g, flags, vbase, vidx, out, VertexLabels<false>{});
  PVO_CHECK_LAUNCH();
  hipLaunchKernelGGL(mesh_faces_kernel<A>, grid, block, 0, s, g, flags, qbase, vidx, out);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

// the "no cell" answer of a mesh call: the counts alone
inline int mesh_no_cell(int32_t* counts, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(counts, 0, 2 * sizeof(int32_t), s);
  if (e != hipSuccess) { pvo_note_hip_error(static_cast<int>(e)); return PVO_ELAUNCH; }
  return PVO_OK;
}

}  // namespace
