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
//   integrate  (a) sparse_frames_kernel      one workgroup per slot: the dense call's constants, zfar = max 1/d, the cull's scalars
//              (b) sparse_integrate_kernel   one workgroup per brick, one thread per voxel: cull per chunk of 512 slots, survivors
//                                            compacted in slot order, then the dense kernel's per-(voxel, frame) function
//   mesh       classify / scan / vertices / faces as in tsdf.hip, one workgroup per brick, neighbours through the grid
//   panoptic   (pvo_tsdf_sparse_integrate_panoptic / _mesh_panoptic) the LAB instantiations of sparse_integrate_kernel and
//              sparse_verts_kernel in the same launches, as in tsdf.hip
//
// No atomics anywhere: marks are same-value stores, every index is a function of flags alone, a voxel is one thread's sequential loop.
#include "tsdf_brick_cull.h"

namespace {

constexpr int kB = PVO_TSDF_BRICK;
constexpr int kBrick = kB * kB * kB;  // 512 voxels, one workgroup
constexpr int kBlock = 256;
constexpr int kScanThreads = 1024;
static_assert(kB == 8 && kBrick == 512, "the index arithmetic below shifts by 3 and 6");

// inclusive scan of one value per thread of a 1024-thread workgroup (Hillis-Steele); total = the last thread's
__device__ __forceinline__ int scan_workgroup(int s, int (*buf)[kScanThreads], int& total) {
  const int tid = threadIdx.x;
  int cur = 0;
  buf[0][tid] = s;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < kScanThreads; off <<= 1) {
    buf[cur ^ 1][tid] = buf[cur][tid] + (tid >= off ? buf[cur][tid - off] : 0);
    cur ^= 1;
    __syncthreads();
  }
  const int inc = buf[cur][tid];
  total = buf[cur][kScanThreads - 1];
  __syncthreads();                        // buf is reused by the next scan
  return inc;
}

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

// nbase[i] = bricks held + the new bricks of the workgroups before i (thread t owns a contiguous chunk, map_points.hip's scan);
// bricks[0] = held + new, not clamped by cap
__global__ __launch_bounds__(kScanThreads) void alloc_scan_kernel(const int* __restrict__ acount, const int* __restrict__ ncount,
                                                                  int* __restrict__ nbase, int32_t* __restrict__ bricks, int M) {
  const int tid = threadIdx.x;
  const int chunk = (M + kScanThreads - 1) / kScanThreads;
  const int lo = static_cast<int>(min(static_cast<long long>(tid) * chunk, static_cast<long long>(M))), hi = min(lo + chunk, M);
  __shared__ int buf[2][kScanThreads];
  int sa = 0, sn = 0;
  for (int i = lo; i < hi; ++i) { sa += acount[i]; sn += ncount[i]; }
  int held, fresh;
  scan_workgroup(sa, buf, held);
  int run = held + scan_workgroup(sn, buf, fresh) - sn;
  for (int i = lo; i < hi; ++i) { nbase[i] = run; run += ncount[i]; }
  if (tid == 0) bricks[0] = held + fresh;
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

// ------------------------------------------------------------------------------------------------------------ integrate

// sparse_frames_kernel (per slot: the dense call's constants, zfar, the cull's scalars) and brick_sees_frame (one slot against one
// brick): tsdf_brick_cull.h, shared with the re-integration (tsdf_reintegrate.hip)

// LAB: with the label vote on the caller's label / lconf pools (pvo_tsdf_sparse_integrate_panoptic)
template <bool RGB, bool LAB>
__global__ __launch_bounds__(kBrick) void sparse_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ wsum, float* __restrict__ rgb,
                                                                 const int32_t* __restrict__ coord, const int32_t* __restrict__ bricks,
                                                                 int cap, const float* __restrict__ fc,
                                                                 const float* __restrict__ intrinsics, const Fuse in, int N, float voxel,
                                                                 int32_t* __restrict__ kept, const VoteVolumes<LAB> pan) {
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
  if constexpr (LAB) { a.L = pan.label[i]; a.lc = pan.lconf[i]; }
  __shared__ int list[kBrick];
  __shared__ int wave_n[kBrick / 64];
  int survivors = 0;
  for (int c0 = 0; c0 < N; c0 += kBrick) {
    // stage 1: slot c0 + tid against the brick; the survivors in slot order
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
    // stage 2: the dense kernel's loop over the survivors
    for (int k = 0; k < n; ++k) {
      const int s = __builtin_amdgcn_readfirstlane(list[k]);
      const float* __restrict__ c = fc + static_cast<long long>(kFrameFloats) * s;    // wave-uniform
      if constexpr (LAB) tsdf_fuse_frame<RGB, true>(a, c, __float_as_int(c[12]), xf, yf, zf, true, K, in, HW, plane, pan.maps);
      else tsdf_fuse_frame<RGB>(a, c, __float_as_int(c[12]), xf, yf, zf, true, K, in, HW, plane);
    }
    __syncthreads();                      // list and wave_n are rewritten by the next chunk
  }
  if (kept && tid == 0) kept[slot] = survivors;
  if (a.touched) {
    tsdf[i] = a.T; wsum[i] = a.W;
    if (RGB) { rgb[3 * i] = a.cr; rgb[3 * i + 1] = a.cg; rgb[3 * i + 2] = a.cb; }
    if constexpr (LAB) { pan.label[i] = a.L; pan.lconf[i] = a.lc; }
  }
}

// ------------------------------------------------------------------------------------------------------------ mesh

struct Bricks {
  const int32_t* grid; const int32_t* coord; const int32_t* bricks;
  const float* tsdf; const float* wsum; const float* rgb;
  int gz, gy, gx, cap;
  float ox, oy, oz, voxel, min_weight;
};

// the slots of the 3 x 3 x 3 bricks around brick (bz,by,bx) into nb (LDS), -1 outside the grid; ends with a barrier
__device__ __forceinline__ void load_neighbours(const Bricks g, int bz, int by, int bx, int* nb) {
  const int tid = threadIdx.x;
  if (tid < 27) {
    const int z = bz + tid / 9 - 1, y = by + (tid / 3) % 3 - 1, x = bx + tid % 3 - 1;
    const bool in = z >= 0 && z < g.gz && y >= 0 && y < g.gy && x >= 0 && x < g.gx;
    const int s = in ? g.grid[(static_cast<long long>(z) * g.gy + y) * g.gx + x] : -1;
    nb[tid] = s < g.cap ? s : -1;         // (a slot the pool does not have is no brick)
  }
  __syncthreads();
}

// pool index of the voxel at local (lz,ly,lx), each in [-1, 8], of the brick whose neighbours are nb; -1 in a brick that does not exist
__device__ __forceinline__ long long voxel_at(const int* nb, int lz, int ly, int lx) {
  const int s = nb[((lz >> 3) + 1) * 9 + ((ly >> 3) + 1) * 3 + ((lx >> 3) + 1)];
  return s < 0 ? -1 : static_cast<long long>(s) * kBrick + (((lz & 7) << 6) | ((ly & 7) << 3) | (lx & 7));
}

// all eight corners of the cell at local (lz,ly,lx), each in [-1, 7], valid
__device__ __forceinline__ bool cell_valid(const Bricks g, const int* nb, int lz, int ly, int lx) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long long v = voxel_at(nb, lz + (j >> 2), ly + ((j >> 1) & 1), lx + (j & 1));
    ok = ok && v >= 0 && g.wsum[v >= 0 ? v : 0] >= g.min_weight;
  }
  return ok;
}

__global__ __launch_bounds__(kBrick) void sparse_classify_kernel(const Bricks g, uint8_t* __restrict__ flags, int* __restrict__ vcount,
                                                                int* __restrict__ qcount) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  if (slot >= min(g.bricks[0], g.cap)) {  // (the whole workgroup) a slot not in use has no cell
    if (tid == 0) { vcount[slot] = 0; qcount[slot] = 0; }
    return;
  }
  __shared__ int nb[27];
  const int bz = g.coord[3 * slot], by = g.coord[3 * slot + 1], bx = g.coord[3 * slot + 2];
  load_neighbours(g, bz, by, bx, nb);
  const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;
  int flag = 0;
  bool valid = true;
  int inside = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long long v = voxel_at(nb, lz + (j >> 2), ly + ((j >> 1) & 1), lx + (j & 1));
    valid = valid && v >= 0 && g.wsum[v >= 0 ? v : 0] >= g.min_weight;
    inside |= (g.tsdf[v >= 0 ? v : 0] < 0.0f ? 1 : 0) << j;
  }
  if (valid && inside != 0 && inside != 255) {
    flag = kActive | ((inside & 1) ? kInsideA : 0);
    const int c[3] = {kB * bx + lx, kB * by + ly, kB * bz + lz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int b = (a + 1) % 3, cc = (a + 2) % 3;
      if ((((inside >> (1 << a)) ^ inside) & 1) == 0 || c[b] < 1 || c[cc] < 1) continue;
      // the three other cells around the edge share it, so they are not all on one side: active = all corners valid
      int eb[3] = {0, 0, 0}, ec[3] = {0, 0, 0};
      eb[b] = 1; ec[cc] = 1;
      if (cell_valid(g, nb, lz - eb[2], ly - eb[1], lx - eb[0]) && cell_valid(g, nb, lz - eb[2] - ec[2], ly - eb[1] - ec[1], lx - eb[0] - ec[0]) &&
          cell_valid(g, nb, lz - ec[2], ly - ec[1], lx - ec[0]))
        flag |= 2 << a;
    }
  }
  flags[static_cast<long long>(slot) * kBrick + tid] = static_cast<uint8_t>(flag);
  const unsigned long long ma = __ballot(flag & kActive);
  const int quads = __popcll(__ballot(flag & 2)) + __popcll(__ballot(flag & 4)) + __popcll(__ballot(flag & 8));
  __shared__ int wave_v[kBrick / 64], wave_q[kBrick / 64];
  if ((tid & 63) == 0) { wave_v[tid >> 6] = __popcll(ma); wave_q[tid >> 6] = quads; }
  __syncthreads();
  if (tid == 0) {
    int v = 0, q = 0;
#pragma unroll
    for (int w = 0; w < kBrick / 64; ++w) { v += wave_v[w]; q += wave_q[w]; }
    vcount[slot] = v; qcount[slot] = q;
  }
}

// exclusive scans of vcount and qcount [M] in slot order; counts = (vertices, faces = 2 * quads), not clamped by any capacity
__global__ __launch_bounds__(kScanThreads) void sparse_scan_kernel(const int* __restrict__ vcount, const int* __restrict__ qcount,
                                                                   int* __restrict__ vbase, int* __restrict__ qbase,
                                                                   int32_t* __restrict__ counts, int M) {
  const int tid = threadIdx.x;
  const int chunk = (M + kScanThreads - 1) / kScanThreads;
  const int lo = static_cast<int>(min(static_cast<long long>(tid) * chunk, static_cast<long long>(M))), hi = min(lo + chunk, M);
  __shared__ int buf[2][kScanThreads];
  int sv = 0, sq = 0;
  for (int i = lo; i < hi; ++i) { sv += vcount[i]; sq += qcount[i]; }
  int nv, nq;
  int rv = scan_workgroup(sv, buf, nv) - sv;
  int rq = scan_workgroup(sq, buf, nq) - sq;
  for (int i = lo; i < hi; ++i) { vbase[i] = rv; rv += vcount[i]; qbase[i] = rq; rq += qcount[i]; }
  if (tid == 0) { counts[0] = nv; counts[1] = 2 * nq; }
}

// LAB: the vertex's label into vlabel as well (pvo_tsdf_sparse_mesh_panoptic)
template <bool LAB>
__global__ __launch_bounds__(kBrick) void sparse_verts_kernel(const Bricks g, const uint8_t* __restrict__ flags, const int* __restrict__ vbase,
                                                             int32_t* __restrict__ vidx, const MeshOut out, const VertexLabels<LAB> lab) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  if (slot >= min(g.bricks[0], g.cap)) return;          // (the whole workgroup)
  __shared__ int nb[27];
  const int bz = g.coord[3 * slot], by = g.coord[3 * slot + 1], bx = g.coord[3 * slot + 2];
  load_neighbours(g, bz, by, bx, nb);
  const long long k = static_cast<long long>(slot) * kBrick + tid;
  const bool active = flags[k] & kActive;
  const unsigned long long m = __ballot(active);
  __shared__ int wave_n[kBrick / 64];
  if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(m);
  __syncthreads();
  if (!active) return;
  int idx = vbase[slot] + lanes_below(m);
  for (int w = 0; w < (tid >> 6); ++w) idx += wave_n[w];
  vidx[k] = idx;                          // (also beyond the capacity: the faces name the vertex by its index)
  if (idx >= out.vcap) return;            // written nowhere; the caller sees counts[0] > vcap
  const int lx = tid & 7, ly = (tid >> 3) & 7, lz = tid >> 6;
  float s[8];
  long long at[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    at[j] = voxel_at(nb, lz + (j >> 2), ly + ((j >> 1) & 1), lx + (j & 1));     // (an active cell: all eight exist)
    s[j] = g.tsdf[at[j]];
  }
  surface_net_vertex(s, g.rgb, at, kB * bx + lx, kB * by + ly, kB * bz + lz, g.ox, g.oy, g.oz, g.voxel, out, idx);
  if constexpr (LAB) lab.vlabel[idx] = surface_net_label(s, lab.label, at);
}

__global__ __launch_bounds__(kBrick) void sparse_faces_kernel(const Bricks g, const uint8_t* __restrict__ flags, const int* __restrict__ qbase,
                                                             const int32_t* __restrict__ vidx, const MeshOut out) {
  const int slot = blockIdx.x, tid = threadIdx.x;
  if (slot >= min(g.bricks[0], g.cap)) return;          // (the whole workgroup)
  __shared__ int nb[27];
  const int bz = g.coord[3 * slot], by = g.coord[3 * slot + 1], bx = g.coord[3 * slot + 2];
  load_neighbours(g, bz, by, bx, nb);
  const long long k = static_cast<long long>(slot) * kBrick + tid;
  const int flag = flags[k];
  // quads are numbered cell by cell, inside a cell by axis: the quads of the lower lanes, whatever their axis, come first
  const unsigned long long mx = __ballot(flag & 2), my = __ballot(flag & 4), mz = __ballot(flag & 8);
  __shared__ int wave_n[kBrick / 64];
  if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(mx) + __popcll(my) + __popcll(mz);
  __syncthreads();
  if (!(flag & 14)) return;
  int q = qbase[slot] + lanes_below(mx) + lanes_below(my) + lanes_below(mz);
  for (int w = 0; w < (tid >> 6); ++w) q += wave_n[w];
  const int l[3] = {tid & 7, (tid >> 3) & 7, tid >> 6};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(flag & (2 << a))) continue;
    int eb[3] = {0, 0, 0}, ec[3] = {0, 0, 0};
    eb[(a + 1) % 3] = 1; ec[(a + 2) % 3] = 1;
    // (a quad's four cells are active: their bricks exist)
    const int q0 = vidx[k], q1 = vidx[voxel_at(nb, l[2] - eb[2], l[1] - eb[1], l[0] - eb[0])],
              q2 = vidx[voxel_at(nb, l[2] - eb[2] - ec[2], l[1] - eb[1] - ec[1], l[0] - eb[0] - ec[0])],
              q3 = vidx[voxel_at(nb, l[2] - ec[2], l[1] - ec[1], l[0] - ec[0])];
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

constexpr size_t kAlign = 256;
inline size_t aligned(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }
inline bool finite_f(float v) { return v - v == 0.0f; }

constexpr int kMaxBricksPerAxis = (1 << 21) / kB;
inline bool world_ok(int gz, int gy, int gx, int cap) {
  return gz >= 0 && gy >= 0 && gx >= 0 && gz <= kMaxBricksPerAxis && gy <= kMaxBricksPerAxis && gx <= kMaxBricksPerAxis &&
         static_cast<long long>(gz) * gy < (1ll << 31) && static_cast<long long>(gz) * gy * gx < (1ll << 31) && cap >= 0 &&
         static_cast<long long>(cap) * kBrick < (1ll << 31);
}

struct AllocLayout { size_t marks, acount, ncount, nbase, frames, total; long long G, blocks; };
inline AllocLayout alloc_layout(int gz, int gy, int gx, int N) {
  AllocLayout L;
  L.G = static_cast<long long>(gz) * gy * gx;
  L.blocks = (L.G + kBlock - 1) / kBlock;
  const size_t per = aligned(sizeof(int) * L.blocks);
  L.marks = 0;
  L.acount = aligned(L.G); L.ncount = L.acount + per; L.nbase = L.ncount + per;
  L.frames = L.nbase + per;
  L.total = L.frames + aligned(sizeof(float) * kFrameFloats * static_cast<size_t>(N > 0 ? N : 0));
  return L;
}

struct SparseMeshLayout { size_t vcount, qcount, vbase, qbase, vidx, flags, total; };
inline SparseMeshLayout sparse_mesh_layout(int cap) {
  SparseMeshLayout L;
  const size_t per = aligned(sizeof(int) * static_cast<size_t>(cap));
  L.vcount = 0; L.qcount = per; L.vbase = 2 * per; L.qbase = 3 * per;
  L.vidx = 4 * per;
  L.flags = L.vidx + aligned(sizeof(int32_t) * static_cast<size_t>(cap) * kBrick);
  L.total = L.flags + aligned(static_cast<size_t>(cap) * kBrick);
  return L;
}

}  // namespace

#define PVO_REQ(c) do { if (!(c)) return PVO_EINVAL; } while (0)

extern "C" size_t pvo_tsdf_sparse_allocate_args_size(void) { return sizeof(pvo_tsdf_sparse_allocate_args); }
extern "C" size_t pvo_tsdf_sparse_integrate_args_size(void) { return sizeof(pvo_tsdf_sparse_integrate_args); }
extern "C" size_t pvo_tsdf_sparse_mesh_args_size(void) { return sizeof(pvo_tsdf_sparse_mesh_args); }

extern "C" size_t pvo_tsdf_sparse_allocate_workspace_bytes(int gz, int gy, int gx, int N) {
  if (!world_ok(gz, gy, gx, 0) || static_cast<long long>(gz) * gy * gx == 0 || N <= 0) return 0;
  return alloc_layout(gz, gy, gx, N).total;
}

extern "C" size_t pvo_tsdf_sparse_integrate_workspace_bytes(int N) {
  return N <= 0 ? 0 : aligned(sizeof(float) * kFrameFloats * static_cast<size_t>(N));
}

extern "C" size_t pvo_tsdf_sparse_mesh_workspace_bytes(int cap) {
  if (cap <= 0 || !world_ok(0, 0, 0, cap)) return 0;
  return sparse_mesh_layout(cap).total;
}

extern "C" int pvo_tsdf_sparse_allocate(const pvo_tsdf_sparse_allocate_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PVO_REQ(a);
  PVO_REQ(world_ok(a->gz, a->gy, a->gx, a->cap));
  PVO_REQ(a->N >= 0 && a->nframes >= 0 && a->ht >= 0 && a->wd >= 0 && static_cast<long long>(a->ht) * a->wd < (1ll << 31));
  PVO_REQ(a->voxel > 0.0f && finite_f(a->voxel) && a->trunc > 0.0f && finite_f(a->trunc) && a->trunc / a->voxel <= 4096.0f);
  PVO_REQ(a->z_near >= 0.0f && finite_f(a->z_near) && a->margin >= 0.0f && a->margin <= static_cast<float>(kB));
  PVO_REQ(finite_f(a->origin[0]) && finite_f(a->origin[1]) && finite_f(a->origin[2]));
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
  if (panoptic) {
    PVO_REQ(p && p->label && p->lconf && p->labels && p->label_div >= 1);
    PVO_REQ(static_cast<long long>(p->lh) * p->label_div >= a->ht && static_cast<long long>(p->lw) * p->label_div >= a->wd);
  }
  PVO_REQ(world_ok(a->gz, a->gy, a->gx, a->cap));
  PVO_REQ(a->N >= 0 && a->nframes >= 0 && a->ht >= 0 && a->wd >= 0 && static_cast<long long>(a->ht) * a->wd < (1ll << 31));
  PVO_REQ(a->voxel > 0.0f && finite_f(a->voxel) && a->trunc > 0.0f && finite_f(a->trunc));
  PVO_REQ(a->z_near >= 0.0f && finite_f(a->z_near) && a->w_max >= 0.0f && finite_f(a->w_max));
  PVO_REQ(finite_f(a->origin[0]) && finite_f(a->origin[1]) && finite_f(a->origin[2]));
  if (a->cap == 0 || a->N == 0 || a->ht * a->wd == 0) return PVO_OK;      // nothing to fuse
  PVO_REQ(a->tsdf && a->wsum && a->coord && a->bricks && a->poses && a->disps && a->intrinsics && a->ix);
  PVO_REQ(!a->rgb || a->images);                 // a colour pool needs the images
  if (a->images) {
    PVO_REQ(a->img_stride >= 1 && a->img_offset >= 0 && a->IH > 0 && a->IW > 0);
    PVO_REQ(static_cast<long long>(a->img_stride) * (a->ht - 1) + a->img_offset < a->IH);
    PVO_REQ(static_cast<long long>(a->img_stride) * (a->wd - 1) + a->img_offset < a->IW);
  }
  if (!workspace || workspace_bytes < pvo_tsdf_sparse_integrate_workspace_bytes(a->N)) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 15));
  hipStream_t s = pvo_stream(stream);
  float* fc = static_cast<float*>(workspace);
  const Vol vol = {a->origin[0], a->origin[1], a->origin[2], a->voxel};
  hipLaunchKernelGGL(sparse_frames_kernel, dim3(a->N), dim3(kCullBlock), 0, s, a->poses, a->ix, a->disps, a->weight, fc, a->nframes,
                     static_cast<long long>(a->ht) * a->wd, vol);
  PVO_CHECK_LAUNCH();
  const Fuse in = {a->disps, a->weight, a->images, a->ht, a->wd, a->IH, a->IW, a->img_stride, a->img_offset, a->trunc, a->z_near, a->w_max};
  if (panoptic) {
    const VoteVolumes<true> pan = {p->label, p->lconf, {p->labels, p->lh, p->lw, p->label_div}};
    if (a->rgb)
      hipLaunchKernelGGL((sparse_integrate_kernel<true, true>), dim3(a->cap), dim3(kBrick), 0, s, a->tsdf, a->wsum, a->rgb, a->coord, a->bricks,
                         a->cap, fc, a->intrinsics, in, a->N, a->voxel, a->kept, pan);
    else
      hipLaunchKernelGGL((sparse_integrate_kernel<false, true>), dim3(a->cap), dim3(kBrick), 0, s, a->tsdf, a->wsum, a->rgb, a->coord, a->bricks,
                         a->cap, fc, a->intrinsics, in, a->N, a->voxel, a->kept, pan);
  } else if (a->rgb)
    hipLaunchKernelGGL((sparse_integrate_kernel<true, false>), dim3(a->cap), dim3(kBrick), 0, s, a->tsdf, a->wsum, a->rgb, a->coord, a->bricks,
                       a->cap, fc, a->intrinsics, in, a->N, a->voxel, a->kept, VoteVolumes<false>{});
  else
    hipLaunchKernelGGL((sparse_integrate_kernel<false, false>), dim3(a->cap), dim3(kBrick), 0, s, a->tsdf, a->wsum, a->rgb, a->coord, a->bricks,
                       a->cap, fc, a->intrinsics, in, a->N, a->voxel, a->kept, VoteVolumes<false>{});
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
  if (panoptic) PVO_REQ(p && p->label && (a->vcap == 0 || p->vlabel));
  PVO_REQ(world_ok(a->gz, a->gy, a->gx, a->cap));
  PVO_REQ(a->voxel > 0.0f && finite_f(a->voxel) && a->min_weight == a->min_weight);
  PVO_REQ(finite_f(a->origin[0]) && finite_f(a->origin[1]) && finite_f(a->origin[2]));
  PVO_REQ(a->vcap >= 0 && a->fcap >= 0 && a->counts && a->bricks);
  PVO_REQ(!((reinterpret_cast<uintptr_t>(a->rgba) & 3)));
  hipStream_t s = pvo_stream(stream);
  if (a->cap == 0 || static_cast<long long>(a->gz) * a->gy * a->gx == 0) {     // no brick: the counts alone
    const hipError_t e = hipMemsetAsync(a->counts, 0, 2 * sizeof(int32_t), s);
    if (e != hipSuccess) { pvo_note_hip_error(static_cast<int>(e)); return PVO_ELAUNCH; }
    return PVO_OK;
  }
  PVO_REQ(a->grid && a->coord && a->tsdf && a->wsum);
  PVO_REQ((a->vcap == 0 || a->verts) && (a->fcap == 0 || a->faces));
  const SparseMeshLayout L = sparse_mesh_layout(a->cap);
  if (!workspace || workspace_bytes < L.total) return PVO_EWORKSPACE;
  PVO_REQ(!(reinterpret_cast<uintptr_t>(workspace) & 7));
  char* ws = static_cast<char*>(workspace);
  int* vcount = reinterpret_cast<int*>(ws + L.vcount);
  int* qcount = reinterpret_cast<int*>(ws + L.qcount);
  int* vbase = reinterpret_cast<int*>(ws + L.vbase);
  int* qbase = reinterpret_cast<int*>(ws + L.qbase);
  int32_t* vidx = reinterpret_cast<int32_t*>(ws + L.vidx);
  uint8_t* flags = reinterpret_cast<uint8_t*>(ws + L.flags);
  const Bricks g = {a->grid, a->coord, a->bricks, a->tsdf, a->wsum, a->rgb, a->gz, a->gy, a->gx, a->cap,
                    a->origin[0], a->origin[1], a->origin[2], a->voxel, a->min_weight};
  const MeshOut out = {a->verts, a->normals, a->rgba, a->faces, a->vcap, a->fcap};
  const dim3 grid(static_cast<unsigned>(a->cap));
  hipLaunchKernelGGL(sparse_classify_kernel, grid, dim3(kBrick), 0, s, g, flags, vcount, qcount);
  PVO_CHECK_LAUNCH();
  hipLaunchKernelGGL(sparse_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, vcount, qcount, vbase, qbase, a->counts, a->cap);
  PVO_CHECK_LAUNCH();
  if (panoptic)
    hipLaunchKernelGGL(sparse_verts_kernel<true>, grid, dim3(kBrick), 0, s, g, flags, vbase, vidx, out, VertexLabels<true>{p->label, p->vlabel});
  else
    hipLaunchKernelGGL(sparse_verts_kernel<false>, grid, dim3(kBrick), 0, s, g, flags, vbase, vidx, out, VertexLabels<false>{});
  PVO_CHECK_LAUNCH();
  hipLaunchKernelGGL(sparse_faces_kernel, grid, dim3(kBrick), 0, s, g, flags, qbase, vidx, out);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

}  // namespace

extern "C" int pvo_tsdf_sparse_mesh(const pvo_tsdf_sparse_mesh_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  return sparse_mesh_impl(a, nullptr, false, workspace, workspace_bytes, stream);
}

extern "C" int pvo_tsdf_sparse_mesh_panoptic(const pvo_tsdf_sparse_mesh_args* a, const pvo_tsdf_mesh_labels_args* p, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  return sparse_mesh_impl(a, p, true, workspace, workspace_bytes, stream);
}
