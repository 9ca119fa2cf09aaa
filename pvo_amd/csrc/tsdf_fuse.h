// tsdf_fuse.h — the arithmetic the dense volume (tsdf.hip) and the brick volume (tsdf_sparse.hip) share: a slot's pre-multiplied frame
// constants, a voxel's load and store, and the update of one voxel by one frame (in, and out again for the re-integration).  Each is
// ONE inline function, called by ONE kernel body (below) that sees either volume through a walker, so a voxel of a brick ends with
// the bytes the dense kernel leaves at that voxel (tests/test_tsdf_sparse_gpu.py holds the two against each other).  The surface-nets
// vertex of a cell: tsdf_mesh.h.
#pragma once
#include "depth_vote.h"

constexpr int kFrameFloats = 16;      // per slot: A[9] row-major, b[3], frame id (as int bits), [13..15] for the caller (tsdf.hip: unused)

struct Vol { float ox, oy, oz, voxel; };

// o[0..12] of frame f (in [0, nframes)): voxel * R,  R origin + t,  the frame id
__device__ __forceinline__ void tsdf_frame_constants(const float* __restrict__ poses, long long f, const Vol vol, float* __restrict__ o) {
  const Pose G = load_pose(poses + 7 * f);
  const Quat q = G.q;
  // R(q) of the quaternion as stored (the matrix map_points.hip transposes)
  const float r[9] = {1.0f - 2.0f * (q.y * q.y + q.z * q.z), 2.0f * (q.x * q.y - q.z * q.w), 2.0f * (q.x * q.z + q.y * q.w),
                      2.0f * (q.x * q.y + q.z * q.w), 1.0f - 2.0f * (q.x * q.x + q.z * q.z), 2.0f * (q.y * q.z - q.x * q.w),
                      2.0f * (q.x * q.z - q.y * q.w), 2.0f * (q.y * q.z + q.x * q.w), 1.0f - 2.0f * (q.x * q.x + q.y * q.y)};
#pragma unroll
  for (int k = 0; k < 9; ++k) o[k] = vol.voxel * r[k];
  o[9] = (r[0] * vol.ox + r[1] * vol.oy) + r[2] * vol.oz + G.t.x;
  o[10] = (r[3] * vol.ox + r[4] * vol.oy) + r[5] * vol.oz + G.t.y;
  o[11] = (r[6] * vol.ox + r[7] * vol.oy) + r[8] * vol.oz + G.t.z;
  o[12] = __int_as_float(static_cast<int>(f));
}

struct Fuse {
  const float* disps; const float* weight; const uint8_t* images;
  int ht, wd, IH, IW, stride, offset;
  float trunc, z_near, w_max;
};

struct Voxel { float T, W, cr, cg, cb; bool touched; int32_t L; float lc; };     // (L, lc: the label vote, LAB only)

// the panoptic extension (pvo_tsdf_panoptic_args): per-frame label maps [nframes,lh,lw] read at (vi / div, ui / div)
struct LabelMaps { const int32_t* labels; int lh, lw, div; };

// what a panoptic kernel takes beyond the plain one's arguments, as its LAST argument: nothing without LAB, so that the plain
// instantiations keep their argument layout and their code
template <bool LAB> struct VoteVolumes {};
template <> struct VoteVolumes<true> { int32_t* label; float* lconf; LabelMaps maps; };      // label, lconf: shaped like tsdf

// the voxel at pool index i as a kernel holds it in registers (an empty one where !live), and back where a frame touched it
template <bool RGB, bool LAB>
__device__ __forceinline__ Voxel load_voxel(const float* __restrict__ tsdf, const float* __restrict__ wsum, const float* __restrict__ rgb,
                                            const VoteVolumes<LAB> pan, long long i, bool live) {
  Voxel a = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, false, 0, 0.0f};
  if (live) {
    a.T = tsdf[i]; a.W = wsum[i];
    if (RGB) { a.cr = rgb[3 * i]; a.cg = rgb[3 * i + 1]; a.cb = rgb[3 * i + 2]; }
    if constexpr (LAB) { a.L = pan.label[i]; a.lc = pan.lconf[i]; }
  }
  return a;
}

template <bool RGB, bool LAB>
__device__ __forceinline__ void store_voxel(const Voxel a, float* __restrict__ tsdf, float* __restrict__ wsum, float* __restrict__ rgb,
                                            const VoteVolumes<LAB> pan, long long i) {
  if (!a.touched) return;                 // (only a live voxel can be)
  tsdf[i] = a.T; wsum[i] = a.W;
  if (RGB) { rgb[3 * i] = a.cr; rgb[3 * i + 1] = a.cg; rgb[3 * i + 2] = a.cb; }
  if constexpr (LAB) { pan.label[i] = a.L; pan.lconf[i] = a.lc; }
}

// frame f (>= 0, with the slot's constants c) applied to the voxel whose INTEGER index is (xf, yf, zf): the contract's sequence of
// include/pvo_hip.h pvo_tsdf_integrate, one test after the other.  LAB: the contribution also casts its pixel's label into the
// voxel's weighted Boyer-Moore vote (pvo_tsdf_integrate_panoptic); without it `lab` is not read and the code is what it was
template <bool RGB, bool LAB = false>
__device__ __forceinline__ void tsdf_fuse_frame(Voxel& a, const float* __restrict__ c, int f, float xf, float yf, float zf, bool live,
                                                const Intr K, const Fuse in, long long HW, long long plane,
                                                const LabelMaps lab = LabelMaps{nullptr, 0, 0, 1}) {
  const float zc = c[6] * xf + c[7] * yf + c[8] * zf + c[11];
  const float xc = c[0] * xf + c[1] * yf + c[2] * zf + c[9];
  const float yc = c[3] * xf + c[4] * yf + c[5] * zf + c[10];
  const float u = K.fx * (xc / zc) + K.cx, v = K.fy * (yc / zc) + K.cy;
  const int ui = pvo_floor_to_int(u + 0.5f), vi = pvo_floor_to_int(v + 0.5f);       // (saturating, NaN -> 0)
  const bool hit = live && zc > in.z_near && ui >= 0 && ui < in.wd && vi >= 0 && vi < in.ht;
  if (!hit) return;                                    // (a wave without a hit branches over the gathers)
  const long long pix = f * HW + static_cast<long long>(vi) * in.wd + ui;
  const float d = in.disps[pix];
  const float w = in.weight ? in.weight[pix] : 1.0f;
  if (!(d > 0.0f && d < __builtin_inff() && w > 0.0f && w < __builtin_inff())) return;   // (NaN fails every comparison)
  const float sdf = 1.0f / d - zc;
  if (sdf < -in.trunc) return;
  const float val = fminf(1.0f, sdf / in.trunc);
  const float Wn = a.W + w;
  a.T = (a.T * a.W + val * w) / Wn;
  if (RGB) {                                           // BGR planes -> RGB
    const uint8_t* im = in.images + 3 * plane * f + static_cast<long long>(in.stride * vi + in.offset) * in.IW + (in.stride * ui + in.offset);
    a.cr = (a.cr * a.W + static_cast<float>(im[2 * plane]) * w) / Wn;
    a.cg = (a.cg * a.W + static_cast<float>(im[plane]) * w) / Wn;
    a.cb = (a.cb * a.W + static_cast<float>(im[0]) * w) / Wn;
  }
  a.W = (in.w_max > 0.0f && Wn > in.w_max) ? in.w_max : Wn;
  a.touched = true;
  if (LAB) {
    if (!(sdf <= in.trunc)) return;                      // free space in front of a surface never votes
    const int32_t L = lab.labels[(static_cast<long long>(f) * lab.lh + vi / lab.div) * lab.lw + ui / lab.div];
    if (L <= 0) return;                                  // no segment
    if (a.L == L) a.lc = a.lc + w;
    else if (a.lc < w) { a.L = L; a.lc = w - a.lc; }
    else a.lc = a.lc - w;
    if (in.w_max > 0.0f && a.lc > in.w_max) a.lc = in.w_max;
  }
}

// ------------------------------------------------------------------------------------------------------------ de-integration

struct Observation { float val, w, cr, cg, cb; };

// what frame f (>= 0, with the slot's constants c) contributes to the voxel (xf, yf, zf) under the operands of `in`: tsdf_fuse_frame's
// tests in its order.  false: the pair contributes nothing (and `o` is not written)
template <bool RGB>
__device__ __forceinline__ bool tsdf_observe(Observation& o, const float* __restrict__ c, int f, float xf, float yf, float zf, bool live,
                                             const Intr K, const Fuse in, long long HW, long long plane) {
  const float zc = c[6] * xf + c[7] * yf + c[8] * zf + c[11];
  const float xc = c[0] * xf + c[1] * yf + c[2] * zf + c[9];
  const float yc = c[3] * xf + c[4] * yf + c[5] * zf + c[10];
  const float u = K.fx * (xc / zc) + K.cx, v = K.fy * (yc / zc) + K.cy;
  const int ui = pvo_floor_to_int(u + 0.5f), vi = pvo_floor_to_int(v + 0.5f);       // (saturating, NaN -> 0)
  const bool hit = live && zc > in.z_near && ui >= 0 && ui < in.wd && vi >= 0 && vi < in.ht;
  if (!hit) return false;                              // (a wave without a hit branches over the gathers)
  const long long pix = f * HW + static_cast<long long>(vi) * in.wd + ui;
  const float d = in.disps[pix];
  const float w = in.weight ? in.weight[pix] : 1.0f;
  if (!(d > 0.0f && d < __builtin_inff() && w > 0.0f && w < __builtin_inff())) return false;   // (NaN fails every comparison)
  const float sdf = 1.0f / d - zc;
  if (sdf < -in.trunc) return false;
  o.val = fminf(1.0f, sdf / in.trunc);
  o.w = w;
  if (RGB) {                                           // BGR planes -> RGB
    const uint8_t* im = in.images + 3 * plane * f + static_cast<long long>(in.stride * vi + in.offset) * in.IW + (in.stride * ui + in.offset);
    o.cr = static_cast<float>(im[2 * plane]); o.cg = static_cast<float>(im[plane]); o.cb = static_cast<float>(im[0]);
  }
  return true;
}

// frame f as `in` holds it taken OUT of the voxel's running average (pvo_tsdf_reintegrate's REMOVE step): Wn = W - w; at or below
// w_floor the voxel becomes empty, otherwise the average without the observation, clamped to its range.  in.w_max plays no part
template <bool RGB>
__device__ __forceinline__ void tsdf_unfuse_frame(Voxel& a, const float* __restrict__ c, int f, float xf, float yf, float zf, bool live,
                                                  const Intr K, const Fuse in, long long HW, long long plane, float w_floor) {
  Observation o;
  if (!tsdf_observe<RGB>(o, c, f, xf, yf, zf, live, K, in, HW, plane)) return;
  const float Wn = a.W - o.w;
  a.touched = true;
  if (!(Wn > w_floor)) {                               // nothing left that the roundings of W have not eaten
    a.T = 0.0f; a.W = 0.0f; a.cr = 0.0f; a.cg = 0.0f; a.cb = 0.0f;
    return;
  }
  a.T = fminf(1.0f, fmaxf(-1.0f, (a.T * a.W - o.val * o.w) / Wn));
  if (RGB) {
    a.cr = fminf(255.0f, fmaxf(0.0f, (a.cr * a.W - o.cr * o.w) / Wn));
    a.cg = fminf(255.0f, fmaxf(0.0f, (a.cg * a.W - o.cg * o.w) / Wn));
    a.cb = fminf(255.0f, fmaxf(0.0f, (a.cb * a.W - o.cb * o.w) / Wn));
  }
  a.W = Wn;
}

// ------------------------------------------------------------------------------------------------------------ the voxel walk
//
// ONE kernel body each for fusion and re-integration: it loads its voxel, runs its frame loops and stores the voxel.  A WALKER, the
// kernel's first argument, says which voxel a thread owns and which slots of a frame table reach it:
//   enter(t)                         false = the WHOLE workgroup has no voxel; else t.i = the pool index, t.live = the thread has a voxel
//   locate(t)                        (t.xf, t.yf, t.zf) = the voxel's global integer index as floats, and what for_each_frame needs; called
//                                    AFTER the voxel's loads are issued, so that they fly while the brick's coordinates are fetched
//   for_each_frame(t, fc, N, K, in, apply)   apply(c, f) for the slots of fc [N] that may reach the voxel, in slot order; returns the
//                                    number of slots kept for the workgroup (0 where nothing is culled)
//   keep(n)                          the workgroup's count of kept slots, where the caller asked for it
//   kThreads                         the workgroup, and the kernel's __launch_bounds__
// DenseWalk (tsdf_dense_walk.h): raster index over [nz,ny,nx], every slot with f >= 0.  BrickWalk (tsdf_brick_cull.h): one workgroup
// per brick in use, the slots culled per brick.  The slot constants are wave-uniform loads either way.

namespace {

// the frame loop runs inside, so the volume is read and written once per call whatever N is.  LAB: with the label vote on the
// caller's label / lconf volumes, the kernel's last argument (empty without LAB, so the plain instantiations keep their code)
template <typename W, bool RGB, bool LAB>
__global__ __launch_bounds__(W::kThreads) void tsdf_integrate_kernel(const W w, float* __restrict__ tsdf, float* __restrict__ wsum,
                                                                    float* __restrict__ rgb, const float* __restrict__ fc,
                                                                    const float* __restrict__ intrinsics, const Fuse in, int N,
                                                                    const VoteVolumes<LAB> pan) {
  typename W::Thread t;
  if (!w.enter(t)) return;                // (the whole workgroup)
  const Intr K = load_intr(intrinsics);
  const long long HW = static_cast<long long>(in.ht) * in.wd;
  const long long plane = static_cast<long long>(in.IH) * in.IW;
  Voxel a = load_voxel<RGB, LAB>(tsdf, wsum, rgb, pan, t.i, t.live);
  w.locate(t);
  const int n = w.for_each_frame(t, fc, N, K, in, [&](const float* __restrict__ c, int f) {
    if constexpr (LAB) tsdf_fuse_frame<RGB, true>(a, c, f, t.xf, t.yf, t.zf, t.live, K, in, HW, plane, pan.maps);
    else tsdf_fuse_frame<RGB>(a, c, f, t.xf, t.yf, t.zf, t.live, K, in, HW, plane);
  });
  w.keep(n);
  store_voxel<RGB, LAB>(a, tsdf, wsum, rgb, pan, t.i);
}

// the REMOVE slots of fc_old [N_old] in order (tsdf_unfuse_frame under in_old), then the ADD slots of fc [N] in order (tsdf_fuse_frame
// under in); keep: both sets summed
template <typename W, bool RGB>
__global__ __launch_bounds__(W::kThreads) void tsdf_reintegrate_kernel(const W w, float* __restrict__ tsdf, float* __restrict__ wsum,
                                                                      float* __restrict__ rgb, const float* __restrict__ fc_old,
                                                                      const float* __restrict__ fc, const float* __restrict__ intrinsics,
                                                                      const Fuse in_old, const Fuse in, int N_old, int N, float w_floor) {
  typename W::Thread t;
  if (!w.enter(t)) return;                // (the whole workgroup)
  const Intr K = load_intr(intrinsics);
  const long long HW = static_cast<long long>(in.ht) * in.wd;
  const long long plane = static_cast<long long>(in.IH) * in.IW;
  const VoteVolumes<false> none = {};
  Voxel a = load_voxel<RGB, false>(tsdf, wsum, rgb, none, t.i, t.live);
  w.locate(t);
  int n = w.for_each_frame(t, fc_old, N_old, K, in_old, [&](const float* __restrict__ c, int f) {
    tsdf_unfuse_frame<RGB>(a, c, f, t.xf, t.yf, t.zf, t.live, K, in_old, HW, plane, w_floor);
  });
  n += w.for_each_frame(t, fc, N, K, in, [&](const float* __restrict__ c, int f) {
    tsdf_fuse_frame<RGB>(a, c, f, t.xf, t.yf, t.zf, t.live, K, in, HW, plane);
  });
  w.keep(n);
  store_voxel<RGB, false>(a, tsdf, wsum, rgb, none, t.i);
}

template <bool LAB>
VoteVolumes<LAB> vote_volumes(const pvo_tsdf_panoptic_args* p) {
  if constexpr (LAB) return {p->label, p->lconf, {p->labels, p->lh, p->lw, p->label_div}};
  else return {};
}

// the operands of a fusion as the kernels take them, from either argument struct; disps / weight: the set's own
template <typename Args>
Fuse fuse_operands(const Args* a, const float* disps, const float* weight) {
  return {disps, weight, a->images, a->ht, a->wd, a->IH, a->IW, a->img_stride, a->img_offset, a->trunc, a->z_near, a->w_max};
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------ labels of a cell

// label of the vertex of the cell with corner values s[j]: the label of the corner with the smallest |tsdf| among the corners that
// have one (> 0), ties to the lowest j, 0 without any; comparisons only (pvo_tsdf_mesh_panoptic)
__device__ __forceinline__ int32_t surface_net_label(const float (&s)[8], const int32_t* __restrict__ label, const long long (&at)[8]) {
  int32_t best = 0;
  float dist = 0.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int32_t L = label[at[j]];
    const float d = fabsf(s[j]);
    if (L > 0 && (best == 0 || d < dist)) { best = L; dist = d; }
  }
  return best;
}
