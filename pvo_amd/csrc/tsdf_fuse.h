// tsdf_fuse.h — the arithmetic the dense volume (tsdf.hip) and the brick volume (tsdf_sparse.hip) share: a slot's pre-multiplied frame
// constants, the update of one voxel by one frame, and the surface-nets vertex of one cell.  Each is ONE inline function that both
// translation units call with the same operands, so a voxel of a brick is meant to end with the bytes the dense kernel leaves at that
// voxel (tests/test_tsdf_sparse_gpu.py holds the two against each other).
#pragma once
#include "depth_vote.h"

constexpr int kFrameFloats = 16;      // per slot: A[9] row-major, b[3], frame id (as int bits), [13..15] for the caller (tsdf.hip: unused)

__device__ __forceinline__ int lanes_below(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(mask), 0));
}

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
template <bool LAB> struct VertexLabels {};
template <> struct VertexLabels<true> { const int32_t* label; int32_t* vlabel; };            // label: shaped like tsdf; vlabel [vcap]

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

// ------------------------------------------------------------------------------------------------------------ surface nets

// flag byte of a cell: bit 0 active, bits 1-3 a quad around the edge corner 0 -> corner 0 + e_a (a = x, y, z), bit 4 corner 0 inside
constexpr int kActive = 1, kInsideA = 16;

struct MeshOut { float* verts; float* normals; uint8_t* rgba; int32_t* faces; int vcap, fcap; };

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
