// tsdf_ray.h — the arithmetic of looking at a TSDF volume from a camera (tsdf_render.hip, tsdf_track.hip), shared by the dense and the brick volume:
// a view's constants, a pixel's ray, the position, cell and fraction of a lattice sample, the trilinear value and its gradient, the
// hit's interpolation and the blend of the two bracketing samples.  Each is ONE inline function, called with the GLOBAL integer cell
// index; a volume only supplies where the eight corners of a cell are stored.  Every multiply-add is written as an explicit fmaf, so
// the sequence of roundings is the one include/pvo_hip.h (pvo_tsdf_render) states and does not depend on what the compiler contracts:
// the brick render is meant to give the BYTES of the dense render (tests/test_tsdf_render_gpu.py holds the two against each other).
#pragma once
#include "tsdf_fuse.h"

constexpr int kViewFloats = 16;       // per slot: M[9] row-major, p0[3], view id (as int bits), [13..15] unused

// o[0..12] of view f (in [0, nviews)):  M = R^T / voxel,  p0 = (-R^T t - origin) / voxel,  the view id
__device__ __forceinline__ void ray_view_constants(const float* __restrict__ poses, long long f, const Vol vol, float* __restrict__ o) {
  const Pose G = load_pose(poses + 7 * f);
  const Quat q = G.q;
  // R(q) of the quaternion as stored, the expressions of tsdf_frame_constants
  const float r[9] = {1.0f - 2.0f * (q.y * q.y + q.z * q.z), 2.0f * (q.x * q.y - q.z * q.w), 2.0f * (q.x * q.z + q.y * q.w),
                      2.0f * (q.x * q.y + q.z * q.w), 1.0f - 2.0f * (q.x * q.x + q.z * q.z), 2.0f * (q.y * q.z - q.x * q.w),
                      2.0f * (q.x * q.z - q.y * q.w), 2.0f * (q.y * q.z + q.x * q.w), 1.0f - 2.0f * (q.x * q.x + q.y * q.y)};
  const float org[3] = {vol.ox, vol.oy, vol.oz};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o[3 * i + j] = r[3 * j + i] / vol.voxel;
    const float c = -fmaf(r[6 + i], G.t.z, fmaf(r[3 + i], G.t.y, r[i] * G.t.x));      // the camera's centre
    o[9 + i] = (c - org[i]) / vol.voxel;
  }
  o[12] = __int_as_float(static_cast<int>(f));
}

// p(z) = z g + p0 in voxel coordinates, axes 0 = x, 1 = y, 2 = z
struct Ray { float g[3], p0[3]; };

__device__ __forceinline__ Ray ray_of_pixel(const float* __restrict__ c, const Intr K, int ui, int vi) {
  const float rx = (static_cast<float>(ui) - K.cx) / K.fx, ry = (static_cast<float>(vi) - K.cy) / K.fy;
  Ray r;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    r.g[i] = fmaf(c[3 * i], rx, fmaf(c[3 * i + 1], ry, c[3 * i + 2]));
    r.p0[i] = c[9 + i];
  }
  return r;
}

// sample k of the global lattice: z_k = float(k) dz, p = z_k g + p0.  Returns whether p lies in [0, n-1] on every axis (n = (nx, ny,
// nz), each >= 2; a NaN fails); then cell = min(floor(p), n-2) and frac = p - cell
__device__ __forceinline__ bool ray_sample_cell(const Ray r, int k, float dz, const int (&n)[3], int (&cell)[3], float (&frac)[3]) {
  const float z = static_cast<float>(k) * dz;
  bool in = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float p = fmaf(z, r.g[i], r.p0[i]);
    in = in && p >= 0.0f && p <= static_cast<float>(n[i] - 1);
    cell[i] = min(pvo_floor_to_int(p), n[i] - 2);
    frac[i] = p - static_cast<float>(cell[i]);
  }
  return in;
}

// the same at an arbitrary depth z along the optical axis (tsdf_track.hip: z = 1 / d of the pixel's own inverse depth)
__device__ __forceinline__ bool ray_point_cell(const Ray r, float z, const int (&n)[3], int (&cell)[3], float (&frac)[3]) {
  bool in = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float p = fmaf(z, r.g[i], r.p0[i]);
    in = in && p >= 0.0f && p <= static_cast<float>(n[i] - 1);
    cell[i] = min(pvo_floor_to_int(p), n[i] - 2);
    frac[i] = p - static_cast<float>(cell[i]);
  }
  return in;
}

__device__ __forceinline__ float ray_lerp(float a, float b, float t) { return fmaf(t, b - a, a); }

// the trilinear interpolant of the corner values s[j] (j = 4 dz + 2 dy + dx) at frac: x first, then y, then z
__device__ __forceinline__ float ray_trilinear(const float (&s)[8], const float (&f)[3]) {
  const float b0 = ray_lerp(ray_lerp(s[0], s[1], f[0]), ray_lerp(s[2], s[3], f[0]), f[1]);
  const float b1 = ray_lerp(ray_lerp(s[4], s[5], f[0]), ray_lerp(s[6], s[7], f[0]), f[1]);
  return ray_lerp(b0, b1, f[2]);
}

// its analytic gradient in the cell (per voxel): every component is the bilinear interpolant of four corner differences
__device__ __forceinline__ void ray_gradient(const float (&s)[8], const float (&f)[3], float (&g)[3]) {
  g[0] = ray_lerp(ray_lerp(s[1] - s[0], s[3] - s[2], f[1]), ray_lerp(s[5] - s[4], s[7] - s[6], f[1]), f[2]);
  g[1] = ray_lerp(ray_lerp(s[2] - s[0], s[3] - s[1], f[0]), ray_lerp(s[6] - s[4], s[7] - s[5], f[0]), f[2]);
  g[2] = ray_lerp(ray_lerp(s[4] - s[0], s[5] - s[1], f[0]), ray_lerp(s[6] - s[2], s[7] - s[3], f[0]), f[1]);
}

// the zero crossing between sample k-1 (value sa >= 0) and sample k (sb < 0): sa - sb > 0
__device__ __forceinline__ float ray_hit_fraction(float sa, float sb) { return sa / (sa - sb); }
__device__ __forceinline__ float ray_hit_depth(int k, float t, float dz) { return (static_cast<float>(k - 1) + t) * dz; }

// normalise(lerp(ga, gb, t)); a zero vector (or a NaN length) gives (0,0,0)
__device__ __forceinline__ void ray_hit_normal(const float (&ga)[3], const float (&gb)[3], float t, float* __restrict__ o) {
  const float x = ray_lerp(ga[0], gb[0], t), y = ray_lerp(ga[1], gb[1], t), z = ray_lerp(ga[2], gb[2], t);
  const float len = sqrtf(fmaf(x, x, fmaf(y, y, z * z)));
  const bool zero = !(len > 0.0f);
  o[0] = zero ? 0.0f : x / len; o[1] = zero ? 0.0f : y / len; o[2] = zero ? 0.0f : z / len;
}

// floor(lerp(ca, cb, t) + 0.5) clamped to [0, 255] (NaN -> 0)
__device__ __forceinline__ uint8_t ray_hit_colour(float ca, float cb, float t) {
  return static_cast<uint8_t>(min(255, max(0, pvo_floor_to_int(ray_lerp(ca, cb, t) + 0.5f))));
}

// The samples that can lie in the box [0, n-1]^3: the slab test in fp32, WIDENED, intersected with [klo, khi].  A crossing depth
// zc = (face - p0) / g carries a few EPS of relative error and so does the sample's own p; with z / dz < 2^22 (the call's limit) both
// stay below 1.5 dz, so the range is opened by two samples at each end (floor - 1, floor + 2) and the per-sample test decides.
// An axis with g == 0 does not narrow the range.
__device__ __forceinline__ void ray_clip(const Ray r, const int (&n)[3], float dz, int klo, int khi, int& ka, int& kb) {
  float zmin = -__builtin_inff(), zmax = __builtin_inff();
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float top = static_cast<float>(n[i] - 1);
    const float z0 = (0.0f - r.p0[i]) / r.g[i], z1 = (top - r.p0[i]) / r.g[i];
    if (r.g[i] > 0.0f) { zmin = fmaxf(zmin, z0); zmax = fminf(zmax, z1); }
    else if (r.g[i] < 0.0f) { zmin = fmaxf(zmin, z1); zmax = fminf(zmax, z0); }
  }
  ka = max(klo, pvo_floor_to_int(zmin / dz) - 1);
  kb = min(khi, pvo_floor_to_int(zmax / dz) + 2);
}

// The first sample that can have left the brick (bx,by,bz) (corner-0 cells 8b .. 8b+7, i.e. p in [8b, 8b+8) on every axis), landing
// EARLY by the same two samples; never below k + 1, so a loop that assigns it always advances.
__device__ __forceinline__ int ray_brick_exit(const Ray r, const int (&b)[3], float dz, int k) {
  float ze = __builtin_inff();
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float lo = static_cast<float>(8 * b[i]);
    if (r.g[i] > 0.0f) ze = fminf(ze, ((lo + 8.0f) - r.p0[i]) / r.g[i]);
    else if (r.g[i] < 0.0f) ze = fminf(ze, (lo - r.p0[i]) / r.g[i]);
  }
  return max(k + 1, pvo_floor_to_int(ze / dz) - 2);
}

// ------------------------------------------------------------------------------------------------------------ the walk
//
// A volume V supplies:  n[3] = (nx, ny, nz);  tsdf, wsum, rgb (or NULL), label (or NULL) and min_weight;
//   int corners(const int (&cell)[3], int (&at)[8])   the storage index of the cell's eight corners; 0 = all stored, 1 = some corner
//                                                     is not stored but corner 0's brick is, 2 = corner 0's brick is not stored
//   static constexpr bool kBricks                      whether result 2 may be answered by a jump (ray_brick_exit)

struct RaySample { int at[8]; float f[3]; float s[8]; float S; };

// sample k: VALID (true) iff in the box, all eight corners stored and wsum >= min_weight; then s, f, at and S are set.  code: V::corners'
// result (0 where the sample is outside the box).  Corner 0's weight is read first: in free space a sample costs one gather.
template <class V>
__device__ __forceinline__ bool ray_sample(V& vol, const Ray r, int k, float dz, RaySample& a, int& code, int (&cell)[3]) {
  code = 0;
  if (!ray_sample_cell(r, k, dz, vol.n, cell, a.f)) return false;
  code = vol.corners(cell, a.at);
  if (code != 0) return false;
  if (!(vol.wsum[a.at[0]] >= vol.min_weight)) return false;
  bool ok = true;
#pragma unroll
  for (int j = 1; j < 8; ++j) ok = ok && vol.wsum[a.at[j]] >= vol.min_weight;
  if (!ok) return false;
#pragma unroll
  for (int j = 0; j < 8; ++j) a.s[j] = vol.tsdf[a.at[j]];
  a.S = ray_trilinear(a.s, a.f);
  return true;
}

struct RenderOut { float* depth; float* normal; uint8_t* rgba; int32_t* label; int32_t* visited; };

// one pixel: the walk over the lattice samples klo .. khi of the ray and the pixel's four outputs at index pix.  live = false (a
// view outside [0, nviews)): a miss without looking at the ray.
template <class V>
__device__ __forceinline__ void ray_pixel(V& vol, const Ray r, bool live, float dz, int klo, int khi, const RenderOut out, long long pix) {
  int ka = 0, kb = -1;
  if (live) ray_clip(r, vol.n, dz, klo, khi, ka, kb);
  RaySample b;
  bool prev = false, hit = false;
  int k = ka, steps = 0;
  while (k <= kb) {
    ++steps;
    int code, cell[3];
    if (!ray_sample(vol, r, k, dz, b, code, cell)) {
      prev = false;
      if (V::kBricks && code == 2) {
        const int brick[3] = {cell[0] >> 3, cell[1] >> 3, cell[2] >> 3};
        k = ray_brick_exit(r, brick, dz, k);
      } else {
        ++k;
      }
      continue;
    }
    if (b.S < 0.0f) { hit = prev; break; }             // the ray ends here; a hit needs sample k-1 valid (then S_{k-1} >= 0)
    prev = true;
    ++k;
  }
  if (out.visited) { out.visited[2 * pix] = steps; out.visited[2 * pix + 1] = max(kb - ka + 1, 0); }
  float depth = 0.0f, nrm[3] = {0.0f, 0.0f, 0.0f};
  uchar4 col = make_uchar4(0, 0, 0, 0);
  int32_t lab = 0;
  RaySample a;
  if (hit) {                                           // sample k-1 again: the same function on the same operands, so valid as the walk saw it
    int code, cell[3];
    hit = ray_sample(vol, r, k - 1, dz, a, code, cell);
  }
  if (hit) {
    const float t = ray_hit_fraction(a.S, b.S);
    depth = ray_hit_depth(k, t, dz);
    if (out.normal) {
      float ga[3], gb[3];
      ray_gradient(a.s, a.f, ga);
      ray_gradient(b.s, b.f, gb);
      ray_hit_normal(ga, gb, t, nrm);
    }
    if (out.rgba) {
      col.w = 255;
      if (vol.rgb) {
        uint8_t c8[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) {
          float ca[8], cb[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) { ca[j] = vol.rgb[3ll * a.at[j] + e]; cb[j] = vol.rgb[3ll * b.at[j] + e]; }
          c8[e] = ray_hit_colour(ray_trilinear(ca, a.f), ray_trilinear(cb, b.f), t);
        }
        col.x = c8[0]; col.y = c8[1]; col.z = c8[2];
      }
    }
    if (out.label) {
      long long at[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) at[j] = b.at[j];
      lab = surface_net_label(b.s, vol.label, at);
    }
  }
  out.depth[pix] = depth;
  if (out.normal) { float* o = out.normal + 3 * pix; o[0] = nrm[0]; o[1] = nrm[1]; o[2] = nrm[2]; }
  if (out.rgba) reinterpret_cast<uchar4*>(out.rgba)[pix] = col;
  if (out.label) out.label[pix] = lab;
}
