// ---------------------------------------------------------------------------
// assemble
// ---------------------------------------------------------------------------
#pragma once
#include "common.h"
#include "se3.h"
#include "ba_workspace.h"

namespace {

struct EdgeGeom { Pose G; float fx, fy, cx, cy; };

// One pixel of an edge, projected (projective_transform_kernel, droid_kernels.cu:266-357): the target point (x, y, 1 / d, hh),
// the MIN_DEPTH test, and per residual row (u, v) the weight w and the residual r.  The ONE statement of these float expressions:
// the assembly, the stereo edges and the calibration stage all form their terms from it, so they agree bit for bit.
struct EdgePixel { float x, y, hh, d, d2, wu, wv, ru, rv; bool ok; };

__device__ __forceinline__ EdgePixel project_pixel(const EdgeGeom& g, float u, float v, float disp,
                                                   float tu, float tv, float wgu, float wgv) {
  float Xi[4] = {(u - g.cx) / g.fx, (v - g.cy) / g.fy, 1.0f, disp};
  float Xj[4];
  act4(g.G, Xi, Xj);
  EdgePixel p;
  p.x = Xj[0]; p.y = Xj[1]; p.hh = Xj[3];
  p.ok = !(Xj[2] < kMinDepth);
  p.d = p.ok ? 1.0f / Xj[2] : 0.0f;
  p.d2 = p.d * p.d;
  // droid_kernels.cu:290-291 write `.001 * weight`: a DOUBLE literal, so the product is formed in double and rounded to
  // float once - not the same number as 0.001f * w (0.001f != 0.001).  Followed literally; `1.0 / Xj[2]` (:287) equals the
  // correctly rounded float division (double rounding of a quotient is innocuous at 53 >= 2 * 24 + 2 bits).
  p.wu = p.ok ? static_cast<float>(0.001 * static_cast<double>(wgu)) : 0.0f;
  p.wv = p.ok ? static_cast<float>(0.001 * static_cast<double>(wgv)) : 0.0f;
  p.ru = tu - (g.fx * p.d * p.x + g.cx);
  p.rv = tv - (g.fy * p.d * p.y + g.cy);
  return p;
}

// Jz = d(residual row)/d(disparity); ROW 0 = u, 1 = v
template <int ROW>
__device__ __forceinline__ float depth_jacobian(const EdgeGeom& g, const EdgePixel& p) {
  if constexpr (ROW == 0) return g.fx * (g.G.t.x * p.d - g.G.t.z * (p.x * p.d2));
  else return g.fy * (g.G.t.y * p.d - g.G.t.z * (p.y * p.d2));
}

// J = [Ji | Jj] of one residual row: Jj, then Ji = -Ad^T Jj
template <int ROW>
__device__ __forceinline__ void pose_jacobian(const EdgeGeom& g, const EdgePixel& p, float (&J)[12]) {
  const float x = p.x, y = p.y, hh = p.hh, d = p.d, d2 = p.d2;
  if constexpr (ROW == 0) {
    J[6] = g.fx * (hh * d); J[7] = 0.0f; J[8] = g.fx * (-x * hh * d2);
    J[9] = g.fx * (-x * y * d2); J[10] = g.fx * (1.0f + x * x * d2); J[11] = g.fx * (-y * d);
  } else {
    J[6] = 0.0f; J[7] = g.fy * (hh * d); J[8] = g.fy * (-y * hh * d2);
    J[9] = g.fy * (-1.0f - y * y * d2); J[10] = g.fy * (x * y * d2); J[11] = g.fy * (x * d);
  }
  adjT(g.G, &J[6], &J[0]);
#pragma unroll
  for (int n = 0; n < 6; ++n) J[n] = -J[n];
}

// one residual row of pixel_terms: row 0 starts the depth-coupling terms, row 1 adds to them
template <int ROW>
__device__ __forceinline__ void pixel_row_terms(const EdgeGeom& g, const EdgePixel& p,
                                                float (&h)[78], float (&vi)[6], float (&vj)[6],
                                                float (&eii)[6], float (&eij)[6], float& cii, float& bzz) {
  const float w = ROW == 0 ? p.wu : p.wv, r = ROW == 0 ? p.ru : p.rv;
  float J[12];
  pose_jacobian<ROW>(g, p, J);
  const float Jz = depth_jacobian<ROW>(g, p);
  {
    int l = 0;
#pragma unroll
    for (int n = 0; n < 12; ++n) {
      const float wj = w * J[n];
#pragma unroll
      for (int m = 0; m <= n; ++m) { h[l] += wj * J[m]; ++l; }
    }
  }
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    vi[n] += w * r * J[n];
    vj[n] += w * r * J[6 + n];
    if constexpr (ROW == 0) { eii[n] = w * Jz * J[n]; eij[n] = w * Jz * J[6 + n]; }
    else { eii[n] += w * Jz * J[n]; eij[n] += w * Jz * J[6 + n]; }
  }
  if constexpr (ROW == 0) { cii = w * Jz * Jz; bzz = w * r * Jz; }
  else { cii += w * Jz * Jz; bzz += w * r * Jz; }
}

// one pixel of projective_transform_kernel (droid_kernels.cu:266-357): accumulates the
// upper triangle h[78] of [Ji Jj]^T W [Ji Jj], the gradients vi/vj, and returns the
// depth-coupling terms.  The two rows in turn: one J[12] is live at a time.
__device__ __forceinline__ void pixel_terms(const EdgeGeom& g, float u, float v, float disp,
                                            float tu, float tv, float wgu, float wgv,
                                            float (&h)[78], float (&vi)[6], float (&vj)[6],
                                            float (&eii)[6], float (&eij)[6], float& cii, float& bzz) {
  const EdgePixel p = project_pixel(g, u, v, disp, tu, tv, wgu, wgv);
  pixel_row_terms<0>(g, p, h, vi, vj, eii, eij, cii, bzz);
  pixel_row_terms<1>(g, p, h, vi, vj, eii, eij, cii, bzz);
}

// one pixel of a STEREO edge (i, i): g.G is the rig's fixed transform, so the residual depends on no pose - only the depth terms
// remain.
__device__ __forceinline__ void stereo_pixel_terms(const EdgeGeom& g, float u, float v, float disp,
                                                   float tu, float tv, float wgu, float wgv, float& cii, float& bzz) {
  const EdgePixel p = project_pixel(g, u, v, disp, tu, tv, wgu, wgv);
  float Jz = depth_jacobian<0>(g, p);
  cii = p.wu * Jz * Jz;
  bzz = p.wu * p.ru * Jz;
  Jz = depth_jacobian<1>(g, p);
  cii += p.wv * Jz * Jz;
  bzz += p.wv * p.rv * Jz;
}

// t -> (n, m), m <= n: the inverse of the row-major rank t = n (n + 1) / 2 + m of a triangle's entry
__device__ __forceinline__ void tri_unrank(int t, int& n, int& m) {
  int base = 0;
  n = 0;
  while (base + n + 1 <= t) { base += n + 1; ++n; }
  m = t - base;
}

// The (at most two) entries of the pose system that entry t of an edge's 90 sums - upper triangle of [Ji Jj]^T W [Ji Jj] (78,
// droid_kernels.cu:309-315 ordering), vi (6), vj (6) - of edge (pi -> pj) is added to; -1 = none.
__device__ __forceinline__ void pose_block_targets(int t, int pi, int pj, int P, long long idx[2]) {
  const bool iok = pi >= 0 && pi < P, jok = pj >= 0 && pj < P;
  const long long n6 = 6 * P;
  idx[0] = idx[1] = -1;
  if (t < 78) {
    int n, m;
    tri_unrank(t, n, m);
    if (n < 6) {                                  // (ii,ii), symmetric
      if (iok) { idx[0] = (6 * pi + n) * n6 + 6 * pi + m; if (n != m) idx[1] = (6 * pi + m) * n6 + 6 * pi + n; }
    } else if (m < 6) {                           // (ii,jj)[m][n-6] and (jj,ii)[n-6][m]
      // only the LOWER block triangle of the system is ever read (the solve factorises it; an edge-sharded run all-reduces
      // exactly those blocks): of the two mirrored off-diagonal blocks the one above the diagonal is not written.  Nothing at
      // window size; a global bundle adjustment's Schur kernel is bound by these atomics (round 4)
      if (iok && jok) idx[0] = (pi > pj) ? (6 * pi + m) * n6 + 6 * pj + (n - 6) : (6 * pj + (n - 6)) * n6 + 6 * pi + m;
    } else {                                      // (jj,jj), symmetric
      if (jok) { idx[0] = (6 * pj + n - 6) * n6 + 6 * pj + m - 6; if (n != m) idx[1] = (6 * pj + m - 6) * n6 + 6 * pj + n - 6; }
    }
  } else if (t < 84) {
    if (iok) idx[0] = n6 * n6 + 6 * pi + (t - 78);
  } else {
    if (jok) idx[0] = n6 * n6 + 6 * pj + (t - 84);
  }
}

// ... and the sum itself added there in fixed point
__device__ __forceinline__ void pose_block_scatter(int t, double val, int pi, int pj, int P, long long* __restrict__ sys, int* __restrict__ meta) {
  long long idx[2];
  pose_block_targets(t, pi, pj, P, idx);
  if (idx[0] >= 0) fix_add(sys, idx[0], val, meta);
  if (idx[1] >= 0) fix_add(sys, idx[1], val, meta);
}

__global__ __launch_bounds__(256) void ba_assemble_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intr,
    const float* __restrict__ targets, const float* __restrict__ weights,
    const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
    float* __restrict__ Eii, float* __restrict__ Eij, float* __restrict__ Cii, float* __restrict__ bz,
    long long* __restrict__ sys, int* __restrict__ meta, int HW, int wd, int t0, int P, int motion_only, float* __restrict__ part) {
  // Every (edge, pixel chunk) workgroup ends with 90 sums.  Added to `sys` right here they are 216 x 90 memory-side atomics on
  // ~1800 addresses at S-B - each address serialises the ~30 workgroups that hit it, 5 of this kernel's 14 us (ablation build).
  // In a depth BA (`part`) the chunk sums are stored instead and the Schur kernel, which follows anyway, adds them up per edge:
  // a sixth of the atomics, issued while its own work starts.
  __shared__ float red[4][90];
  BA_WG_PROBE(0, 0);
  const int e = blockIdx.y;
  const int ix = static_cast<int>(ii[e]), jx = static_cast<int>(jj[e]);
  EdgeGeom g;
  g.fx = intr[0]; g.fy = intr[1]; g.cx = intr[2]; g.cy = intr[3];
  const float baseline = __int_as_float(meta[8]);
  if (baseline != 0.0f && ix == jx) {
    // A stereo edge (uniform over the workgroup: e is blockIdx.y).  The rig is rigid: no pose sums, so none of the reduce-scatter
    // below; the depth terms go out with ZERO coupling rows, which the depth phase, the Schur kernel and the back-substitution read
    // like any edge's.  Motion-only: it adds nothing at all.
    if (motion_only) return;
    g.G = rig_pose(baseline);
#pragma unroll
    for (int s = 0; s < kPPT; ++s) {
      const int k = blockIdx.x * kChunkA + s * 256 + threadIdx.x;
      if (k < HW) {
        const int i = k / wd, j = k - i * wd;
        const float* __restrict__ tg = targets + static_cast<long long>(e) * 2 * HW;
        const float* __restrict__ wg = weights + static_cast<long long>(e) * 2 * HW;
        float cii, bzz;
        stereo_pixel_terms(g, static_cast<float>(j), static_cast<float>(i), disps[static_cast<long long>(ix) * HW + k], tg[k], tg[HW + k],
                           wg[k], wg[HW + k], cii, bzz);
        const long long eb = static_cast<long long>(e) * 6 * HW + k;
#pragma unroll
        for (int n = 0; n < 6; ++n) { Eii[eb + static_cast<long long>(n) * HW] = 0.0f; Eij[eb + static_cast<long long>(n) * HW] = 0.0f; }
        Cii[static_cast<long long>(e) * HW + k] = cii;
        bz[static_cast<long long>(e) * HW + k] = bzz;
      }
    }
    // (the Schur kernel adds every edge's chunk sums into the pose system: this edge's are zero)
    if (part && threadIdx.x < 90) part[(static_cast<long long>(e) * gridDim.x + blockIdx.x) * 90 + threadIdx.x] = 0.0f;
    return;
  }
  g.G = rel_pose(load_pose(poses + 7 * static_cast<long long>(ix)), load_pose(poses + 7 * static_cast<long long>(jx)));

  float h[78], vi[6], vj[6];
#pragma unroll
  for (int l = 0; l < 78; ++l) h[l] = 0.0f;
#pragma unroll
  for (int n = 0; n < 6; ++n) { vi[n] = 0.0f; vj[n] = 0.0f; }

  const float* __restrict__ d_i = disps + static_cast<long long>(ix) * HW;
  const float* __restrict__ tg = targets + static_cast<long long>(e) * 2 * HW;
  const float* __restrict__ wg = weights + static_cast<long long>(e) * 2 * HW;
#pragma unroll
  for (int s = 0; s < kPPT; ++s) {
    const int k = blockIdx.x * kChunkA + s * 256 + threadIdx.x;
    if (k < HW) {
      const int i = k / wd, j = k - i * wd;
      float eii[6], eij[6], cii, bzz;
      pixel_terms(g, static_cast<float>(j), static_cast<float>(i), d_i[k], tg[k], tg[HW + k], wg[k], wg[HW + k],
                  h, vi, vj, eii, eij, cii, bzz);
      if (!motion_only) {
        const long long eb = static_cast<long long>(e) * 6 * HW + k;
#pragma unroll
        for (int n = 0; n < 6; ++n) { Eii[eb + static_cast<long long>(n) * HW] = eii[n]; Eij[eb + static_cast<long long>(n) * HW] = eij[n]; }
        Cii[static_cast<long long>(e) * HW + k] = cii;
        bz[static_cast<long long>(e) * HW + k] = bzz;
      }
    }
  }
  BA_WG_PROBE(0, 1);                     // pixel terms done (stores issued)
  // 90 sums per wave.  Ninety separate wave reductions (6 DPP steps each) were 5.2 of this kernel's 9.5 us at S-B
  // (profiles/r04_ba_kernel_timeline.txt); a reduce-SCATTER does the same work in a third of the instructions: the values sit in
  // 96 registers, and at every step a lane and its partner each keep one half of the array and add the other's copy of it -
  // 48, 24, 12, 6, 3 additions, then one plain exchange.  Partners: lane ^ 32 and lane ^ 16 by v_permlane32_swap /
  // v_permlane16_swap (gfx950: the two halves change places in one instruction, no select), then the DPP mirrors inside a row
  // (i <-> 15 - i, i <-> 7 - i, i <-> 3 - i) and quad_perm [1,0,3,2]; which half a lane keeps is its bit 5, 4, 3, 2, 1 in turn,
  // so lane L ends with the sums of entries [48 b5 + 24 b4 + 12 b3 + 6 b2 + 3 b1, + 3).  A fixed order of additions, as before.
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    float c[96];
#pragma unroll
    for (int l = 0; l < 78; ++l) c[l] = h[l];
#pragma unroll
    for (int n = 0; n < 6; ++n) { c[78 + n] = vi[n]; c[84 + n] = vj[n]; c[90 + n] = 0.0f; }
    auto fbits = [](float x) { return __builtin_bit_cast(unsigned, x); };
    auto bitsf = [](unsigned x) { return __builtin_bit_cast(float, x); };
#pragma unroll
    for (int q = 0; q < 48; ++q) {
      const auto r = __builtin_amdgcn_permlane32_swap(fbits(c[q]), fbits(c[q + 48]), false, false);
      c[q] = bitsf(r[0]) + bitsf(r[1]);
    }
#pragma unroll
    for (int q = 0; q < 24; ++q) {
      const auto r = __builtin_amdgcn_permlane16_swap(fbits(c[q]), fbits(c[q + 24]), false, false);
      c[q] = bitsf(r[0]) + bitsf(r[1]);
    }
    const bool b3 = lane & 8, b2 = lane & 4, b1 = lane & 2;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      const float keep = b3 ? c[q + 12] : c[q], send = b3 ? c[q] : c[q + 12];
      c[q] = keep + pvo_dpp_move<0x140>(send);      // row_mirror
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const float keep = b2 ? c[q + 6] : c[q], send = b2 ? c[q] : c[q + 6];
      c[q] = keep + pvo_dpp_move<0x141>(send);      // row_half_mirror
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float keep = b1 ? c[q + 3] : c[q], send = b1 ? c[q] : c[q + 3];
      c[q] = keep + pvo_dpp_move<0x1b>(send);       // quad_perm [3,2,1,0]
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
      c[q] = pvo_dpp_step<0xb1>(c[q]);             // quad_perm [1,0,3,2]
    const int start = ((lane >> 5) & 1) * 48 + ((lane >> 4) & 1) * 24 + ((lane >> 3) & 1) * 12 + ((lane >> 2) & 1) * 6 + ((lane >> 1) & 1) * 3;
    if (!(lane & 1)) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (start + q < 90) red[wave][start + q] = c[q];
    }
  }
  __syncthreads();
  BA_WG_PROBE(0, 2);                     // wave reductions done
  const int t = threadIdx.x;
  if (t < 90) {
    const float sum = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
    if (part) part[(static_cast<long long>(e) * gridDim.x + blockIdx.x) * 90 + t] = sum;      // summed per edge by the Schur kernel
    else pose_block_scatter(t, static_cast<double>(sum), ix - t0, jx - t0, P, sys, meta);
  }
  BA_WG_PROBE(0, 3);
}

}  // namespace
