// ---------------------------------------------------------------------------
// assemble
// ---------------------------------------------------------------------------
#pragma once
#include "common.h"
#include "se3.h"
#include "ba_workspace.h"

namespace {

struct EdgeGeom { Pose G; float fx, fy, cx, cy; };

// one pixel of projective_transform_kernel (droid_kernels.cu:266-357): accumulates the
// upper triangle h[78] of [Ji Jj]^T W [Ji Jj], the gradients vi/vj, and returns the
// depth-coupling terms.
__device__ __forceinline__ void pixel_terms(const EdgeGeom& g, float u, float v, float disp,
                                            float tu, float tv, float wgu, float wgv,
                                            float (&h)[78], float (&vi)[6], float (&vj)[6],
                                            float (&eii)[6], float (&eij)[6], float& cii, float& bzz) {
  float Xi[4] = {(u - g.cx) / g.fx, (v - g.cy) / g.fy, 1.0f, disp};
  float Xj[4];
  act4(g.G, Xi, Xj);
  const float x = Xj[0], y = Xj[1], hh = Xj[3];
  const bool ok = !(Xj[2] < kMinDepth);
  const float d = ok ? 1.0f / Xj[2] : 0.0f;
  const float d2 = d * d;
  // droid_kernels.cu:290-291 write `.001 * weight`: a DOUBLE literal, so the product is formed in double and rounded to
  // float once - not the same number as 0.001f * w (0.001f != 0.001).  Followed literally; `1.0 / Xj[2]` (:287) equals the
  // correctly rounded float division (double rounding of a quotient is innocuous at 53 >= 2 * 24 + 2 bits).
  const float wu = ok ? static_cast<float>(0.001 * static_cast<double>(wgu)) : 0.0f;
  const float wv = ok ? static_cast<float>(0.001 * static_cast<double>(wgv)) : 0.0f;
  const float ru = tu - (g.fx * d * x + g.cx);
  const float rv = tv - (g.fy * d * y + g.cy);
  float J[12];   // [Ji | Jj]
  float Jz;
  // ---- x residual
  J[6] = g.fx * (hh * d); J[7] = 0.0f; J[8] = g.fx * (-x * hh * d2);
  J[9] = g.fx * (-x * y * d2); J[10] = g.fx * (1.0f + x * x * d2); J[11] = g.fx * (-y * d);
  Jz = g.fx * (g.G.t.x * d - g.G.t.z * (x * d2));
  adjT(g.G, &J[6], &J[0]);
#pragma unroll
  for (int n = 0; n < 6; ++n) J[n] = -J[n];
  {
    int l = 0;
#pragma unroll
    for (int n = 0; n < 12; ++n) {
      const float wj = wu * J[n];
#pragma unroll
      for (int m = 0; m <= n; ++m) { h[l] += wj * J[m]; ++l; }
    }
  }
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    vi[n] += wu * ru * J[n];
    vj[n] += wu * ru * J[6 + n];
    eii[n] = wu * Jz * J[n];
    eij[n] = wu * Jz * J[6 + n];
  }
  cii = wu * Jz * Jz;
  bzz = wu * ru * Jz;
  // ---- y residual
  J[6] = 0.0f; J[7] = g.fy * (hh * d); J[8] = g.fy * (-y * hh * d2);
  J[9] = g.fy * (-1.0f - y * y * d2); J[10] = g.fy * (x * y * d2); J[11] = g.fy * (x * d);
  Jz = g.fy * (g.G.t.y * d - g.G.t.z * (y * d2));
  adjT(g.G, &J[6], &J[0]);
#pragma unroll
  for (int n = 0; n < 6; ++n) J[n] = -J[n];
  {
    int l = 0;
#pragma unroll
    for (int n = 0; n < 12; ++n) {
      const float wj = wv * J[n];
#pragma unroll
      for (int m = 0; m <= n; ++m) { h[l] += wj * J[m]; ++l; }
    }
  }
#pragma unroll
  for (int n = 0; n < 6; ++n) {
    vi[n] += wv * rv * J[n];
    vj[n] += wv * rv * J[6 + n];
    eii[n] += wv * Jz * J[n];
    eij[n] += wv * Jz * J[6 + n];
  }
  cii += wv * Jz * Jz;
  bzz += wv * rv * Jz;
}

// one pixel of a STEREO edge (i, i): g.G is the rig's fixed transform, so the residual depends on no pose - only the depth terms
// remain.  The projection, the Z test, the weights and Jz are pixel_terms' own expressions in its own order.
__device__ __forceinline__ void stereo_pixel_terms(const EdgeGeom& g, float u, float v, float disp,
                                                   float tu, float tv, float wgu, float wgv, float& cii, float& bzz) {
  float Xi[4] = {(u - g.cx) / g.fx, (v - g.cy) / g.fy, 1.0f, disp};
  float Xj[4];
  act4(g.G, Xi, Xj);
  const float x = Xj[0], y = Xj[1];
  const bool ok = !(Xj[2] < kMinDepth);
  const float d = ok ? 1.0f / Xj[2] : 0.0f;
  const float d2 = d * d;
  const float wu = ok ? static_cast<float>(0.001 * static_cast<double>(wgu)) : 0.0f;
  const float wv = ok ? static_cast<float>(0.001 * static_cast<double>(wgv)) : 0.0f;
  const float ru = tu - (g.fx * d * x + g.cx);
  const float rv = tv - (g.fy * d * y + g.cy);
  float Jz = g.fx * (g.G.t.x * d - g.G.t.z * (x * d2));
  cii = wu * Jz * Jz;
  bzz = wu * ru * Jz;
  Jz = g.fy * (g.G.t.y * d - g.G.t.z * (y * d2));
  cii += wv * Jz * Jz;
  bzz += wv * rv * Jz;
}

// Entry t of an edge's 90 sums - upper triangle of [Ji Jj]^T W [Ji Jj] (78, droid_kernels.cu:309-315 ordering), vi (6), vj (6) -
// added to the pose system in fixed point.
__device__ __forceinline__ void pose_block_scatter(int t, double val, int pi, int pj, int P, long long* __restrict__ sys, int* __restrict__ meta) {
  const bool iok = pi >= 0 && pi < P, jok = pj >= 0 && pj < P;
  const int n6 = 6 * P;
  if (t < 78) {
    // invert l -> (n, m), m <= n
    int n = 0, base = 0;
    while (base + n + 1 <= t) { base += n + 1; ++n; }
    const int m = t - base;
    if (n < 6) {                                  // (ii,ii), symmetric
      if (iok) {
        fix_add(sys, static_cast<long long>(6 * pi + n) * n6 + 6 * pi + m, val, meta);
        if (n != m) fix_add(sys, static_cast<long long>(6 * pi + m) * n6 + 6 * pi + n, val, meta);
      }
    } else if (m < 6) {                           // (ii,jj)[m][n-6] and (jj,ii)[n-6][m]
      // only the LOWER block triangle of the system is ever read (the solve factorises it; an edge-sharded run all-reduces
      // exactly those blocks): of the two mirrored off-diagonal blocks the one above the diagonal is not written.  Nothing at
      // window size; a global bundle adjustment's Schur kernel is bound by these atomics (round 4)
      if (iok && jok) {
        if (pi > pj) fix_add(sys, static_cast<long long>(6 * pi + m) * n6 + 6 * pj + (n - 6), val, meta);
        else fix_add(sys, static_cast<long long>(6 * pj + (n - 6)) * n6 + 6 * pi + m, val, meta);
      }
    } else {                                      // (jj,jj), symmetric
      if (jok) {
        fix_add(sys, static_cast<long long>(6 * pj + n - 6) * n6 + 6 * pj + m - 6, val, meta);
        if (n != m) fix_add(sys, static_cast<long long>(6 * pj + m - 6) * n6 + 6 * pj + n - 6, val, meta);
      }
    }
  } else if (t < 84) {
    if (iok) fix_add(sys, static_cast<long long>(n6) * n6 + 6 * pi + (t - 78), val, meta);
  } else {
    if (jok) fix_add(sys, static_cast<long long>(n6) * n6 + 6 * pj + (t - 84), val, meta);
  }
}

// The (at most two) entries of the pose system pose_block_scatter adds entry t of edge (pi -> pj) to; -1 = none.  Same case
// analysis, kept beside it.
__device__ __forceinline__ void pose_block_targets(int t, int pi, int pj, int P, long long idx[2]) {
  const bool iok = pi >= 0 && pi < P, jok = pj >= 0 && pj < P;
  const long long n6 = 6 * P;
  idx[0] = idx[1] = -1;
  if (t < 78) {
    int n = 0, base = 0;
    while (base + n + 1 <= t) { base += n + 1; ++n; }
    const int m = t - base;
    if (n < 6) {
      if (iok) { idx[0] = (6 * pi + n) * n6 + 6 * pi + m; if (n != m) idx[1] = (6 * pi + m) * n6 + 6 * pi + n; }
    } else if (m < 6) {
      if (iok && jok) idx[0] = (pi > pj) ? (6 * pi + m) * n6 + 6 * pj + (n - 6) : (6 * pj + (n - 6)) * n6 + 6 * pi + m;
    } else {
      if (jok) { idx[0] = (6 * pj + n - 6) * n6 + 6 * pj + m - 6; if (n != m) idx[1] = (6 * pj + m - 6) * n6 + 6 * pj + n - 6; }
    }
  } else if (t < 84) {
    if (iok) idx[0] = n6 * n6 + 6 * pi + (t - 78);
  } else {
    if (jok) idx[0] = n6 * n6 + 6 * pj + (t - 84);
  }
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
