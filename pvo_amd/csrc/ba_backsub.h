// ---------------------------------------------------------------------------
// backsub: dz = Q (w - sum_r E_r^T dx[pose(r)]), disps += dz
// ---------------------------------------------------------------------------
#pragma once
#include "ba_schur.h"

namespace {
// CALIB (pvo_ba_calib's step, the intrinsics as a border): Gc^T dc joins the pose rows' sum, and a REJECTED step (dcw[4], or the
// eta-row mismatch that rejects it too) writes zeros to dz_out and nothing else.  Compile-time: the plain instantiation is the code it was.
template <bool CALIB>
__device__ __forceinline__ void ba_backsub_body(
    const Plan& pl, const int64_t* __restrict__ jj, const float* __restrict__ Ei, const float* __restrict__ Eij,
    const float* __restrict__ Q, const float* __restrict__ w, const float* __restrict__ dx,
    float* __restrict__ disps, float* __restrict__ dz_out, int dz_rows, int HW, int t0, int P,
    int clamp_frames, float disp_min, const float* __restrict__ Gc = nullptr, const float* __restrict__ dcw = nullptr) {
  const int k = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  // (round 4) the depth frame's out-edges, their target poses and the pose updates those rows multiply, once per workgroup in LDS:
  // row_of() walked eptr -> eidx -> jj per row and pixel, three dependent loads in front of every row's six products
  __shared__ int s_edge[256], s_pose[256];
  __shared__ float s_dx[256][6];
  const bool live = k < pl.meta[0] && !pl.meta[2];        // (uniform; meta[2]: eta's row count != K - nothing is updated)
  const int e0 = live ? pl.eptr[k] : 0, deg = live ? pl.eptr[k + 1] - e0 : 0;
  const bool in_lds = deg <= 255;
  constexpr int lo = 1;                                   // EvT6x1_kernel returns early for pose index <= 0 (:1084): window pose 0 never reaches dz
  if (live && in_lds && static_cast<int>(threadIdx.x) <= deg) {
    const int r = static_cast<int>(threadIdx.x) - 1;      // row -1 = the frame's own pose row (Ei), rows 0.. = its out-edges (Eij)
    int e = 0, p;
    if (r < 0) p = pl.kx[k] - t0;
    else { e = pl.eidx[e0 + r]; p = static_cast<int>(jj[e]) - t0; }
    const bool ok = p >= 0 && p < P && p >= lo;
    s_edge[threadIdx.x] = e; s_pose[threadIdx.x] = ok ? p : -1;
#pragma unroll
    for (int n = 0; n < 6; ++n) s_dx[threadIdx.x][n] = ok ? dx[6 * p + n] : 0.0f;
  }
  BA_WG_PROBE(2, 0);
  __syncthreads();
  BA_WG_PROBE(2, 1);
  if (x >= HW) return;
  // clamp_frames > 0: disps[:clamp_frames].clamp_(min=disp_min) in the same launch (depth_video.py:214) - frames this BA
  // does not optimise here, by frame index; optimised ones below, after their update
  if (k < clamp_frames && pl.kidx[k] < 0) {
    const float v = disps[static_cast<long long>(k) * HW + x];
    if (v < disp_min) disps[static_cast<long long>(k) * HW + x] = disp_min;            // NaN stays NaN, as in torch.clamp
  }
  if constexpr (CALIB) {
    if (k >= pl.meta[0]) return;
    if (!live || reinterpret_cast<const int*>(dcw)[4] != 0) {      // nothing changes; the step's dz is reported as zero
      if (dz_out && k < dz_rows) dz_out[static_cast<long long>(k) * HW + x] = 0.0f;
      return;
    }
  }
  if (!live) return;
  float acc = 0.0f;
  if (in_lds) {
    for (int q = 0; q <= deg; ++q) {
      const int p = s_pose[q];
      if (p < 0) continue;
      const float* base = (q == 0) ? Ei + static_cast<long long>(p) * 6 * HW : Eij + static_cast<long long>(s_edge[q]) * 6 * HW;
      float sacc = 0.0f;
#pragma unroll
      for (int n = 0; n < 6; ++n) sacc += base[static_cast<long long>(n) * HW + x] * s_dx[q][n];
      acc += sacc;
    }
  } else {
    for (int r = -1; r < deg; ++r) {
      const RowRef R = row_of(r, k, pl, Ei, Eij, jj, HW, t0, P);
      if (R.pose < lo) continue;
      float sacc = 0.0f;
#pragma unroll
      for (int n = 0; n < 6; ++n) sacc += R.base[static_cast<long long>(n) * HW + x] * dx[6 * R.pose + n];
      acc += sacc;
    }
  }
  if constexpr (CALIB) {
    float cacc = 0.0f;
#pragma unroll
    for (int n = 0; n < 4; ++n) cacc += Gc[(static_cast<long long>(k) * 4 + n) * HW + x] * dcw[n];
    acc += cacc;
  }
  const float dz = Q[static_cast<long long>(k) * HW + x] * (w[static_cast<long long>(k) * HW + x] - acc);
  float d = disps[static_cast<long long>(pl.kx[k]) * HW + x] + dz;  // disp_retr_kernel (:912-925)
  if (pl.kx[k] < clamp_frames && d < disp_min) d = disp_min;
  disps[static_cast<long long>(pl.kx[k]) * HW + x] = d;
  if (dz_out && k < dz_rows) dz_out[static_cast<long long>(k) * HW + x] = dz;
  BA_WG_PROBE(2, 2);
}

__global__ __launch_bounds__(256) void ba_backsub_kernel(
    Plan pl, const int64_t* __restrict__ jj, const float* __restrict__ Ei, const float* __restrict__ Eij,
    const float* __restrict__ Q, const float* __restrict__ w, const float* __restrict__ dx,
    float* __restrict__ disps, float* __restrict__ dz_out, int dz_rows, int HW, int t0, int P,
    int clamp_frames, float disp_min) {
  ba_backsub_body<false>(pl, jj, Ei, Eij, Q, w, dx, disps, dz_out, dz_rows, HW, t0, P, clamp_frames, disp_min);
}
}  // namespace
