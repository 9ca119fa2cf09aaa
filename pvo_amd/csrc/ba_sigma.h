// ---------------------------------------------------------------------------
// sigma: depth and pose uncertainty from the step's normal equations (pvo_ba_sigma, include/pvo_hip.h)
// ---------------------------------------------------------------------------
#pragma once
#include "ba_schur.h"

namespace {
// A read-only stage behind pvo_ba_local: `sys` holds A - E Q E^T in fixed point, the workspace Q, Ei and Eij.  Five launches:
//   prepare   fixed point -> fp64 with the finish path's damping (ba_prepare_kernel's expression), the UPPER triangle of the
//             symmetric system into the workspace's `chol` scratch (only the lower block triangle of `sys` is ever written:
//             entry (r, c), r <= c, is read at (c, r)).  `sys` is not zeroed: nothing of it changes.
//   factor    S_d = R^T R, R upper triangular, in place, one workgroup: block rows of 8, each thread owning columns - so
//             that the long dot products read R[k][i] coalesced over i.  Not latency critical (it is off the tracking path).
//             The reciprocal diagonal 1 / R[j][j] is kept behind the factor, at chol[n * n + 1 + j].
//   invtri    W = R^-T, one WAVE per column j: R^T y = e_j forwards in the column-oriented (axpy) form - the wave holds the
//             running right-hand side in registers, lanes over rows, and reads row i of R coalesced.  W is lower triangular
//             and goes into the strictly lower triangle of the same scratch (its diagonal is the reciprocal diagonal), which
//             the factor's readers never touch.
//   product   S_d^-1 = W^T W, one thread per entry (a, b), a <= b, written to (a, b) and (b, a): pose_cov is symmetric bit for
//             bit.
//   sigma     grid (256-pixel chunk, depth frame) like the back-substitution, with the quadratic form
//             q = sum_r sum_s E_r^T Sigma[p_r, p_s] E_s over the frame's LIVE rows where that has a dot product, in fp64
//             (Ei ~ -sum Eij: the double sum cancels heavily).  The frame's rows and the upper triangle of its blocks
//             Sigma[p_r, p_s] (r <= s, 288 B each) are staged in LDS while at most kSigmaBlocks of them; a frame with more
//             live rows, or more than 255 out-edges, reads them from global memory (uniform addresses).
// The failure flag (non-SPD, or the step's own meta[2] / meta[3] / meta[4]) sits behind the factor, at chol[n * n].
constexpr int kSigmaMaxPoses = 64;
constexpr int kSigmaBlocks = 210;        // 20 live rows: 60480 B of LDS, two workgroups per CU beside the row table

__global__ __launch_bounds__(256) void ba_sigma_prepare_kernel(const long long* __restrict__ sys, double* __restrict__ out, int n, float lm, float ep) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= n * n) return;
  const int r = idx / n, c = idx - r * n;
  if (r > c) { out[idx] = 0.0; return; }
  double v = static_cast<double>(sys[static_cast<long long>(c) * n + r]) * kInvFix;
  if (r == c) v += static_cast<double>(ep) + static_cast<double>(lm) * v;      // (ba_prepare_kernel, droid_kernels.cu:1176)
  out[idx] = v;
}

__global__ __launch_bounds__(1024) void ba_sigma_factor_kernel(double* R, int n, const int* __restrict__ meta, int* __restrict__ status_out) {
  __shared__ double s_col[8][8];          // R[k][j0 + c] of the rows above the panel, eight rows at a time
  int* flag = reinterpret_cast<int*>(R + static_cast<long long>(n) * n);
  double* rdiag = R + static_cast<long long>(n) * n + 1;
  const int tid = threadIdx.x, c = tid >> 7, il = tid & 127;
  int failed = (meta[2] | meta[3] | meta[4]) ? 1 : 0;      // (meta[3]: the elimination's row table overflowed - the system is incomplete)
  for (int j0 = 0; j0 < n && !failed; j0 += 8) {
    const int j = j0 + c;                 // this thread's row of the panel
    // rows above the panel: R[j][i] -= sum_{k < j0} R[k][j] R[k][i]
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < j0; k0 += 8) {
      __syncthreads();
      if (tid < 64) s_col[tid >> 3][tid & 7] = (j0 + (tid & 7) < n) ? R[static_cast<long long>(k0 + (tid >> 3)) * n + j0 + (tid & 7)] : 0.0;
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const double a = s_col[kk][c];
        const double* row = R + static_cast<long long>(k0 + kk) * n;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const int i = j0 + il + 128 * u;
          if (i < n) acc[u] += a * row[i];
        }
      }
    }
    if (j < n) {
#pragma unroll
      for (int u = 0; u < 3; ++u) {
        const int i = j0 + il + 128 * u;
        if (i >= j && i < n) R[static_cast<long long>(j) * n + i] -= acc[u];
      }
    }
    __syncthreads();
    // the panel's own eight rows, one after the other
    for (int cc = 0; cc < 8 && j0 + cc < n; ++cc) {
      const int jj = j0 + cc;
      const double d = R[static_cast<long long>(jj) * n + jj];       // (every thread reads the same value: the branch is uniform)
      if (!(d > 0.0) || !(d < 1.0e300)) { failed = 1; break; }
      const double rinv = 1.0 / sqrt(d);
      __syncthreads();
      if (c == cc) {
        for (int i = jj + il; i < n; i += 128) R[static_cast<long long>(jj) * n + i] *= rinv;
        if (il == 0) rdiag[jj] = rinv;
      }
      __syncthreads();
      if (c > cc && j < n) {
        const double a = R[static_cast<long long>(jj) * n + j];
        for (int i = j + il; i < n; i += 128) R[static_cast<long long>(j) * n + i] -= a * R[static_cast<long long>(jj) * n + i];
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    *flag = failed;
    if (status_out) { status_out[0] = failed; status_out[1] = meta[0]; status_out[2] = meta[2]; status_out[3] = meta[3]; }
  }
}

constexpr int kSigmaSlots = (6 * kSigmaMaxPoses + 63) / 64;      // rows per lane of the triangular solve

__global__ __launch_bounds__(64) void ba_sigma_invtri_kernel(double* R, int n) {
  const int j = blockIdx.x;                                             // one wave per column
  if (j >= n) return;
  const int failed = *reinterpret_cast<const int*>(R + static_cast<long long>(n) * n);
  if (failed) return;
  const double* rdiag = R + static_cast<long long>(n) * n + 1;
  const int lane = threadIdx.x;
  // s[v] = the running right-hand side of row 64 v + lane; rows above j stay 0 and are never read
  double s[kSigmaSlots], rn[kSigmaSlots];
#pragma unroll
  for (int v = 0; v < kSigmaSlots; ++v) s[v] = (64 * v + lane == j) ? 1.0 : 0.0;
  auto load_row = [&](int i) {                                          // row i of R right of its diagonal (the next step's, in flight early)
#pragma unroll
    for (int v = 0; v < kSigmaSlots; ++v) {
      const int k = 64 * v + lane;
      rn[v] = (i < n && k > i && k < n) ? R[static_cast<long long>(i) * n + k] : 0.0;
    }
  };
  load_row(j);
#pragma unroll
  for (int u = 0; u < kSigmaSlots; ++u) {
    const int l0 = (j > 64 * u) ? j - 64 * u : 0;                       // (uniform: one column per wave)
    for (int l = l0; l < 64 && 64 * u + l < n; ++l) {
      const int i = 64 * u + l;
      const double yi = __shfl(s[u], l) * rdiag[i];
      double rc[kSigmaSlots];
#pragma unroll
      for (int v = 0; v < kSigmaSlots; ++v) rc[v] = rn[v];
      load_row(i + 1);
#pragma unroll
      for (int v = 0; v < kSigmaSlots; ++v) s[v] -= rc[v] * yi;
      if (lane == 0 && i > j) R[static_cast<long long>(i) * n + j] = yi;     // W[i][j], strictly below the diagonal
    }
  }
}

// S_d^-1 = W^T W: entry (a, b), a <= b, = sum_{i >= b} W[i][a] W[i][b]
__global__ __launch_bounds__(64) void ba_sigma_product_kernel(const double* __restrict__ R, double* __restrict__ X, int n) {
  const int a = blockIdx.y, b = blockIdx.x * 64 + threadIdx.x;
  if (b >= n || a > b) return;
  const int failed = *reinterpret_cast<const int*>(R + static_cast<long long>(n) * n);
  if (failed) {                                                         // +inf on the diagonal, 0 elsewhere
    X[static_cast<long long>(a) * n + b] = (a == b) ? __builtin_inf() : 0.0;
    X[static_cast<long long>(b) * n + a] = (a == b) ? __builtin_inf() : 0.0;
    return;
  }
  const double* rdiag = R + static_cast<long long>(n) * n + 1;
  double acc = rdiag[b] * (a == b ? rdiag[b] : R[static_cast<long long>(b) * n + a]);
  for (int i = b + 1; i < n; ++i) acc += R[static_cast<long long>(i) * n + a] * R[static_cast<long long>(i) * n + b];
  X[static_cast<long long>(a) * n + b] = acc;
  X[static_cast<long long>(b) * n + a] = acc;
}

// E_r^T B E_s for one 6 x 6 block B (row stride `ld` doubles)
template <class Ptr>
__device__ __forceinline__ double sigma_block(const double (&er)[6], const double (&es)[6], Ptr B, int ld) {
  double q = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    double t = 0.0;
#pragma unroll
    for (int b = 0; b < 6; ++b) t += B[a * ld + b] * es[b];
    q += er[a] * t;
  }
  return q;
}

__device__ __forceinline__ void sigma_load6(const float* __restrict__ base, int HW, int x, double (&e)[6]) {
#pragma unroll
  for (int n = 0; n < 6; ++n) e[n] = static_cast<double>(base[static_cast<long long>(n) * HW + x]);
}

__global__ __launch_bounds__(256) void ba_sigma_kernel(
    Plan pl, const int64_t* __restrict__ jj, const float* __restrict__ Ei, const float* __restrict__ Eij,
    const float* __restrict__ Q, const double* __restrict__ X, const int* __restrict__ flag,
    float* __restrict__ var_cond, float* __restrict__ var_pose, int HW, int t0, int P, int* __restrict__ status_out) {
  const int k = blockIdx.y;
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int n = 6 * P;
  if (status_out && blockIdx.x == 0 && k == 0 && threadIdx.x == 0) {      // (P == 0 only: with a pose system the factorisation reports)
    status_out[0] = pl.meta[2] ? 1 : 0; status_out[1] = pl.meta[0]; status_out[2] = pl.meta[2]; status_out[3] = pl.meta[3];
  }
  __shared__ int s_edge[256], s_pose[256], s_live[256];
  __shared__ int s_L;
  __shared__ double s_blk[kSigmaBlocks * 36];
  if (k >= pl.meta[0]) return;                            // (uniform)
  const int failed = (P > 0 ? flag[0] : 0) | pl.meta[2];
  const int e0 = pl.eptr[k], deg = pl.eptr[k + 1] - e0;
  const bool rows_lds = deg <= 255;
  if (rows_lds && static_cast<int>(threadIdx.x) <= deg) {
    const int r = static_cast<int>(threadIdx.x) - 1;      // row -1 = the frame's own pose row (Ei), rows 0.. = its out-edges (Eij)
    int e = 0, p;
    if (r < 0) p = pl.kx[k] - t0;
    else { e = pl.eidx[e0 + r]; p = static_cast<int>(jj[e]) - t0; }
    s_edge[threadIdx.x] = e; s_pose[threadIdx.x] = (p >= 0 && p < P) ? p : -1;
  }
  __syncthreads();
  if (rows_lds && threadIdx.x == 0) {                     // the live rows, in row order
    int L = 0;
    for (int q = 0; q <= deg; ++q) if (s_pose[q] >= 0) s_live[L++] = q;
    s_L = L;
  }
  __syncthreads();
  const int L = rows_lds ? s_L : 0;
  const bool blk_lds = rows_lds && !failed && L * (L + 1) / 2 <= kSigmaBlocks;
  if (blk_lds) {
    for (int r = 0; r < L; ++r) {
      const int pr = s_pose[s_live[r]], base = r * L - r * (r - 1) / 2;
      for (int i = threadIdx.x; i < (L - r) * 36; i += 256) {
        const int s = r + i / 36, el = i - (i / 36) * 36, a = el / 6, b = el - a * 6;
        s_blk[(base + s - r) * 36 + el] = X[static_cast<long long>(6 * pr + a) * n + 6 * s_pose[s_live[s]] + b];
      }
    }
  }
  __syncthreads();
  if (x >= HW) return;
  const long long o = static_cast<long long>(pl.kx[k]) * HW + x;
  const float qv = Q[static_cast<long long>(k) * HW + x];
  if (var_cond) var_cond[o] = qv;
  if (!var_pose) return;
  if (failed) { var_pose[o] = __builtin_inff(); return; }
  double q = 0.0;
  if (rows_lds) {
    for (int r = 0; r < L; ++r) {
      const int qr = s_live[r], pr = s_pose[qr];
      double er[6], es[6];
      sigma_load6(qr == 0 ? Ei + static_cast<long long>(pr) * 6 * HW : Eij + static_cast<long long>(s_edge[qr]) * 6 * HW, HW, x, er);
      const int base = r * L - r * (r - 1) / 2;
      q += blk_lds ? sigma_block(er, er, s_blk + base * 36, 6) : sigma_block(er, er, X + static_cast<long long>(6 * pr) * n + 6 * pr, n);
      double off = 0.0;
      for (int s = r + 1; s < L; ++s) {
        const int qs = s_live[s], ps = s_pose[qs];
        sigma_load6(Eij + static_cast<long long>(s_edge[qs]) * 6 * HW, HW, x, es);      // (row 0, the own pose row, is never a later row)
        off += blk_lds ? sigma_block(er, es, s_blk + (base + s - r) * 36, 6) : sigma_block(er, es, X + static_cast<long long>(6 * pr) * n + 6 * ps, n);
      }
      q += 2.0 * off;
    }
  } else {
    for (int r = -1; r < deg; ++r) {
      const RowRef Rr = row_of(r, k, pl, Ei, Eij, jj, HW, t0, P);
      if (Rr.pose < 0) continue;
      double er[6], es[6];
      sigma_load6(Rr.base, HW, x, er);
      q += sigma_block(er, er, X + static_cast<long long>(6 * Rr.pose) * n + 6 * Rr.pose, n);
      double off = 0.0;
      for (int s = r + 1; s < deg; ++s) {
        const RowRef Rs = row_of(s, k, pl, Ei, Eij, jj, HW, t0, P);
        if (Rs.pose < 0) continue;
        sigma_load6(Rs.base, HW, x, es);
        off += sigma_block(er, es, X + static_cast<long long>(6 * Rr.pose) * n + 6 * Rs.pose, n);
      }
      q += 2.0 * off;
    }
  }
  const double qd = static_cast<double>(qv);
  var_pose[o] = static_cast<float>(qd * qd * (q > 0.0 ? q : 0.0));
}
}  // namespace
