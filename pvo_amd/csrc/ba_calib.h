// ---------------------------------------------------------------------------
// calib: the four intrinsics c = (fx, fy, cx, cy) as a border of the depth BA's system (pvo_ba_calib, include/pvo_hip.h)
// ---------------------------------------------------------------------------
#pragma once
#include "ba_assemble.h"
#include "ba_backsub.h"
#include "ba_sigma.h"

namespace {
// A stage behind pvo_ba_local, like sigma: `sys` holds A - E Q E^T and the right-hand side in fixed point, the workspace Q, w, Ei, Eij.
// Per Gauss-Newton step, after pvo_ba_local's own launches:
//   assemble  grid (256-pixel chunk, edge): pixel_terms' geometry again (its float expressions, so w, r, J and Jz are the bits the
//             assembly used) plus Jc = d(projection)/dc in fp64 from an fp64 relative pose; writes gc = w Jz Jc^T [E][4][HW] and reduces
//             the edge's 62 sums (Hc_i 24, Hc_j 24, Hcc 10, vc 4) per workgroup in a fixed order, then adds them in 64-bit fixed point.
//   schur     grid (256-pixel chunk, depth frame): Gc = sum of the frame's gc, stored for the back-substitution; subtracts
//             Q m Gc^T per live row (24 sums each), Q Gc Gc^T (10) and Q w Gc (4) from the same fixed-point border.
//   inverse   the sigma stage's prepare / factor / invtri / product kernels as they are: S_d^-1 in fp64.
//   solve     one workgroup: dx0 = S_d^-1 b, Y = S_d^-1 Sc, the 4 x 4 complement T = Scc + damping - Sc^T Y restricted to the free
//             parameters, dc = T^-1 (rc - Sc^T dx0), dx = dx0 - Y dc; the acceptance tests; retraction of poses and intrinsics.
//   backsub   ba_backsub_kernel's arithmetic with Gc^T dc beside the pose rows; a rejected step returns before it writes.
// The border's sums are integers (units of 2^-32; addends are fp64 workgroup sums, |v| < 4e6: a few thousand times a real window's
// largest entry, and 500 addends of that size still fit): they commute, so the border is bitwise reproducible like `sys`.
constexpr int kCalibMaxPoses = 64;
constexpr double kFixC = 4294967296.0, kInvFixC = 1.0 / 4294967296.0;

struct CalibWs {
  long long* fix;        // [6P * 4 + 16 + 4]  Sc row-major, Scc, rc
  float* gc;             // [E][4][HW]
  float* Gc;             // [F'][4][HW]
  double* X;             // [(6P)^2]  S_d^-1
  float* dc;             // [4] the step's dc, then int: [4] step rejected, [5] a border addend was out of range
  size_t bytes;
};

__host__ CalibWs carve_calib(void* base, int E, int P, int F, int HW) {
  CalibWs c{};
  char* p = static_cast<char*>(base);
  size_t off = 0;
  auto take = [&](size_t bytes) { char* r = p ? p + off : nullptr; off += align_up(bytes); return r; };
  const int Kmax = depth_rows_bound(F, P, E);
  const size_t n6 = static_cast<size_t>(6) * (P > 0 ? P : 0);
  c.fix = reinterpret_cast<long long*>(take(sizeof(long long) * (n6 * 4 + 20)));
  c.gc = reinterpret_cast<float*>(take(sizeof(float) * static_cast<size_t>(E) * 4 * HW));
  c.Gc = reinterpret_cast<float*>(take(sizeof(float) * static_cast<size_t>(Kmax) * 4 * HW));
  c.X = reinterpret_cast<double*>(take(sizeof(double) * (n6 * n6 + 8)));
  c.dc = reinterpret_cast<float*>(take(sizeof(float) * 8));
  c.bytes = off;
  return c;
}

__device__ __forceinline__ void cfix_add(long long* fix, int idx, double v, int* cflag) {
  if (!(fabs(v) < 4.0e6)) { *cflag = 1; return; }
  atomicAdd(reinterpret_cast<unsigned long long*>(fix + idx), static_cast<unsigned long long>(__double2ll_rn(v * kFixC)));
}

__device__ __forceinline__ double wave_sum_f64(double v) {      // fixed order; every lane ends with the sum
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// Sums v[0..N) over the workgroup's 256 threads (wave sums, then the four waves in order) and hands sum n to emit(n, sum) on
// thread n.  Uniform: every thread of the workgroup calls it.
template <int N, class Emit>
__device__ __forceinline__ void calib_block_sums(const double (&v)[N], double (*red)[64], Emit emit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const double s = wave_sum_f64(v[n]);
    if (lane == 0) red[wave][n] = s;
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < N) {
    const int n = threadIdx.x;
    emit(n, (red[0][n] + red[1][n]) + (red[2][n] + red[3][n]));
  }
}

// G_ij = G_j G_i^-1 in fp64 from the stored fp32 poses: rotation matrix R (row-major) and translation t.  rotate()'s formula,
// R = I + 2 w K + 2 K^2 with K = [q_xyz]x, on the quaternion product.
__device__ __forceinline__ void calib_rel_pose_f64(const float* __restrict__ pi, const float* __restrict__ pj, double (&R)[9], double (&t)[3]) {
  const double ax = pj[3], ay = pj[4], az = pj[5], aw = pj[6];
  const double bx = -static_cast<double>(pi[3]), by = -static_cast<double>(pi[4]), bz = -static_cast<double>(pi[5]), bw = pi[6];
  const double x = aw * bx + ax * bw + ay * bz - az * by;
  const double y = aw * by + ay * bw + az * bx - ax * bz;
  const double z = aw * bz + az * bw + ax * by - ay * bx;
  const double w = aw * bw - ax * bx - ay * by - az * bz;
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
  const double tx = pi[0], ty = pi[1], tz = pi[2];
  t[0] = pj[0] - (R[0] * tx + R[1] * ty + R[2] * tz);
  t[1] = pj[1] - (R[3] * tx + R[4] * ty + R[5] * tz);
  t[2] = pj[2] - (R[6] * tx + R[7] * ty + R[8] * tz);
}

__global__ __launch_bounds__(256) void ba_calib_assemble_kernel(
    const float* __restrict__ poses, const float* __restrict__ disps, const float* __restrict__ intr,
    const float* __restrict__ targets, const float* __restrict__ weights,
    const int64_t* __restrict__ ii, const int64_t* __restrict__ jj,
    float* __restrict__ gc, long long* __restrict__ fix, int* __restrict__ cflag, int HW, int wd, int t0, int P) {
  __shared__ double red[4][64];
  const int e = blockIdx.y;
  const int ix = static_cast<int>(ii[e]), jx = static_cast<int>(jj[e]);
  EdgeGeom g;
  g.fx = intr[0]; g.fy = intr[1]; g.cx = intr[2]; g.cy = intr[3];
  g.G = rel_pose(load_pose(poses + 7 * static_cast<long long>(ix)), load_pose(poses + 7 * static_cast<long long>(jx)));
  double R[9], t[3];
  calib_rel_pose_f64(poses + 7 * static_cast<long long>(ix), poses + 7 * static_cast<long long>(jx), R, t);
  const double fx = g.fx, fy = g.fy, cx = g.cx, cy = g.cy;
  double s[62];      // Hc_i [6][4], Hc_j [6][4], Hcc upper triangle (n, m <= n), vc [4]
#pragma unroll
  for (int n = 0; n < 62; ++n) s[n] = 0.0;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < HW) {
    const int i = k / wd, j = k - i * wd;
    const float* __restrict__ tg = targets + static_cast<long long>(e) * 2 * HW;
    const float* __restrict__ wg = weights + static_cast<long long>(e) * 2 * HW;
    const float disp = disps[static_cast<long long>(ix) * HW + k];
    // the assembly's own pixel (ba_assemble.h), both rows kept: J = [Ji | Jj], Jz, residual, weight
    const EdgePixel pix = project_pixel(g, static_cast<float>(j), static_cast<float>(i), disp, tg[k], tg[HW + k], wg[k], wg[HW + k]);
    float Ju[12], Jv[12];
    pose_jacobian<0>(g, pix, Ju);
    pose_jacobian<1>(g, pix, Jv);
    const float Jzu = depth_jacobian<0>(g, pix), Jzv = depth_jacobian<1>(g, pix);
    // Jc in fp64 (include/pvo_hip.h: the closed form)
    const double px = (static_cast<double>(j) - cx) / fx, py = (static_cast<double>(i) - cy) / fy, dd = disp;
    const double X = R[0] * px + R[1] * py + R[2] + dd * t[0];
    const double Y = R[3] * px + R[4] * py + R[5] + dd * t[1];
    const double Z = R[6] * px + R[7] * py + R[8] + dd * t[2];
    const double d = pix.ok ? 1.0 / Z : 0.0, d2 = d * d;
    const double a0 = fx * (d * R[0] - X * d2 * R[6]), a1 = fx * (d * R[1] - X * d2 * R[7]);
    const double b0 = fy * (d * R[3] - Y * d2 * R[6]), b1 = fy * (d * R[4] - Y * d2 * R[7]);
    const double ju[4] = {X * d - a0 * px / fx, -a1 * py / fy, 1.0 - a0 / fx, -a1 / fy};
    const double jv[4] = {-b0 * px / fx, Y * d - b1 * py / fy, -b0 / fx, 1.0 - b1 / fy};
    const double wud = pix.wu, wvd = pix.wv;
    const double zu = wud * static_cast<double>(Jzu), zv = wvd * static_cast<double>(Jzv);
#pragma unroll
    for (int n = 0; n < 4; ++n)
      gc[(static_cast<long long>(e) * 4 + n) * HW + k] = static_cast<float>(zu * ju[n] + zv * jv[n]);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double iu = wud * static_cast<double>(Ju[a]), iv = wvd * static_cast<double>(Jv[a]);
      const double ju_ = wud * static_cast<double>(Ju[6 + a]), jv_ = wvd * static_cast<double>(Jv[6 + a]);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        s[a * 4 + n] = iu * ju[n] + iv * jv[n];
        s[24 + a * 4 + n] = ju_ * ju[n] + jv_ * jv[n];
      }
    }
    {
      int l = 48;
#pragma unroll
      for (int n = 0; n < 4; ++n) {
#pragma unroll
        for (int m = 0; m <= n; ++m) { s[l] = wud * ju[n] * ju[m] + wvd * jv[n] * jv[m]; ++l; }
      }
    }
    const double rwu = wud * static_cast<double>(pix.ru), rwv = wvd * static_cast<double>(pix.rv);
#pragma unroll
    for (int n = 0; n < 4; ++n) s[58 + n] = rwu * ju[n] + rwv * jv[n];
  }
  const int pi = ix - t0, pj = jx - t0, n6 = 6 * P;
  calib_block_sums<62>(s, red, [&](int n, double sum) {
    if (n < 24) { if (pi >= 0 && pi < P) cfix_add(fix, (6 * pi) * 4 + n, sum, cflag); }
    else if (n < 48) { if (pj >= 0 && pj < P) cfix_add(fix, (6 * pj) * 4 + (n - 24), sum, cflag); }
    else if (n < 58) {
      int r, m;
      tri_unrank(n - 48, r, m);
      cfix_add(fix, 4 * n6 + r * 4 + m, sum, cflag);
      if (r != m) cfix_add(fix, 4 * n6 + m * 4 + r, sum, cflag);
    } else cfix_add(fix, 4 * n6 + 16 + (n - 58), sum, cflag);
  });
}

__global__ __launch_bounds__(256) void ba_calib_schur_kernel(
    Plan pl, const int64_t* __restrict__ jj, const float* __restrict__ Ei, const float* __restrict__ Eij,
    const float* __restrict__ Q, const float* __restrict__ w, const float* __restrict__ gc, float* __restrict__ Gc,
    long long* __restrict__ fix, int* __restrict__ cflag, int HW, int t0, int P) {
  __shared__ double red[4][64];
  const int k = blockIdx.y;
  if (k >= pl.meta[0]) return;                            // (uniform)
  const int x = blockIdx.x * 256 + threadIdx.x;
  const bool in = x < HW;
  const int e0 = pl.eptr[k], deg = pl.eptr[k + 1] - e0, n6 = 6 * P;
  float G[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (in) {
    for (int o = 0; o < deg; ++o) {
      const int e = pl.eidx[e0 + o];
#pragma unroll
      for (int n = 0; n < 4; ++n) G[n] += gc[(static_cast<long long>(e) * 4 + n) * HW + x];
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) Gc[(static_cast<long long>(k) * 4 + n) * HW + x] = G[n];
  }
  const double q = in ? static_cast<double>(Q[static_cast<long long>(k) * HW + x]) : 0.0;
  const double qw = in ? q * static_cast<double>(w[static_cast<long long>(k) * HW + x]) : 0.0;
  const double Gd[4] = {G[0], G[1], G[2], G[3]};
  {
    double s[14];
    int l = 0;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
#pragma unroll
      for (int m = 0; m <= n; ++m) { s[l] = -(q * Gd[n] * Gd[m]); ++l; }
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) s[10 + n] = -(qw * Gd[n]);
    calib_block_sums<14>(s, red, [&](int n, double sum) {
      if (n < 10) {
        int r, m;
        tri_unrank(n, r, m);
        cfix_add(fix, 4 * n6 + r * 4 + m, sum, cflag);
        if (r != m) cfix_add(fix, 4 * n6 + m * 4 + r, sum, cflag);
      } else cfix_add(fix, 4 * n6 + 16 + (n - 10), sum, cflag);
    });
  }
  for (int r = -1; r < deg; ++r) {                        // the rows the sigma kernel walks: LIVE iff 0 <= pose < P
    const RowRef Rr = row_of(r, k, pl, Ei, Eij, jj, HW, t0, P);
    if (Rr.pose < 0) continue;                            // (uniform)
    double s[24];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double m = in ? q * static_cast<double>(Rr.base[static_cast<long long>(a) * HW + x]) : 0.0;
#pragma unroll
      for (int n = 0; n < 4; ++n) s[a * 4 + n] = -(m * Gd[n]);
    }
    const int p = Rr.pose;
    calib_block_sums<24>(s, red, [&](int n, double sum) { cfix_add(fix, (6 * p) * 4 + n, sum, cflag); });
  }
}

// The bordered solve and the retraction of poses and intrinsics: one workgroup of 1024 threads.  X = S_d^-1 (symmetric), `flag`
// the factorisation's failure word.  Rejected (include/pvo_hip.h): nothing is retracted, dx / dc are zeros, dcw[4] tells the
// back-substitution to leave the depth maps alone.
__global__ __launch_bounds__(1024) void ba_calib_solve_kernel(
    const long long* __restrict__ sys, const double* __restrict__ X, const int* __restrict__ flag, const long long* __restrict__ fix,
    int* __restrict__ meta, float* __restrict__ poses, float* __restrict__ intr, float* __restrict__ dx_ws, float* __restrict__ dx_out,
    float* __restrict__ dcw, float* __restrict__ dc_out, int* __restrict__ status_out, int P, int t0, float lm, float ep_c, int free_mask) {
  constexpr int kN = 6 * kCalibMaxPoses;
  __shared__ double s_b[kN], s_dx0[kN], s_Sc[kN * 4], s_Y[kN * 4];
  __shared__ double s_Scc[16], s_rc[4], s_T[16], s_g[4], s_dc[4];
  __shared__ int s_fail;
  const int n = 6 * P, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* cflags = reinterpret_cast<int*>(dcw) + 4;
  for (int i = tid; i < n; i += 1024) s_b[i] = static_cast<double>(sys[static_cast<long long>(n) * n + i]) * kInvFix;
  for (int i = tid; i < 4 * n; i += 1024) s_Sc[i] = static_cast<double>(fix[i]) * kInvFixC;
  if (tid < 16) s_Scc[tid] = static_cast<double>(fix[4 * n + tid]) * kInvFixC;
  if (tid < 4) s_rc[tid] = static_cast<double>(fix[4 * n + 16 + tid]) * kInvFixC;
  if (tid == 0) s_fail = (flag[0] | meta[2] | meta[3] | meta[4] | cflags[1]) ? 1 : 0;
  __syncthreads();
  const bool pre_failed = s_fail != 0;                    // (uniform; X is not finite after a failed factorisation)
  if (!pre_failed) {
    for (int a = wave; a < n; a += 16) {                  // dx0 = X b, Y = X Sc: one wave per row
      double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int k = lane; k < n; k += 64) {
        const double xv = X[static_cast<long long>(a) * n + k];
        acc[0] += xv * s_b[k];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[1 + c] += xv * s_Sc[k * 4 + c];
      }
#pragma unroll
      for (int c = 0; c < 5; ++c) acc[c] = wave_sum_f64(acc[c]);
      if (lane == 0) {
        s_dx0[a] = acc[0];
#pragma unroll
        for (int c = 0; c < 4; ++c) s_Y[a * 4 + c] = acc[1 + c];
      }
    }
  }
  __syncthreads();
  if (!pre_failed) {
    for (int item = wave; item < 20; item += 16) {        // T = Scc - Sc^T Y (16), g = rc - Sc^T dx0 (4)
      const int c = (item < 16) ? item >> 2 : item - 16, c2 = item & 3;
      double acc = 0.0;
      for (int i = lane; i < n; i += 64) acc += s_Sc[i * 4 + c] * (item < 16 ? s_Y[i * 4 + c2] : s_dx0[i]);
      acc = wave_sum_f64(acc);
      if (lane == 0) { if (item < 16) s_T[item] = s_Scc[item] - acc; else s_g[c] = s_rc[c] - acc; }
    }
  }
  __syncthreads();
  if (tid == 0) {
    double dc[4] = {0.0, 0.0, 0.0, 0.0};
    int failed = pre_failed ? 1 : 0;
    if (!failed) {
      int idx[4], m = 0;
      for (int c = 0; c < 4; ++c) if ((free_mask >> c) & 1) idx[m++] = c;
      double L[4][4], y[4];
      for (int a = 0; a < m && !failed; ++a) {            // Cholesky of the free parameters' block (its upper triangle, mirrored)
        for (int b = 0; b <= a; ++b) {
          const int ca = idx[a], cb = idx[b];
          double v = s_T[cb * 4 + ca];
          if (a == b) v += static_cast<double>(ep_c) + static_cast<double>(lm) * s_Scc[ca * 4 + ca];
          for (int k = 0; k < b; ++k) v -= L[a][k] * L[b][k];
          if (a == b) {
            if (!(v > 0.0) || !(v < 1.0e300)) { failed = 1; break; }
            L[a][a] = sqrt(v);
          } else L[a][b] = v / L[b][b];
        }
      }
      if (!failed) {
        for (int a = 0; a < m; ++a) { double v = s_g[idx[a]]; for (int k = 0; k < a; ++k) v -= L[a][k] * y[k]; y[a] = v / L[a][a]; }
        for (int a = m - 1; a >= 0; --a) { double v = y[a]; for (int k = a + 1; k < m; ++k) v -= L[k][a] * y[k]; y[a] = v / L[a][a]; }
        for (int a = 0; a < m; ++a) dc[idx[a]] = y[a];
        for (int c = 0; c < 4; ++c) if (!(fabs(dc[c]) < 1.0e300)) failed = 1;
        // the focal lengths must stay positive (in the arithmetic of the retraction: float)
        if (!failed && (!(intr[0] + static_cast<float>(dc[0]) > 0.0f) || !(intr[1] + static_cast<float>(dc[1]) > 0.0f))) failed = 1;
      }
    }
    for (int c = 0; c < 4; ++c) s_dc[c] = dc[c];
    s_fail = failed;
  }
  __syncthreads();
  int bad = 0;
  if (!s_fail) {
    for (int i = tid; i < n; i += 1024) {
      double v = s_dx0[i];
#pragma unroll
      for (int c = 0; c < 4; ++c) v -= s_Y[i * 4 + c] * s_dc[c];
      s_dx0[i] = v;
      if (!(fabs(v) < 1.0e30)) bad = 1;
    }
  }
  const int failed = __syncthreads_or(bad) | s_fail;
  for (int i = tid; i < n; i += 1024) {
    const float v = failed ? 0.0f : static_cast<float>(s_dx0[i]);
    dx_ws[i] = v;
    if (dx_out) dx_out[i] = v;
  }
  __syncthreads();
  if (!failed) {
    for (int p = tid; p < P; p += 1024) {                 // pose_retr_kernel, as solve_epilogue
      float xi[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) xi[c] = dx_ws[6 * p + c];
      float* ps = poses + 7 * static_cast<long long>(t0 + p);
      const Pose T = retract(xi, load_pose(ps));
      ps[0] = T.t.x; ps[1] = T.t.y; ps[2] = T.t.z;
      ps[3] = T.q.x; ps[4] = T.q.y; ps[5] = T.q.z; ps[6] = T.q.w;
    }
  }
  if (tid == 0) {
    for (int c = 0; c < 4; ++c) {
      const float v = failed ? 0.0f : static_cast<float>(s_dc[c]);
      dcw[c] = v;
      if (dc_out) dc_out[c] = v;
      if (!failed && ((free_mask >> c) & 1)) intr[c] = intr[c] + v;
    }
    cflags[0] = failed;
    cflags[1] = 0;
    meta[4] = 0;
    if (failed) meta[1] = 1;
    if (status_out) { status_out[0] = meta[1]; status_out[1] = meta[0]; status_out[2] = meta[2]; status_out[3] = meta[3]; }
  }
}

// ba_backsub_body with the intrinsics' term: dz = Q (w - sum_r E_r^T dx[pose(r)] - Gc^T dc), the same live rows, the skip of
// window pose 0 included.  No clamp (pvo_ba_calib has none, as pvo_ba).
__global__ __launch_bounds__(256) void ba_calib_backsub_kernel(
    Plan pl, const int64_t* __restrict__ jj, const float* __restrict__ Ei, const float* __restrict__ Eij,
    const float* __restrict__ Q, const float* __restrict__ w, const float* __restrict__ dx,
    const float* __restrict__ Gc, const float* __restrict__ dcw,
    float* __restrict__ disps, float* __restrict__ dz_out, int dz_rows, int HW, int t0, int P) {
  ba_backsub_body<true>(pl, jj, Ei, Eij, Q, w, dx, disps, dz_out, dz_rows, HW, t0, P, 0, 0.0f, Gc, dcw);
}
}  // namespace
