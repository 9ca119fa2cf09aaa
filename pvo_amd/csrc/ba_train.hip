// ba_train.hip — the differentiable bundle adjustment of the training path: one Gauss-Newton step of pvo_amd.geom.ba.BA
// (reference VO_Module/droid_slam/geom/ba.py:31-106, geom/chol.py:5-73) forward and backward, a handful of launches per
// direction and no host synchronisation.
//
// Forward (pvo_ba_train):
//   proj_fwd_kernel (se3_ops.hip, through pvo_proj_transform)  coordinates, validity and the three Jacobians of every edge
//   ba_train_assemble   (pixel chunk, edge, batch)     Ei / Ej / Ck / wk per edge and pixel; per-chunk partials of the 12x12
//                                                      upper triangle [Ji Jj]^T W [Ji Jj] and of the gradient [vi vj]
//   ba_train_depth      (pixel chunk, keyframe, batch) C, wz, Q = 1/C and E[a,k,p] summed over the keyframe's edges in edge order
//                                                      (CSR of the edges by keyframe); each pixel is owned by one thread
//   ba_train_schur      (pixel chunk, pose pair, batch) per-chunk partials of sum Q E_a E_c^T and sum Q wz E_a
//   ba_train_solve      (batch)                        H gathered from the edge partials, damped, S = Hd - E Q E^T, y = v - E Q wz,
//                                                      Cholesky of S in LDS, dx, the failure flag, retraction of the poses
//   ba_train_backsub    (pixel chunk, frame, batch)    dz = Q (wz - E^T dx), disps += dz, the `> 10 -> 0` / clamp(min=0) masks
// Partials are summed in a fixed order and there are no floating-point atomics: two identical calls give bit-identical outputs.
//
// Backward (pvo_ba_train_vjp; reads the forward's state, works in a scratch buffer of its own), with u = S^-1 gdx (the gradient
// of S is the rank-1 -dx u^T, so nothing of size (6Pf)^2 is built):
//   ba_train_vjp_reduce   (pixel chunk, pose, batch)  per-chunk partials of sum Q gdz E_a (the part of gdx that comes through dz)
//   ba_train_vjp_solve    (batch)                     retraction VJP (dual numbers on se3_dual.h's templates), gdx, u = S^-1 gdx
//   ba_train_vjp_depth    (pixel chunk, frame, batch) mask VJP, g_eta, and per (keyframe, pixel) the four scalars the edges need
//   ba_train_vjp_assemble (pixel chunk, edge, batch)  g_target, g_weight and the gradients of coordinates and Jacobians
//   proj_vjp_kernel (se3_ops.hip, through pvo_proj_transform_vjp)  pose and depth gradients through the Jacobians (fp atomics)
//
// Layouts: poses [B,P,7], disps [B,P,HW], intr [B,P,4], target / weight [B,N,HW,2], eta [B,M,HW], ii / jj [N] int64 on the
// device; the plan kx [M] (keyframes, ascending), kk [N] (keyframe of each edge), kptr [M+1] / kedge [N] (edges of each keyframe
// in edge order) int32.  Free poses a = frame - fixedp in [0, Pf); blocks that touch a fixed pose are dropped.
#include "se3_dual.h"

namespace {

constexpr int kChunk = 256;        // pixels per chunk of the per-pixel kernels (one thread each; 64-thread reductions visit 4)
constexpr int kMaxFree = 16;       // free poses: the reduced system is at most 96 x 96
constexpr int kHv = 90;            // 78 upper-triangle entries of the 12x12 edge block + 12 gradient entries
constexpr int kSv = 42;            // 36 entries of a 6x6 Schur block + 6 of its right-hand side
constexpr double kEp = 0.1, kLm = 1e-4;

// the call's buffers (see ws_layout): the forward's state, kept with the call until its backward (x1 .. flag), and the
// backward's scratch, needed only while pvo_ba_train_vjp runs (gp .. gJz)
template <typename F> struct Bufs {
  F *x1, *valid, *Ji, *Jj, *Jz, *Ei, *Ej, *Ck, *wk, *Hp, *E, *Q, *wz, *Sp, *L, *dx, *d1, *flag;
  F *gp, *u, *gC, *gwz, *qa, *qb, *gx1, *gJi, *gJj, *gJz;
};

struct Dims { int B, P, N, M, HW, Pf, fixedp, nch; };

// scratch == false: the state's buffers carved from `base` (NULL: sizes only), true: the backward's scratch; returns the bytes used
template <typename F> __host__ size_t ws_layout(const Dims& d, bool scratch, char* base, Bufs<F>* b) {
  const long long BN = 1LL * d.B * d.N * d.HW, BM = 1LL * d.B * d.M * d.HW, n = 6LL * d.Pf;
  size_t off = 0;
  auto take = [&](F** p, long long elems) {
    if (b) *p = reinterpret_cast<F*>(base + off);
    off += (static_cast<size_t>(elems > 0 ? elems : 1) * sizeof(F) + 255) & ~static_cast<size_t>(255);
  };
  Bufs<F> tmp;
  Bufs<F>* o = b ? b : &tmp;
  if (!scratch) {
    take(&o->x1, BN * 2); take(&o->valid, BN); take(&o->Ji, BN * 12); take(&o->Jj, BN * 12); take(&o->Jz, BN * 2);
    take(&o->Ei, BN * 6); take(&o->Ej, BN * 6); take(&o->Ck, BN); take(&o->wk, BN);
    take(&o->Hp, 1LL * d.B * d.N * d.nch * kHv);
    take(&o->E, BM * d.Pf * 6); take(&o->Q, BM); take(&o->wz, BM);
    take(&o->Sp, 1LL * d.B * d.Pf * d.Pf * d.nch * kSv);
    take(&o->L, d.B * n * n); take(&o->dx, d.B * n); take(&o->d1, 1LL * d.B * d.P * d.HW); take(&o->flag, d.B);
  } else {
    take(&o->gp, 1LL * d.B * d.Pf * d.nch * 6); take(&o->u, d.B * n);
    take(&o->gC, BM); take(&o->gwz, BM); take(&o->qa, BM); take(&o->qb, BM);
    take(&o->gx1, BN * 2); take(&o->gJi, BN * 12); take(&o->gJj, BN * 12); take(&o->gJz, BN * 2);
  }
  return off;
}

__device__ __forceinline__ int free_pose(long long f, int fixedp, int Pf) {
  const long long a = f - fixedp;
  return (a >= 0 && a < Pf) ? static_cast<int>(a) : -1;
}
__device__ __forceinline__ int keyframe_of(const int* kx, int M, int f) {
  for (int m = 0; m < M; ++m)
    if (kx[m] == f) return m;
  return -1;
}
// gradient of where(d1 > 10, 0, d1).clamp(min=0) with respect to d1 (torch: where's and clamp_min's backward)
template <typename F> __device__ __forceinline__ F mask_grad(F d1, F g) { return (!(d1 > F(10)) && d1 >= F(0)) ? g : F(0); }

// sum of K values over the 64 threads of a workgroup, in a fixed order (red: 64 * (K + 1) elements of LDS)
template <typename F, int K> __device__ __forceinline__ void block64_sum(const F* acc, F* red, F* out) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < K; ++k) red[t * (K + 1) + k] = acc[k];
  __syncthreads();
  for (int k = t; k < K; k += 64) {
    F s = F(0);
    for (int i = 0; i < 64; ++i) s += red[i * (K + 1) + k];
    out[k] = s;
  }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(64) void ba_train_assemble(Bufs<F> w, Dims d, const F* __restrict__ target, const F* __restrict__ weight) {
  __shared__ F red[64 * (kHv + 1)];
  const int ch = blockIdx.x, n = blockIdx.y, b = blockIdx.z;
  F acc[kHv];
#pragma unroll
  for (int k = 0; k < kHv; ++k) acc[k] = F(0);
  for (int q = 0; q < kChunk / 64; ++q) {
    const int p = ch * kChunk + q * 64 + threadIdx.x;
    if (p >= d.HW) break;
    const long long row = (1LL * b * d.N + n) * d.HW + p;
    const F vld = w.valid[row];
    F ei[6], ej[6], ck = F(0), wkv = F(0);
#pragma unroll
    for (int k = 0; k < 6; ++k) { ei[k] = F(0); ej[k] = F(0); }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      F J[12], wJ[12];
#pragma unroll
      for (int k = 0; k < 6; ++k) { J[k] = w.Ji[row * 12 + c * 6 + k]; J[6 + k] = w.Jj[row * 12 + c * 6 + k]; }
      const F jz = w.Jz[row * 2 + c];
      const F wc = F(0.001) * (vld * weight[row * 2 + c]);
      const F rc = target[row * 2 + c] - w.x1[row * 2 + c];
#pragma unroll
      for (int k = 0; k < 12; ++k) wJ[k] = wc * J[k];
      int idx = 0;
#pragma unroll
      for (int r = 0; r < 12; ++r)
#pragma unroll
        for (int s = r; s < 12; ++s) acc[idx++] += wJ[r] * J[s];
#pragma unroll
      for (int r = 0; r < 12; ++r) acc[78 + r] += wJ[r] * rc;
#pragma unroll
      for (int k = 0; k < 6; ++k) { ei[k] += wJ[k] * jz; ej[k] += wJ[6 + k] * jz; }
      ck += (wc * jz) * jz;
      wkv += (wc * rc) * jz;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) { w.Ei[row * 6 + k] = ei[k]; w.Ej[row * 6 + k] = ej[k]; }
    w.Ck[row] = ck;
    w.wk[row] = wkv;
  }
  block64_sum<F, kHv>(acc, red, w.Hp + ((1LL * b * d.N + n) * d.nch + ch) * kHv);
}

template <typename F>
__global__ __launch_bounds__(256) void ba_train_depth(Bufs<F> w, Dims d, const F* __restrict__ eta, const int64_t* __restrict__ ii,
                                                      const int64_t* __restrict__ jj, const int* __restrict__ kptr, const int* __restrict__ kedge) {
  const int p = blockIdx.x * kChunk + threadIdx.x, k = blockIdx.y, b = blockIdx.z;
  if (p >= d.HW) return;
  const int e0 = kptr[k], e1 = kptr[k + 1];
  F C = F(0), wz = F(0);
  for (int t = e0; t < e1; ++t) {
    const long long row = (1LL * b * d.N + kedge[t]) * d.HW + p;
    C += w.Ck[row];
    wz += w.wk[row];
  }
  const long long kp = (1LL * b * d.M + k) * d.HW + p;
  C = (C + eta[kp]) + F(1e-7);
  w.Q[kp] = F(1) / C;
  w.wz[kp] = wz;
  for (int a = 0; a < d.Pf; ++a) {
    F s[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c] = F(0);
    for (int t = e0; t < e1; ++t) {                     // (pose a as the edges' frame i, then as their frame j: the PyTorch sum's order)
      const int e = kedge[t];
      if (free_pose(ii[e], d.fixedp, d.Pf) == a) {
        const long long row = (1LL * b * d.N + e) * d.HW + p;
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c] += w.Ei[row * 6 + c];
      }
    }
    for (int t = e0; t < e1; ++t) {
      const int e = kedge[t];
      if (free_pose(jj[e], d.fixedp, d.Pf) == a) {
        const long long row = (1LL * b * d.N + e) * d.HW + p;
#pragma unroll
        for (int c = 0; c < 6; ++c) s[c] += w.Ej[row * 6 + c];
      }
    }
    F* dst = w.E + (((1LL * b * d.Pf + a) * d.M + k) * d.HW + p) * 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) dst[c] = s[c];
  }
}

// workgroup (chunk, a * Pf + c, b), a <= c: sum over the chunk's pixels of every keyframe of Q E_a E_c^T (and, for a == c, Q wz E_a)
template <typename F>
__global__ __launch_bounds__(64) void ba_train_schur(Bufs<F> w, Dims d) {
  __shared__ F red[64 * (kSv + 1)];
  const int ch = blockIdx.x, a = blockIdx.y / d.Pf, c = blockIdx.y % d.Pf, b = blockIdx.z;
  if (a > c) return;
  F acc[kSv];
#pragma unroll
  for (int k = 0; k < kSv; ++k) acc[k] = F(0);
  for (int k = 0; k < d.M; ++k) {
    const F* Ea = w.E + ((1LL * b * d.Pf + a) * d.M + k) * d.HW * 6;
    const F* Ec = w.E + ((1LL * b * d.Pf + c) * d.M + k) * d.HW * 6;
    for (int q = 0; q < kChunk / 64; ++q) {
      const int p = ch * kChunk + q * 64 + threadIdx.x;
      if (p >= d.HW) break;
      const long long kp = (1LL * b * d.M + k) * d.HW + p;
      const F Qv = w.Q[kp];
      F ea[6], ec[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) { ea[i] = Ea[p * 6LL + i]; ec[i] = Ec[p * 6LL + i]; }
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const F qe = Qv * ea[i];
#pragma unroll
        for (int j = 0; j < 6; ++j) acc[i * 6 + j] += qe * ec[j];
        acc[36 + i] += qe * w.wz[kp];
      }
    }
  }
  block64_sum<F, kSv>(acc, red, w.Sp + ((1LL * b * d.Pf * d.Pf + a * d.Pf + c) * d.nch + ch) * kSv);
}

// L L^T x = y in place on x (LDS), L row-major n x n (LDS or global); 256 threads
template <typename F> __device__ void chol_solve(const F* L, F* x, int n) {
  const int t = threadIdx.x;
  for (int k = 0; k < n; ++k) {
    if (t == 0) x[k] = x[k] / L[k * n + k];
    __syncthreads();
    for (int i = k + 1 + t; i < n; i += 256) x[i] -= L[i * n + k] * x[k];
    __syncthreads();
  }
  for (int k = n - 1; k >= 0; --k) {
    if (t == 0) x[k] = x[k] / L[k * n + k];
    __syncthreads();
    for (int i = t; i < k; i += 256) x[i] -= L[k * n + i] * x[k];
    __syncthreads();
  }
}

template <typename F>
__global__ __launch_bounds__(256) void ba_train_solve(Bufs<F> w, Dims d, const F* __restrict__ poses, const int64_t* __restrict__ ii,
                                                      const int64_t* __restrict__ jj, F* __restrict__ poses_out, F* __restrict__ dx_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  F* S = reinterpret_cast<F*>(lds_raw);
  const int n = 6 * d.Pf, t = threadIdx.x, b = blockIdx.x;
  F* y = S + n * n;
  __shared__ int fail;
  if (t == 0) fail = 0;
  for (int i = t; i < n * n + n; i += 256) S[i] = F(0);
  __syncthreads();
  // H and v: the edges' blocks in edge order; an edge with i == j adds its four blocks into one, one after another
  for (int e = 0; e < d.N; ++e) {
    const int pi = free_pose(ii[e], d.fixedp, d.Pf), pj = free_pose(jj[e], d.fixedp, d.Pf);
    if (pi < 0 && pj < 0) continue;
    F val = F(0);
    int r = 0, s = 0;
    if (t < 156) {
      int idx;
      if (t < 144) {
        r = t / 12; s = t % 12;
        const int lo = r < s ? r : s, hi = r < s ? s : r;
        idx = lo * 12 - lo * (lo - 1) / 2 + (hi - lo);
      } else {
        r = t - 144; idx = 78 + r;
      }
      const F* src = w.Hp + (1LL * b * d.N + e) * d.nch * kHv + idx;
      for (int ch = 0; ch < d.nch; ++ch) val += src[ch * kHv];
    }
    const int phases = pi == pj ? 4 : 1;
    for (int ph = 0; ph < phases; ++ph) {
      if (t < 144) {
        const int bi = r / 6, bj = s / 6;
        const int pr = bi ? pj : pi, pc = bj ? pj : pi;
        if ((phases == 1 || ph == bi * 2 + bj) && pr >= 0 && pc >= 0) S[(pr * 6 + r % 6) * n + pc * 6 + s % 6] += val;
      } else if (t < 156) {
        const int pv = r < 6 ? pi : pj;
        if ((phases == 1 || ph == r / 6) && pv >= 0) y[pv * 6 + r % 6] += val;
      }
      __syncthreads();
    }
  }
  // damping on the true diagonal (chol._damp_diagonal), then the Schur complement and its right-hand side
  for (int i = t; i < n; i += 256) {
    const F dg = S[i * n + i];
    S[i * n + i] = dg + (F(kEp) + F(kLm) * dg);
  }
  __syncthreads();
  for (int idx = t; idx < n * n; idx += 256) {
    const int R = idx / n, Cc = idx % n, a = R / 6, c = Cc / 6;
    const F* src = a <= c ? w.Sp + ((1LL * b * d.Pf * d.Pf + a * d.Pf + c) * d.nch) * kSv + (R % 6) * 6 + Cc % 6
                          : w.Sp + ((1LL * b * d.Pf * d.Pf + c * d.Pf + a) * d.nch) * kSv + (Cc % 6) * 6 + R % 6;
    F v = F(0);
    for (int ch = 0; ch < d.nch; ++ch) v += src[ch * kSv];
    S[idx] -= v;
  }
  for (int i = t; i < n; i += 256) {
    const int a = i / 6;
    const F* src = w.Sp + ((1LL * b * d.Pf * d.Pf + a * d.Pf + a) * d.nch) * kSv + 36 + i % 6;
    F v = F(0);
    for (int ch = 0; ch < d.nch; ++ch) v += src[ch * kSv];
    y[i] -= v;
  }
  __syncthreads();
  // Cholesky S = L L^T in place (lower triangle), right-looking; a pivot that is not > 0 (or NaN) marks the system as failed
  for (int k = 0; k < n; ++k) {
    if (t == 0) {
      const F dg = S[k * n + k];
      if (!(dg > F(0))) fail = 1;
      S[k * n + k] = sqrt(dg > F(0) ? dg : F(1));
    }
    __syncthreads();
    for (int i = k + 1 + t; i < n; i += 256) S[i * n + k] /= S[k * n + k];
    __syncthreads();
    const int m = n - k - 1;
    for (int idx = t; idx < m * m; idx += 256) {
      const int i = k + 1 + idx / m, j = k + 1 + idx % m;
      if (j <= i) S[i * n + j] -= S[i * n + k] * S[j * n + k];
    }
    __syncthreads();
  }
  const bool ok = fail == 0;
  if (ok) chol_solve(S, y, n);
  __syncthreads();
  // state: the factor (identity where the factorisation failed, as chol.CholeskySolver), dx (0 there), the flag
  F* L = w.L + 1LL * b * n * n;
  for (int idx = t; idx < n * n; idx += 256) {
    const int i = idx / n, j = idx % n;
    L[idx] = ok ? (j <= i ? S[idx] : F(0)) : (i == j ? F(1) : F(0));
  }
  for (int i = t; i < n; i += 256) {
    const F v = ok ? y[i] : F(0);
    y[i] = v;
    w.dx[1LL * b * n + i] = v;
    if (dx_out) dx_out[1LL * b * n + i] = v;
  }
  if (t == 0) w.flag[b] = ok ? F(1) : F(0);
  __syncthreads();
  // retraction Exp(dx) * G of the free poses; the fixed ones are copied (Exp(0) * G == G)
  for (int f = t; f < d.P; f += 256) {
    const F* G = poses + (1LL * b * d.P + f) * 7;
    F* out = poses_out + (1LL * b * d.P + f) * 7;
    const int a = free_pose(f, d.fixedp, d.Pf);
    if (a < 0) {
      for (int k = 0; k < 7; ++k) out[k] = G[k];
    } else {
      F xi[6], g[7], e[7], o[7];
      for (int k = 0; k < 6; ++k) xi[k] = y[a * 6 + k];
      for (int k = 0; k < 7; ++k) g[k] = G[k];
      se3_exp(xi, e);
      se3_bin(OP_MUL, e, g, o);
      for (int k = 0; k < 7; ++k) out[k] = o[k];
    }
  }
}

template <typename F>
__global__ __launch_bounds__(256) void ba_train_backsub(Bufs<F> w, Dims d, const F* __restrict__ disps, const int* __restrict__ kx,
                                                        F* __restrict__ disps_out) {
  const int p = blockIdx.x * kChunk + threadIdx.x, f = blockIdx.y, b = blockIdx.z;
  if (p >= d.HW) return;
  const long long fp = (1LL * b * d.P + f) * d.HW + p;
  F v = disps[fp];
  const int k = keyframe_of(kx, d.M, f);
  if (k >= 0) {
    const long long kp = (1LL * b * d.M + k) * d.HW + p;
    F edx = F(0);
    for (int a = 0; a < d.Pf; ++a) {
      const F* Ea = w.E + (((1LL * b * d.Pf + a) * d.M + k) * d.HW + p) * 6;
      const F* x = w.dx + (1LL * b * d.Pf + a) * 6;
#pragma unroll
      for (int c = 0; c < 6; ++c) edx += Ea[c] * x[c];
    }
    v = v + w.Q[kp] * (w.wz[kp] - edx);
  }
  w.d1[fp] = v;
  F o = v > F(10) ? F(0) : v;
  disps_out[fp] = o < F(0) ? F(0) : o;
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(64) void ba_train_vjp_reduce(Bufs<F> w, Dims d, const int* __restrict__ kx, const F* __restrict__ g_disps_out) {
  __shared__ F red[64 * 7];
  const int ch = blockIdx.x, a = blockIdx.y, b = blockIdx.z;
  F acc[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) acc[c] = F(0);
  for (int k = 0; k < d.M; ++k) {
    const int f = kx[k];
    for (int q = 0; q < kChunk / 64; ++q) {
      const int p = ch * kChunk + q * 64 + threadIdx.x;
      if (p >= d.HW) break;
      const long long fp = (1LL * b * d.P + f) * d.HW + p, kp = (1LL * b * d.M + k) * d.HW + p;
      const F s = w.Q[kp] * mask_grad(w.d1[fp], g_disps_out[fp]);
      const F* Ea = w.E + (((1LL * b * d.Pf + a) * d.M + k) * d.HW + p) * 6;
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[c] += s * Ea[c];
    }
  }
  block64_sum<F, 6>(acc, red, w.gp + ((1LL * b * d.Pf + a) * d.nch + ch) * 6);
}

template <typename F>
__global__ __launch_bounds__(256) void ba_train_vjp_solve(Bufs<F> w, Dims d, const F* __restrict__ poses, const F* __restrict__ g_poses_out,
                                                          F* __restrict__ g_poses) {
  __shared__ F x[6 * kMaxFree];
  const int n = 6 * d.Pf, t = threadIdx.x, b = blockIdx.x;
  for (int f = t; f < d.P; f += 256) {
    const F* gy = g_poses_out + (1LL * b * d.P + f) * 7;
    F* gG = g_poses + (1LL * b * d.P + f) * 7;
    const int a = free_pose(f, d.fixedp, d.Pf);
    if (a < 0) {
      for (int k = 0; k < 7; ++k) gG[k] = gy[k];
      continue;
    }
    // vector-Jacobian product of (xi, G) -> Exp(xi) G: one evaluation on dual numbers per input component (6 + 7)
    F xi[6], G[7], g[7];
    for (int k = 0; k < 6; ++k) xi[k] = w.dx[1LL * b * n + a * 6 + k];
    for (int k = 0; k < 7; ++k) { G[k] = poses[(1LL * b * d.P + f) * 7 + k]; g[k] = gy[k]; }
#pragma unroll 1
    for (int q = 0; q < 13; ++q) {
      Dual<F> X[6], Gd[7], e[7], o[7];
      for (int k = 0; k < 6; ++k) X[k] = Dual<F>(xi[k], k == q ? F(1) : F(0));
      for (int k = 0; k < 7; ++k) Gd[k] = Dual<F>(G[k], k + 6 == q ? F(1) : F(0));
      se3_exp(X, e);
      se3_bin(OP_MUL, e, Gd, o);
      F s = F(0);
      for (int k = 0; k < 7; ++k) s += g[k] * o[k].d;
      if (q < 6) {
        F r = F(0);
        for (int ch = 0; ch < d.nch; ++ch) r += w.gp[((1LL * b * d.Pf + a) * d.nch + ch) * 6 + q];
        x[a * 6 + q] = s - r;
      } else {
        gG[q - 6] = s;
      }
    }
  }
  __syncthreads();
  const bool ok = w.flag[b] != F(0);
  if (ok) chol_solve(w.L + 1LL * b * n * n, x, n);
  __syncthreads();
  for (int i = t; i < n; i += 256) w.u[1LL * b * n + i] = ok ? x[i] : F(0);
}

template <typename F>
__global__ __launch_bounds__(256) void ba_train_vjp_depth(Bufs<F> w, Dims d, const int* __restrict__ kx, const F* __restrict__ g_disps_out,
                                                          F* __restrict__ g_eta, F* __restrict__ g_disps) {
  const int p = blockIdx.x * kChunk + threadIdx.x, f = blockIdx.y, b = blockIdx.z;
  if (p >= d.HW) return;
  const long long fp = (1LL * b * d.P + f) * d.HW + p;
  const F gd = mask_grad(w.d1[fp], g_disps_out[fp]);
  g_disps[fp] = gd;                                        // the direct term; pvo_proj_transform_vjp adds the rest
  const int k = keyframe_of(kx, d.M, f);
  if (k < 0) return;
  const long long kp = (1LL * b * d.M + k) * d.HW + p;
  F edx = F(0), eu = F(0);
  for (int a = 0; a < d.Pf; ++a) {
    const F* Ea = w.E + (((1LL * b * d.Pf + a) * d.M + k) * d.HW + p) * 6;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      edx += Ea[c] * w.dx[(1LL * b * d.Pf + a) * 6 + c];
      eu += Ea[c] * w.u[(1LL * b * d.Pf + a) * 6 + c];
    }
  }
  const F Qv = w.Q[kp], wz = w.wz[kp];
  // dz = Q (wz - E.dx); y = v - Q wz E; S = Hd - Q E E^T with g_S = -dx u^T
  const F gQ = gd * (wz - edx) - wz * eu + edx * eu;
  const F gC = -(Qv * Qv) * gQ;
  g_eta[kp] = gC;
  w.gC[kp] = gC;
  w.gwz[kp] = Qv * (gd - eu);
  w.qa[kp] = Qv * (eu - gd);                                // g_E[a] = qa dx[a] + qb u[a]
  w.qb[kp] = Qv * (edx - wz);
}

template <typename F>
__global__ __launch_bounds__(256) void ba_train_vjp_assemble(Bufs<F> w, Dims d, const F* __restrict__ target, const F* __restrict__ weight,
                                                             const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, const int* __restrict__ kk,
                                                             F* __restrict__ g_target, F* __restrict__ g_weight) {
  const int p = blockIdx.x * kChunk + threadIdx.x, n = blockIdx.y, b = blockIdx.z;
  if (p >= d.HW) return;
  const int pi = free_pose(ii[n], d.fixedp, d.Pf), pj = free_pose(jj[n], d.fixedp, d.Pf), k = kk[n];
  const long long row = (1LL * b * d.N + n) * d.HW + p, kp = (1LL * b * d.M + k) * d.HW + p;
  const F qa = w.qa[kp], qb = w.qb[kp], gC = w.gC[kp], gwz = w.gwz[kp];
  const bool same = pi == pj && pi >= 0;
  F X[12], U[12], Mu[12], gE[12];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int a = s ? pj : pi;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const F xv = a >= 0 ? w.dx[(1LL * b * d.Pf + a) * 6 + c] : F(0);
      const F uv = a >= 0 ? w.u[(1LL * b * d.Pf + a) * 6 + c] : F(0);
      X[s * 6 + c] = xv; U[s * 6 + c] = uv; Mu[s * 6 + c] = xv * uv; gE[s * 6 + c] = qa * xv + qb * uv;
    }
  }
  const F vld = w.valid[row];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    F J[12], DJ[12];
#pragma unroll
    for (int k2 = 0; k2 < 6; ++k2) { J[k2] = w.Ji[row * 12 + c * 6 + k2]; J[6 + k2] = w.Jj[row * 12 + c * 6 + k2]; }
    const F jz = w.Jz[row * 2 + c];
    const F wc = F(0.001) * (vld * weight[row * 2 + c]);
    const F rc = target[row * 2 + c] - w.x1[row * 2 + c];
    F jx = F(0), ju = F(0), jg = F(0), jd = F(0);
#pragma unroll
    for (int k2 = 0; k2 < 12; ++k2) {
      DJ[k2] = Mu[k2] * (J[k2] + (same ? J[(k2 + 6) % 12] : F(0)));      // the damping's diagonal blocks (both when i == j)
      jx += J[k2] * X[k2]; ju += J[k2] * U[k2]; jg += J[k2] * gE[k2]; jd += J[k2] * DJ[k2];
    }
    const F gw = -(jx * ju) - F(kLm) * jd + rc * ju + jz * jg + gC * jz * jz + gwz * rc * jz;
    const F gr = wc * (ju + gwz * jz);
    const F gjz = wc * (jg + F(2) * jz * gC + gwz * rc);
#pragma unroll
    for (int k2 = 0; k2 < 12; ++k2) {
      const F gj = wc * (-(X[k2] * ju) - U[k2] * jx - F(2 * kLm) * DJ[k2] + rc * U[k2] + jz * gE[k2]);
      (k2 < 6 ? w.gJi : w.gJj)[row * 12 + c * 6 + k2 % 6] = gj;
    }
    w.gJz[row * 2 + c] = gjz;
    w.gx1[row * 2 + c] = -gr;
    g_target[row * 2 + c] = gr;
    g_weight[row * 2 + c] = F(0.001) * vld * gw;
  }
}

template <typename F> int lds_bytes(int Pf) { return static_cast<int>(sizeof(F) * (36 * Pf * Pf + 6 * Pf + 2)); }

bool dims_ok(int B, int P, int N, int M, int ht, int wd, int fixedp) {
  return B > 0 && P > 0 && N > 0 && M > 0 && M <= P && ht > 0 && wd > 0 && fixedp >= 0 && fixedp <= P && 1LL * ht * wd < (1LL << 31);
}

Dims make_dims(int B, int P, int N, int M, int HW, int fixedp) {
  return Dims{B, P, N, M, HW, P - fixedp, fixedp, (HW + kChunk - 1) / kChunk};
}

template <typename F>
int train_fwd(const F* poses, const F* disps, const F* intr, const F* target, const F* weight, const F* eta, const int64_t* ii, const int64_t* jj,
              const int* kx, const int* kptr, const int* kedge, int ht, const Dims& d, F* poses_out, F* disps_out, F* dx_out, void* ws,
              int dtype, hipStream_t st) {
  Bufs<F> w;
  ws_layout<F>(d, false, static_cast<char*>(ws), &w);
  int rc = pvo_proj_transform(poses, disps, intr, ii, jj, d.B, d.P, d.N, ht, d.HW / ht, 2, w.x1, w.valid, w.Ji, w.Jj, w.Jz, dtype, st);
  if (rc != PVO_OK) return rc;
  hipLaunchKernelGGL(ba_train_assemble<F>, dim3(d.nch, d.N, d.B), dim3(64), 0, st, w, d, target, weight);
  hipLaunchKernelGGL(ba_train_depth<F>, dim3(d.nch, d.M, d.B), dim3(256), 0, st, w, d, eta, ii, jj, kptr, kedge);
  if (d.Pf > 0) hipLaunchKernelGGL(ba_train_schur<F>, dim3(d.nch, d.Pf * d.Pf, d.B), dim3(64), 0, st, w, d);
  const int lds = lds_bytes<F>(d.Pf);
  // (the largest system, 96 x 96, is asked for at once: one grant per device and type)
  if (lds > 48 * 1024 && !pvo_allow_lds<ba_train_solve<F>>(lds_bytes<F>(kMaxFree))) return PVO_ELAUNCH;
  hipLaunchKernelGGL(ba_train_solve<F>, dim3(d.B), dim3(256), lds, st, w, d, poses, ii, jj, poses_out, dx_out);
  hipLaunchKernelGGL(ba_train_backsub<F>, dim3(d.nch, d.P, d.B), dim3(256), 0, st, w, d, disps, kx, disps_out);
  PVO_CHECK_LAUNCH();
  return PVO_OK;
}

template <typename F>
int train_vjp(const F* poses, const F* disps, const F* intr, const F* target, const F* weight, const int64_t* ii, const int64_t* jj,
              const int* kx, const int* kk, int ht, const Dims& d, const F* g_poses_out, const F* g_disps_out, F* g_target, F* g_weight,
              F* g_eta, F* g_poses, F* g_disps, const void* ws, void* scratch, int dtype, hipStream_t st) {
  Bufs<F> w;
  ws_layout<F>(d, false, const_cast<char*>(static_cast<const char*>(ws)), &w);      // (the state is only read here)
  ws_layout<F>(d, true, static_cast<char*>(scratch), &w);
  if (d.Pf > 0) hipLaunchKernelGGL(ba_train_vjp_reduce<F>, dim3(d.nch, d.Pf, d.B), dim3(64), 0, st, w, d, kx, g_disps_out);
  hipLaunchKernelGGL(ba_train_vjp_solve<F>, dim3(d.B), dim3(256), 0, st, w, d, poses, g_poses_out, g_poses);
  hipLaunchKernelGGL(ba_train_vjp_depth<F>, dim3(d.nch, d.P, d.B), dim3(256), 0, st, w, d, kx, g_disps_out, g_eta, g_disps);
  hipLaunchKernelGGL(ba_train_vjp_assemble<F>, dim3(d.nch, d.N, d.B), dim3(256), 0, st, w, d, target, weight, ii, jj, kk, g_target, g_weight);
  PVO_CHECK_LAUNCH();
  // g_poses / g_disps hold the direct terms: the Jacobians' and coordinates' gradients are added to them
  return pvo_proj_transform_vjp(poses, disps, intr, ii, jj, d.B, d.P, d.N, ht, d.HW / ht, 2, w.gx1, w.gJi, w.gJj, w.gJz, g_poses, g_disps,
                                dtype, st);
}

}  // namespace

namespace {
size_t layout_bytes(int B, int P, int N, int M, int HW, int dtype, bool scratch) {
  if (B <= 0 || P <= 0 || N <= 0 || M <= 0 || HW <= 0 || (dtype != PVO_F32 && dtype != PVO_F64)) return 0;
  const Dims d = make_dims(B, P, N, M, HW, P < kMaxFree ? 0 : P - kMaxFree);    // (the largest Pf this P allows)
  return dtype == PVO_F32 ? ws_layout<float>(d, scratch, nullptr, nullptr) : ws_layout<double>(d, scratch, nullptr, nullptr);
}
}  // namespace

extern "C" size_t pvo_ba_train_workspace_bytes(int B, int P, int N, int M, int HW, int dtype) {
  return layout_bytes(B, P, N, M, HW, dtype, false);
}

extern "C" size_t pvo_ba_train_vjp_scratch_bytes(int B, int P, int N, int M, int HW, int dtype) {
  return layout_bytes(B, P, N, M, HW, dtype, true);
}

extern "C" int pvo_ba_train(const void* poses, const void* disps, const void* intr, const void* target, const void* weight, const void* eta,
                            const int64_t* ii, const int64_t* jj, const int* kx, const int* kk, const int* kptr, const int* kedge,
                            int B, int P, int N, int M, int ht, int wd, int fixedp, void* poses_out, void* disps_out, void* dx_out,
                            void* workspace, size_t workspace_bytes, int dtype, void* stream) {
  if (!dims_ok(B, P, N, M, ht, wd, fixedp)) return PVO_EINVAL;
  if (!poses || !disps || !intr || !target || !weight || !eta || !ii || !jj || !kx || !kk || !kptr || !kedge || !poses_out || !disps_out || !workspace)
    return PVO_EINVAL;
  if (dtype != PVO_F32 && dtype != PVO_F64) return PVO_EUNSUPPORTED;
  if (P - fixedp > kMaxFree || N > 65535 || B > 65535 || P > 65535) return PVO_EUNSUPPORTED;
  if (workspace_bytes < pvo_ba_train_workspace_bytes(B, P, N, M, ht * wd, dtype)) return PVO_EWORKSPACE;
  const Dims d = make_dims(B, P, N, M, ht * wd, fixedp);
  const hipStream_t st = pvo_stream(stream);
  return pvo_dispatch<float, double>(dtype, [&](auto tag) -> int {
    using F = decltype(tag);
    return train_fwd<F>(static_cast<const F*>(poses), static_cast<const F*>(disps), static_cast<const F*>(intr), static_cast<const F*>(target),
                        static_cast<const F*>(weight), static_cast<const F*>(eta), ii, jj, kx, kptr, kedge, ht, d,
                        static_cast<F*>(poses_out), static_cast<F*>(disps_out), static_cast<F*>(dx_out), workspace, dtype, st);
  });
}

extern "C" int pvo_ba_train_vjp(const void* poses, const void* disps, const void* intr, const void* target, const void* weight,
                                const int64_t* ii, const int64_t* jj, const int* kx, const int* kk, const int* kptr, const int* kedge,
                                int B, int P, int N, int M, int ht, int wd, int fixedp, const void* g_poses_out, const void* g_disps_out,
                                void* g_target, void* g_weight, void* g_eta, void* g_poses, void* g_disps,
                                const void* workspace, size_t workspace_bytes, void* scratch, size_t scratch_bytes, int dtype, void* stream) {
  if (!dims_ok(B, P, N, M, ht, wd, fixedp)) return PVO_EINVAL;
  if (!poses || !disps || !intr || !target || !weight || !ii || !jj || !kx || !kk || !kptr || !kedge || !g_poses_out || !g_disps_out ||
      !g_target || !g_weight || !g_eta || !g_poses || !g_disps || !workspace || !scratch)
    return PVO_EINVAL;
  if (dtype != PVO_F32 && dtype != PVO_F64) return PVO_EUNSUPPORTED;
  if (P - fixedp > kMaxFree || N > 65535 || B > 65535 || P > 65535) return PVO_EUNSUPPORTED;
  if (workspace_bytes < pvo_ba_train_workspace_bytes(B, P, N, M, ht * wd, dtype) ||
      scratch_bytes < pvo_ba_train_vjp_scratch_bytes(B, P, N, M, ht * wd, dtype)) return PVO_EWORKSPACE;
  const Dims d = make_dims(B, P, N, M, ht * wd, fixedp);
  const hipStream_t st = pvo_stream(stream);
  return pvo_dispatch<float, double>(dtype, [&](auto tag) -> int {
    using F = decltype(tag);
    return train_vjp<F>(static_cast<const F*>(poses), static_cast<const F*>(disps), static_cast<const F*>(intr), static_cast<const F*>(target),
                        static_cast<const F*>(weight), ii, jj, kx, kk, ht, d, static_cast<const F*>(g_poses_out), static_cast<const F*>(g_disps_out),
                        static_cast<F*>(g_target), static_cast<F*>(g_weight), static_cast<F*>(g_eta), static_cast<F*>(g_poses), static_cast<F*>(g_disps),
                        workspace, scratch, dtype, st);
  });
}
