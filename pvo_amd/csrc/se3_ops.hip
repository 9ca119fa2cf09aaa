// se3_ops.hip — the SE3 subset of lietorch the VO path uses, as fused element-wise kernels.
//
// Replaces the lietorch CUDA element-wise kernels (reference VO_Module/thirdparty/lietorch/lietorch/src/lietorch_gpu.cu:21-296;
// group maths lietorch/include/se3.h:36-56,84-86,124-142, so3.h:55-60,115-208, EPS = 1e-6 common.h:7): one thread per group
// element, fp32 and fp64.  lietorch broadcasts by MATERIALISING the pose once per pixel (`broadcast_inputs` -> .repeat,
// broadcasting.py:27-29); here an operand with fewer elements is indexed i / rep (a pose per edge acting on H*W points),
// so nothing is copied.
// Backward (round 4; lietorch: hand-written backward kernels, lietorch_gpu.cu:21-296 / groups.py:141-178): pvo_se3_vjp, the
// vector-Jacobian product of every operation in AMBIENT coordinates (the 7 / 6 / 4 / 3 numbers of each operand) - what
// torch.autograd computes for the PyTorch formulation of the same formulas in pvo_amd/geom/se3.py, which stays the reference
// the kernels are tested against.  Not derived by hand: the forward templates (se3_dual.h) are instantiated with a forward-mode dual
// number and evaluated once per input component (at most 14 evaluations of a few dozen flops; the operations are launch- and
// memory-bound), so a derivative can only be wrong if the forward formula is.
//   data layout [n,7] = (tx,ty,tz, qx,qy,qz,qw); tangent (tau, phi).
#include "se3_dual.h"

namespace {

// Vector-Jacobian products.  Unary: gx[i, :] = gy[i, :] . d op(x[i]) / dx.  Binary: the per-ELEMENT products ga [n,7] and gb [n,nb]
// (element i reads a[i / rep_a], b[i / rep_b] as in the forward kernel); the caller sums ga / gb over the repeats of a broadcast
// operand.  One forward evaluation on dual numbers per input component.
template <typename F>
__global__ __launch_bounds__(256) void se3_unary_vjp_kernel(int op, const F* __restrict__ x, const F* __restrict__ gy, F* __restrict__ gx, long long n) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int ni = se3_nin(op), no = se3_nout(op);
  F xv[7], g[7];
  for (int k = 0; k < ni; ++k) xv[k] = x[i * ni + k];
  for (int k = 0; k < no; ++k) g[k] = gy[i * no + k];
#pragma unroll 1
  for (int j = 0; j < ni; ++j) {
    Dual<F> in[7], out[7];
    for (int k = 0; k < 7; ++k) in[k] = Dual<F>(k < ni ? xv[k] : F(0), k == j ? F(1) : F(0));
    if (op == OP_EXP) se3_exp(in, out); else if (op == OP_LOG) se3_log(in, out); else se3_inv(in, out);
    F acc = 0;
    for (int k = 0; k < no; ++k) acc += g[k] * out[k].d;
    gx[i * ni + j] = acc;
  }
}
template <typename F>
__global__ __launch_bounds__(256) void se3_binary_vjp_kernel(int op, const F* __restrict__ a, long long rep_a, const F* __restrict__ b, long long rep_b,
                                                             const F* __restrict__ gy, F* __restrict__ ga, F* __restrict__ gb, long long n) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int nb = se3_nb(op);
  F av[7], bv[7], g[7];
  for (int k = 0; k < 7; ++k) av[k] = a[(i / rep_a) * 7 + k];
  for (int k = 0; k < nb; ++k) { bv[k] = b[(i / rep_b) * nb + k]; g[k] = gy[i * nb + k]; }
#pragma unroll 1
  for (int j = 0; j < 7 + nb; ++j) {
    Dual<F> A[7], B[7], out[7];
    for (int k = 0; k < 7; ++k) A[k] = Dual<F>(av[k], k == j ? F(1) : F(0));
    for (int k = 0; k < 7; ++k) B[k] = Dual<F>(k < nb ? bv[k] : F(0), k + 7 == j ? F(1) : F(0));
    se3_bin(op, A, B, out);
    F acc = 0;
    for (int k = 0; k < nb; ++k) acc += g[k] * out[k].d;
    if (j < 7) { if (ga) ga[i * 7 + j] = acc; } else if (gb) gb[i * nb + (j - 7)] = acc;
  }
}

template <typename F>
__global__ __launch_bounds__(256) void se3_unary_kernel(int op, const F* __restrict__ x, F* __restrict__ y, long long n) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  if (op == OP_EXP) {
    F xi[6], o[7];
#pragma unroll
    for (int k = 0; k < 6; ++k) xi[k] = x[i * 6 + k];
    se3_exp(xi, o);
#pragma unroll
    for (int k = 0; k < 7; ++k) y[i * 7 + k] = o[k];
  } else if (op == OP_LOG) {
    F g[7], o[6];
#pragma unroll
    for (int k = 0; k < 7; ++k) g[k] = x[i * 7 + k];
    se3_log(g, o);
#pragma unroll
    for (int k = 0; k < 6; ++k) y[i * 6 + k] = o[k];
  } else {                                         // inverse
    F g[7], o[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) g[k] = x[i * 7 + k];
    se3_inv(g, o);
#pragma unroll
    for (int k = 0; k < 7; ++k) y[i * 7 + k] = o[k];
  }
}

// element i reads a[i / rep_a] (a group element) and b[i / rep_b]
template <typename F>
__global__ __launch_bounds__(256) void se3_binary_kernel(int op, const F* __restrict__ a, long long rep_a, const F* __restrict__ b,
                                                         long long rep_b, F* __restrict__ y, long long n) {
  const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int nb = se3_nb(op);
  F g[7], x[7], o[7];
  for (int k = 0; k < 7; ++k) g[k] = a[(i / rep_a) * 7 + k];
  for (int k = 0; k < nb; ++k) x[k] = b[(i / rep_b) * nb + k];
  se3_bin(op, g, x, o);
  for (int k = 0; k < nb; ++k) y[i * nb + k] = o[k];
}

// ---- projective_transform (VO_Module/droid_slam/geom/projective_ops.py:106-130: iproj :21-41, actp :76-103, proj :44-73) ----------
// The training path's reprojection i -> j with its closed-form Jacobians, ONE kernel per direction instead of the ~90 element-wise
// operators of the PyTorch formulation (pvo_amd/geom/projective_ops.py, which stays the reference these are tested against and
// what CPU tensors use).  Forward: one thread per (batch, edge, pixel).  Backward: the same template on dual numbers, one
// evaluation per input component (7 + 7 pose numbers, the pixel's inverse depth) - ambient-coordinate vector-Jacobian products,
// as for the group operations above; the pose gradients of a workgroup's pixels are summed in LDS before the atomics.
//   out[0..2]  x, y, (inverse depth in frame j)      out[3..14]  Jj [2][6]      out[15..26]  Ji [2][6]      out[27..28]  Jz [2]
// returns Z (the validity test Z > MIN_DEPTH is the caller's: :113)
constexpr double kMinDepth = 0.2;
template <typename F, typename S>
__device__ __forceinline__ F proj_terms(const F* Pi, const F* Pj, F d, S u, S v, const S* Ki, const S* Kj, bool jac, F* out) {
  F Pinv[7], G[7], X0[4], X1[4];
  se3_inv(Pi, Pinv);
  se3_bin(OP_MUL, Pj, Pinv, G);
  X0[0] = F((u - Ki[2]) / Ki[0]); X0[1] = F((v - Ki[3]) / Ki[1]); X0[2] = F(S(1)); X0[3] = d;
  se3_bin(OP_ACT4, G, X0, X1);
  const F X = X1[0], Y = X1[1], Z = X1[2], W = X1[3];
  const F fx = F(Kj[0]), fy = F(Kj[1]);
  const F dinv = F(S(1)) / (Z < F(S(0.5 * kMinDepth)) ? F(S(1)) : Z);
  out[0] = fx * (X * dinv) + F(Kj[2]);
  out[1] = fy * (Y * dinv) + F(Kj[3]);
  out[2] = W * dinv;
  if (!jac) return Z;
  const F fxd = fx * dinv, fyd = fy * dinv;
  const F gx = -(fx * X * dinv * dinv), gy = -(fy * Y * dinv * dinv);
  const F o = F(S(0));
  F* Jj = out + 3;
  Jj[0] = fxd * W; Jj[1] = o; Jj[2] = gx * W; Jj[3] = gx * Y; Jj[4] = fxd * Z - gx * X; Jj[5] = -(fxd * Y);
  Jj[6] = o; Jj[7] = fyd * W; Jj[8] = gy * W; Jj[9] = gy * Y - fyd * Z; Jj[10] = -(gy * X); Jj[11] = fyd * X;
  F* Ji = out + 15;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    F a[6];
    se3_bin(OP_ADJT, G, Jj + 6 * r, a);
#pragma unroll
    for (int k = 0; k < 6; ++k) Ji[6 * r + k] = -a[k];
  }
  out[27] = fxd * G[0] + gx * G[2];
  out[28] = fyd * G[1] + gy * G[2];
  return Z;
}

// poses [B,P,7], depths [B,P,HW], intr [B,P,4], ii / jj [N]; x1 [B,N,HW,nx] (nx = 2 or 3), valid [B,N,HW], Jj / Ji [B,N,HW,2,6], Jz [B,N,HW,2]
template <typename F>
__global__ __launch_bounds__(256) void proj_fwd_kernel(const F* __restrict__ poses, const F* __restrict__ depths, const F* __restrict__ intr,
                                                       const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, int P, int N, int HW, int wd, int nx,
                                                       F* __restrict__ x1, F* __restrict__ valid, F* __restrict__ Ji, F* __restrict__ Jj, F* __restrict__ Jz) {
  const int px = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y, b = blockIdx.z;
  if (px >= HW) return;
  // frame indices as torch indexing reads them: a negative index counts from the end; anything still outside [0, P) - which the
  // PyTorch formulation answers with an IndexError - leaves this edge NaN / invalid instead of reading beside the buffers
  long long i = ii[n], j = jj[n];
  i += (i < 0) ? P : 0; j += (j < 0) ? P : 0;
  if (i < 0 || i >= P || j < 0 || j >= P) {
    const long long row = (static_cast<long long>(b) * N + n) * HW + px;
    const F nan = F(0) / F(0);
    for (int k = 0; k < nx; ++k) x1[row * nx + k] = nan;
    valid[row] = F(0);
    if (Jj) {
      for (int k = 0; k < 12; ++k) { Jj[row * 12 + k] = nan; Ji[row * 12 + k] = nan; }
      Jz[row * 2] = nan; Jz[row * 2 + 1] = nan;
    }
    return;
  }
  const F* Pi = poses + (static_cast<long long>(b) * P + i) * 7;
  const F* Pj = poses + (static_cast<long long>(b) * P + j) * 7;
  F pi[7], pj[7], Ki[4], Kj[4], out[29];
#pragma unroll
  for (int k = 0; k < 7; ++k) { pi[k] = Pi[k]; pj[k] = Pj[k]; }
#pragma unroll
  for (int k = 0; k < 4; ++k) { Ki[k] = intr[(static_cast<long long>(b) * P + i) * 4 + k]; Kj[k] = intr[(static_cast<long long>(b) * P + j) * 4 + k]; }
  const F d = depths[(static_cast<long long>(b) * P + i) * HW + px];
  const F Z = proj_terms<F, F>(pi, pj, d, F(px % wd), F(px / wd), Ki, Kj, Jj != nullptr, out);
  const long long row = (static_cast<long long>(b) * N + n) * HW + px;
  for (int k = 0; k < nx; ++k) x1[row * nx + k] = out[k];
  valid[row] = Z > F(kMinDepth) ? F(1) : F(0);
  if (Jj) {
#pragma unroll
    for (int k = 0; k < 12; ++k) { Jj[row * 12 + k] = out[3 + k]; Ji[row * 12 + k] = out[15 + k]; }
    Jz[row * 2] = out[27]; Jz[row * 2 + 1] = out[28];
  }
}

// g_* : the incoming gradients of x1 / Ji / Jj / Jz (NULL = none); gposes [B,P,7] and gdepths [B,P,HW] are ACCUMULATED into (zeroed by the caller)
template <typename F>
__global__ __launch_bounds__(256) void proj_vjp_kernel(const F* __restrict__ poses, const F* __restrict__ depths, const F* __restrict__ intr,
                                                       const int64_t* __restrict__ ii, const int64_t* __restrict__ jj, int P, int N, int HW, int wd, int nx,
                                                       const F* __restrict__ g_x1, const F* __restrict__ g_Ji, const F* __restrict__ g_Jj, const F* __restrict__ g_Jz,
                                                       F* __restrict__ gposes, F* __restrict__ gdepths) {
  __shared__ F red[4][14];
  const int px = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y, b = blockIdx.z;
  long long i = ii[n], j = jj[n];                           // (as in the forward kernel: negatives wrap, an edge outside [0, P) adds nothing)
  i += (i < 0) ? P : 0; j += (j < 0) ? P : 0;
  if (i < 0 || i >= P || j < 0 || j >= P) return;           // (uniform over the workgroup: n is blockIdx.y)
  const bool jac = g_Ji || g_Jj || g_Jz;
  F s[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) s[k] = F(0);
  if (px < HW) {
    F pi[7], pj[7], Ki[4], Kj[4], g[29];
#pragma unroll
    for (int k = 0; k < 7; ++k) { pi[k] = poses[(static_cast<long long>(b) * P + i) * 7 + k]; pj[k] = poses[(static_cast<long long>(b) * P + j) * 7 + k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { Ki[k] = intr[(static_cast<long long>(b) * P + i) * 4 + k]; Kj[k] = intr[(static_cast<long long>(b) * P + j) * 4 + k]; }
    const F d = depths[(static_cast<long long>(b) * P + i) * HW + px];
    const long long row = (static_cast<long long>(b) * N + n) * HW + px;
#pragma unroll
    for (int k = 0; k < 29; ++k) g[k] = F(0);
    if (g_x1) for (int k = 0; k < nx; ++k) g[k] = g_x1[row * nx + k];
    if (g_Jj) for (int k = 0; k < 12; ++k) g[3 + k] = g_Jj[row * 12 + k];
    if (g_Ji) for (int k = 0; k < 12; ++k) g[15 + k] = g_Ji[row * 12 + k];
    if (g_Jz) { g[27] = g_Jz[row * 2]; g[28] = g_Jz[row * 2 + 1]; }
    const F u = F(px % wd), v = F(px / wd);
#pragma unroll 1
    for (int q = 0; q < 15; ++q) {
      Dual<F> A[7], Bq[7], out[29];
#pragma unroll
      for (int k = 0; k < 7; ++k) { A[k] = Dual<F>(pi[k], k == q ? F(1) : F(0)); Bq[k] = Dual<F>(pj[k], k + 7 == q ? F(1) : F(0)); }
      const Dual<F> dd(d, q == 14 ? F(1) : F(0));
      proj_terms<Dual<F>, F>(A, Bq, dd, u, v, Ki, Kj, jac, out);
      F acc = F(0);
      const int nout = jac ? 29 : 3;
      for (int k = 0; k < nout; ++k) acc += g[k] * out[k].d;
      s[q] = acc;
    }
    // (i == j: both seeds move the same pose; the two partial derivatives add, which the two accumulations below do)
    atomicAdd(&gdepths[(static_cast<long long>(b) * P + i) * HW + px], s[14]);
  }
  // the 14 pose sums of this workgroup's pixels: wave shuffle, then across the four waves through LDS
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 14; ++k) {
    F v = s[k];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 14) {
    const F v = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    const int k = threadIdx.x;
    F* dst = gposes + (static_cast<long long>(b) * P + (k < 7 ? i : j)) * 7 + (k < 7 ? k : k - 7);
    atomicAdd(dst, v);
  }
}

}  // namespace

extern "C" int pvo_se3_unary(int op, const void* x, void* y, long long n, int dtype, void* stream) {
  if (n < 0 || op < OP_EXP || op > OP_INV) return PVO_EINVAL;
  if (n == 0) return PVO_OK;
  if (!x || !y) return PVO_EINVAL;
  const dim3 grid(static_cast<unsigned>((n + 255) / 256));
  return pvo_dispatch<float, double>(dtype, [&](auto tag) -> int {
    using F = decltype(tag);
    hipLaunchKernelGGL(se3_unary_kernel<F>, grid, dim3(256), 0, pvo_stream(stream), op, static_cast<const F*>(x), static_cast<F*>(y), n);
    PVO_CHECK_LAUNCH();
    return PVO_OK;
  });
}

extern "C" int pvo_se3_binary(int op, const void* a, long long rep_a, const void* b, long long rep_b, void* y, long long n,
                              int dtype, void* stream) {
  if (n < 0 || op < OP_MUL || op > OP_ADJT || rep_a <= 0 || rep_b <= 0) return PVO_EINVAL;
  if (n == 0) return PVO_OK;
  if (!a || !b || !y) return PVO_EINVAL;
  const dim3 grid(static_cast<unsigned>((n + 255) / 256));
  return pvo_dispatch<float, double>(dtype, [&](auto tag) -> int {
    using F = decltype(tag);
    hipLaunchKernelGGL(se3_binary_kernel<F>, grid, dim3(256), 0, pvo_stream(stream), op, static_cast<const F*>(a), rep_a,
                       static_cast<const F*>(b), rep_b, static_cast<F*>(y), n);
    PVO_CHECK_LAUNCH();
    return PVO_OK;
  });
}

// Backward of pvo_se3_unary / pvo_se3_binary (ambient-coordinate vector-Jacobian products; see the head of this file).
//   unary : gx [n, in] = gy [n, out] . J          binary: ga [n,7], gb [n,nb] PER OUTPUT ELEMENT (either may be NULL); the caller sums
//   them over the `rep` repeats of a broadcast operand (element i belongs to a[i / rep_a], b[i / rep_b]).
extern "C" int pvo_se3_unary_vjp(int op, const void* x, const void* gy, void* gx, long long n, int dtype, void* stream) {
  if (n < 0 || op < OP_EXP || op > OP_INV) return PVO_EINVAL;
  if (n == 0) return PVO_OK;
  if (!x || !gy || !gx) return PVO_EINVAL;
  const dim3 grid(static_cast<unsigned>((n + 255) / 256));
  return pvo_dispatch<float, double>(dtype, [&](auto tag) -> int {
    using F = decltype(tag);
    hipLaunchKernelGGL(se3_unary_vjp_kernel<F>, grid, dim3(256), 0, pvo_stream(stream), op, static_cast<const F*>(x), static_cast<const F*>(gy), static_cast<F*>(gx), n);
    PVO_CHECK_LAUNCH();
    return PVO_OK;
  });
}

extern "C" int pvo_se3_binary_vjp(int op, const void* a, long long rep_a, const void* b, long long rep_b, const void* gy,
                                  void* ga, void* gb, long long n, int dtype, void* stream) {
  if (n < 0 || op < OP_MUL || op > OP_ADJT || rep_a <= 0 || rep_b <= 0) return PVO_EINVAL;
  if (n == 0) return PVO_OK;
  if (!a || !b || !gy || (!ga && !gb)) return PVO_EINVAL;
  const dim3 grid(static_cast<unsigned>((n + 255) / 256));
  return pvo_dispatch<float, double>(dtype, [&](auto tag) -> int {
    using F = decltype(tag);
    hipLaunchKernelGGL(se3_binary_vjp_kernel<F>, grid, dim3(256), 0, pvo_stream(stream), op, static_cast<const F*>(a), rep_a, static_cast<const F*>(b), rep_b,
                       static_cast<const F*>(gy), static_cast<F*>(ga), static_cast<F*>(gb), n);
    PVO_CHECK_LAUNCH();
    return PVO_OK;
  });
}

// projective_transform forward / backward (see proj_terms above).  Jj == NULL: coordinates and validity only.
extern "C" int pvo_proj_transform(const void* poses, const void* depths, const void* intr, const int64_t* ii, const int64_t* jj,
                                  int B, int P, int N, int ht, int wd, int nx, void* x1, void* valid, void* Ji, void* Jj, void* Jz,
                                  int dtype, void* stream) {
  if (B < 0 || P <= 0 || N < 0 || ht <= 0 || wd <= 0 || (nx != 2 && nx != 3)) return PVO_EINVAL;
  if (B == 0 || N == 0) return PVO_OK;
  if (!poses || !depths || !intr || !ii || !jj || !x1 || !valid) return PVO_EINVAL;
  if ((Jj != nullptr) != (Ji != nullptr) || (Jj != nullptr) != (Jz != nullptr)) return PVO_EINVAL;
  if (N > 65535 || B > 65535) return PVO_EUNSUPPORTED;      // an edge / batch index is a grid coordinate (include/pvo_hip.h "Limits")
  const int HW = ht * wd;
  const dim3 grid((HW + 255) / 256, N, B);
  return pvo_dispatch<float, double>(dtype, [&](auto tag) -> int {
    using F = decltype(tag);
    hipLaunchKernelGGL(proj_fwd_kernel<F>, grid, dim3(256), 0, pvo_stream(stream), static_cast<const F*>(poses), static_cast<const F*>(depths),
                       static_cast<const F*>(intr), ii, jj, P, N, HW, wd, nx, static_cast<F*>(x1), static_cast<F*>(valid),
                       static_cast<F*>(Ji), static_cast<F*>(Jj), static_cast<F*>(Jz));
    PVO_CHECK_LAUNCH();
    return PVO_OK;
  });
}

// gposes [B,P,7] and gdepths [B,P,ht*wd] must be ZERO on entry (the products of all edges and pixels are added into them)
extern "C" int pvo_proj_transform_vjp(const void* poses, const void* depths, const void* intr, const int64_t* ii, const int64_t* jj,
                                      int B, int P, int N, int ht, int wd, int nx, const void* g_x1, const void* g_Ji, const void* g_Jj, const void* g_Jz,
                                      void* gposes, void* gdepths, int dtype, void* stream) {
  if (B < 0 || P <= 0 || N < 0 || ht <= 0 || wd <= 0 || (nx != 2 && nx != 3)) return PVO_EINVAL;
  if (B == 0 || N == 0) return PVO_OK;
  if (!poses || !depths || !intr || !ii || !jj || !gposes || !gdepths) return PVO_EINVAL;
  if (!g_x1 && !g_Ji && !g_Jj && !g_Jz) return PVO_OK;
  if (N > 65535 || B > 65535) return PVO_EUNSUPPORTED;
  const int HW = ht * wd;
  const dim3 grid((HW + 255) / 256, N, B);
  return pvo_dispatch<float, double>(dtype, [&](auto tag) -> int {
    using F = decltype(tag);
    hipLaunchKernelGGL(proj_vjp_kernel<F>, grid, dim3(256), 0, pvo_stream(stream), static_cast<const F*>(poses), static_cast<const F*>(depths),
                       static_cast<const F*>(intr), ii, jj, P, N, HW, wd, nx, static_cast<const F*>(g_x1), static_cast<const F*>(g_Ji),
                       static_cast<const F*>(g_Jj), static_cast<const F*>(g_Jz), static_cast<F*>(gposes), static_cast<F*>(gdepths));
    PVO_CHECK_LAUNCH();
    return PVO_OK;
  });
}
