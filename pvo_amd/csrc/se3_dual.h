// se3_dual.h — the SE3 group operations as templates over the scalar type (F, or the forward-mode dual number Dual<F>).
// Shared by se3_ops.hip (lietorch's element-wise operations and the projective transform) and ba_train.hip (the retraction
// of the training BA and its vector-Jacobian product).  Data layout [7] = (tx,ty,tz, qx,qy,qz,qw); tangent (tau, phi).
#pragma once
#include "common.h"
#include <type_traits>

namespace {

template <typename F> struct V3 { F x, y, z; };
template <typename F> struct Q4 { F x, y, z, w; };

template <typename F> __device__ __forceinline__ V3<F> cross(V3<F> a, V3<F> b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
template <typename F> __device__ __forceinline__ V3<F> qrot(Q4<F> q, V3<F> v) {
  const V3<F> qv = {q.x, q.y, q.z};
  V3<F> uv = cross(qv, v);
  uv = {F(2) * uv.x, F(2) * uv.y, F(2) * uv.z};
  const V3<F> c = cross(qv, uv);
  return {v.x + q.w * uv.x + c.x, v.y + q.w * uv.y + c.y, v.z + q.w * uv.z + c.z};
}
template <typename F> __device__ __forceinline__ Q4<F> qmul(Q4<F> a, Q4<F> b) {
  return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
          a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
template <typename F> __device__ __forceinline__ Q4<F> qconj(Q4<F> q) { return {-q.x, -q.y, -q.z, q.w}; }

// forward-mode dual number over F (value, derivative along ONE seeded input direction)
template <typename F> struct Dual {
  F v, d;
  __device__ __forceinline__ Dual() : v(0), d(0) {}
  __device__ __forceinline__ Dual(F v_) : v(v_), d(0) {}
  __device__ __forceinline__ Dual(F v_, F d_) : v(v_), d(d_) {}
  template <typename C, typename = typename std::enable_if<std::is_arithmetic<C>::value && !std::is_same<C, F>::value>::type>
  __device__ __forceinline__ explicit Dual(C c) : v(static_cast<F>(c)), d(0) {}      // literals: F(2), F(0.5), F(kEps)
};
template <typename F> struct ScalarOf { using type = F; };
template <typename F> struct ScalarOf<Dual<F>> { using type = F; };
using ::sqrt; using ::sin; using ::cos; using ::atan; using ::fabs;      // (the overloads below must not hide the float / double ones)
#define DU __device__ __forceinline__
template <typename F> DU Dual<F> operator+(Dual<F> a, Dual<F> b) { return {a.v + b.v, a.d + b.d}; }
template <typename F> DU Dual<F> operator-(Dual<F> a, Dual<F> b) { return {a.v - b.v, a.d - b.d}; }
template <typename F> DU Dual<F> operator-(Dual<F> a) { return {-a.v, -a.d}; }
template <typename F> DU Dual<F> operator*(Dual<F> a, Dual<F> b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
template <typename F> DU Dual<F> operator/(Dual<F> a, Dual<F> b) { const F q = a.v / b.v; return {q, (a.d - q * b.d) / b.v}; }
template <typename F> DU bool operator<(Dual<F> a, Dual<F> b) { return a.v < b.v; }
template <typename F> DU bool operator>(Dual<F> a, Dual<F> b) { return a.v > b.v; }
template <typename F> DU Dual<F> sqrt(Dual<F> a) { const F r = sqrt(a.v); return {r, a.d / (F(2) * r)}; }
template <typename F> DU Dual<F> sin(Dual<F> a) { return {sin(a.v), cos(a.v) * a.d}; }
template <typename F> DU Dual<F> cos(Dual<F> a) { return {cos(a.v), -sin(a.v) * a.d}; }
template <typename F> DU Dual<F> atan(Dual<F> a) { return {atan(a.v), a.d / (F(1) + a.v * a.v)}; }
template <typename F> DU Dual<F> fabs(Dual<F> a) { return a.v < F(0) ? Dual<F>{-a.v, -a.d} : a; }
#undef DU

constexpr double kEps = 1e-6;                      // lietorch's common.h: log's |w| -> 0 branch only
constexpr double kPi = 3.14159265358979323846;
enum { OP_EXP = 0, OP_LOG = 1, OP_INV = 2, OP_MUL = 3, OP_ACT4 = 4, OP_ACT3 = 5, OP_ADJ = 6, OP_ADJT = 7 };

// ---- exp / log: where series, where closed forms ---------------------------------------------------------------------------------
// With x = theta^2, exp needs  imag = sin(theta/2)/theta,  real = cos(theta/2),  c1 = (1 - cos theta)/x,  c2 = (theta - sin theta)/
// (x theta);  log needs  c2' = (1 - (theta/2) cot(theta/2))/x  and, of the quaternion (v, w), n = |v|,  s = 2 atan(n/w)/n.
// lietorch switches to two-term series at theta < 1e-6 and uses the closed forms above it.  In a type of unit roundoff eps that loses
//   c1  as (1 - cos theta)/x:    1 - cos is known to eps absolutely, so c1 to eps/x;  times |phi x tau| <= theta |tau|:  eps |tau| / theta
//   c2, c2':                     numerator ~ theta^3/6 known to eps theta, so c2 to eps/x;  times theta^2 |tau|:  eps |tau| - harmless
//   d c2/d theta (dual numbers, autograd: (1 - cos)/theta^3 - 3 (theta - sin)/theta^4, two terms of 1/(2 theta) that cancel to
//   theta/60):                   eps/theta^3;  times theta^2 |tau|:  eps |tau| / theta, of a gradient whose size is |tau| / 2
// i.e. in fp32 a translation wrong by 1e-3 |tau| at theta = 1e-4 and a gradient wrong by its own size below 1e-4.  Here:
//   * c1 = 2 imag^2 (half angle): no cancellation at any angle, in value or derivative; imag, real and s never cancelled.
//   * below theta < Cut<S>::theta every coefficient is its Taylor series in x, whose derivative is as well conditioned as its value,
//     and nothing depends on theta itself - so phi = 0 exactly has a finite derivative (sqrt is not evaluated there).
//   * above it the closed forms of c2 and c2' remain, each with a relative gradient error that grows as u / theta (u the unit
//     roundoff, 2^-24 / 2^-53).  The tests bound gradients by 64 u of their largest entry (tests/test_se3_angles.py).  What binds is
//     log's c2', through the inverse-function test (the VJP of log(exp(xi)) is the cotangent, |tau| up to 30): just above a cutoff
//     c its error is 11 - 24 u / c in both types (704 u at c = 0.02, 265 u at 0.05, 190 u at 0.1, 50 u at 0.25, 22 u at 0.5, float),
//     over a floor of 10 - 30 u that the chain has at every angle.  exp's c2 alone would allow far less: 1.4 - 2 u / c (84 u at
//     0.02, 4 u at 0.5), i.e. a cutoff of 0.03.  tools/se3_cutoff.py prints these figures.  One cutoff serves both operations, so
//     it is 0.5; the figures are in units of u, so it is the same for float and double, and is kept per type only because nothing
//     else ties the two.
//   * terms: the slowest series at x = 0.25 are c2 (ratio of terms x / ((2k+2)(2k+3)), relative size 6 x^k/(2k+3)!) and c2' (ratio ->
//     x / (4 pi^2) = 6.3e-3).  The first omitted term must be below u: float (6e-8) 5 terms - c2: 6 x^5/13! = 9e-13, c2':
//     (6.3e-3)^5 = 1e-11;  double (1.1e-16) 8 terms - c2: 6 x^8/19! = 8e-22, c2': (6.3e-3)^8 = 2.5e-18 (7 terms: 4e-16, too many).
//   * s = (2/w) atan(u)/u, u = n/w, is the five-term series in u^2 below n < Cut<S>::n: first omitted term u^10/11 = 9e-11 at
//     n = 0.125 (float), 8e-21 at n = 0.0125 (double).  Above it the closed form; at |w| < 1e-6, where n/w overflows,
//     2 atan(n/w) = +-pi - 2 atan(w/n), which is exact (lietorch: +-pi, wrong by 2 |w|).
// pvo_amd/geom/se3.py carries the same tables and cutoffs (CUTOFF, TERMS, Q_CUTOFF); the parity tests of tests/test_se3.py rely on it,
// and tests/test_se3_angles.py reads the Cut<> lines and the SE3_SERIES tables below as text and compares them with that module's.
template <typename S> struct Cut;
template <> struct Cut<float> { static constexpr double theta = 0.5, n = 0.125; static constexpr int terms = 5; };
template <> struct Cut<double> { static constexpr double theta = 0.5, n = 0.0125; static constexpr int terms = 8; };

#define SE3_SERIES(name, ...) constexpr double name[8] = {__VA_ARGS__};
SE3_SERIES(kImag, 1.0 / 2.0, -1.0 / 48.0, 1.0 / 3840.0, -1.0 / 645120.0, 1.0 / 185794560.0, -1.0 / 81749606400.0,
           1.0 / 51011754393600.0, -1.0 / 42849873690624000.0)
SE3_SERIES(kReal, 1.0, -1.0 / 8.0, 1.0 / 384.0, -1.0 / 46080.0, 1.0 / 10321920.0, -1.0 / 3715891200.0, 1.0 / 1961990553600.0,
           -1.0 / 1428329123020800.0)
SE3_SERIES(kC1, 1.0 / 2.0, -1.0 / 24.0, 1.0 / 720.0, -1.0 / 40320.0, 1.0 / 3628800.0, -1.0 / 479001600.0, 1.0 / 87178291200.0,
           -1.0 / 20922789888000.0)
SE3_SERIES(kC2, 1.0 / 6.0, -1.0 / 120.0, 1.0 / 5040.0, -1.0 / 362880.0, 1.0 / 39916800.0, -1.0 / 6227020800.0, 1.0 / 1307674368000.0,
           -1.0 / 355687428096000.0)
SE3_SERIES(kLogC2, 1.0 / 12.0, 1.0 / 720.0, 1.0 / 30240.0, 1.0 / 1209600.0, 1.0 / 47900160.0, 691.0 / 1307674368000.0,
           1.0 / 74724249600.0, 3617.0 / 10670622842880000.0)
SE3_SERIES(kAtan, 1.0, -1.0 / 3.0, 1.0 / 5.0, -1.0 / 7.0, 1.0 / 9.0, 0.0, 0.0, 0.0)
#undef SE3_SERIES

// sum_k c[k] x^k, k < N, by Horner's rule
template <int N, typename F> __device__ __forceinline__ F series(F x, const double (&c)[8]) {
  F y = F(c[N - 1]);
#pragma unroll
  for (int k = N - 2; k >= 0; --k) y = y * x + F(c[k]);
  return y;
}

template <typename F> __device__ __forceinline__ void se3_exp(const F* xi, F* out) {
  using C = Cut<typename ScalarOf<F>::type>;
  const V3<F> tau = {xi[0], xi[1], xi[2]}, phi = {xi[3], xi[4], xi[5]};
  const F th2 = phi.x * phi.x + phi.y * phi.y + phi.z * phi.z;
  F imag, real, c1, c2;
  if (th2 < F(C::theta * C::theta)) {
    imag = series<C::terms>(th2, kImag); real = series<C::terms>(th2, kReal);
    c1 = series<C::terms>(th2, kC1); c2 = series<C::terms>(th2, kC2);
  } else {
    const F th = sqrt(th2);
    imag = sin(F(0.5) * th) / th; real = cos(F(0.5) * th);
    c1 = F(2) * imag * imag; c2 = (th - sin(th)) / (th2 * th);
  }
  const V3<F> pt = cross(phi, tau), ppt = cross(phi, pt);
  out[0] = tau.x + c1 * pt.x + c2 * ppt.x; out[1] = tau.y + c1 * pt.y + c2 * ppt.y; out[2] = tau.z + c1 * pt.z + c2 * ppt.z;
  out[3] = imag * phi.x; out[4] = imag * phi.y; out[5] = imag * phi.z; out[6] = real;
}

template <typename F> __device__ __forceinline__ void se3_log(const F* g, F* out) {
  using C = Cut<typename ScalarOf<F>::type>;
  const V3<F> t = {g[0], g[1], g[2]}, v = {g[3], g[4], g[5]};
  const F w = g[6];
  const F n2 = v.x * v.x + v.y * v.y + v.z * v.z;
  F s;
  if (n2 < F(C::n * C::n)) {
    s = F(2) / w * series<5>(n2 / (w * w), kAtan);
  } else {
    const F n = sqrt(n2);
    if (fabs(w) < F(kEps)) s = ((w > F(0) ? F(kPi) : -F(kPi)) - F(2) * atan(w / n)) / n;
    else s = F(2) * atan(n / w) / n;
  }
  const V3<F> phi = {s * v.x, s * v.y, s * v.z};
  const F th2 = phi.x * phi.x + phi.y * phi.y + phi.z * phi.z;
  F c2;
  if (th2 < F(C::theta * C::theta)) {
    c2 = series<C::terms>(th2, kLogC2);
  } else {
    const F th = sqrt(th2), half = F(0.5) * th;
    c2 = (F(1) - th * cos(half) / (F(2) * sin(half))) / th2;
  }
  const V3<F> pt = cross(phi, t), ppt = cross(phi, pt);
  out[0] = t.x - F(0.5) * pt.x + c2 * ppt.x; out[1] = t.y - F(0.5) * pt.y + c2 * ppt.y; out[2] = t.z - F(0.5) * pt.z + c2 * ppt.z;
  out[3] = phi.x; out[4] = phi.y; out[5] = phi.z;
}

// ---- the remaining operations as templates over the scalar (F or Dual<F>): inputs / outputs as small arrays ----------------
template <typename F> __device__ __forceinline__ void se3_inv(const F* g, F* out) {
  const V3<F> t = {g[0], g[1], g[2]};
  const Q4<F> qi = qconj(Q4<F>{g[3], g[4], g[5], g[6]});
  const V3<F> r = qrot(qi, t);
  out[0] = -r.x; out[1] = -r.y; out[2] = -r.z; out[3] = qi.x; out[4] = qi.y; out[5] = qi.z; out[6] = qi.w;
}
// op in {MUL, ACT4, ACT3, ADJ, ADJT}: g [7] group element, x the second operand ([7] / [4] / [3] / [6]), out [7] / [4] / [3] / [6]
template <typename F> __device__ __forceinline__ void se3_bin(int op, const F* g, const F* x, F* out) {
  const V3<F> t = {g[0], g[1], g[2]};
  const Q4<F> q = {g[3], g[4], g[5], g[6]};
  if (op == OP_MUL) {
    const V3<F> r = qrot(q, V3<F>{x[0], x[1], x[2]});
    const Q4<F> qq = qmul(q, Q4<F>{x[3], x[4], x[5], x[6]});
    out[0] = t.x + r.x; out[1] = t.y + r.y; out[2] = t.z + r.z; out[3] = qq.x; out[4] = qq.y; out[5] = qq.z; out[6] = qq.w;
  } else if (op == OP_ACT4) {
    const V3<F> r = qrot(q, V3<F>{x[0], x[1], x[2]});
    out[0] = r.x + t.x * x[3]; out[1] = r.y + t.y * x[3]; out[2] = r.z + t.z * x[3]; out[3] = x[3];
  } else if (op == OP_ACT3) {
    const V3<F> r = qrot(q, V3<F>{x[0], x[1], x[2]});
    out[0] = r.x + t.x; out[1] = r.y + t.y; out[2] = r.z + t.z;
  } else if (op == OP_ADJ) {
    const V3<F> rphi = qrot(q, V3<F>{x[3], x[4], x[5]}), rt = qrot(q, V3<F>{x[0], x[1], x[2]}), c = cross(t, rphi);
    out[0] = rt.x + c.x; out[1] = rt.y + c.y; out[2] = rt.z + c.z; out[3] = rphi.x; out[4] = rphi.y; out[5] = rphi.z;
  } else {                                         // adjT
    const Q4<F> qi = qconj(q);
    const V3<F> at = {x[0], x[1], x[2]};
    const V3<F> r0 = qrot(qi, at), r1 = qrot(qi, V3<F>{x[3], x[4], x[5]}), r2 = qrot(qi, cross(at, t));
    out[0] = r0.x; out[1] = r0.y; out[2] = r0.z; out[3] = r1.x + r2.x; out[4] = r1.y + r2.y; out[5] = r1.z + r2.z;
  }
}
__host__ __device__ __forceinline__ int se3_nb(int op) { return op == OP_MUL ? 7 : (op == OP_ACT4 ? 4 : (op == OP_ACT3 ? 3 : 6)); }      // second operand = output size
__host__ __device__ __forceinline__ int se3_nin(int op) { return op == OP_EXP ? 6 : 7; }
__host__ __device__ __forceinline__ int se3_nout(int op) { return op == OP_EXP ? 7 : (op == OP_LOG ? 6 : 7); }

}  // namespace
