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

constexpr double kEps = 1e-6;
enum { OP_EXP = 0, OP_LOG = 1, OP_INV = 2, OP_MUL = 3, OP_ACT4 = 4, OP_ACT3 = 5, OP_ADJ = 6, OP_ADJT = 7 };

template <typename F> __device__ __forceinline__ void se3_exp(const F* xi, F* out) {
  const V3<F> tau = {xi[0], xi[1], xi[2]}, phi = {xi[3], xi[4], xi[5]};
  const F th2 = phi.x * phi.x + phi.y * phi.y + phi.z * phi.z, th = sqrt(th2);
  const bool small = th < F(kEps);
  const F ths = small ? F(1) : th, th2s = small ? F(1) : th2;
  const F imag = small ? F(0.5) - th2 / F(48) + th2 * th2 / F(3840) : sin(F(0.5) * ths) / ths;
  const F real = small ? F(1) - th2 / F(8) + th2 * th2 / F(384) : cos(F(0.5) * ths);
  const F c1 = small ? F(0.5) - th2 / F(24) : (F(1) - cos(ths)) / th2s;
  const F c2 = small ? F(1) / F(6) - th2 / F(120) : (ths - sin(ths)) / (th2s * ths);
  const V3<F> pt = cross(phi, tau), ppt = cross(phi, pt);
  out[0] = tau.x + c1 * pt.x + c2 * ppt.x; out[1] = tau.y + c1 * pt.y + c2 * ppt.y; out[2] = tau.z + c1 * pt.z + c2 * ppt.z;
  out[3] = imag * phi.x; out[4] = imag * phi.y; out[5] = imag * phi.z; out[6] = real;
}

template <typename F> __device__ __forceinline__ void se3_log(const F* g, F* out) {
  const V3<F> t = {g[0], g[1], g[2]}, v = {g[3], g[4], g[5]};
  const F w = g[6];
  const F n2 = v.x * v.x + v.y * v.y + v.z * v.z;
  const bool smallq = n2 < F(kEps * kEps);
  const F n = sqrt(smallq ? F(1) : n2);
  const F ws = fabs(w) < F(kEps) ? F(kEps) : w;
  F big = F(2) * atan(n / ws) / n;
  if (fabs(w) < F(kEps)) big = (w > F(0) ? F(3.14159265358979323846) : -F(3.14159265358979323846)) / n;
  const F sm = F(2) / w - (F(2) / F(3)) * n2 / (w * w * w);
  const F s = smallq ? sm : big;
  const V3<F> phi = {s * v.x, s * v.y, s * v.z};
  const F th2 = phi.x * phi.x + phi.y * phi.y + phi.z * phi.z, th = sqrt(th2);
  const bool small = th < F(kEps);
  const F ths = small ? F(1) : th, half = F(0.5) * ths;
  const F c2 = small ? F(1) / F(12) : (F(1) - ths * cos(half) / (F(2) * sin(half))) / (ths * ths);
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
