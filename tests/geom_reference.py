"""The reprojection family's yardstick (tests/test_geom_fp64_host.py, tests/test_geom_fp64_gpu.py): the contracts of pvo_projmap, pvo_iproj,
pvo_reproject(_rig), pvo_frame_distance and pvo_depth_filter (pvo_amd/csrc/geom.hip, depth_vote.h, se3.h) restated in numpy fp64 on the
fp32 inputs, every value with a per-element bound on what the fp32 kernel may differ by, every decision with a flag that says whether
rounding could flip it.

THE BOUND.  geom.hip is compiled without multiply-add contraction and with correctly rounded division and square root, so every operation
of the kernel text rounds exactly once: fl(x op y) = (x op y)(1 + delta), |delta| <= EPS = 2^-24.  The reference performs THE SAME
OPERATIONS IN THE SAME ORDER as the kernel text (class F below), carrying next to each exact value v the first-order bound e on
|kernel's value - v|.  One rounding is counted per operation, on top of what the operands bring along:
  a + b, a - b   e = e_a + e_b + EPS |a + b|
  a * b          e = |a| e_b + |b| e_a + EPS |a b|
  a / b          e = e_a / |b| + |a / b| e_b / |b| + EPS |a / b|        <- the 1/Z amplification: an error of Z enters a projection
                                                                           X / Z as |X / Z| e_Z / |Z|, i.e. with 1 / Z^2
  2 a, -a        exact
  sqrt(a^2+b^2)  e = e_a + e_b + 2 EPS d: the Euclidean norm is 1-Lipschitz, and two squares and a sum (relative 2 EPS under the root,
                 so 1 EPS outside it) plus the root's own rounding make 2 EPS
Inputs (poses, disparities, intrinsics, beta, integer pixel coordinates) are exact.  The chain, operation for operation:
  q_ij = q_j * conj(q_i)           per component four products and three sums, left to right                       (se3.h qmul)
  R(q) v = v + w uv + q x uv, uv = 2 (q x v): a cross product is two products and a difference per component         (se3.h rotate)
  t_ij = t_j - R(q_ij) t_i         (se3.h rel_pose);   Y = R(q_ij) X + d t_ij, X = ((u - cx) / fx, (v - cy) / fy, 1)   (se3.h act4)
  projmap:   K.fx (Y0 / Z) + K.cx          reproject: 1 / Z first, then K_j.fx (Y0 * (1 / Z)) + K_j.cx          iproj: Y_i / d
  depth vote: u_j, v_j as projmap, d_j = d / Z; the comparison |1 / d_j - 1 / d_tap| < t runs in DOUBLE in the kernel, so only d_j's
  fp32 error counts: e = e_dj / d_j^2.
frame_distance: the two terms beta * d and (1 - beta) * d' of a pixel (1 - beta is one fp32 subtraction) are added to three per-thread
registers in the order the kernel's thread `tid` meets them: pixels tid, tid + 256, ... - ceil(HW / 256) trips of two terms.  That
serial sum is replayed HERE term by term with the rule for a + b above, per thread.  The wave reduction (common.h pvo_wave_sum) is a
pairwise tree of depth six - four butterfly steps inside each row of 16 lanes, then (r0 + r1) + (r2 + r3) - over non-negative partial
sums: every level rounds a value that is at most the wave's sum once, e = sum of e_lane + 6 EPS sum |lane|.  The four waves' sums are
added as (w0 + w1) + (w2 + w3), again with the rule for a + b, and the mean is one division.  An any-order bound would have cost
~2 HW EPS relative; this one is ~(2 ceil(HW / 256) + 8) EPS on the sum plus the terms' own errors.
No constant here is fitted to anything a kernel produced.

SETTLED DECISIONS.  A decision of the contract - Z > 0.25 (native validity), Z > 0.2 (the projective transform's validity), Z < 0.1 (its
clamp, fp32 0.5 * 0.2), Z > 0.01 (projmap projects), floor and in-bounds of the depth filter's four taps, each |1/dj - 1/d| < t, and
va / (to + 1e-8) < 0.75 - is SETTLED when the fp64 quantity is further from its threshold than its own bound; then the kernel must
decide as the reference does.  A value is compared only where every decision it depends on is settled: projmap's coordinates need
Z > 0.01, reproject's the clamp, a depth-filter pixel all six neighbour views (a view: the tap cell, then the four comparisons, where a
settled hit makes the rest irrelevant), a frame_distance pair every pixel's validity and the ratio.  The unsettled share of a case must
stay within UNSETTLED_CAP (1 %); tests/test_geom_fp64_host.py shows that for the case lists below with the reference alone.
Non-finite and zero disparities (one depth-filter case) are evaluated under IEEE rules: a pixel whose own disparity is 0, inf or NaN gets
no vote (1 / dj is inf or NaN and every comparison is false) and counts as settled; as a TAP such a value is compared like any other,
and a comparison whose difference is not finite is false on both sides.

MUTANTS.  Every function takes mutant=: a deliberately wrong variant that check() must reject against a correct kernel (MUTANTS)."""
import numpy as np

EPS = 2.0 ** -24
UNSETTLED_CAP = 0.01

# the kernels' own fp32 constants
MIN_DEPTH_NATIVE = np.float32(0.25)                    # droid_kernels.cu:26
MIN_DEPTH_PY = np.float32(0.2)                         # projective_ops.py:6
CLAMP_DEPTH = np.float32(0.5) * np.float32(0.2)        # projective_ops.py:48, an fp32 product
PROJ_DEPTH = np.float32(0.01)                          # droid_kernels.cu:487

MUTANTS = {
    "projmap": ("pose_inverted", "valid_0.2"),
    "iproj": ("pose_inverted",),
    "reproject": ("pose_inverted", "intr_i", "no_clamp"),
    "frame_distance": ("pose_inverted", "valid_0.2", "mean_all", "no_beta", "ratio_fp32"),
    "depth_filter": ("symmetric", "inverse_depth"),
}


# ------------------------------------------------------------------------------------------------------------ arithmetic with bounds
class F:
    """v: the exact (fp64) value on the fp32 inputs; e: first-order bound on |the kernel's fp32 value - v|"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.asarray(e, np.float64)


def _f(x):
    return x if isinstance(x, F) else F(x)


def _rnd(v, e):
    return F(v, e + EPS * np.abs(v))


def add(a, b):
    a, b = _f(a), _f(b)
    return _rnd(a.v + b.v, a.e + b.e)


def sub(a, b):
    a, b = _f(a), _f(b)
    return _rnd(a.v - b.v, a.e + b.e)


def mul(a, b):
    a, b = _f(a), _f(b)
    return _rnd(a.v * b.v, np.abs(a.v) * b.e + np.abs(b.v) * a.e)


def div(a, b):
    a, b = _f(a), _f(b)
    q = a.v / b.v
    return _rnd(q, a.e / np.abs(b.v) + np.abs(q) * b.e / np.abs(b.v))


def dbl(a):
    return F(2.0 * a.v, 2.0 * a.e)


def neg(a):
    return F(-a.v, a.e)


def hyp(a, b):
    d = np.sqrt(a.v * a.v + b.v * b.v)
    return F(d, a.e + b.e + 2.0 * EPS * d)


def where(m, a, b):
    a, b = _f(a), _f(b)
    return F(np.where(m, a.v, b.v), np.where(m, a.e, b.e))


def _cross(a, b):
    return (sub(mul(a[1], b[2]), mul(a[2], b[1])), sub(mul(a[2], b[0]), mul(a[0], b[2])), sub(mul(a[0], b[1]), mul(a[1], b[0])))


def _rotate(q, v):
    qv = q[:3]
    uv = [dbl(c) for c in _cross(qv, v)]
    c = _cross(qv, uv)
    return tuple(add(add(v[i], mul(q[3], uv[i])), c[i]) for i in range(3))


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (sub(add(add(mul(aw, bx), mul(ax, bw)), mul(ay, bz)), mul(az, by)),
            sub(add(add(mul(aw, by), mul(ay, bw)), mul(az, bx)), mul(ax, bz)),
            sub(add(add(mul(aw, bz), mul(az, bw)), mul(ax, by)), mul(ay, bx)),
            sub(sub(sub(mul(aw, bw), mul(ax, bx)), mul(ay, by)), mul(az, bz)))


def _pose(poses, idx):
    """(t, q) of the frames idx as tuples of F, each [len(idx), 1]"""
    p = np.asarray(poses, np.float32)[np.asarray(idx, np.int64)].astype(np.float64)
    return tuple(F(p[:, k:k + 1]) for k in range(3)), tuple(F(p[:, k:k + 1]) for k in range(3, 7))


def _rel(Pi, Pj):
    """G_ij = G_j * G_i^-1 (se3.h rel_pose)"""
    (ti, qi), (tj, qj) = Pi, Pj
    q = _qmul(qj, (neg(qi[0]), neg(qi[1]), neg(qi[2]), qi[3]))
    r = _rotate(q, ti)
    return tuple(sub(tj[k], r[k]) for k in range(3)), q


def _act(G, X, d):
    t, q = G
    r = _rotate(q, X)
    return tuple(add(r[k], mul(d, t[k])) for k in range(3))


def _edge_pose(poses, ii, jj, mutant, baseline=0.0):
    Pi, Pj = _pose(poses, ii), _pose(poses, jj)
    t, q = _rel(Pj, Pi) if mutant == "pose_inverted" else _rel(Pi, Pj)
    if baseline != 0.0:                                    # se3.h rig_pose on the edges (i, i): exact
        rig = (np.asarray(ii) == np.asarray(jj))[:, None]
        b = np.float64(np.float32(baseline))
        t = (where(rig, -b, t[0]), where(rig, 0.0, t[1]), where(rig, 0.0, t[2]))
        q = (where(rig, 0.0, q[0]), where(rig, 0.0, q[1]), where(rig, 0.0, q[2]), where(rig, 1.0, q[3]))
    return t, q


def _grid(ht, wd):
    k = np.arange(ht * wd)
    i = k // wd
    return (k - i * wd).astype(np.float64), i.astype(np.float64)


def _rays(K, ht, wd):
    """K = (fx, fy, cx, cy), scalars or [E,1] -> X = ((u - cx) / fx, (v - cy) / fy, 1) as F [.., HW]"""
    u, v = _grid(ht, wd)
    fx, fy, cx, cy = K
    return (div(sub(u, cx), fx), div(sub(v, cy), fy), F(np.ones_like(u)))


def _intr(intr, idx=None):
    a = np.asarray(intr, np.float32).astype(np.float64)
    if idx is None:
        return tuple(a.reshape(-1)[:4])
    a = a[np.asarray(idx, np.int64)]
    return tuple(a[:, k:k + 1] for k in range(4))


def _inputs(poses, disps, ii=None):
    poses, disps = np.asarray(poses, np.float32), np.asarray(disps, np.float32)
    nf, ht, wd = disps.shape
    d = None
    if ii is not None:
        d = F(disps.reshape(nf, -1)[np.asarray(ii, np.int64)].astype(np.float64).reshape(len(ii), ht * wd))
    return poses, disps, nf, ht, wd, d


def _decide(Z, thr):
    """(Z > thr, settled) for an F and an fp32 threshold"""
    t = np.float64(thr)
    return Z.v > t, np.abs(Z.v - t) > Z.e


def _sides(dec, settled):
    return bool(np.any(dec & settled)), bool(np.any(~dec & settled))


# ------------------------------------------------------------------------------------------------------------ the five contracts
def projmap(poses, disps, intr, ii, jj, mutant=None):
    """pvo_projmap: coords [E,ht,wd,3] = (u', v', 0) where Z > 0.01, else the pixel's own (u, v, 0); valid = Z > 0.25"""
    poses, disps, nf, ht, wd, d = _inputs(poses, disps, ii)
    E = len(ii)
    with np.errstate(all="ignore"):
        fx, fy, cx, cy = _intr(intr)
        Y = _act(_edge_pose(poses, ii, jj, mutant), _rays((fx, fy, cx, cy), ht, wd), d)
        Z = Y[2]
        cu, cv = add(mul(fx, div(Y[0], Z)), cx), add(mul(fy, div(Y[1], Z)), cy)
        proj, proj_s = _decide(Z, PROJ_DEPTH)
        valid, valid_s = _decide(Z, MIN_DEPTH_PY if mutant == "valid_0.2" else MIN_DEPTH_NATIVE)
        u, v = _grid(ht, wd)
        zero = np.zeros((E, ht * wd))
        value = np.stack([np.where(proj, cu.v, u), np.where(proj, cv.v, v), zero], -1)
        bound = np.stack([np.where(proj, cu.e, 0.0), np.where(proj, cv.e, 0.0), zero], -1)
    hi, lo = _sides(valid, valid_s)
    phi, plo = _sides(proj, proj_s)
    return dict(value=value.reshape(E, ht, wd, 3), bound=bound.reshape(E, ht, wd, 3),
                value_settled=np.repeat(proj_s[..., None], 3, -1).reshape(E, ht, wd, 3),
                decision=valid.reshape(E, ht, wd), decision_settled=valid_s.reshape(E, ht, wd),
                cover={"Z>0.25": hi, "Z<=0.25": lo, "Z>0.01": phi, "Z<=0.01": plo, "Z<0": bool(np.any(Z.v + Z.e < 0))})


def iproj(poses, disps, intr, mutant=None):
    """pvo_iproj: points [N,ht,wd,3] = act(G_n, X) / d - the pose itself, not its inverse (droid_kernels.cu:822)"""
    poses, disps, nf, ht, wd, d = _inputs(poses, disps, np.arange(np.asarray(disps).shape[0]))
    with np.errstate(all="ignore"):
        t, q = _pose(poses, np.arange(nf))
        if mutant == "pose_inverted":                       # G^-1 = (-R^T t, conj q)
            q = (neg(q[0]), neg(q[1]), neg(q[2]), q[3])
            t = tuple(neg(c) for c in _rotate(q, t))
        Y = _act((t, q), _rays(_intr(intr), ht, wd), d)
        P = [div(Y[k], d) for k in range(3)]
    shape = (nf, ht, wd, 3)
    return dict(value=np.stack([p.v for p in P], -1).reshape(shape), bound=np.stack([p.e for p in P], -1).reshape(shape),
                value_settled=np.ones(shape, bool), cover={})


def reproject(poses, disps, intr, ii, jj, baseline=0.0, mutant=None):
    """pvo_reproject / pvo_reproject_rig: intr [F,4] per frame; coords [E,ht,wd,2] = K_j (X1 / Z'), Z' = 1 where Z < 0.1;
    valid = Z > 0.2 (X0's own Z is 1)"""
    poses, disps, nf, ht, wd, d = _inputs(poses, disps, ii)
    E = len(ii)
    with np.errstate(all="ignore"):
        Ki, Kj = _intr(intr, ii), _intr(intr, ii if mutant == "intr_i" else jj)
        Y = _act(_edge_pose(poses, ii, jj, mutant, baseline), _rays(Ki, ht, wd), d)
        Z = Y[2]
        t = np.float64(CLAMP_DEPTH)
        clamp, clamp_s = Z.v < t, np.abs(Z.v - t) > Z.e
        Zc = Z if mutant == "no_clamp" else where(clamp, 1.0, Z)
        r = div(1.0, Zc)
        cu, cv = add(mul(Kj[0], mul(Y[0], r)), Kj[2]), add(mul(Kj[1], mul(Y[1], r)), Kj[3])
        valid, valid_s = _decide(Z, MIN_DEPTH_PY)
    hi, lo = _sides(valid, valid_s)
    chi, clo = _sides(clamp, clamp_s)
    return dict(value=np.stack([cu.v, cv.v], -1).reshape(E, ht, wd, 2), bound=np.stack([cu.e, cv.e], -1).reshape(E, ht, wd, 2),
                value_settled=np.repeat(clamp_s[..., None], 2, -1).reshape(E, ht, wd, 2),
                decision=valid.reshape(E, ht, wd), decision_settled=valid_s.reshape(E, ht, wd),
                cover={"Z>0.2": hi, "Z<=0.2": lo, "Z<0.1": chi, "Z>=0.1": clo, "Z<0": bool(np.any(Z.v + Z.e < 0))})


def _thread_sum(terms, HW):
    """terms: list of (mask [M,HW] bool, F [M,HW] or a scalar F) in the order a thread meets them per pixel -> the workgroup's sum as
    the kernel forms it: 256 serial per-thread sums over the pixels tid, tid + 256, ...; the wave tree; the four-wave tree"""
    M = terms[0][0].shape[0]
    T = (HW + 255) // 256
    pad = T * 256 - HW

    def lanes(a, fill):
        a = np.broadcast_to(np.asarray(a), (M, HW))
        return np.concatenate([a, np.full((M, pad), fill, a.dtype)], 1).reshape(M, T, 256)
    acc = F(np.zeros((M, 256)), np.zeros((M, 256)))
    prepared = [(lanes(m, False), lanes(_f(x).v, 0.0), lanes(_f(x).e, 0.0)) for m, x in terms]
    for t in range(T):
        for m, v, e in prepared:
            acc = where(m[:, t], add(acc, F(v[:, t], e[:, t])), acc)
    v, e = acc.v.reshape(M, 4, 64), acc.e.reshape(M, 4, 64)
    w = [F(v[:, k].sum(1), e[:, k].sum(1) + 6.0 * EPS * np.abs(v[:, k]).sum(1)) for k in range(4)]
    return add(add(w[0], w[1]), add(w[2], w[3]))


def frame_distance(poses, disps, intr, ii, jj, beta, mutant=None):
    """pvo_frame_distance, one direction: the mean over the VALID (Z > 0.25) pixels of beta |flow| + (1 - beta) |translation-only flow|,
    or 1000 where valid / (total + 1e-8) < 0.75 (evaluated in double)"""
    poses, disps, nf, ht, wd, d = _inputs(poses, disps, ii)
    M, HW = len(ii), ht * wd
    if M == 0:
        return dict(value=np.zeros(0), bound=np.zeros(0), value_settled=np.zeros(0, bool), cover={})
    with np.errstate(all="ignore"):
        fx, fy, cx, cy = _intr(intr)
        u, v = _grid(ht, wd)
        beta = F(np.float64(np.float32(1.0 if mutant == "no_beta" else beta)))
        omb = sub(1.0, beta)
        thr = MIN_DEPTH_PY if mutant == "valid_0.2" else MIN_DEPTH_NATIVE
        G = _edge_pose(poses, ii, jj, mutant)
        X = _rays((fx, fy, cx, cy), ht, wd)

        def flow(Y):
            du = sub(add(mul(fx, div(Y[0], Y[2])), cx), u)
            dv = sub(add(mul(fy, div(Y[1], Y[2])), cy), v)
            return hyp(du, dv)
        Y1 = _act(G, X, d)
        Y2 = tuple(add(X[k], mul(d, G[0][k])) for k in range(3))
        ok1, s1 = _decide(Y1[2], thr)
        ok2, s2 = _decide(Y2[2], thr)
        every = np.ones((M, HW), bool)
        a = _thread_sum([(ok1, mul(beta, flow(Y1))), (ok2, mul(omb, flow(Y2)))], HW)
        va = _thread_sum([(ok1, beta), (ok2, omb)], HW)
        to = _thread_sum([(every, beta), (every, omb)], HW)
        ratio = va.v / (to.v + 1e-8)
        e_ratio = va.e / to.v + ratio * to.e / to.v
        if mutant == "ratio_fp32":
            far = np.float32(va.v) / (np.float32(to.v) + np.float32(1e-8)) < np.float32(0.75)
        else:
            far = ratio < 0.75
        mean = div(a, to if mutant == "mean_all" else va)
        settled = (np.abs(ratio - 0.75) > e_ratio)
        if beta.v != 0:
            settled &= s1.all(1)
        if omb.v != 0:
            settled &= s2.all(1)
    return dict(value=np.where(far, 1000.0, mean.v), bound=np.where(far, 0.0, mean.e), value_settled=settled,
                cover={"finite": bool(np.any(~far & settled)), "1000": bool(np.any(far & settled)),
                       "finite with 0.2<Z<=0.25": bool(np.any((~far & settled)[:, None] & (Y1[2].v > 0.2) & (Y1[2].v <= 0.25)))})


NEIGHBOURS = (-1, -2, -3, 3, 4, 5)                         # droid_kernels.cu:674: deliberately not symmetric


def depth_filter(poses, disps, intr, ix, thresh, mutant=None):
    """pvo_depth_filter: votes [N,ht,wd] - in how many of the views ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 (those inside [0, nframes)) one
    of the four taps around the projection (floor inside [0, wd-1) x [0, ht-1)) has |1/dj - 1/d_tap| < t"""
    poses, disps, nf, ht, wd, _ = _inputs(poses, disps)
    ix = [int(x) for x in np.asarray(ix).reshape(-1)]
    thresh = np.asarray(thresh, np.float32).astype(np.float64).reshape(-1)
    HW = ht * wd
    flat = disps.reshape(nf, HW).astype(np.float64)
    votes = np.zeros((len(ix), HW), np.int64)
    settled = np.ones((len(ix), HW), bool)
    border = {"left": False, "top": False, "right": False, "bottom": False}
    offsets = (-1, -2, -3, 1, 2, 3) if mutant == "symmetric" else NEIGHBOURS
    with np.errstate(all="ignore"):
        fx, fy, cx, cy = _intr(intr)
        X = _rays((fx, fy, cx, cy), ht, wd)
        for b, f in enumerate(ix):
            d = F(flat[f][None])
            dead = ~np.isfinite(d.v[0]) | (d.v[0] == 0)      # no vote under IEEE rules, whatever the view
            for off in offsets:
                jx = f + off
                if jx < 0 or jx >= nf:
                    continue
                Y = _act(_rel(_pose(poses, [f]), _pose(poses, [jx])), X, d)
                uj, vj = add(mul(fx, div(Y[0], Y[2])), cx), add(mul(fy, div(Y[1], Y[2])), cy)
                dj = div(d, Y[2])
                cell, cell_s, refused = [], [], []
                for c, n in ((uj, wd), (vj, ht)):
                    c0 = np.clip(np.where(np.isnan(c.v), 0.0, np.floor(c.v)), -2.0 ** 30, 2.0 ** 30).astype(np.int64)[0]
                    lo, hi = (c.v - c.e)[0], (c.v + c.e)[0]
                    out = (hi < 0) | (lo >= n - 1)               # refused whatever the rounding
                    cell.append(c0); refused.append(out)
                    cell_s.append((np.floor(lo) == np.floor(hi)) | out)
                u0, v0 = cell
                inb = (u0 >= 0) & (v0 >= 0) & (u0 < wd - 1) & (v0 < ht - 1)
                tap_s = (cell_s[0] & cell_s[1]) | refused[0] | refused[1]
                for name, m in (("left", u0 < 0), ("top", v0 < 0), ("right", u0 >= wd - 1), ("bottom", v0 >= ht - 1)):
                    border[name] = border[name] or bool(np.any(m & tap_s & ~dead))
                uc, vc = np.clip(u0, 0, max(wd - 2, 0)), np.clip(v0, 0, max(ht - 2, 0))
                taps = [flat[jx][np.minimum((vc + a) * wd + uc + c, HW - 1)] for a, c in ((0, 0), (0, 1), (1, 0), (1, 1))]
                if mutant == "inverse_depth":
                    mine, e = dj.v[0], dj.e[0]
                    diffs = [mine - tp for tp in taps]
                else:
                    mine, e = 1.0 / dj.v[0], dj.e[0] / (dj.v[0] * dj.v[0])
                    diffs = [mine - 1.0 / tp for tp in taps]
                close = [np.abs(df) < thresh[b] for df in diffs]
                close_s = [~np.isfinite(df) | (np.abs(np.abs(df) - thresh[b]) > e) for df in diffs]
                hit = inb & (close[0] | close[1] | close[2] | close[3]) & ~dead
                sure_hit = (close[0] & close_s[0]) | (close[1] & close_s[1]) | (close[2] & close_s[2]) | (close[3] & close_s[3])
                view_s = dead | (tap_s & (~inb | sure_hit | (close_s[0] & close_s[1] & close_s[2] & close_s[3])))
                votes[b] += hit
                settled[b] &= view_s
    cover = {"votes%d" % n: bool(np.any((votes == n) & settled)) for n in range(7)}
    cover.update(border)
    shape = (len(ix), ht, wd)
    return dict(value=votes.astype(np.float64).reshape(shape), bound=np.zeros(shape), value_settled=settled.reshape(shape), cover=cover)


# ------------------------------------------------------------------------------------------------------------ the check
def check(kind, got, ref, exact=False, cap=UNSETTLED_CAP):
    """got: what a kernel (or the C oracle) returned for `kind` - (coords, valid) for projmap and reproject, one array otherwise; ref:
    the dict of the function of that name above.  Values are held to err <= bound on every element whose decisions are settled,
    decisions to equality where settled; exact=True (inputs on which the kernel's arithmetic is exact) exempts nothing.
    Returns (ok, report): report = dict(worst = max err / bound, unsettled = the larger unsettled share, mismatches = elements over
    their bound + settled decisions that differ + validity flags that are neither 0 nor 1)."""
    if kind in ("projmap", "reproject"):
        values, flags = [np.asarray(g, np.float64) for g in got]
        flags = flags.reshape(ref["decision"].shape)
    else:
        values, flags = np.asarray(got, np.float64), None
    values = values.reshape(ref["value"].shape)
    mismatches, shares = 0, [0.0]
    vs = np.ones_like(ref["value_settled"]) if exact else ref["value_settled"]
    with np.errstate(all="ignore"):
        err = np.abs(values - ref["value"])
        ratio = np.where(err == 0, 0.0, err / ref["bound"])
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
    worst = float(ratio[vs].max()) if vs.any() else 0.0
    mismatches += int(np.count_nonzero(ratio[vs] > 1.0))
    if vs.size:
        shares.append(1.0 - np.count_nonzero(ref["value_settled"]) / float(vs.size))
    if flags is not None:
        ds = np.ones_like(ref["decision_settled"]) if exact else ref["decision_settled"]
        mismatches += int(np.count_nonzero((flags != 0.0) & (flags != 1.0)))
        mismatches += int(np.count_nonzero(((flags > 0.5) != ref["decision"]) & ds))
        if ds.size:
            shares.append(1.0 - np.count_nonzero(ref["decision_settled"]) / float(ds.size))
    rep = dict(worst=worst, unsettled=float(max(shares)), mismatches=mismatches)
    return mismatches == 0 and (exact or rep["unsettled"] <= cap), rep


# ------------------------------------------------------------------------------------------------------------ the case lists
def _quat(w):
    """unit quaternion (x, y, z, w) of the rotation vector w, fp64"""
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.concatenate([np.sin(0.5 * th) * np.asarray(w) / th, [np.cos(0.5 * th)]])


# (ht, wd): 15 pixels, less than one wave - three of frame_distance's four waves add nothing; 261 = 256 + 5, a second workgroup of five
# pixels and a second stride trip; 288; 1032 = 4 * 256 + 8 with an odd width
GRAPH_MAPS = ((3, 5), (9, 29), (18, 16), (24, 43))
LINE_MAPS = ((1, 70), (70, 1))                             # k / wd with wd == 1, a map no tap of the depth filter fits into
GRAPH_II = (0, 1, 1, 2, 3, 5, 0, 5, 2, 0, 4, 5, 3, 4)      # both directions, (2, 2) and (5, 5), (0, 1) twice; frame 5 far behind,
GRAPH_JJ = (1, 0, 2, 1, 5, 3, 5, 0, 2, 1, 5, 5, 4, 3)      # frame 4 half as far
BETAS = (0.3, 1.0, 0.0)
BASELINE = 0.1
SEED = 7


def graph_case(ht, wd, seed=SEED):
    """six frames with small random twists, frame 5 1.2 behind the others, inverse depths in (0.05, 1.55): Z = r_z + d t_z lands on both
    sides of 0.25, 0.2, 0.1 and 0.01 and below zero on the edges into and out of frame 5.  Frame 4 is 0.55 behind: on the edge 3 -> 4
    most pixels stay valid, so the distance is finite, while some Z fall between 0.2 and 0.25; pixel (0, 1) of frame 3 is PLACED there
    (Z = 0.225 in the fp64 reference: Z is linear in d), so that even the 15-pixel map has one.  Intrinsics differ from frame to frame.
    Returns numpy fp32 poses [6,7], disps [6,ht,wd], intr [6,4] and int64 ii, jj."""
    rng = np.random.default_rng(seed + 1000 * ht + wd)
    F_ = 6
    poses = np.zeros((F_, 7))
    for f in range(F_):
        poses[f, :3] = 0.15 * rng.standard_normal(3)
        poses[f, 3:] = _quat(0.08 * rng.standard_normal(3))
    poses[5, :3] = [0.02, -0.03, -1.2]
    poses[3, :3] = [0.05, -0.04, 0.03]
    poses[4, :3] = [-0.03, 0.02, -0.55]
    disps = rng.random((F_, ht, wd)) * 1.5 + 0.05
    s = max(ht, wd)
    intr = np.array([[0.8 * s, 0.7 * s, wd / 2.0 - 0.3, ht / 2.0 + 0.2]]).repeat(F_, 0) * (1.0 + 0.03 * np.arange(F_))[:, None]
    poses, disps, intr = poses.astype(np.float32), disps.astype(np.float32), intr.astype(np.float32)
    if ht * wd > 1:
        probe = np.zeros((F_, ht, wd), np.float32)
        probe[3].reshape(-1)[1] = 1.0
        X, G = _rays(_intr(intr[0]), ht, wd), _edge_pose(poses, [3], [4], None)
        z0, z1 = [_act(G, X, F(np.full((1, ht * wd), dd)))[2].v[0, 1] for dd in (0.0, 1.0)]
        disps[3].reshape(-1)[1] = np.float32((0.225 - z0) / (z1 - z0))
    return poses, disps, intr, np.array(GRAPH_II, np.int64), np.array(GRAPH_JJ, np.int64)


# (name, nframes, ht, wd, noise, thresholds, special): 1 frame: no view at all; 3: views at distance 1 and 2 only; 4: the first +3; 10:
# frame 4 has all six.  Every frame is filtered (ix = 0 .. nframes-1), once per threshold.
DEPTH_CASES = (
    ("1x3x5", 1, 3, 5, 0.0, (0.05, 0.2), False),
    ("3x9x29", 3, 9, 29, 0.02, (0.02, 0.2), False),
    ("4x18x16", 4, 18, 16, 0.02, (0.02, 0.2), False),
    ("10x24x43", 10, 24, 43, 0.01, (0.01, 0.3), False),
    ("10x9x29s", 10, 9, 29, 0.02, (0.02, 0.2), True),
    ("4x1x70", 4, 1, 70, 0.02, (0.02, 0.2), False),
    ("4x70x1", 4, 70, 1, 0.02, (0.02, 0.2), False),
)
SPECIAL_VALUES = (0.0, -0.5, np.inf, np.nan, 0.0, -0.25, np.inf, np.nan)


def depth_case(name):
    """the constant-twist, smooth-field scene of tests/map_reference.py with the principal point moved off the pixel lattice; `special` puts eight pixels with disparity 0, negative, inf and
    NaN into frames 3 and 5.  Returns numpy poses, disps, intr [4], ix int64 [2 nframes], thresh fp32 [2 nframes]."""
    import map_reference as M
    _, nf, ht, wd, noise, ths, special = [c for c in DEPTH_CASES if c[0] == name][0]
    poses, disps, intr = [x.numpy() for x in M.scene(M.SEED, nf, ht, wd, noise)]
    intr = intr + np.array([0.0, 0.0, 0.2, -0.3], np.float32)   # off the lattice: with cy on a pixel row v_j = cy on that whole row, a tie
    if special:
        rng = np.random.default_rng(3)
        for n, val in enumerate(SPECIAL_VALUES):
            disps[3 if n < 4 else 5, rng.integers(1, ht - 1), rng.integers(1, wd - 1)] = val
    ix = np.concatenate([np.arange(nf), np.arange(nf)]).astype(np.int64)
    thresh = np.repeat(np.asarray(ths, np.float32), nf)
    return poses, disps, intr.astype(np.float32), ix, thresh


def exact_threshold_case():
    """identity rotations, frame 1 at t = (0, 0, -1): on the edge 0 -> 1 Z = 1 - d EXACTLY in fp32 for d in [0.5, 1] (the rotation of
    (X, Y, 1) by the identity quaternion adds zeros, d * -1 is exact and so is 1 - d by Sterbenz' lemma), and every such Z is a multiple
    of 2^-24.  The pixels carry Z = 0.25 and its two neighbours on that lattice, and the two lattice points either side of fp32 0.2,
    fp32 0.1 and fp32 0.01; the rest is padding at Z = 0.5.  A 3 x 5 map.  Returns poses, disps, intr [2,4], ii, jj, Z fp64 [15]."""
    step = 2.0 ** -24
    zs = [0.25, 0.25 - step, 0.25 + step]
    for thr in (MIN_DEPTH_PY, CLAMP_DEPTH, PROJ_DEPTH):
        k = np.floor(np.float64(thr) / step)
        zs += [k * step, (k + 1) * step] if k * step != np.float64(thr) else [(k - 1) * step, (k + 1) * step]
    zs = np.array(zs + [0.5] * (15 - len(zs)))
    d = (1.0 - zs).astype(np.float32)
    assert np.array_equal(1.0 - d.astype(np.float64), zs) and d.min() >= 0.5 and d.max() <= 1.0
    poses = np.array([[0, 0, 0, 0, 0, 0, 1], [0, 0, -1, 0, 0, 0, 1]], np.float32)
    disps = np.stack([d.reshape(3, 5), np.full((3, 5), 0.75, np.float32)])
    intr = np.array([[4.0, 4.0, 2.0, 1.0], [4.0, 4.0, 2.0, 1.0]], np.float32)
    return poses, disps, intr, np.array([0], np.int64), np.array([1], np.int64), zs


def exact_ratio_case(nvalid):
    """the same two frames on a 4 x 4 map, beta = 1: nvalid pixels at Z = 0.5, the others at Z = 0.125.  valid and total are small
    integers, exact in fp32 in any order.  12 of 16: 12 / (16 + 1e-8) < 0.75 in double - exactly 1000.0 - while 12.f / 16.f is not."""
    d = np.full(16, 0.875, np.float32)
    d[np.arange(16)[::-1][:nvalid] if nvalid < 16 else slice(None)] = 0.5
    poses = np.array([[0, 0, 0, 0, 0, 0, 1], [0, 0, -1, 0, 0, 0, 1]], np.float32)
    disps = np.stack([d.reshape(4, 4), np.full((4, 4), 0.75, np.float32)])
    return poses, disps, np.array([4.0, 4.0, 2.0, 2.0], np.float32), np.array([0], np.int64), np.array([1], np.int64)
