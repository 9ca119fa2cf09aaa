"""The stereo tests' own yardstick: one Gauss-Newton step of the dense bundle adjustment with STEREO edges, in numpy fp64.  Neither
the reference nor oracle/ has a stereo mode, so there is nothing of theirs to record.  Built like tests/rgbd_reference.py:
oracle.ba_assemble for ordinary edges, and for a stereo edge (i, i) - with baseline b > 0 - this file's own fp64 per-pixel terms:

    T_b: [X, Y, 1, d] -> [X - b d, Y, 1, d],   u_right = fx (X - b d) + cx = u - fx b d,   v_right = v
    Jz = d u_right / d d = -fx b  (x residual),  0  (y residual);  no pose Jacobian: the rig is rigid
    C += 0.001 w_u Jz^2,   w += 0.001 w_u (target_u - u_right) Jz;   Hs = vs = Eii = Eij = 0

Everything behind the assembly is rgbd_reference.gn_step's arithmetic in its order (the sensor-depth prior included: the two terms are
independent and both apply), so without a stereo edge the two agree bit for bit.  tests/test_stereo_host.py qualifies this file
before anything is held to it."""
import numpy as np

import rgbd_reference as R
from oracle import oracle as O

ALPHA = R.ALPHA


def stereo_project(u, v, d, intr, b):
    """fp64: pixel (u, v) of the left view with inverse depth d -> its pixel in the right view of a rectified rig with baseline b"""
    fx, fy, cx, cy = [float(x) for x in intr]
    X, Y, Z = (u - cx) / fx - b * d, (v - cy) / fy, 1.0
    return fx * X / Z + cx, fy * Y / Z + cy


def stereo_jz(intr, b):
    """(d u_right / d d, d v_right / d d) of stereo_project: constants"""
    return -float(intr[0]) * b, 0.0


def stereo_terms(disp, intr, target, weight, b):
    """Cii, bz [HW] (fp64) of one stereo edge: disp [ht,wd], target / weight [2,ht,wd]"""
    ht, wd = disp.shape
    v, u = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
    d = disp.astype(np.float64)
    pu, pv = stereo_project(u, v, d, intr, b)
    ju, jv = stereo_jz(intr, b)
    wu, wv = 0.001 * weight[0].astype(np.float64), 0.001 * weight[1].astype(np.float64)
    ru, rv = target[0].astype(np.float64) - pu, target[1].astype(np.float64) - pv
    C = wu * ju * ju + wv * jv * jv
    w = wu * ru * ju + wv * rv * jv
    return C.reshape(-1), w.reshape(-1)


def reproject(poses, disps, intr_all, ii, jj, b=0.0):
    """oracle.reproject, with the closed form for the stereo edges (i, i) when b > 0 -> (coords [E,ht,wd,2] fp64, valid [E,ht,wd,1])"""
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    c, val = O.reproject(poses, disps, intr_all, ii, jj)
    c = c.astype(np.float64)
    if b > 0:
        ht, wd = disps.shape[1:]
        v, u = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
        for e in np.nonzero(ii == jj)[0]:
            pu, pv = stereo_project(u, v, np.asarray(disps[ii[e]], np.float64), intr_all[ii[e]], b)
            c[e, ..., 0], c[e, ..., 1] = pu, pv
            val[e] = 1.0                                            # (Z = 1 on both sides: above the 0.2 of projective_ops.py)
    return c, val


def gn_step(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, lm, ep, baseline=0.0, sens=None, alpha=ALPHA):
    """-> (poses, disps, dz [K,HW], kx) after one step; inputs are not modified.  eta [K,ht,wd] or [1,ht,wd]."""
    poses, disps = np.ascontiguousarray(poses, np.float32), np.ascontiguousarray(disps, np.float32)
    target, weight = np.ascontiguousarray(target, np.float32), np.ascontiguousarray(weight, np.float32)
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    F, ht, wd = disps.shape
    HW, E, P = ht * wd, ii.shape[0], t1 - t0
    n6 = 6 * P
    st = (ii == jj) if baseline > 0 else np.zeros(E, bool)
    o = np.nonzero(~st)[0]
    Hs, vs = np.zeros((4, E, 6, 6)), np.zeros((2, E, 6))
    Eii, Eij = np.zeros((E, 6, HW)), np.zeros((E, 6, HW))
    Cii, bz = np.zeros((E, HW)), np.zeros((E, HW))
    if o.size:
        a = O.ba_assemble(poses, disps, intr, np.ascontiguousarray(target[o]), np.ascontiguousarray(weight[o]), ii[o], jj[o])
        Hs[:, o] = a["Hs"].astype(np.float32).astype(np.float64)       # (the reference stores fp32 sums: rounded as the oracle does)
        vs[:, o] = a["vs"].astype(np.float32).astype(np.float64)
        Eii[o], Eij[o] = a["Eii"].astype(np.float64), a["Eij"].astype(np.float64)
        Cii[o], bz[o] = a["Cii"].astype(np.float64), a["bz"].astype(np.float64)
    for e in np.nonzero(st)[0]:                                        # stereo edges: depth terms only, zero pose rows
        Cii[e], bz[e] = stereo_terms(disps[ii[e]], intr, target[e], weight[e], baseline)
    A, b = np.zeros((n6, n6)), np.zeros(n6)
    blk = lambda p: slice(6 * p, 6 * p + 6)
    for e in range(E):
        pi, pj = int(ii[e]) - t0, int(jj[e]) - t0
        iok, jok = 0 <= pi < P, 0 <= pj < P
        if iok:
            A[blk(pi), blk(pi)] += Hs[0, e]; b[blk(pi)] += vs[0, e]
        if jok:
            A[blk(pj), blk(pj)] += Hs[3, e]; b[blk(pj)] += vs[1, e]
        if iok and jok:
            A[blk(pi), blk(pj)] += Hs[1, e]; A[blk(pj), blk(pi)] += Hs[2, e]
    kx = np.unique(np.concatenate([np.arange(t0, t1, dtype=np.int64), ii]))
    K = kx.shape[0]
    kidx = {int(f): k for k, f in enumerate(kx)}
    C, w, deg = np.zeros((K, HW)), np.zeros((K, HW)), np.zeros(K, np.int64)
    Ei = np.zeros((P, 6, HW))
    for e in range(E):
        k = kidx[int(ii[e])]
        C[k] += Cii[e]; w[k] += bz[e]; deg[k] += 1
        if 0 <= int(ii[e]) - t0 < P:
            Ei[int(ii[e]) - t0] += Eii[e]
    eta = np.asarray(eta, np.float64).reshape(-1, HW)
    add = np.broadcast_to(eta, (K, HW)).copy() if eta.shape[0] == 1 else eta.copy()
    assert add.shape == (K, HW)
    if sens is not None:
        s = np.asarray(sens, np.float64).reshape(F, HW)[kx]
        d = disps.astype(np.float64).reshape(F, HW)[kx]
        m = (s > 0) & (deg > 0)[:, None]
        add = np.where(m, alpha, add)
        w = w - np.where(m, alpha * (d - s), 0.0)
    Q = 1.0 / (C + add)
    rows = [[] for _ in range(K)]
    for p in range(P):
        rows[kidx[t0 + p]].append((p, Ei[p]))
    for e in range(E):
        rows[kidx[int(ii[e])]].append((int(jj[e]) - t0, Eij[e]))
    for k in range(K):
        live = [(p, M) for p, M in rows[k] if 0 <= p < P]
        if not live:
            continue
        M = np.concatenate([m_ for _, m_ in live], 0)                  # [6r, HW]
        S = (M * Q[k]) @ M.T
        v = M @ (Q[k] * w[k])
        for x, (pa, _) in enumerate(live):
            b[blk(pa)] -= v[6 * x:6 * x + 6]
            for y, (pb, _) in enumerate(live):
                A[blk(pa), blk(pb)] -= S[6 * x:6 * x + 6, 6 * y:6 * y + 6]
    if P > 0:
        A[np.diag_indices(n6)] += ep + lm * np.diag(A)
        L = np.linalg.cholesky(A)
        dx = np.linalg.solve(L.T, np.linalg.solve(L, b)).reshape(P, 6)
    else:                                                              # a depth-only step: no pose block, no solve
        dx = np.zeros((0, 6))
    acc = np.zeros((K, HW))
    for k in range(K):
        for p, M in rows[k]:
            if 1 <= p < P:
                acc[k] += dx[p] @ M
    dz = Q * (w - acc)
    poses_out = O.pose_retr(poses, dx.astype(np.float32), t0, t1) if P > 0 else poses.copy()
    disps_out = disps.astype(np.float64).reshape(F, HW).copy()
    disps_out[kx] += dz
    return poses_out, disps_out.reshape(F, ht, wd).astype(np.float32), dz, kx


def ba(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, iters, lm, ep, baseline=0.0, sens=None, alpha=ALPHA):
    """`iters` steps; disps pass through fp32 between steps, as the device's and the oracle's do"""
    for _ in range(iters):
        poses, disps, _, _ = gn_step(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, lm, ep, baseline, sens, alpha)
    return poses, disps


def with_stereo_edges(ii, jj, frames):
    """the edge lists with the stereo edge (f, f) of every frame of `frames` in FRONT (as the factor graph requests them)"""
    f = np.asarray(list(frames), np.int64)
    return np.concatenate([f, np.asarray(ii, np.int64)]), np.concatenate([f, np.asarray(jj, np.int64)])


def window(seed, F, ht, wd, baseline, stereo_frames, radius=2, t0=1, ii=None, jj=None, eta_rows=None):
    """rgbd_reference.window (poses one step behind the truth, depths off, weights in [0.5, 1.5]) with the stereo edges of
    `stereo_frames` in front of the graph's edges; their targets are the TRUE right-view pixels u - fx b d_true plus the same 0.1 px
    of noise.  eta_rows = 1: a single broadcast row."""
    import torch
    if ii is None:
        ii, jj = R.radius_graph(F, radius)
    ii, jj = with_stereo_edges(ii, jj, stereo_frames)
    s = R.window(seed, F, ht, wd, t0=t0, ii=ii, jj=jj)
    ns = len(list(stereo_frames))
    # the truth R.window drew its targets from: depths from the same seeded generator, first draw
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(1, 1, 6, 8, generator=g) * 0.8 + 0.2
    disps_gt = torch.nn.functional.interpolate(low, size=(ht, wd), mode="bilinear", align_corners=True)[0, 0]
    v, u = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
    pu, pv = stereo_project(u, v, disps_gt.numpy().astype(np.float64), s["intr"].numpy(), baseline)
    g2 = torch.Generator().manual_seed(seed + 7919)
    tgt = s["target"].clone()
    for e in range(ns):
        tgt[e, 0] = torch.from_numpy(pu).float() + 0.1 * torch.randn(ht, wd, generator=g2)
        tgt[e, 1] = torch.from_numpy(pv).float() + 0.1 * torch.randn(ht, wd, generator=g2)
    s["target"] = tgt.contiguous()
    s["baseline"], s["n_stereo"] = float(baseline), ns
    if eta_rows == 1:
        s["eta"] = s["eta"][:1].contiguous()
    return s


def reference(s, iters, baseline="own", lm=1e-4, ep=0.1, sens=None):
    n = lambda t: t.numpy()
    b = s["baseline"] if isinstance(baseline, str) else baseline
    return ba(n(s["poses"]), n(s["disps"]), n(s["intr"]), n(s["target"]), n(s["weight"]), n(s["eta"]), n(s["ii"]), n(s["jj"]),
              s["t0"], s["t1"], iters, lm, ep, b, sens)
