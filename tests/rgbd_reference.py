"""The RGB-D tests' own yardstick: one Gauss-Newton step of the dense bundle adjustment WITH the sensor-depth prior, in numpy fp64
on top of the oracle's assembly (oracle.ba_assemble) - the reference has no RGB-D mode, so there is nothing of it to record.

    C' = C + (m ? alpha : eta),   w' = w - (m ? alpha (d - s) : 0),   Q = 1 / C',     m = s > 0 and the frame has an out-edge

Everything else is ba_cuda's step as oracle/oracle_ba.c restates it: pose blocks for poses in [t0, t1), Schur rows [Ei (P); Eij (E)]
paired where they share a depth frame, diag += ep + lm diag, Cholesky, dz = Q (w' - sum E^T dx) without the rows of window pose 0
(EvT6x1's `<= 0`), oracle.pose_retr.  tests/test_rgbd_host.py qualifies it against oracle.ba before anything is held to it."""
import numpy as np

from oracle import oracle as O

ALPHA = 0.05


def gn_step(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, lm, ep, sens=None, alpha=ALPHA):
    """-> (poses, disps, dz [K,HW], kx) after one step; inputs are not modified.  eta [K,ht,wd] or [1,ht,wd]."""
    poses, disps = np.ascontiguousarray(poses, np.float32), np.ascontiguousarray(disps, np.float32)
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    F, ht, wd = disps.shape
    HW, E, P = ht * wd, ii.shape[0], t1 - t0
    n6 = 6 * P
    a = O.ba_assemble(poses, disps, intr, target, weight, ii, jj)
    Hs = a["Hs"].astype(np.float32).astype(np.float64)               # (the reference stores fp32 sums: rounded as the oracle does)
    vs = a["vs"].astype(np.float32).astype(np.float64)
    Eii, Eij = a["Eii"].astype(np.float64), a["Eij"].astype(np.float64)
    Cii, bz = a["Cii"].astype(np.float64), a["bz"].astype(np.float64)
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
    # Schur rows by depth frame: (pose, rows [6,HW])
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
    A[np.diag_indices(n6)] += ep + lm * np.diag(A)
    L = np.linalg.cholesky(A)
    dx = np.linalg.solve(L.T, np.linalg.solve(L, b)).reshape(P, 6)
    acc = np.zeros((K, HW))
    for k in range(K):
        for p, M in rows[k]:
            if 1 <= p < P:
                acc[k] += dx[p] @ M
    dz = Q * (w - acc)
    poses_out = O.pose_retr(poses, dx.astype(np.float32), t0, t1)
    disps_out = disps.astype(np.float64).reshape(F, HW).copy()
    disps_out[kx] += dz
    return poses_out, disps_out.reshape(F, ht, wd).astype(np.float32), dz, kx


def ba(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, iters, lm, ep, sens=None, alpha=ALPHA):
    """`iters` steps; disps pass through fp32 between steps, as the device's and the oracle's do"""
    for _ in range(iters):
        poses, disps, _, _ = gn_step(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, lm, ep, sens, alpha)
    return poses, disps


def radius_graph(n, radius, lo=0):
    pairs = [(i, j) for i in range(lo, n) for j in range(lo, n) if i != j and abs(i - j) <= radius]
    return np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)


def window(seed, F, ht, wd, radius=2, t0=1, ii=None, jj=None, measured=0.7, residual=0.1):
    """a synthetic window in the recipe of tests/test_geom_ba_gpu.py's `_scene` with weights in [0.5, 1.5] and a sensor map: about
    `measured` of the pixels carry a value, `residual` (relative) away from the current inverse depth - 0 gives residual exactly 0"""
    import torch
    from pvo_amd.geom.se3 import SE3
    g = torch.Generator().manual_seed(seed)
    intr = torch.tensor([wd * 0.625, wd * 0.625, wd / 2.0, ht / 2.0])
    xi = torch.tensor([0.05, 0.0, 0.02, 0.0, 0.01, 0.0])
    poses_gt = torch.stack([SE3.exp(k * xi).data for k in range(F)], 0)
    low = torch.rand(1, 1, 6, 8, generator=g) * 0.8 + 0.2
    disps_gt = torch.nn.functional.interpolate(low, size=(ht, wd), mode="bilinear", align_corners=True)[0, 0][None].repeat(F, 1, 1)
    if ii is None:
        ii, jj = radius_graph(F, radius)
    ii, jj = torch.as_tensor(ii), torch.as_tensor(jj)
    E = ii.shape[0]
    c, _ = O.reproject(poses_gt.numpy(), disps_gt.numpy(), intr[None].repeat(F, 1).numpy(), ii.numpy(), jj.numpy())
    target = torch.from_numpy(c) + 0.1 * torch.randn(E, ht, wd, 2, generator=g)
    weight = torch.rand(E, ht, wd, 2, generator=g) + 0.5
    poses0 = torch.stack([poses_gt[max(k - 1, 0)] for k in range(F)], 0)
    disps0 = torch.ones(F, ht, wd) + 0.2 * torch.rand(F, ht, wd, generator=g)
    K = int(np.unique(np.concatenate([np.arange(t0, F), ii.numpy()])).shape[0])
    eta = torch.full((K, ht, wd), 1e-4) + 0.01 * torch.rand(K, ht, wd, generator=g)
    has = torch.rand(F, ht, wd, generator=g) < measured
    sens = torch.where(has, disps0 * (1.0 + residual * (2 * torch.rand(F, ht, wd, generator=g) - 1)), torch.zeros(F, ht, wd))
    return dict(intr=intr, poses=poses0, disps=disps0, target=target.permute(0, 3, 1, 2).contiguous(),
                weight=weight.permute(0, 3, 1, 2).contiguous(), eta=eta, ii=ii.contiguous(), jj=jj.contiguous(), t0=t0, t1=F, sens=sens)


def depth_frames(s):
    """kx: the frames whose depth maps the BA optimises, unique([t0, t1) U ii) - one eta row each"""
    return np.unique(np.concatenate([np.arange(s["t0"], s["t1"]), s["ii"].numpy()]))


def swapped_eta(s, alpha=ALPHA):
    """eta' = where(sens > 0, alpha, eta): what a residual-zero map turns the damping into"""
    import torch
    return torch.where(s["sens"][torch.from_numpy(depth_frames(s))] > 0, torch.full_like(s["eta"], alpha), s["eta"])


def reference(s, iters, sens="own", lm=1e-4, ep=0.1, eta=None):
    n = lambda t: t.numpy()
    return ba(n(s["poses"]), n(s["disps"]), n(s["intr"]), n(s["target"]), n(s["weight"]), n(s["eta"] if eta is None else eta),
              n(s["ii"]), n(s["jj"]), s["t0"], s["t1"], iters, lm, ep, n(s["sens"]) if isinstance(sens, str) else sens)
