"""The calibration tests' own yardstick: one Gauss-Newton step of the dense bundle adjustment with the four intrinsics
c = (fx, fy, cx, cy) as a border of the reduced pose system (include/pvo_hip.h, pvo_ba_calib), in numpy fp64.

`step` is rgbd_reference.gn_step's arithmetic line for line - pose blocks, Schur rows [Ei; Eij] by depth frame, diag += ep + lm diag,
Cholesky, dz without the rows of window pose 0 - plus the border

    Hcc += w Jc^T Jc,  Hc[i] += w Ji^T Jc,  Hc[j] += w Jj^T Jc,  vc += w r Jc^T,  gc[e] = w Jz Jc^T,  Gc_k = sum of gc over k's out-edges
    Sc = Hc - sum M Q Gc^T,   Scc = Hcc - sum Q Gc Gc^T,   rc = vc - sum Q w' Gc
    T = Scc + diag(ep_c + lm diag(Scc)) - Sc^T S_d^-1 Sc  on the free parameters,  dc = T^-1 (rc - Sc^T dx0),  dx = dx0 - S_d^-1 Sc dc

so that free_mask = 0 IS gn_step.  The assembled fields come from `fields`: the pose and depth fields either from the oracle's
projective_transform restatement (fp32 pixel arithmetic, what the device is held to) or, like the border always, from the closed-form
fp64 Jacobians of `pixel_jacobians` (tests/test_ba_calib_host.py checks those against autograd and the whole route against the full
normal equations)."""
import numpy as np

from oracle import oracle as O

MIN_DEPTH = 0.25
FIELDS = ("Hs", "vs", "Eii", "Eij", "Cii", "bz", "Hci", "Hcj", "Hcc", "vc", "gc")


def _rot(q):
    """rotation matrix of the (unit) quaternion (x, y, z, w): I + 2 w K + 2 K^2"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rel_pose(pi, pj):
    """G_ij = G_j G_i^-1 of two stored poses (t, xyzw quaternion) -> (R, t) in fp64"""
    pi, pj = np.asarray(pi, np.float64), np.asarray(pj, np.float64)
    ax, ay, az, aw = pj[3:]
    bx, by, bz, bw = -pi[3], -pi[4], -pi[5], pi[6]
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                  aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])
    R = _rot(q)
    return R, pj[:3] - R @ pi[:3]


def pixel_jacobians(poses, disps, intr, target, weight, ii, jj):
    """per edge, residual row (u, v) and pixel, in fp64 from the stored fp32 operands:
    Ji, Jj [E,2,6,HW], Jz [E,2,HW], Jc [E,2,4,HW], r [E,2,HW], w [E,2,HW] (0.001 * weight formed in double, rounded to float; 0 where
    Z < MIN_DEPTH) and proj [E,2,HW].  Tangent order (tau, phi), left perturbation, as the assembly's.  (fp64 operands are taken as
    they are: the host tests pass quaternions normalised in fp64, for which the closed forms are exact.)"""
    poses, disps = np.asarray(poses, np.float64), np.asarray(disps, np.float64)      # (fp32 operands widen exactly)
    fx, fy, cx, cy = (float(v) for v in np.asarray(intr, np.float64))
    F, ht, wd = disps.shape
    HW, E = ht * wd, len(ii)
    v_, u_ = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
    u_, v_ = u_.reshape(-1), v_.reshape(-1)
    px, py = (u_ - cx) / fx, (v_ - cy) / fy
    Ji, Jj = np.zeros((E, 2, 6, HW)), np.zeros((E, 2, 6, HW))
    Jz, Jc = np.zeros((E, 2, HW)), np.zeros((E, 2, 4, HW))
    r, w, proj = np.zeros((E, 2, HW)), np.zeros((E, 2, HW)), np.zeros((E, 2, HW))
    tg = np.asarray(target, np.float32).reshape(E, 2, HW).astype(np.float64)
    wg = np.asarray(weight, np.float32).reshape(E, 2, HW)
    for e in range(E):
        i, j = int(ii[e]), int(jj[e])
        R, t = rel_pose(poses[i], poses[j])
        h = disps[i].reshape(-1).astype(np.float64)
        X = R[0, 0] * px + R[0, 1] * py + R[0, 2] + h * t[0]
        Y = R[1, 0] * px + R[1, 1] * py + R[1, 2] + h * t[1]
        Z = R[2, 0] * px + R[2, 1] * py + R[2, 2] + h * t[2]
        ok = ~(Z < MIN_DEPTH)
        d = np.where(ok, 1.0 / np.where(ok, Z, 1.0), 0.0)
        d2 = d * d
        w[e] = np.where(ok, (0.001 * wg[e].astype(np.float64)).astype(np.float32).astype(np.float64), 0.0)
        proj[e, 0], proj[e, 1] = fx * d * X + cx, fy * d * Y + cy
        r[e] = tg[e] - proj[e]
        z = np.zeros(HW)
        Jj[e, 0] = fx * np.stack([h * d, z, -X * h * d2, -X * Y * d2, 1.0 + X * X * d2, -Y * d])
        Jj[e, 1] = fy * np.stack([z, h * d, -Y * h * d2, -1.0 - Y * Y * d2, X * Y * d2, X * d])
        Jz[e, 0] = fx * (t[0] * d - t[2] * (X * d2))
        Jz[e, 1] = fy * (t[1] * d - t[2] * (Y * d2))
        for c in range(2):                                                     # Ji = -adjT(G_ij) Jj
            a, b = R.T @ Jj[e, c, :3], R.T @ Jj[e, c, 3:]
            tau = Jj[e, c, :3]
            uu = np.stack([t[2] * tau[1] - t[1] * tau[2], t[0] * tau[2] - t[2] * tau[0], t[1] * tau[0] - t[0] * tau[1]])
            Ji[e, c] = -np.concatenate([a, b + R.T @ uu])
        a0, a1 = fx * (d * R[0, 0] - X * d2 * R[2, 0]), fx * (d * R[0, 1] - X * d2 * R[2, 1])
        b0, b1 = fy * (d * R[1, 0] - Y * d2 * R[2, 0]), fy * (d * R[1, 1] - Y * d2 * R[2, 1])
        Jc[e, 0] = np.stack([X * d - a0 * px / fx, -a1 * py / fy, 1.0 - a0 / fx, -a1 / fy])
        Jc[e, 1] = np.stack([-b0 * px / fx, Y * d - b1 * py / fy, -b0 / fx, 1.0 - b1 / fy])
    return dict(Ji=Ji, Jj=Jj, Jz=Jz, Jc=Jc, r=r, w=w, proj=proj)


def fields(poses, disps, intr, target, weight, ii, jj, assembly="oracle"):
    """the step's assembled fields.  Hs [4,E,6,6] (ii, ij, ji, jj), vs [2,E,6], Eii, Eij [E,6,HW], Cii, bz [E,HW] as oracle.ba_assemble's
    (assembly="oracle": from it, Hs / vs rounded to fp32 as rgbd_reference.gn_step does; "fp64": from pixel_jacobians), and the border
    Hci, Hcj [E,6,4], Hcc [E,4,4], vc [E,4], gc [E,4,HW] from pixel_jacobians always."""
    J = pixel_jacobians(poses, disps, intr, target, weight, ii, jj)
    w, r = J["w"], J["r"]
    es = lambda spec, *ops: np.einsum(spec, *ops, optimize=True)
    f = dict(Hci=es("ecx,ecax,ecnx->ean", w, J["Ji"], J["Jc"]), Hcj=es("ecx,ecax,ecnx->ean", w, J["Jj"], J["Jc"]),
             Hcc=es("ecx,ecnx,ecmx->enm", w, J["Jc"], J["Jc"]), vc=es("ecx,ecx,ecnx->en", w, r, J["Jc"]),
             gc=es("ecx,ecx,ecnx->enx", w, J["Jz"], J["Jc"]))
    if assembly == "oracle":
        a = O.ba_assemble(np.ascontiguousarray(poses, np.float32), np.ascontiguousarray(disps, np.float32), intr, target, weight,
                          np.asarray(ii, np.int64), np.asarray(jj, np.int64))
        f.update(Hs=a["Hs"].astype(np.float32).astype(np.float64), vs=a["vs"].astype(np.float32).astype(np.float64),
                 Eii=a["Eii"].astype(np.float64), Eij=a["Eij"].astype(np.float64), Cii=a["Cii"].astype(np.float64), bz=a["bz"].astype(np.float64))
    else:
        Ji, Jj, Jz = J["Ji"], J["Jj"], J["Jz"]
        f.update(Hs=np.stack([es("ecx,ecax,ecbx->eab", w, A, B) for A, B in ((Ji, Ji), (Ji, Jj), (Jj, Ji), (Jj, Jj))]),
                 vs=np.stack([es("ecx,ecx,ecax->ea", w, r, A) for A in (Ji, Jj)]),
                 Eii=es("ecx,ecx,ecax->eax", w, Jz, Ji), Eij=es("ecx,ecx,ecax->eax", w, Jz, Jj),
                 Cii=es("ecx,ecx,ecx->ex", w, Jz, Jz), bz=es("ecx,ecx,ecx->ex", w, r, Jz))
    return f


def perturbed(f, seed, scale=2.0 ** -20):
    """every entry of the assembled fields times (1 + scale u), u uniform in [-1, 1], independently"""
    g = np.random.default_rng(seed)
    return {k: f[k] * (1.0 + scale * g.uniform(-1.0, 1.0, f[k].shape)) for k in FIELDS}


def prior_terms(add, w, disps, kx, deg, sens, alpha, factor=None):
    """the sensor-depth prior of include/pvo_hip.h (pvo_ba_depth_prior) on a step's depth terms: with s = sens[kx], d = disps[kx] and
    m = (s > 0) & (the frame has an out-edge), add = where(m, alpha, add) and w = w - where(m, alpha (d - s), 0) -> (add, w).
    factor [K,HW]: the addend alpha (d - s) times it (the perturbation of tests/ba_rider_reference.sensitivity)"""
    F = disps.shape[0]
    s = np.asarray(sens, np.float64).reshape(F, -1)[kx]
    d = np.asarray(disps, np.float64).reshape(F, -1)[kx]
    with np.errstate(invalid="ignore"):
        m = (s > 0) & (np.asarray(deg) > 0)[:, None]
        r = alpha * (d - s)
    if factor is not None:
        r = r * factor
    return np.where(m, alpha, add), w - np.where(m, r, 0.0)


ALPHA = 0.05      # rgbd_reference.ALPHA, the default of pvo_ba_prior's callers


def step(f, poses, disps, intr, eta, ii, jj, t0, t1, lm, ep, ep_c=0.1, free_mask=15, sens=None, alpha=ALPHA, prior_factor=None):
    """one step from the assembled fields `f` -> dict(poses, disps, intr [fp32], dx [P,6], dc [4], dz [K,HW], kx, rejected,
    S_diag, Scc_diag [the undamped diagonals the damping read], reason); inputs are not modified.  A rejected step returns the inputs'
    values and zeros; reason names the test that rejected it ("pose system", "complement", "non-finite", "focal"), None = accepted.
    sens [F,ht,wd] (optional): the sensor-depth prior with weight alpha (prior_terms); None is the step without it, bit for bit."""
    poses, disps = np.ascontiguousarray(poses, np.float32), np.ascontiguousarray(disps, np.float32)
    intr = np.ascontiguousarray(intr, np.float32)
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    F, ht, wd = disps.shape
    HW, E, P = ht * wd, ii.shape[0], t1 - t0
    n6 = 6 * P
    Hs, vs, Eii, Eij, Cii, bz = (f[k] for k in FIELDS[:6])
    A, b = np.zeros((n6, n6)), np.zeros(n6)
    Sc, Scc, rc = np.zeros((n6, 4)), np.zeros((4, 4)), np.zeros(4)
    blk = lambda p: slice(6 * p, 6 * p + 6)
    for e in range(E):
        pi, pj = int(ii[e]) - t0, int(jj[e]) - t0
        iok, jok = 0 <= pi < P, 0 <= pj < P
        if iok:
            A[blk(pi), blk(pi)] += Hs[0, e]; b[blk(pi)] += vs[0, e]; Sc[blk(pi)] += f["Hci"][e]
        if jok:
            A[blk(pj), blk(pj)] += Hs[3, e]; b[blk(pj)] += vs[1, e]; Sc[blk(pj)] += f["Hcj"][e]
        if iok and jok:
            A[blk(pi), blk(pj)] += Hs[1, e]; A[blk(pj), blk(pi)] += Hs[2, e]
        Scc += f["Hcc"][e]; rc += f["vc"][e]
    kx = np.unique(np.concatenate([np.arange(t0, t1, dtype=np.int64), ii]))
    K = kx.shape[0]
    kidx = {int(fr): k for k, fr in enumerate(kx)}
    C, w = np.zeros((K, HW)), np.zeros((K, HW))
    Ei, Gc = np.zeros((P, 6, HW)), np.zeros((K, 4, HW))
    for e in range(E):
        k = kidx[int(ii[e])]
        C[k] += Cii[e]; w[k] += bz[e]; Gc[k] += f["gc"][e]
        if 0 <= int(ii[e]) - t0 < P:
            Ei[int(ii[e]) - t0] += Eii[e]
    eta = np.asarray(eta, np.float64).reshape(-1, HW)
    add = np.broadcast_to(eta, (K, HW)).copy() if eta.shape[0] == 1 else eta.copy()
    assert add.shape == (K, HW)
    if sens is not None:
        add, w = prior_terms(add, w, disps, kx, np.bincount(ii, minlength=F)[kx], sens, alpha, prior_factor)
    Q = 1.0 / (C + add)
    rows = [[] for _ in range(K)]
    for p in range(P):
        rows[kidx[t0 + p]].append((p, Ei[p]))
    for e in range(E):
        rows[kidx[int(ii[e])]].append((int(jj[e]) - t0, Eij[e]))
    for k in range(K):
        Scc -= (Gc[k] * Q[k]) @ Gc[k].T
        rc -= Gc[k] @ (Q[k] * w[k])
        live = [(p, M) for p, M in rows[k] if 0 <= p < P]
        if not live:
            continue
        M = np.concatenate([m_ for _, m_ in live], 0)                  # [6r, HW]
        S = (M * Q[k]) @ M.T
        v = M @ (Q[k] * w[k])
        G = (M * Q[k]) @ Gc[k].T                                        # [6r, 4]
        for x, (pa, _) in enumerate(live):
            b[blk(pa)] -= v[6 * x:6 * x + 6]
            Sc[blk(pa)] -= G[6 * x:6 * x + 6]
            for y, (pb, _) in enumerate(live):
                A[blk(pa), blk(pb)] -= S[6 * x:6 * x + 6, 6 * y:6 * y + 6]
    S_diag, Scc_diag = np.diag(A).copy(), np.diag(Scc).copy()
    rejected = lambda why: dict(reason=why, poses=poses.copy(), disps=disps.copy(), intr=intr.copy(), dx=np.zeros((P, 6)), dc=np.zeros(4), dz=np.zeros((K, HW)),
                    kx=kx, rejected=True, S_diag=S_diag, Scc_diag=Scc_diag)
    A[np.diag_indices(n6)] += ep + lm * np.diag(A)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return rejected("pose system")
    solve = lambda rhs: np.linalg.solve(L.T, np.linalg.solve(L, rhs))
    dx = solve(b)
    dc = np.zeros(4)
    free = [n for n in range(4) if (free_mask >> n) & 1]
    if free:
        Sf = Sc[:, free]
        Y = solve(Sf)
        T = Scc[np.ix_(free, free)] + np.diag(ep_c + lm * Scc_diag[free]) - Sf.T @ Y
        T = 0.5 * (T + T.T)
        try:
            Lc = np.linalg.cholesky(T)
        except np.linalg.LinAlgError:
            return rejected("complement")
        dcf = np.linalg.solve(Lc.T, np.linalg.solve(Lc, rc[free] - Sf.T @ dx))
        dc[free] = dcf
        dx = dx - Y @ dcf
    dx = dx.reshape(P, 6)
    intr_out = intr.copy()
    intr_out[free] = (intr[free] + dc[free].astype(np.float32)).astype(np.float32)
    if not (np.isfinite(dx).all() and np.isfinite(dc).all()):
        return rejected("non-finite")
    if not (intr_out[0] > 0 and intr_out[1] > 0):
        return rejected("focal")
    acc = np.zeros((K, HW))
    for k in range(K):
        for p, M in rows[k]:
            if 1 <= p < P:
                acc[k] += dx[p] @ M
        acc[k] += dc @ Gc[k]
    dz = Q * (w - acc)
    poses_out = O.pose_retr(poses, dx.astype(np.float32), t0, t1)
    disps_out = disps.astype(np.float64).reshape(F, HW).copy()
    disps_out[kx] += dz
    return dict(poses=poses_out, disps=disps_out.reshape(F, ht, wd).astype(np.float32), intr=intr_out, dx=dx, dc=dc, dz=dz, kx=kx,
                rejected=False, reason=None, S_diag=S_diag, Scc_diag=Scc_diag)


def gn_step_calib(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, lm, ep, ep_c=0.1, free_mask=15, assembly="oracle"):
    """rgbd_reference.gn_step (no sensor map) with the intrinsics' border -> step's dict"""
    f = fields(poses, disps, intr, target, weight, ii, jj, assembly)
    return step(f, poses, disps, intr, eta, ii, jj, t0, t1, lm, ep, ep_c, free_mask)


def ba_calib(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, iters, lm, ep, ep_c=0.1, free_mask=15, perturb_seed=None, assembly="oracle"):
    """`iters` steps; poses, disps and intrinsics pass through fp32 between steps, as the device's do -> the last step's dict.
    perturb_seed: every step's assembled fields are `perturbed` (seed + step index) - the sensitivity of a chain of steps.
    assembly: `fields`' (the default is the oracle's fp32 pixel arithmetic; "fp64" with free_mask = 0 is a chain of plain fp64 steps)"""
    out = None
    for it in range(iters):
        f = fields(poses, disps, intr, target, weight, ii, jj, assembly)
        if perturb_seed is not None:
            f = perturbed(f, perturb_seed + it)
        out = step(f, poses, disps, intr, eta, ii, jj, t0, t1, lm, ep, ep_c, free_mask)
        poses, disps, intr = out["poses"], out["disps"], out["intr"]
    return out


def scene_args(s):
    """rgbd_reference.window's dict -> the positional operands of gn_step_calib / fields (numpy)"""
    n = lambda t: t.numpy()
    return (n(s["poses"]), n(s["disps"]), n(s["intr"]), n(s["target"]), n(s["weight"]), n(s["eta"]), n(s["ii"]), n(s["jj"]), s["t0"], s["t1"])


def scene_step(s, lm, ep, ep_c=0.1, free_mask=15, f=None):
    a = scene_args(s)
    f = fields(a[0], a[1], a[2], a[3], a[4], a[6], a[7]) if f is None else f
    return step(f, a[0], a[1], a[2], a[5], a[6], a[7], a[8], a[9], lm, ep, ep_c, free_mask)


GENERAL_XI = (0.05, 0.02, 0.02, 0.012, 0.01, 0.015)


def window_general(seed, F, ht, wd, radius=2, t0=1, xi=GENERAL_XI):
    """rgbd_reference.window's recipe with a GENERAL motion between frames - rotation about all three axes and a y translation, where
    that recipe has translation in x, z and rotation about y only (which makes half the entries of G_ij and the whole fy column of Jc
    exact zeros).  Same dict, without the sensor map."""
    import torch
    import rgbd_reference as R
    from pvo_amd.geom.se3 import SE3
    g = torch.Generator().manual_seed(seed)
    intr = torch.tensor([wd * 0.625, wd * 0.7, wd / 2.0 - 0.3, ht / 2.0 + 0.4])
    xi = torch.tensor(xi)
    poses_gt = torch.stack([SE3.exp(k * xi).data for k in range(F)], 0)
    low = torch.rand(1, 1, 6, 8, generator=g) * 0.8 + 0.2
    disps_gt = torch.nn.functional.interpolate(low, size=(ht, wd), mode="bilinear", align_corners=True)[0, 0][None].repeat(F, 1, 1)
    ii, jj = (torch.as_tensor(v) for v in R.radius_graph(F, radius))
    E = ii.shape[0]
    c, _ = O.reproject(poses_gt.numpy(), disps_gt.numpy(), intr[None].repeat(F, 1).numpy(), ii.numpy(), jj.numpy())
    target = torch.from_numpy(c) + 0.1 * torch.randn(E, ht, wd, 2, generator=g)
    weight = torch.rand(E, ht, wd, 2, generator=g) + 0.5
    poses0 = torch.stack([poses_gt[max(k - 1, 0)] for k in range(F)], 0)
    disps0 = torch.ones(F, ht, wd) + 0.2 * torch.rand(F, ht, wd, generator=g)
    K = int(np.unique(np.concatenate([np.arange(t0, F), ii.numpy()])).shape[0])
    eta = torch.full((K, ht, wd), 1e-4) + 0.01 * torch.rand(K, ht, wd, generator=g)
    return dict(intr=intr, poses=poses0, disps=disps0, target=target.permute(0, 3, 1, 2).contiguous(),
                weight=weight.permute(0, 3, 1, 2).contiguous(), eta=eta, ii=ii.contiguous(), jj=jj.contiguous(), t0=t0, t1=F)


# How two results are compared.  dc: PER COMPONENT - its four scalars differ by orders of magnitude.  dx: per POSE (a 6-vector), dz: per
# DEPTH FRAME (a map) - inside such a block the entries change sign and cross 0, so the block is held on its own largest entry.
# Absolute floors, for the units that are 0 or nearly 0:
#   dc[n]   2^-24 |c[n]|: half a unit in the last place of the fp32 parameter the step adds it to (c += dc in fp32) - a difference
#           below it cannot change the calibrated vector.  (dfy is ~1e-18 under a motion that does not observe fy.)
#   dx, dz  2^-20 of the quantity's largest magnitude: the relative size of the perturbation that defines s_case, and what the device's
#           assembled sums are held to - a pose or a depth map that barely moves cannot be resolved below that fraction of the scale.
FLOOR = 2.0 ** -20


def units(name, v):
    """the quantity as [units, entries]: dc [4,1], dx [P,6], dz [K,HW]"""
    v = np.asarray(v, np.float64)
    return v.reshape(4, 1) if name == "dc" else v.reshape(v.shape[0], -1)


def floors(name, b, intr):
    """the absolute floor of every unit of the yardstick's quantity b (see above)"""
    b = units(name, b)
    if name == "dc":
        return 2.0 ** -24 * np.abs(np.asarray(intr, np.float64).reshape(4))
    return np.full(b.shape[0], FLOOR * (float(np.abs(b).max()) if b.size else 0.0))


def _unit_errors(name, a, b, intr):
    a, b = units(name, a), units(name, b)
    return np.abs(a - b).max(1), np.abs(b).max(1), floors(name, b, intr)


def relchange(name, a, b, intr):
    """the largest relative change over the quantity's units: max(max|a_u - b_u| - floor_u, 0) / max|b_u| over the units with b_u != 0;
    a unit with b_u == 0 must agree within its floor"""
    d, m, fl = _unit_errors(name, a, b, intr)
    assert np.all(d[m == 0] <= fl[m == 0])
    nz = m > 0
    return float((np.maximum(d[nz] - fl[nz], 0.0) / m[nz]).max()) if nz.any() else 0.0


def within(name, a, b, rel, intr):
    """every unit: max|a_u - b_u| <= rel max|b_u| + floor_u -> (ok, relchange); a non-finite entry of `a` fails"""
    if not np.isfinite(np.asarray(a, np.float64)).all():
        return False, float("inf")
    d, m, fl = _unit_errors(name, a, b, intr)
    nz = m > 0
    return bool(np.all(d <= rel * m + fl)), (float((np.maximum(d[nz] - fl[nz], 0.0) / m[nz]).max()) if nz.any() else 0.0)


def sensitivity(s, base, f, lm, ep, ep_c=0.1, free_mask=15, seeds=(0, 1, 2, 3)):
    """s_case: the largest relative change (relchange) of dx, of dc and of dz - each separately - under four seeded relative
    perturbations of 2^-20 of the assembled fields, the border's included"""
    out, intr = dict(dx=0.0, dc=0.0, dz=0.0), s["intr"].numpy()
    for seed in seeds:
        r = scene_step(s, lm, ep, ep_c, free_mask, perturbed(f, seed))
        for k in out:
            out[k] = max(out[k], relchange(k, r[k], base[k], intr))
    return out
