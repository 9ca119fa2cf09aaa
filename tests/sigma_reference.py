"""The uncertainty tests' own yardstick: depth and pose (co)variances from the normal equations of one depth-BA Gauss-Newton step, in
numpy fp64.  Neither the reference nor oracle/ computes them, so there is nothing of theirs to record.  The assembled fields come from
oracle.ba_assemble (stereo edges: stereo_reference.stereo_terms) and the rows are built as stereo_reference.gn_step builds them, the
sensor-depth prior and the stereo term included.  Two independent routes:

    (a) schur:  S_d = (A - sum_k M_k Q_k M_k^T) + diag(ep + lm diag(.)),  pose_cov = S_d^-1,
                var_cond = Q,  var_pose = Q^2 m^T S_d^-1 m
    (b) dense:  the full information matrix [[A + D, B], [B^T, diag(C + add)]] over 6P + K HW variables, inverted as a whole;
                its diagonal is var_cond + var_pose and its leading block pose_cov

tests/test_ba_sigma_host.py qualifies both against each other before anything is held to them."""
import numpy as np

import stereo_reference as SR
from oracle import oracle as O

ALPHA = SR.ALPHA
FIELDS = ("Hs", "Eii", "Eij", "Cii")


def assemble(poses, disps, intr, target, weight, ii, jj, baseline=0.0):
    """the step's assembled fields in fp64: Hs [4,E,6,6] (rounded through fp32 as the oracle stores them), Eii / Eij [E,6,HW], Cii [E,HW]"""
    poses, disps = np.ascontiguousarray(poses, np.float32), np.ascontiguousarray(disps, np.float32)
    target, weight = np.ascontiguousarray(target, np.float32), np.ascontiguousarray(weight, np.float32)
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    F, ht, wd = disps.shape
    HW, E = ht * wd, ii.shape[0]
    st = (ii == jj) if baseline > 0 else np.zeros(E, bool)
    o = np.nonzero(~st)[0]
    f = dict(Hs=np.zeros((4, E, 6, 6)), Eii=np.zeros((E, 6, HW)), Eij=np.zeros((E, 6, HW)), Cii=np.zeros((E, HW)))
    if o.size:
        a = O.ba_assemble(poses, disps, intr, np.ascontiguousarray(target[o]), np.ascontiguousarray(weight[o]), ii[o], jj[o])
        f["Hs"][:, o] = a["Hs"].astype(np.float32).astype(np.float64)
        f["Eii"][o], f["Eij"][o] = a["Eii"].astype(np.float64), a["Eij"].astype(np.float64)
        f["Cii"][o] = a["Cii"].astype(np.float64)
    for e in np.nonzero(st)[0]:                                        # stereo edges: a depth term only, zero pose rows
        f["Cii"][e], _ = SR.stereo_terms(disps[ii[e]], intr, target[e], weight[e], baseline)
    return f


def perturbed(f, seed, scale=2.0 ** -20):
    """every entry of the assembled fields times (1 + scale u), u uniform in [-1, 1], independently"""
    g = np.random.default_rng(seed)
    return {k: f[k] * (1.0 + scale * g.uniform(-1.0, 1.0, f[k].shape)) for k in FIELDS}


def system(f, eta, ii, jj, t0, t1, F, HW, sens=None, alpha=ALPHA):
    """-> A [6P,6P] (the pose blocks before the elimination), Q [K,HW], B [6P, K, HW] (column (k, x): the pixel's live rows at their
    poses), kx.  The rows as in stereo_reference.gn_step."""
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    E, P = ii.shape[0], t1 - t0
    n6 = 6 * P
    Hs, Eii, Eij, Cii = (f[k] for k in FIELDS)
    A = np.zeros((n6, n6))
    blk = lambda p: slice(6 * p, 6 * p + 6)
    for e in range(E):
        pi, pj = int(ii[e]) - t0, int(jj[e]) - t0
        iok, jok = 0 <= pi < P, 0 <= pj < P
        if iok:
            A[blk(pi), blk(pi)] += Hs[0, e]
        if jok:
            A[blk(pj), blk(pj)] += Hs[3, e]
        if iok and jok:
            A[blk(pi), blk(pj)] += Hs[1, e]; A[blk(pj), blk(pi)] += Hs[2, e]
    kx = np.unique(np.concatenate([np.arange(t0, t1, dtype=np.int64), ii]))
    K = kx.shape[0]
    kidx = {int(fr): k for k, fr in enumerate(kx)}
    C, deg = np.zeros((K, HW)), np.zeros(K, np.int64)
    Ei = np.zeros((P, 6, HW))
    for e in range(E):
        k = kidx[int(ii[e])]
        C[k] += Cii[e]; deg[k] += 1
        if 0 <= int(ii[e]) - t0 < P:
            Ei[int(ii[e]) - t0] += Eii[e]
    eta = np.asarray(eta, np.float64).reshape(-1, HW)
    add = np.broadcast_to(eta, (K, HW)).copy() if eta.shape[0] == 1 else eta.copy()
    assert add.shape == (K, HW)
    if sens is not None:
        s = np.asarray(sens, np.float64).reshape(F, HW)[kx]
        add = np.where((s > 0) & (deg > 0)[:, None], alpha, add)
    Q = 1.0 / (C + add)
    B = np.zeros((n6, K, HW))
    for p in range(P):
        B[blk(p), kidx[t0 + p]] += Ei[p]
    for e in range(E):
        p = int(jj[e]) - t0
        if 0 <= p < P:
            B[blk(p), kidx[int(ii[e])]] += Eij[e]
    return A, Q, B, kx


def schur(f, eta, ii, jj, t0, t1, F, HW, lm, ep, sens=None, alpha=ALPHA):
    """route (a) -> dict(pose_cov [6P,6P], var_cond [K,HW], var_pose [K,HW], kx, S_d)"""
    A, Q, B, kx = system(f, eta, ii, jj, t0, t1, F, HW, sens, alpha)
    n6 = A.shape[0]
    S = A - np.einsum("akx,kx,bkx->ab", B, Q, B)
    S_d = S + np.diag(ep + lm * np.diag(S))
    if n6:
        np.linalg.cholesky(S_d)                                        # (raises when the damped system is not positive definite)
        cov = np.linalg.inv(S_d)
        cov = 0.5 * (cov + cov.T)
    else:
        cov = np.zeros((0, 0))
    var_pose = Q * Q * np.einsum("akx,ab,bkx->kx", B, cov, B) if n6 else np.zeros_like(Q)
    return dict(pose_cov=cov, var_cond=Q, var_pose=var_pose, kx=kx, S_d=S_d)


def full_information(f, eta, ii, jj, t0, t1, F, HW, lm, ep, sens=None, alpha=ALPHA):
    """the full damped information matrix over [6P poses | K HW depths] and kx"""
    A, Q, B, kx = system(f, eta, ii, jj, t0, t1, F, HW, sens, alpha)
    n6, nz = A.shape[0], Q.size
    S = A - np.einsum("akx,kx,bkx->ab", B, Q, B)
    H = np.zeros((n6 + nz, n6 + nz))
    H[:n6, :n6] = A + np.diag(ep + lm * np.diag(S))
    H[:n6, n6:] = B.reshape(n6, nz)
    H[n6:, :n6] = B.reshape(n6, nz).T
    H[np.arange(n6, n6 + nz), np.arange(n6, n6 + nz)] = 1.0 / Q.reshape(-1)
    return H, kx


def dense(f, eta, ii, jj, t0, t1, F, HW, lm, ep, sens=None, alpha=ALPHA):
    """route (b) -> dict(pose_cov, var_total [K,HW], kx)"""
    H, kx = full_information(f, eta, ii, jj, t0, t1, F, HW, lm, ep, sens, alpha)
    n6 = 6 * (t1 - t0)
    Hi = np.linalg.inv(H)
    return dict(pose_cov=Hi[:n6, :n6], var_total=np.diag(Hi)[n6:].reshape(len(kx), HW), kx=kx)


def scene_fields(s, baseline=0.0):
    """assemble() on a scene dict of rgbd_reference.window / stereo_reference.window (torch tensors)"""
    n = lambda t: t.numpy()
    return assemble(n(s["poses"]), n(s["disps"]), n(s["intr"]), n(s["target"]), n(s["weight"]), n(s["ii"]), n(s["jj"]), baseline)


def scene_schur(s, f=None, lm=1e-4, ep=0.1, baseline=0.0, sens=None):
    F, ht, wd = s["disps"].shape
    f = scene_fields(s, baseline) if f is None else f
    return schur(f, s["eta"].numpy(), s["ii"].numpy(), s["jj"].numpy(), s["t0"], s["t1"], F, ht * wd, lm, ep, sens)


def scene_dense(s, f=None, lm=1e-4, ep=0.1, baseline=0.0, sens=None):
    F, ht, wd = s["disps"].shape
    f = scene_fields(s, baseline) if f is None else f
    return dense(f, s["eta"].numpy(), s["ii"].numpy(), s["jj"].numpy(), s["t0"], s["t1"], F, ht * wd, lm, ep, sens)


def relmax(a, b, floor=0.0):
    """largest max(|a - b| - floor, 0) / |b| over the entries where b != 0; where b == 0, a may differ by at most `floor`"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = np.abs(a - b)
    nz = np.abs(b) > 0
    assert np.all(d[~nz] <= floor), float(d[~nz].max())
    return float((np.maximum(d[nz] - floor, 0.0) / np.abs(b[nz])).max()) if nz.any() else 0.0


def within(a, b, rel, floor=0.0):
    """|a - b| <= rel |b| + floor everywhere -> (ok, the largest (|a - b| - floor) / |b| over b != 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d, nz = np.abs(a - b), np.abs(b) > 0
    worst = float((np.maximum(d[nz] - floor, 0.0) / np.abs(b[nz])).max()) if nz.any() else 0.0
    return bool(np.all(d <= rel * np.abs(b) + floor)), worst


def sensitivity(s, base, lm=1e-4, ep=0.1, baseline=0.0, sens=None, seeds=(0, 1, 2, 3), f=None):
    """s_case: the largest relative change of var_pose, var_cond and diag(pose_cov) - each separately - under four seeded relative
    perturbations of 2^-20 of the assembled fields (the 1e-6 to which the device's assembled sums are held)"""
    f = scene_fields(s, baseline) if f is None else f
    out = dict(var_pose=0.0, var_cond=0.0, cov_diag=0.0)
    for seed in seeds:
        r = scene_schur(s, perturbed(f, seed), lm, ep, baseline, sens)
        out["var_pose"] = max(out["var_pose"], relmax(r["var_pose"], base["var_pose"]))      # (an exact 0 stays an exact 0)
        out["var_cond"] = max(out["var_cond"], relmax(r["var_cond"], base["var_cond"]))
        out["cov_diag"] = max(out["cov_diag"], relmax(np.diag(r["pose_cov"]), np.diag(base["pose_cov"])))
    return out
