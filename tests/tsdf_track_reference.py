"""The frame-to-model tracker's yardstick (tests/test_tsdf_track_host.py, tests/test_tsdf_track_gpu.py): the contract of pvo_tsdf_track
(include/pvo_hip.h) restated in numpy.  Geometry, interpolation, sums, the solve and the retraction are evaluated in fp64 on the fp32
inputs; what the contract stores in fp32 is stored in fp32 here as well (the step xi and the pose between evaluations), and
wsum >= min_weight is compared in fp32.

The scene.  tsdf_reference.scene (a plane and one sphere) is RANK-DEFICIENT for this problem: a rotation about the axis through the
sphere's centre along the plane's normal leaves both surfaces in place (H at the true pose has condition number 1.5e3 and starts 0.5
degrees off drift to 2.9 degrees).  This module adds a second sphere, centre (-0.45, -0.3, 1.6), radius 0.25, to the same cameras and
plane; test_tsdf_track_host.py prints the condition number it gets (87 in the prototype) and asserts what the tests rely on.

Error bound of the kernel (pvo_amd/csrc/tsdf_track.hip on tsdf_ray.h: fp32, every multiply-add one fma; EPS = 2^-24, first order).
E_S and the roundings of g and p are counted as in tests/tsdf_render_reference.py, with z = 1 / d (a correctly rounded division: the one
rounding K_RAY already counts for z_k); two of its terms are taken at their own magnitude instead of an upper bound of it, because the
tracker's sums add the pixels' errors up:
  g_i    10 EPS sum_j |M_ij| |r_j|  (r = (rx, ry, 1); the render's bound has (|rx| + |ry| + 1) / voxel in place of the sum)
  p0_i = (c_i - o_i) / voxel:  c's 8 EPS |t|_1, the difference EPS (|t|_1 + |o_i|), the division EPS |p0_i|
  p_i    E_p = EPS (K_RAY z sum_j |M_ij| |r_j| + (K_C |t|_1 + |o_i|) / voxel + |p0_i| + |p_i|),  K_RAY = 12, K_C = 9
  S      E_S = K_TRI EPS + sum_i |grad_i| E_p_i
  grad_i E_grad_i = K_GRAD EPS + sum_{j != i} c_ij E_p_j,  c_ij >= |d grad_i / d f_j|: the larger of the two mixed second differences of the
         corner values that d grad_i / d f_j interpolates (the render's bound puts 4, their largest possible value, in their place)
  gc_i = fma(M_0i, grad_0, fma(M_1i, grad_1, M_2i grad_2)):  M's 6 EPS / voxel, a product and two fma roundings of magnitude
         <= sum_j |M_ji grad_j|, second order:   E_gc_i = sum_j |M_ji| E_grad_j + K_GC EPS sum_j |M_ji| |grad_j|,  K_GC = 10
  Xc     rx's 2, z's 1, the product:             E_X_i = K_X EPS |X_i|,  K_X = 4
  (Xc x gc)_i = fma(X_a, gc_b, -(X_b gc_a)):     E = |X_a| E_gc_b + |gc_b| E_X_a + |X_b| E_gc_a + |gc_a| E_X_b + 2 EPS (|X_a gc_b| + |X_b gc_a|)
  k = huber / a beyond the threshold:            E_k = k (E_S / a + 2 EPS)
  a term w k J_i J_j (w k, (w k) J_i, the product: K_TERM = 4 with second order):
         E_term = w k (|J_i| E_J_j + |J_j| E_J_i) + w E_k |J_i J_j| + K_TERM EPS |term|;  likewise w k S J_i and w rho
  the sums: a fixed tree of TREE_DEPTH = 8 fp32 levels (six in the wave, two across the waves), then fp64:  TREE_DEPTH EPS sum |terms|
  the step: |d xi| <= |A^-1| (E_b + E_H |xi|) with the ABSOLUTE VALUES of the entries (the componentwise form of |H^-1| (E_b + E_H |xi|)),
         + EPS |xi| (its rounding to fp32); the fp64 factorisation adds nothing visible
  the retraction (csrc/se3.h in fp32): fewer than K_RETR = 32 roundings on any path from (xi, G) to a component of the new pose, each on a
         magnitude <= 1 + |t|_1 + |xi|_1, sinf / cosf within 2 ulp:   K_RETR EPS (1 + |t|_1 + |xi|_1)
Over several iterations the two trackers' poses drift apart by at most the SUM of the steps' own bounds: a pose error that enters an
evaluation leaves it multiplied by I - A^-1 H, which inside the basin of convergence (where the host test shows every start to end at
one pose) is a contraction.  Once both have converged the distance is also bounded at the fixed point itself: both poses are zeros of
their own b, which differ by at most E_b, so |d G| <= |A^-1| (E_b + E_H |xi|) of the LAST evaluation, plus what the two last steps still
moved (2 sqrt(6) max|xi| of the last step taken).  pose_bound is the smaller of the two.  Per-pixel outputs are compared only where no
step was taken (the two trackers then evaluate the same fp32 pose).

Decisions.  A pixel is FLAGGED when a decision is within rounding of flipping: a component of p within E_p of an integer (the cell, and
with it the gradient and possibly validity, changes at a cell face) or of a face of the box; ||S| - band| <= E_S; ||S| - huber| <= E_S.
Flagged pixels are left out of the per-pixel comparison; in the bounds of H, b and E they count with their full possible contribution:
the magnitude of their term as evaluated plus that of the alternative (the same pixel evaluated across the cell face, or with the band
ignored).  They must stay below 1 % (test_tsdf_track_host.py asserts it on this reference alone)."""
import numpy as np

import tsdf_reference as R
import tsdf_render_reference as V

EPS = R.EPS
K_RAY, K_TRI, K_GRAD = V.K_RAY, V.K_TRI, V.K_GRAD
K_C, K_GC, K_X, K_TERM, K_RETR, TREE_DEPTH = 9, 10, 4, 4, 32, 8
MUTANTS = ("nearest", "unrotated", "right_retraction", "no_band")

SPHERE2_C = np.array([-0.45, -0.3, 1.6])
SPHERE2_R = 0.25
# the volume every test tracks against: tsdf_reference's "5x24x32" world, fused from this module's scene
NFRAMES, FUSE_SIZE = 5, (24, 32)
DIMS, ORIGIN, VOXEL, TRUNC = (24, 28, 40), (-1.013, -0.717, 0.953), 0.05, 0.15
SIZES = ((24, 32), (9, 12), (13, 19))            # three workgroups; tails in both directions
PARAMS = dict(iters=10, band=0.9, huber=0.0, lm=1e-4, ep=1e-6, min_count=32, min_weight=1.0)


# ------------------------------------------------------------------------------------------------------------ scene
def analytic_depth(pose, intr, ht, wd):
    """depth along the optical axis [ht,wd] of the plane and the two spheres seen from `pose` (world-to-camera), fp64; inf = nothing"""
    fx, fy, cx, cy = [np.float64(v) for v in np.asarray(intr, np.float32)]
    pose = np.asarray(pose, np.float64)
    Rm, t = R.rotation(pose[3:] / np.linalg.norm(pose[3:])), pose[:3]
    c = -Rm.T @ t
    yy, xx = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    dw = np.stack([(xx - cx) / fx, (yy - cy) / fy, np.ones_like(xx, float)], -1) @ Rm
    with np.errstate(all="ignore"):
        depth = (R.PLANE_D - R.PLANE_N @ c) / (dw @ R.PLANE_N)
        depth = np.where(depth > 0, depth, np.inf)
        for centre, radius in ((R.SPHERE_C, R.SPHERE_R), (SPHERE2_C, SPHERE2_R)):
            oc = c - centre
            qa, qb, qc = (dw * dw).sum(-1), 2.0 * (dw @ oc), oc @ oc - radius ** 2
            disc = qb * qb - 4 * qa * qc
            s = np.where(disc > 0, (-qb - np.sqrt(np.maximum(disc, 0))) / (2 * qa), np.inf)
            depth = np.minimum(depth, np.where(s > 0, s, np.inf))
    return depth


def scene(ht, wd, seed=0):
    """tsdf_reference.scene's cameras, intrinsics and weights at ht x wd with this module's surfaces: poses [5,7] f32, disps [5,ht,wd]
    f32, intr [4] f32, weight [5,ht,wd] f32"""
    poses, _, intr, _, weight, _ = R.scene(NFRAMES, ht, wd, seed)
    with np.errstate(all="ignore"):
        disps = np.stack([1.0 / analytic_depth(p, intr, ht, wd) for p in poses]).astype(np.float32)
    return poses, disps, intr, weight


def fused_volume():
    """the reference's own fused volume of the scene (fp32 tsdf, wsum) as the dict evaluate() takes"""
    poses, disps, intr, weight = scene(*FUSE_SIZE)
    v = R.integrate_reference(DIMS, ORIGIN, VOXEL, TRUNC, poses, disps, intr, range(NFRAMES), weight=weight)
    return dict(tsdf=v["tsdf"].astype(np.float32), wsum=v["wsum"], origin=ORIGIN, voxel=VOXEL)


# ------------------------------------------------------------------------------------------------------------ SE(3), fp64
def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def se3_exp(xi):
    """(t, q) of Exp(xi), xi = (tau, phi)"""
    xi = np.asarray(xi, np.float64)
    tau, phi = xi[:3], xi[3:]
    th = np.linalg.norm(phi)
    if th < 1e-9:
        q = np.concatenate([0.5 * phi, [1.0]])
        return tau + 0.5 * np.cross(phi, tau), q / np.linalg.norm(q)
    q = np.concatenate([np.sin(0.5 * th) / th * phi, [np.cos(0.5 * th)]])
    a, b = (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    pt = np.cross(phi, tau)
    return tau + a * pt + b * np.cross(phi, pt), q


def retract(xi, pose, right=False):
    """Exp(xi) G (right: the wrong G Exp(xi)), stored in fp32"""
    pose = np.asarray(pose, np.float32).astype(np.float64)
    dt, dq = se3_exp(xi)
    t, q = pose[:3], pose[3:]
    if right:
        out = np.concatenate([R.rotation(q) @ dt + t, _qmul(q, dq)])
    else:
        out = np.concatenate([R.rotation(dq) @ t + dt, _qmul(dq, q)])
    return out.astype(np.float32)


def pose_difference(a, b):
    """|delta|_2 of Exp(delta) b = a (first order in the translation part)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    qa, qb = a[3:] / np.linalg.norm(a[3:]), b[3:] / np.linalg.norm(b[3:])
    dq = _qmul(qa, np.array([-qb[0], -qb[1], -qb[2], qb[3]]))
    if dq[3] < 0:
        dq = -dq
    nv = np.linalg.norm(dq[:3])
    phi = 2.0 * np.arctan2(nv, dq[3]) * (dq[:3] / nv if nv > 0 else np.zeros(3))
    return float(np.linalg.norm(np.concatenate([a[:3] - R.rotation(dq) @ b[:3], phi])))


def perturbed(pose, xi):
    """Exp(xi) pose in fp32: a start near `pose`"""
    return retract(xi, pose)


def starts(count, max_t=0.10, max_deg=2.0, seed=1):
    """a fixed list of tangent offsets [count,6]: translations up to max_t, rotations up to max_deg, the first at the full extent"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        u, v = rng.normal(size=3), rng.normal(size=3)
        scale = 1.0 if k == 0 else rng.uniform(0.2, 1.0)
        out.append(np.concatenate([scale * max_t * u / np.linalg.norm(u), scale * np.radians(max_deg) * v / np.linalg.norm(v)]))
    return np.array(out)


# ------------------------------------------------------------------------------------------------------------ one evaluation
_IJ = [(i, j) for i in range(6) for j in range(i, 6)]


def _terms(c, p, ignore_band):
    """everything the contract derives from the positions p [P,3] of the pixels (c: the evaluation's constants)"""
    n, E_p = c["n"], c["E_p"]
    with np.errstate(all="ignore"):
        inbox = c["ok"] & np.all((p >= 0) & (p <= n - 1), 1)
    cell = np.minimum(np.floor(np.where(inbox[:, None], p, 0)).astype(np.int64), n - 2)
    valid = inbox.copy()
    valid[inbox] = V._corners(c["valid_vox"], cell[inbox]).all(1)
    frac = p - cell
    s = V._corners(c["s64"], np.where(valid[:, None], cell, 0))
    S, grad = V._trilinear(s, np.where(valid[:, None], frac, 0.0))
    if c["mutant"] == "nearest":
        near = np.clip(np.floor(np.where(valid[:, None], p, 0) + 0.5).astype(np.int64), 0, n - 1)
        S = c["s64"][near[:, 2], near[:, 1], near[:, 0]]
    E_S = K_TRI * EPS + (np.abs(grad) * E_p).sum(1)
    votes = valid & ((np.abs(S) < c["band"]) | ignore_band | (c["mutant"] == "no_band"))
    mixed = lambda a, b, c, d, e, f, g, h: np.maximum(np.abs(s[:, a] - s[:, b] - s[:, c] + s[:, d]), np.abs(s[:, e] - s[:, f] - s[:, g] + s[:, h]))
    c_xy, c_xz, c_yz = mixed(3, 2, 1, 0, 7, 6, 5, 4), mixed(5, 4, 1, 0, 7, 6, 3, 2), mixed(6, 4, 2, 0, 7, 5, 3, 1)
    E_grad = K_GRAD * EPS + np.stack([c_xy * E_p[:, 1] + c_xz * E_p[:, 2], c_xy * E_p[:, 0] + c_yz * E_p[:, 2],
                                      c_xz * E_p[:, 0] + c_yz * E_p[:, 1]], 1)
    M = c["M"]
    if c["mutant"] == "unrotated":
        gc, E_gc = grad / c["voxel"], E_grad / c["voxel"]
    else:
        gc = grad @ M
        E_gc = E_grad @ np.abs(M) + K_GC * EPS * (np.abs(grad) @ np.abs(M))
    X = c["X"]
    E_X = K_X * EPS * np.abs(X)
    cr, E_cr = np.cross(X, gc), np.zeros_like(gc)
    for i, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
        E_cr[:, i] = (np.abs(X[:, a]) * E_gc[:, b] + np.abs(gc[:, b]) * E_X[:, a] + np.abs(X[:, b]) * E_gc[:, a] + np.abs(gc[:, a]) * E_X[:, b]
                      + 2 * EPS * (np.abs(X[:, a] * gc[:, b]) + np.abs(X[:, b] * gc[:, a])))
    J, E_J = -np.concatenate([gc, cr], 1), np.concatenate([E_gc, E_cr], 1)
    a = np.abs(S)
    h = c["huber"]
    with np.errstate(all="ignore"):
        quad = (h == 0) | (a <= h)
        k = np.where(quad, 1.0, h / a)
        rho = np.where(quad, S * S, h * (2 * a - h))
        E_k = np.where(quad, 0.0, k * (E_S / a + 2 * EPS))
    w = c["w"]
    wk = w * k
    tH = np.stack([wk * J[:, i] * J[:, j] for i, j in _IJ], 1)
    E_tH = np.stack([wk * (np.abs(J[:, i]) * E_J[:, j] + np.abs(J[:, j]) * E_J[:, i]) + w * E_k * np.abs(J[:, i] * J[:, j]) for i, j in _IJ], 1)
    tb = (wk * S)[:, None] * J
    E_tb = wk[:, None] * (np.abs(S)[:, None] * E_J + np.abs(J) * E_S[:, None]) + (w * E_k * np.abs(S))[:, None] * np.abs(J)
    tE = w * rho
    E_tE = w * np.where(quad, 2 * a * E_S, 2 * h * E_S)
    terms = np.concatenate([tH, tb, tE[:, None]], 1)                   # [P,28]
    E_terms = np.concatenate([E_tH, E_tb, E_tE[:, None]], 1) + K_TERM * EPS * np.abs(terms)
    return dict(inbox=inbox, valid=valid, votes=votes, S=S, J=J, E_S=E_S, E_J=E_J, terms=terms, E_terms=E_terms)


def unpack(v27):
    """(H [6,6] symmetric, b [6]) of the 27 numbers of `system`"""
    H = np.zeros((6, 6))
    for k, (i, j) in enumerate(_IJ):
        H[i, j] = H[j, i] = v27[k]
    return H, np.asarray(v27[21:27], np.float64)


def evaluate(vol, disp, weight, intr, pose, band=0.9, huber=0.0, min_weight=1.0, mutant=None):
    """one evaluation of the contract for one frame (disp, weight [ht,wd] f32; weight None = 1) at `pose` [7] f32.  vol: dict tsdf, wsum
    f32 [nz,ny,nx], origin, voxel and optionally allocated bool [nz/8,ny/8,nx/8].  Returns per pixel [ht,wd(,6)] S, J, votes, flagged,
    bound_S, bound_J; sums [28] = (H 21, b 6, E) with bound_sums [28]; count, nflag; H [6,6], b [6]."""
    assert mutant is None or mutant in MUTANTS
    tsdf, wsum = np.asarray(vol["tsdf"], np.float32), np.asarray(vol["wsum"], np.float32)
    nz, ny, nx = tsdf.shape
    n = np.array([nx, ny, nz])
    o = np.asarray(vol["origin"], np.float32).astype(np.float64)
    voxel = np.float64(np.float32(vol["voxel"]))
    disp = np.asarray(disp, np.float32)
    ht, wd = disp.shape
    fx, fy, cx, cy = [np.float64(v) for v in np.asarray(intr, np.float32)]
    pose = np.asarray(pose, np.float32)
    Rm, t = R.rotation(pose[3:]), pose[:3].astype(np.float64)
    M = Rm.T / voxel
    p0 = (-(Rm.T @ t) - o) / voxel
    vv, uu = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    rx, ry = ((uu - cx) / fx).reshape(-1), ((vv - cy) / fy).reshape(-1)
    d32 = disp.reshape(-1)
    w32 = np.ones_like(d32) if weight is None else np.asarray(weight, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        ok = np.isfinite(d32) & (d32 > 0) & np.isfinite(w32) & (w32 > 0)
        z = 1.0 / np.where(ok, d32, 1).astype(np.float64)
    z = np.where(np.isfinite(z), z, 0.0)
    rays = np.stack([rx, ry, np.ones_like(rx)], 1)
    p = z[:, None] * (rays @ M.T) + p0
    gmag = np.abs(rays) @ np.abs(M).T                                     # sum_j |M_ij| |r_j| >= |g_i|
    E_p = EPS * (K_RAY * z[:, None] * gmag + (K_C * np.abs(t).sum() + np.abs(o)) / voxel + np.abs(p0) + np.abs(p))
    valid_vox = wsum >= np.float32(min_weight)
    if vol.get("allocated") is not None:
        valid_vox = valid_vox & np.repeat(np.repeat(np.repeat(np.asarray(vol["allocated"], bool), 8, 0), 8, 1), 8, 2)
    c = dict(n=n, E_p=E_p, ok=ok, valid_vox=valid_vox, s64=tsdf.astype(np.float64), mutant=mutant, band=np.float64(np.float32(band)),
             huber=np.float64(np.float32(huber)), M=M, voxel=voxel, X=np.stack([z * rx, z * ry, z], 1), w=np.where(ok, w32, 0).astype(np.float64))
    e = _terms(c, p, False)
    # decisions within rounding of flipping
    with np.errstate(all="ignore"):
        near_int = ok & np.all((p >= -1) & (p <= n), 1) & np.any(np.abs(p - np.round(p)) <= E_p, 1)
        near_band = e["valid"] & (np.abs(np.abs(e["S"]) - c["band"]) <= e["E_S"]) & (mutant != "no_band")
        near_huber = e["valid"] & (c["huber"] > 0) & (np.abs(np.abs(e["S"]) - c["huber"]) <= e["E_S"])
    flagged = near_int | near_band | near_huber            # (a face of the box is an integer)
    # a flagged pixel's alternative: across the cell face, the band ignored
    side = np.where(np.abs(p - np.round(p)) <= E_p, np.where(p >= np.round(p), -1.0, 1.0), 0.0)
    alt = _terms(c, np.where(side != 0, np.round(p) + side * 2 * E_p, p), True)
    mine = np.where(e["votes"][:, None], np.abs(e["terms"]), 0.0)
    other = np.where(alt["votes"][:, None], np.abs(alt["terms"]), 0.0)
    un = e["votes"] & ~flagged
    sums = np.where(e["votes"][:, None], e["terms"], 0.0).sum(0)
    bound = (np.where(un[:, None], e["E_terms"], 0.0).sum(0) + np.where(flagged[:, None], mine + other, 0.0).sum(0)
             + TREE_DEPTH * EPS * mine.sum(0))
    H, b = unpack(sums[:27])
    E_H, E_b = unpack(bound[:27])
    sh = (ht, wd)
    return dict(S=e["S"].reshape(sh), J=e["J"].reshape(sh + (6,)), votes=e["votes"].reshape(sh), valid=e["valid"].reshape(sh),
                flagged=flagged.reshape(sh), bound_S=e["E_S"].reshape(sh), bound_J=e["E_J"].reshape(sh + (6,)), sums=sums, bound_sums=bound,
                count=int(e["votes"].sum()), nflag=int(flagged.sum()), H=H, b=b, E=float(sums[27]), E_H=E_H, E_b=E_b,
                terms=e["terms"].reshape(sh + (28,)), weight=c["w"].reshape(sh))


def solve_step(H, b, count, lm=1e-4, ep=1e-6, min_count=32):
    """(xi f64 [6] as rounded to fp32, status, the absolute values of A^-1 [6,6])"""
    A = H + np.diag(np.float64(np.float32(lm)) * np.diag(H) + np.float64(np.float32(ep)))
    L, good = np.zeros((6, 6)), True
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j] - L[j, :j] @ L[j, :j]
            good = good and bool(np.isfinite(d) and d > 0)
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, 6):
                L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
        xi = np.zeros(6)
        if good:
            xi = -np.linalg.solve(L.T, np.linalg.solve(L, b))
        xi = xi.astype(np.float32).astype(np.float64)
        good = good and bool(np.all(np.isfinite(xi)))
    status = 1 if count < min_count else (0 if good else 2)
    ainv = np.abs(np.linalg.inv(A)) if good else np.full((6, 6), np.inf)
    return xi, status, ainv


def track_reference(vol, poses, disps, intr, ix, weight=None, iters=10, band=0.9, huber=0.0, lm=1e-4, ep=1e-6, min_count=32, min_weight=1.0,
                    mutant=None):
    """pvo_tsdf_track.  Returns dict: poses f32 [N,7], info f64 [N,iters+1,4], system f64 [N,27], residual [N,ht,wd] (NaN = no vote), jac
    [N,ht,wd,6], votes, flagged bool [N,ht,wd], bound_S [N,ht,wd], bound_J [N,ht,wd,6] (all of the LAST evaluation), bound_sums
    [N,iters+1,28], nflag [N,iters+1], pose_bound [N] (the drift allowed between this tracker's final pose and the kernel's), xi0 [N,6]
    and xi0_bound [N] (the first step), trail f32 [N,iters+1,7] (the pose of every evaluation), weight [N,ht,wd] (the weights used, 0 where the pixel has no depth)."""
    poses, disps = np.asarray(poses, np.float32), np.asarray(disps, np.float32)
    nf, ht, wd = disps.shape
    ix = [int(v) for v in np.asarray(ix).reshape(-1)]
    N = len(ix)
    out = dict(poses=poses.copy(), info=np.zeros((N, iters + 1, 4)), system=np.zeros((N, 27)), residual=np.full((N, ht, wd), np.nan),
               jac=np.zeros((N, ht, wd, 6)), votes=np.zeros((N, ht, wd), bool), flagged=np.zeros((N, ht, wd), bool),
               bound_S=np.zeros((N, ht, wd)), bound_J=np.zeros((N, ht, wd, 6)), bound_sums=np.zeros((N, iters + 1, 28)),
               nflag=np.zeros((N, iters + 1), int), pose_bound=np.zeros(N), xi0=np.zeros((N, 6)), xi0_bound=np.zeros(N),
               weight=np.zeros((N, ht, wd)), terms=np.zeros((N, ht, wd, 28)), trail=np.repeat(poses[:, None], iters + 1, 1))
    for s, f in enumerate(ix):
        if not 0 <= f < nf:
            out["info"][s, :, 3] = 4
            continue
        pose, drift, moved = poses[s].copy(), 0.0, 0.0
        for e in range(iters + 1):
            ev = evaluate(vol, disps[f], None if weight is None else weight[f], intr, pose, band, huber, min_weight, mutant)
            xi, status, ainv = solve_step(ev["H"], ev["b"], ev["count"], lm, ep, min_count)
            out["trail"][s, e] = pose
            step = status == 0 and e < iters
            out["info"][s, e] = (ev["E"], ev["count"], np.abs(xi).max() if step else 0.0, status)
            # (E's bound also carries the drift: dE = 2 b . delta)
            out["bound_sums"][s, e] = ev["bound_sums"] + np.concatenate([np.zeros(27), [2 * np.abs(ev["b"]).sum() * drift]])
            out["nflag"][s, e] = ev["nflag"]
            own = float(np.linalg.norm(ainv @ (ev["E_b"] + ev["E_H"] @ np.abs(xi)) + EPS * np.abs(xi))) if status == 0 else 0.0
            if e == 0:
                out["xi0"][s], out["xi0_bound"][s] = xi, own
            if step:
                moved = 2 * np.sqrt(6.0) * np.abs(xi).max()
                drift += own + K_RETR * EPS * (1.0 + np.abs(pose[:3]).sum() + np.abs(xi).sum())
                pose = retract(xi, pose, right=mutant == "right_retraction")
        out["poses"][s] = pose
        out["system"][s] = ev["sums"][:27]
        out["residual"][s] = np.where(ev["votes"], ev["S"], np.nan)
        out["jac"][s] = np.where(ev["votes"][..., None], ev["J"], 0.0)
        for k in ("votes", "flagged", "bound_S", "bound_J", "weight", "terms"):
            out[k][s] = ev[k]
        out["pose_bound"][s] = min(drift, own + moved + K_RETR * EPS * (1.0 + np.abs(pose[:3]).sum())) if status == 0 else drift
    return out


# ------------------------------------------------------------------------------------------------------------ the check
def track_matches(got, ref):
    """the check of the tracking tests.  got: dict of numpy poses [N,7], info [N,iters+1,4], residual [N,ht,wd], jac [N,ht,wd,6] (and
    optionally system [N,27]) of a tracker run on the operands of `ref`.  On unflagged pixels of the last evaluation of the slots that took no step: votes / does not
    vote EQUAL (a residual that is not NaN; NaN and a zero J otherwise), S and J within the bounds; per evaluation the status EQUAL, the
    count within the number of flagged pixels, E within its bound; the final pose within pose_bound; system within its bounds for the slots that took no step (test_the_reduction_alone holds it
    everywhere).
    Returns (ok, report)."""
    still = ref["pose_bound"] == 0                          # (no step: both evaluate the same fp32 pose)
    un = ~ref["flagged"] & still[:, None, None]
    res, jac = got["residual"].astype(np.float64), got["jac"].astype(np.float64)
    voted = ~np.isnan(res)
    v_ok = np.array_equal(voted[un], ref["votes"][un]) and not jac[~voted].any()
    on = un & ref["votes"] & voted
    s_err = np.abs(np.where(on, res - np.where(ref["votes"], ref["residual"], 0), 0.0))
    j_err = np.abs(np.where(on[..., None], jac - ref["jac"], 0.0))
    s_ok = bool(np.all(s_err <= ref["bound_S"]))
    j_ok = bool(np.all(j_err <= ref["bound_J"]))
    info = got["info"].astype(np.float64)
    st_ok = np.array_equal(info[..., 3], ref["info"][..., 3])
    c_ok = bool(np.all(np.abs(info[..., 1] - ref["info"][..., 1]) <= ref["nflag"]))
    E_err = np.abs(info[..., 0] - ref["info"][..., 0])
    E_bound = ref["bound_sums"][..., 27] + 2 * EPS * np.abs(ref["info"][..., 0])          # (its rounding to fp32)
    e_ok = bool(np.all(E_err <= E_bound))
    dist = np.array([pose_difference(a, b) for a, b in zip(got["poses"], ref["poses"])])
    p_ok = bool(np.all(dist <= ref["pose_bound"]))
    y_ok = True
    if got.get("system") is not None:                       # (where no step was taken: H and b move with the pose)
        still = (ref["pose_bound"] == 0) & (ref["info"][:, -1, 3] != 4)
        y_ok = bool(np.all(np.abs(got["system"] - ref["system"])[still] <= ref["bound_sums"][:, -1, :27][still]))
        y_ok = y_ok and not np.asarray(got["system"])[ref["info"][:, -1, 3] == 4].any()
    with np.errstate(all="ignore"):
        report = ("votes %s, S %s (max err %.3e, max err / bound %.3f), J %s (max err / bound %.3f), status %s, count %s, E %s (max err / bound %.3f), "
                  "pose %s (max distance %.3e, bound %.3e), system %s, flagged %.4f" % (
                      v_ok, s_ok, s_err.max(), np.nanmax(np.where(on, s_err / ref["bound_S"], 0)), j_ok,
                      np.nanmax(np.where(on[..., None], j_err / ref["bound_J"], 0)), st_ok, c_ok, e_ok, np.nanmax(E_err / np.maximum(E_bound, 1e-300)),
                      p_ok, dist.max(), ref["pose_bound"].max(), y_ok, ref["flagged"].mean()))
    return v_ok and s_ok and j_ok and st_ok and c_ok and e_ok and p_ok and y_ok, report


def as_got(ref):
    """a reference's own outputs in the form track_matches takes (for holding one reference against another)"""
    return dict(poses=ref["poses"], info=ref["info"].astype(np.float32), residual=ref["residual"].astype(np.float32),
                jac=ref["jac"].astype(np.float32))


def reduction_check(system, info_row, residual, jac, weight, huber=0.0):
    """the reduction alone: H, b, E and count from a tracker's OWN residual [ht,wd] / jac [ht,wd,6] (fp32) and the weights against its
    system [27] and info row.  No flags.  The terms are reproduced bit for bit in fp32 as the contract rounds them (w k; (w k) J_i; its
    product with J_j or S; k = huber / a; rho = S S or huber fma(2, a, -huber); w rho) and summed in fp64, so the bound is the rounding of
    the fixed reduction tree alone, TREE_DEPTH EPS sum |terms|, plus E's rounding to fp32; count is exact.
    Returns (ok, worst err / bound)."""
    f = np.float32
    S, J, w = np.asarray(residual, f).reshape(-1), np.asarray(jac, f).reshape(-1, 6), np.asarray(weight, f).reshape(-1)
    v = ~np.isnan(S)
    S, J, w = S[v], J[v], w[v]
    a, h = np.abs(S), f(huber)
    with np.errstate(all="ignore"):
        quad = (h == 0) | (a <= h)
        k = np.where(quad, f(1), h / a).astype(f)
        rho = np.where(quad, S * S, h * (2.0 * a.astype(np.float64) - np.float64(h)).astype(f)).astype(f)      # (2 a is exact: one rounding)
    wk = (w * k).astype(f)
    wj = (wk[:, None] * J).astype(f)
    terms = np.concatenate([np.stack([wj[:, i] * J[:, j] for i, j in _IJ], 1), wj * S[:, None], (w * rho)[:, None]], 1)
    assert terms.dtype == f
    terms = terms.astype(np.float64)
    want, mag = terms.sum(0), np.abs(terms).sum(0)
    bound = TREE_DEPTH * EPS * mag
    bound[27] += 2 * EPS * abs(want[27])
    err = np.abs(np.concatenate([np.asarray(system, np.float64), [np.float64(info_row[0])]]) - want)
    ok = bool(np.all(err <= bound)) and int(info_row[1]) == int(v.sum())
    with np.errstate(all="ignore"):
        return ok, float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))
