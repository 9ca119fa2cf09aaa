"""The object-motion call's yardstick (tests/test_object_motion_host.py, tests/test_object_motion_gpu.py): the contract of
pvo_object_motion (include/pvo_hip.h) restated in numpy.  Geometry, sums, the solve and the retraction are evaluated in fp64 on the fp32
inputs; what the contract stores in fp32 is stored in fp32 here as well (the step xi and A between evaluations).

The scene.  tsdf_reference.scene(5, ht, wd): a plane and a sphere seen from five cameras.  Labels: 1 on the plane, 2 where the pixel sees
the sphere (`hit`), and a 2 x 2 patch of label 7 in the top-left corner of the plane (too small to solve).  Between the two frames of
every edge the sphere moves by T_w = C Exp(XI_O) C^-1 in the world, C the translation to the sphere's centre; the plane stays.  The
targets are the analytic projections of the (moved) points into frame j, rounded to fp32: point correspondences, so the rotation about
the centre is observable.  Edges (1,2), (3,1), (0,4), (2,2) - frame 2 is the identity camera, so there motion = rel - and (1,7), a frame
that does not exist.  The edge weights are the scene's weights of frame i.  What was checked on the CPU for this scene
(test_object_motion_host.py asserts it): at the three sizes of SIZES the sphere has 163 / 23 / 54 contributing pixels on edge (1,2) and at
least 159 / 23 / 54 on the first three edges, cond(H) at the start is 6e2 to 1.3e3, eight Gauss-Newton steps (lm 1e-4) from the NULL start reach the true A to
below 1e-10 in fp64, and the plane's job has zero residual at its start.

Error bound of the kernel (pvo_amd/csrc/object_motion.hip as written: fp32, the multiply-adds the contract writes as fma fused;
EPS = 2^-24, first order; a division and a square root are counted as within one ulp = 2 EPS although the build rounds them correctly):
  rx = (ui - cx) / fx: the difference 1, the division 2;  z = 1 / d: 2;  Xi_0 = z rx: 3 + 2 + 1:   E_X_i = K_X EPS |Xi_i|,  K_X = 6
  R_kj of the quaternion as stored: off the diagonal a product, an fma (magnitudes <= 1/2) and an exact doubling, on it two roundings of
         magnitude <= 1 doubled and the outer fma:                                                  E_R = K_ROT EPS,  K_ROT = 5
  Y_k = fma(R_k0, X_0, fma(R_k1, X_1, fma(R_k2, X_2, t_k))): three fma roundings of magnitude <= S_k = sum_j |R_kj X_j| + |t_k|:
         E_Y_k = sum_j |R_kj| E_X_j + K_ROT EPS sum_j |X_j| + K_CHAIN EPS S_k,  K_CHAIN = 3
  iz = 1 / Y_z:                                 E_iz = iz (E_Y_z / Y_z + 2 EPS)
  qx = Y_x iz:                                  E_qx = iz E_Y_x + |Y_x| E_iz + EPS |qx|
  r_u = fma(fx, qx, cx) - tu:                   E_r_u = fx E_qx + EPS |fx qx + cx| + EPS |r_u|
  ax = fx iz:                                   E_ax = fx E_iz + EPS ax
  mx = -(ax qx):                                E_mx = |qx| E_ax + ax E_qx + EPS |mx|
  a product p = s Y_k of J (s = ax or mx):      E_p = |Y_k| E_s + |s| E_Y_k + EPS |p|
  fma(ax, Y_z, -(mx Y_x)) (the cross products): the two products' E_p without their EPS terms + 2 EPS (|ax Y_z| + |mx Y_x|)
  a = sqrt(fma(r_u, r_u, r_v r_v)), 1-Lipschitz in r; a product, the fma and half the root's 2:  E_a = E_r_u + E_r_v + K_A EPS a,  K_A = 3
  k = huber / a beyond the threshold:           E_k = k (E_a / a + 2 EPS)
  rho = a a: 2 a E_a + EPS rho;  rho = huber fma(2, a, -huber): 2 huber E_a + 2 EPS |rho|
  a term fma(wu_i, J_u,j, wv_i J_v,j) (w k, (w k) J_i, the product, the fma: K_TERM = 4, second order absorbed):
         E_term = w k sum_rows (|J_i| E_J_j + |J_j| E_J_i) + w E_k sum_rows |J_i J_j| + K_TERM EPS sum_rows |w k J_i J_j|;
         likewise fma(wu_i, r_u, wv_i r_v);  w rho: w E_rho + EPS |w rho|;  the count is exact;  c's terms are Xi: E_X
  the sums: a fixed tree of TREE_DEPTH = 8 fp32 levels (six in the wave, two across the waves), then fp64:  TREE_DEPTH EPS sum |terms|
  the step: |d xi| <= |A_d^-1| (E_b + E_H |xi|) with the ABSOLUTE VALUES of the entries, + EPS |xi| (its rounding to fp32); the fp64
         factorisation adds nothing visible
  the retraction (csrc/se3.h in fp32): fewer than K_RETR = 32 roundings on any path from (xi, A) to a component of the new A, each on a
         magnitude <= 1 + |t|_1 + |xi|_1, sinf / cosf within 2 ulp:   K_RETR EPS (1 + |t|_1 + |xi|_1).  The NULL start G_j G_i^-1 is one
         such product: K_RETR EPS (1 + |t_i|_1 + |t_j|_1) before the first evaluation
  motion = G_j^-1 (A G_i): an error delta of A arrives as Ad(G_j^-1) delta, at most (1 + |t_j|_2) |delta|; the two products are fewer
         than K_MOTION = 64 roundings on any path, on magnitudes <= 1 + |t_i|_1 + |t_j|_1 + |t_A|_1
  centroid = G_i^-1 (c / count): (sum E_X + TREE_DEPTH EPS sum |Xi|) / count, the mean's rounding to fp32 and the inverse action
         (K_RETR roundings on magnitudes <= 1 + |t_i|_1 + |mean|_1); with a differing count (flagged pixels) both alternatives
E of an evaluation whose A may differ by delta between the two sides (after a step, or from the NULL start) carries
         2 |b|_1 |delta| + trace(H) |delta|^2 in its bound (E is quadratic in delta in the Gauss-Newton model)
Over several iterations the two solvers' A drift apart by at most the SUM of the steps' own bounds (the argument of
tests/tsdf_track_reference.py: inside the basin I - A_d^-1 H is a contraction); once both have converged the distance is also bounded at
the fixed point: |A_d^-1| (E_b + E_H |xi|) of the LAST evaluation plus what the two last steps still moved (2 sqrt(6) max|xi|).
pose_bound is the smaller of the two.  Per-pixel outputs are compared only where both evaluate the same fp32 A (a given start, no step).
Against the TRUE motion the converged A is off by the targets' rounding to fp32 as well: at the fixed point b = 0 on both sides, and
the true A's b is sum w k J^T dt with |dt| <= EPS |target|:  |A_d^-1| sum w k |J|^T EPS |target|  (truth_bound adds it).

Decisions.  A pixel is FLAGGED when a decision is within its bound of flipping: |Y_z - z_min| <= E_Y_z, or ||r| - huber| <= E_a.
Flagged pixels are left out of the per-pixel comparison; in the bounds of the sums they count with both alternatives (the magnitude of
their terms as evaluated plus that of the alternative: z_min ignored, the other branch of k).  They must stay below 1 %
(test_object_motion_host.py asserts it on this reference alone)."""
import numpy as np

import tsdf_reference as R
import tsdf_track_reference as T

EPS = R.EPS
K_X, K_ROT, K_CHAIN, K_A, K_TERM, K_RETR, K_MOTION, TREE_DEPTH = 6, 5, 3, 3, 4, 32, 64, 8
MUTANTS = ("right_retraction", "camera_motion", "label_of_target", "relative_target", "no_huber")

NFRAMES = 5
SIZES = ((24, 32), (9, 12), (13, 19))            # three workgroups; tails in both directions
XI_O = np.array([0.06, -0.03, 0.04, 0.05, -0.08, 0.03])
EDGES = ((1, 2), (3, 1), (0, 4), (2, 2), (1, 7))
MIN_MEMBERS = {(24, 32): 163, (9, 12): 23, (13, 19): 54}
PARAMS = dict(iters=8, z_min=0.25, huber=0.0, lm=1e-4, ep=1e-6, min_count=16)
# the parameter variants the tests run (over PARAMS).  z_min 1.15 cuts THROUGH the sphere (its depths run from 0.95 to 1.3), z_min 1.5 leaves
# the whole sphere out (count 0, status 1) and the plane (depth >= 1.7) in; huber 0.5 pixels is below the residuals of the perturbed starts
CASES = {"plain": {}, "huber": dict(huber=0.5), "zcut": dict(z_min=1.15), "zfar": dict(z_min=1.5)}
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1], np.float64)
_IJ = T._IJ
unpack = T.unpack
pose_difference = T.pose_difference


# ------------------------------------------------------------------------------------------------------------ SE(3), fp64
def pose_mul(a, b):
    """a b of two poses (t, q) [7], fp64, the quaternion as the product comes"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.concatenate([R.rotation(a[3:]) @ b[:3] + a[:3], T._qmul(a[3:], b[3:])])


def pose_inv(a):
    a = np.asarray(a, np.float64)
    qi = np.array([-a[3], -a[4], -a[5], a[6]])
    return np.concatenate([-(R.rotation(qi) @ a[:3]), qi])


def true_motion():
    """T_w = C Exp(XI_O) C^-1 [7] fp64"""
    t, q = T.se3_exp(XI_O)
    c = np.concatenate([R.SPHERE_C, [0, 0, 0, 1.0]])
    return pose_mul(pose_mul(c, np.concatenate([t, q])), pose_inv(c))


# ------------------------------------------------------------------------------------------------------------ scene
def scene(ht, wd, exact=False):
    """dict: poses [5,7] f32, disps [5,ht,wd] f32, intr [4] f32, labels [5,ht,wd] int32, ii, jj int64 [5], target [5,ht,wd,2] f32 (fp64
    with exact=True), weight [5,ht,wd] f32, truth [5,7] fp64: the true A of the sphere per edge (NaN for the edge without frames)"""
    poses, disps, intr, _, weight, hit = R.scene(NFRAMES, ht, wd)
    labels = np.where(hit, 2, 1).astype(np.int32)
    assert not hit[:, :2, :2].any()
    labels[:, :2, :2] = 7
    fx, fy, cx, cy = [np.float64(v) for v in intr]
    ii, jj = np.array([e[0] for e in EDGES], np.int64), np.array([e[1] for e in EDGES], np.int64)
    vv, uu = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    Tw = true_motion()
    target = np.zeros((len(EDGES), ht, wd, 2))
    wgt = np.ones((len(EDGES), ht, wd), np.float32)
    truth = np.full((len(EDGES), 7), np.nan)
    for e, (i, j) in enumerate(EDGES):
        if not (0 <= i < NFRAMES and 0 <= j < NFRAMES):
            continue
        wgt[e] = weight[i]
        z = 1.0 / disps[i].astype(np.float64)
        X = np.stack([z * (uu - cx) / fx, z * (vv - cy) / fy, z], -1)
        static, moving = pose_mul(poses[j], pose_inv(poses[i])), pose_mul(pose_mul(poses[j], Tw), pose_inv(poses[i]))
        truth[e] = moving
        Ys = X @ R.rotation(static[3:]).T + static[:3]
        Ym = X @ R.rotation(moving[3:]).T + moving[:3]
        Y = np.where(hit[i][..., None], Ym, Ys)
        target[e] = np.stack([fx * Y[..., 0] / Y[..., 2] + cx, fy * Y[..., 1] / Y[..., 2] + cy], -1)
    return dict(poses=poses, disps=disps, intr=intr, labels=labels, ii=ii, jj=jj, target=target if exact else target.astype(np.float32),
                weight=wgt, truth=truth, hit=hit)


def jobs(sc):
    """the tests' job list: per valid edge the sphere (2), the plane (1), the patch (7); then a label nobody has, a repeat of job 0 and
    the edge without frames: (job_edge int64 [N], job_label int32 [N])"""
    je, jl = [], []
    for e in range(4):
        for lab in (2, 1, 7):
            je.append(e); jl.append(lab)
    je += [0, 0, 4]; jl += [99, 2, 2]
    return np.array(je, np.int64), np.array(jl, np.int32)


def perturbed_start(sc, job_edge, seed=3):
    """Exp(delta) G_j G_i^-1 in fp32 per job (the identity for a job without frames): translations up to 0.03, rotations up to 1 degree"""
    d = T.starts(len(job_edge), max_t=0.03, max_deg=1.0, seed=seed)
    out = np.zeros((len(job_edge), 7), np.float32)
    for n, e in enumerate(job_edge):
        i, j = int(sc["ii"][e]), int(sc["jj"][e])
        if 0 <= i < NFRAMES and 0 <= j < NFRAMES:
            out[n] = T.retract(d[n], pose_mul(sc["poses"][j], pose_inv(sc["poses"][i])).astype(np.float32))
        else:
            out[n] = IDENTITY
    return out


# ------------------------------------------------------------------------------------------------------------ one evaluation
def _terms(c, ignore_zmin, flip):
    """everything the contract derives from a job's pixels at the evaluation's constants c; flip [P] bool: the other branch of k"""
    X, Rm, t, E_X = c["X"], c["R"], c["t"], c["E_X"]
    fx, fy, cx, cy = c["K"]
    with np.errstate(all="ignore"):
        Y = X @ Rm.T + t
        E_Y = E_X @ np.abs(Rm).T + K_ROT * EPS * np.abs(X).sum(1)[:, None] + K_CHAIN * EPS * (np.abs(X) @ np.abs(Rm).T + np.abs(t))
        votes = c["ok"] & ((Y[:, 2] > c["z_min"]) | ignore_zmin) & np.isfinite(c["tgt"]).all(1)
        Y = np.where(votes[:, None], Y, 1.0)
        tgt = np.where(votes[:, None], c["tgt"], 0.0)
        iz = 1.0 / Y[:, 2]
        E_iz = np.abs(iz) * (E_Y[:, 2] / np.abs(Y[:, 2]) + 2 * EPS)
        f = np.array([fx, fy])
        q = Y[:, :2] * iz[:, None]
        E_q = np.abs(iz)[:, None] * E_Y[:, :2] + np.abs(Y[:, :2]) * E_iz[:, None] + EPS * np.abs(q)
        proj = f * q + np.array([cx, cy])
        r = proj - tgt
        E_r = f * E_q + EPS * np.abs(proj) + EPS * np.abs(r)
        ax = f * iz[:, None]                                     # (ax, ay)
        E_ax = f * E_iz[:, None] + EPS * np.abs(ax)
        m = -ax * q                                              # (mx, my)
        E_m = np.abs(q) * E_ax + np.abs(ax) * E_q + EPS * np.abs(m)
        prod = lambda s, E_s, k: (s * Y[:, k], np.abs(Y[:, k]) * E_s + np.abs(s) * E_Y[:, k])
        z0 = np.zeros(len(X))
        mxYy, e1 = prod(m[:, 0], E_m[:, 0], 1)
        axYz, e2 = prod(ax[:, 0], E_ax[:, 0], 2)
        mxYx, e3 = prod(m[:, 0], E_m[:, 0], 0)
        axYy, e4 = prod(ax[:, 0], E_ax[:, 0], 1)
        myYy, e5 = prod(m[:, 1], E_m[:, 1], 1)
        ayYz, e6 = prod(ax[:, 1], E_ax[:, 1], 2)
        myYx, e7 = prod(m[:, 1], E_m[:, 1], 0)
        ayYx, e8 = prod(ax[:, 1], E_ax[:, 1], 0)
        Ju = np.stack([ax[:, 0], z0, m[:, 0], mxYy, axYz - mxYx, -axYy], 1)
        Jv = np.stack([z0, ax[:, 1], m[:, 1], myYy - ayYz, -myYx, ayYx], 1)
        E_Ju = np.stack([E_ax[:, 0], z0, E_m[:, 0], e1 + EPS * np.abs(mxYy), e2 + e3 + 2 * EPS * (np.abs(axYz) + np.abs(mxYx)),
                         e4 + EPS * np.abs(axYy)], 1)
        E_Jv = np.stack([z0, E_ax[:, 1], E_m[:, 1], e5 + e6 + 2 * EPS * (np.abs(myYy) + np.abs(ayYz)), e7 + EPS * np.abs(myYx),
                         e8 + EPS * np.abs(ayYx)], 1)
        J, E_J = np.stack([Ju, Jv], 1), np.stack([E_Ju, E_Jv], 1)            # [P,2,6]
        a = np.sqrt((r * r).sum(1))
        E_a = E_r.sum(1) + K_A * EPS * a
        h = c["huber"]
        quad = ((h == 0) | (a <= h)) ^ (flip & (h > 0))
        k = np.where(quad, 1.0, h / np.where(a > 0, a, 1.0))
        rho = np.where(quad, a * a, h * (2 * a - h))
        E_k = np.where(quad, 0.0, k * (E_a / np.where(a > 0, a, 1.0) + 2 * EPS))
        E_rho = np.where(quad, 2 * a * E_a + EPS * rho, 2 * h * E_a + 2 * EPS * np.abs(rho))
        w = c["w"]
        wk = w * k
        aJ = np.abs(J)
        tH = np.stack([wk * (J[:, :, i] * J[:, :, j]).sum(1) for i, j in _IJ], 1)
        E_tH = np.stack([wk * (aJ[:, :, i] * E_J[:, :, j] + aJ[:, :, j] * E_J[:, :, i]).sum(1)
                         + (w * E_k + K_TERM * EPS * wk) * (aJ[:, :, i] * aJ[:, :, j]).sum(1) for i, j in _IJ], 1)
        tb = wk[:, None] * (J * r[:, :, None]).sum(1)
        E_tb = (wk[:, None] * (aJ * E_r[:, :, None] + np.abs(r)[:, :, None] * E_J).sum(1)
                + (w * E_k + K_TERM * EPS * wk)[:, None] * (aJ * np.abs(r)[:, :, None]).sum(1))
        tE = w * rho
        E_tE = w * E_rho + EPS * np.abs(tE)
        one = np.ones(len(X))
        terms = np.concatenate([tH, tb, tE[:, None], one[:, None], X], 1)                      # [P,32]
        E_terms = np.concatenate([E_tH, E_tb, E_tE[:, None], z0[:, None], E_X], 1)
        # what the true A's b gains from the targets' rounding to fp32
        b_tgt = wk[:, None] * (aJ * (EPS * np.abs(tgt))[:, :, None]).sum(1)
    v = votes[:, None]
    return dict(votes=votes, Yz=Y[:, 2], E_Yz=E_Y[:, 2], a=a, E_a=E_a, r=r, J=J, E_r=E_r, E_J=E_J,
                terms=np.where(v, terms, 0.0), E_terms=np.where(v, E_terms, 0.0), b_tgt=np.where(v, b_tgt, 0.0))


def evaluate(sc, edge, label, A, z_min=0.25, huber=0.0, weight="scene", mutant=None):
    """one evaluation of the contract for the job (edge, label) at A [7] (fp32 values).  weight: "scene" = sc["weight"], None = 1, or an
    array [E,ht,wd].  Returns per pixel [ht,wd(,2(,6))] r, J, votes, flagged, bound_r, bound_J, terms [ht,wd,32]; sums [32] with
    bound_sums [32]; count, nflag; H, b, E, E_H, E_b, b_tgt [6]."""
    assert mutant is None or mutant in MUTANTS
    if mutant == "no_huber":
        huber = 0.0
    i, j = int(sc["ii"][edge]), int(sc["jj"][edge])
    disp = np.asarray(sc["disps"][i], np.float32)
    ht, wd = disp.shape
    fx, fy, cx, cy = [np.float64(v) for v in np.asarray(sc["intr"], np.float32)]
    A = np.asarray(A, np.float64)
    vv, uu = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    rx, ry = ((uu - cx) / fx).reshape(-1), ((vv - cy) / fy).reshape(-1)
    d32 = disp.reshape(-1)
    wsrc = sc["weight"] if isinstance(weight, str) else weight
    w32 = np.ones_like(d32) if wsrc is None else np.asarray(wsrc[edge], np.float32).reshape(-1)
    member = (np.asarray(sc["labels"][j if mutant == "label_of_target" else i]) == label).reshape(-1)
    tgt = np.asarray(sc["target"][edge], np.float64).reshape(-1, 2)
    if mutant == "relative_target":
        tgt = tgt + np.stack([uu, vv], -1).reshape(-1, 2)
    with np.errstate(all="ignore"):
        ok = member & np.isfinite(d32) & (d32 > 0) & np.isfinite(w32) & (w32 > 0)
        z = 1.0 / np.where(ok, d32, 1).astype(np.float64)
    X = np.stack([z * rx, z * ry, z], 1)
    c = dict(X=X, E_X=K_X * EPS * np.abs(X), R=R.rotation(A[3:]), t=A[:3], K=(fx, fy, cx, cy), ok=ok, tgt=tgt,
             z_min=np.float64(np.float32(z_min)), huber=np.float64(np.float32(huber)), w=np.where(ok, w32, 0).astype(np.float64))
    none = np.zeros(len(X), bool)
    e = _terms(c, False, none)
    with np.errstate(all="ignore"):
        near_z = ok & np.isfinite(tgt).all(1) & (np.abs(e["Yz"] - c["z_min"]) <= e["E_Yz"])
        near_h = e["votes"] & (c["huber"] > 0) & (np.abs(e["a"] - c["huber"]) <= e["E_a"])
    flagged = near_z | near_h
    alt = _terms(c, True, near_h)
    mine, other = np.abs(e["terms"]), np.abs(alt["terms"])
    un = e["votes"] & ~flagged
    sums = e["terms"].sum(0)
    bound = (np.where(un[:, None], e["E_terms"], 0.0).sum(0) + np.where(flagged[:, None], mine + other, 0.0).sum(0)
             + TREE_DEPTH * EPS * mine.sum(0))
    H, b = unpack(sums[:27])
    E_H, E_b = unpack(bound[:27])
    sh = (ht, wd)
    return dict(r=e["r"].reshape(sh + (2,)), J=e["J"].reshape(sh + (2, 6)), votes=e["votes"].reshape(sh), flagged=flagged.reshape(sh),
                bound_r=e["E_r"].reshape(sh + (2,)), bound_J=e["E_J"].reshape(sh + (2, 6)), sums=sums, bound_sums=bound,
                count=int(e["votes"].sum()), nflag=int(flagged.sum()), H=H, b=b, E=float(sums[27]), E_H=E_H, E_b=E_b,
                b_tgt=e["b_tgt"].sum(0), terms=e["terms"].reshape(sh + (32,)), weight=c["w"].reshape(sh), members=int(member.sum()))


def _f32(p, store32):
    return np.asarray(p, np.float32).astype(np.float64) if store32 else np.asarray(p, np.float64)


def _retract(xi, A, right, store32):
    if store32:
        return T.retract(xi, A, right=right).astype(np.float64)
    dt, dq = T.se3_exp(xi)
    d = np.concatenate([dt, dq])
    return pose_mul(A, d) if right else pose_mul(d, A)


def motion_reference(sc, job_edge, job_label, start=None, iters=8, z_min=0.25, huber=0.0, lm=1e-4, ep=1e-6, min_count=16, weight="scene",
                     mutant=None, store32=True):
    """pvo_object_motion.  Returns dict: rel, motion [N,7] (fp32 values with store32), info f64 [N,iters+1,4], system [N,27], centroid
    [N,3], residual [N,ht,wd,2] (NaN = does not contribute), jac [N,ht,wd,2,6], votes, flagged bool [N,ht,wd], bound_r, bound_J,
    weight, terms (all of the LAST evaluation), bound_sums [N,iters+1,32], nflag [N,iters+1], pose_bound, motion_bound, truth_bound,
    centroid_bound [N], same_start [N] bool (both sides evaluate the same fp32 A at the last evaluation), xi0 [N,6]."""
    poses = np.asarray(sc["poses"], np.float32)
    nf, ht, wd = sc["disps"].shape
    E, N = len(sc["ii"]), len(job_edge)
    out = dict(rel=np.tile(IDENTITY, (N, 1)), motion=np.tile(IDENTITY, (N, 1)), info=np.zeros((N, iters + 1, 4)), system=np.zeros((N, 27)),
               centroid=np.zeros((N, 3)), residual=np.full((N, ht, wd, 2), np.nan), jac=np.zeros((N, ht, wd, 2, 6)),
               votes=np.zeros((N, ht, wd), bool), flagged=np.zeros((N, ht, wd), bool), bound_r=np.zeros((N, ht, wd, 2)),
               bound_J=np.zeros((N, ht, wd, 2, 6)), weight=np.zeros((N, ht, wd)), terms=np.zeros((N, ht, wd, 32)),
               bound_sums=np.zeros((N, iters + 1, 32)), nflag=np.zeros((N, iters + 1), int), pose_bound=np.zeros(N),
               motion_bound=np.zeros(N), truth_bound=np.zeros(N), centroid_bound=np.zeros(N), same_start=np.zeros(N, bool),
               xi0=np.zeros((N, 6)), cond=np.zeros(N))
    for n in range(N):
        e, lab = int(job_edge[n]), int(job_label[n])
        i, j = (int(sc["ii"][e]), int(sc["jj"][e])) if 0 <= e < E else (-1, -1)
        if start is not None:
            out["rel"][n] = _f32(start[n], store32)
        if not (0 <= i < nf and 0 <= j < nf):
            out["info"][n, :, 3] = 4
            continue
        Gi, Gj = poses[i].astype(np.float64), poses[j].astype(np.float64)
        ti, tj = np.abs(Gi[:3]).sum(), np.abs(Gj[:3]).sum()
        A, drift, moved = out["rel"][n].copy(), 0.0, 0.0
        if start is None:
            A = _f32(pose_mul(Gj, pose_inv(Gi)), store32)
            drift = K_RETR * EPS * (1.0 + ti + tj)
        for it in range(iters + 1):
            ev = evaluate(sc, e, lab, A, z_min, huber, weight, mutant)
            xi, status, ainv = T.solve_step(ev["H"], ev["b"], ev["count"], lm, ep, min_count)
            if not store32 and status == 0:
                Ad = ev["H"] + np.diag(lm * np.diag(ev["H"]) + ep)
                xi = -np.linalg.solve(Ad, ev["b"])
            step = status == 0 and it < iters
            out["info"][n, it] = (ev["E"], ev["count"], np.abs(xi).max() if step else 0.0, status)
            out["bound_sums"][n, it] = ev["bound_sums"]
            # (E under a drift delta of A: dE = 2 b . delta + delta^T H delta, at most 2 |b|_1 |delta| + trace(H) |delta|^2; the second
            # term is the larger one where the residual is at rounding level, as on the plane)
            out["bound_sums"][n, it, 27] += 2 * np.abs(ev["b"]).sum() * drift + np.trace(ev["H"]) * drift ** 2
            out["nflag"][n, it] = ev["nflag"]
            own = float(np.linalg.norm(ainv @ (ev["E_b"] + ev["E_H"] @ np.abs(xi)) + EPS * np.abs(xi))) if status == 0 else 0.0
            if it == 0:
                out["xi0"][n] = xi
                with np.errstate(all="ignore"):
                    out["cond"][n] = np.linalg.cond(ev["H"]) if ev["count"] >= 6 else np.inf
            if step:
                moved = 2 * np.sqrt(6.0) * np.abs(xi).max()
                drift += own + K_RETR * EPS * (1.0 + np.abs(A[:3]).sum() + np.abs(xi).sum())
                A = _retract(xi, A, mutant == "right_retraction", store32)
        out["rel"][n] = A
        out["same_start"][n] = drift == 0.0
        out["system"][n] = ev["sums"][:27]
        out["residual"][n] = np.where(ev["votes"][..., None], ev["r"], np.nan)
        out["jac"][n] = np.where(ev["votes"][..., None, None], ev["J"], 0.0)
        for k in ("votes", "flagged", "bound_r", "bound_J", "weight", "terms"):
            out[k][n] = ev[k]
        fixed = own + moved + K_RETR * EPS * (1.0 + np.abs(A[:3]).sum())
        pb = min(drift, fixed) if status == 0 else drift
        out["pose_bound"][n] = pb
        reach = 1.0 + np.linalg.norm(Gj[:3])
        rounding = K_MOTION * EPS * (1.0 + ti + tj + np.abs(A[:3]).sum())
        out["motion_bound"][n] = reach * pb + rounding
        at_truth = float(np.linalg.norm(ainv @ ev["b_tgt"])) + moved if status == 0 else np.inf
        out["truth_bound"][n] = reach * (pb + at_truth) + rounding
        if mutant == "camera_motion":
            out["motion"][n] = pose_mul(pose_mul(A, Gi), pose_inv(Gj))
        else:
            out["motion"][n] = pose_mul(pose_inv(Gj), pose_mul(A, Gi))
        cnt, c = ev["count"], ev["sums"][29:32]
        if cnt > 0:
            mean = c / cnt
            out["centroid"][n] = R.rotation(pose_inv(Gi)[3:]) @ (mean - Gi[:3])
            # a flagged pixel may be in or out on the other side: its point moves the mean by at most (|X| + |mean|) / (count - nflag)
            Xf = np.abs(ev["terms"][..., 29:32]).reshape(-1, 3)[ev["flagged"].reshape(-1)].sum()
            fl = ev["nflag"] * (np.abs(mean).sum()) + Xf
            out["centroid_bound"][n] = (np.sqrt(3.0) * (ev["bound_sums"][29:32].max() + fl) / max(cnt - ev["nflag"], 1)
                                        + (K_RETR + 2) * EPS * (1.0 + ti + np.abs(mean).sum()))
    return out


# ------------------------------------------------------------------------------------------------------------ the checks
def motion_matches(got, ref):
    """the check of the tests.  got: dict of numpy rel, motion [N,7], info [N,iters+1,4] and optionally system, centroid, residual, jac
    of a solver run on the operands of `ref`.  On unflagged pixels of the jobs where both sides evaluate the same A: contributes / does
    not EQUAL, r and J within the bounds; per evaluation the status EQUAL, the count within the number of flagged pixels, E within its
    bound; rel within pose_bound, motion within motion_bound, centroid within centroid_bound; system within its bounds where both
    evaluate the same A.  Returns (ok, report)."""
    same = ref["same_start"]
    info = got["info"].astype(np.float64)
    st_ok = np.array_equal(info[..., 3], ref["info"][..., 3])
    c_ok = bool(np.all(np.abs(info[..., 1] - ref["info"][..., 1]) <= ref["nflag"]))
    E_err = np.abs(info[..., 0] - ref["info"][..., 0])
    E_bound = ref["bound_sums"][..., 27] + 2 * EPS * np.abs(ref["info"][..., 0])
    e_ok = bool(np.all(E_err <= E_bound))
    dist = np.array([pose_difference(a, b) for a, b in zip(got["rel"], ref["rel"])])
    p_ok = bool(np.all(dist <= ref["pose_bound"]))
    mdist = np.array([pose_difference(a, b) for a, b in zip(got["motion"], ref["motion"])])
    m_ok = bool(np.all(mdist <= ref["motion_bound"]))
    v_ok = s_ok = j_ok = y_ok = n_ok = True
    worst_r = worst_j = 0.0
    if got.get("residual") is not None:
        res = got["residual"].astype(np.float64)
        voted = ~np.isnan(res).any(-1)
        un = ~ref["flagged"] & same[:, None, None]
        v_ok = np.array_equal(voted[un], ref["votes"][un]) and np.array_equal(np.isnan(res[..., 0]), np.isnan(res[..., 1]))
        on = un & ref["votes"] & voted
        r_err = np.abs(np.where(on[..., None], res - np.where(ref["votes"][..., None], ref["residual"], 0), 0.0))
        s_ok = bool(np.all(r_err <= ref["bound_r"]))
        with np.errstate(all="ignore"):
            worst_r = float(np.nanmax(np.where(on[..., None] & (ref["bound_r"] > 0), r_err / ref["bound_r"], 0), initial=0.0))
        if got.get("jac") is not None:
            jac = got["jac"].astype(np.float64)
            v_ok = v_ok and not jac[~voted].any()
            j_err = np.abs(np.where(on[..., None, None], jac - ref["jac"], 0.0))
            j_ok = bool(np.all(j_err <= ref["bound_J"]))
            with np.errstate(all="ignore"):
                worst_j = float(np.nanmax(np.where(on[..., None, None] & (ref["bound_J"] > 0), j_err / ref["bound_J"], 0), initial=0.0))
    valid = ref["info"][:, -1, 3] != 4
    if got.get("system") is not None:
        still = same & valid
        y_ok = bool(np.all(np.abs(got["system"] - ref["system"])[still] <= ref["bound_sums"][:, -1, :27][still]))
        y_ok = y_ok and not np.asarray(got["system"])[~valid].any()
    cdist = np.zeros(len(same))
    if got.get("centroid") is not None:
        cdist = np.linalg.norm(got["centroid"].astype(np.float64) - ref["centroid"], axis=1)
        n_ok = bool(np.all(cdist <= ref["centroid_bound"]))
    report = ("votes %s, r %s (max err / bound %.3f), J %s (max err / bound %.3f), status %s, count %s, E %s (max err / bound %.3f), "
              "rel %s (max distance %.3e, bound %.3e), motion %s (max %.3e), system %s, centroid %s (max %.3e), flagged %.4f" % (
                  v_ok, s_ok, worst_r, j_ok, worst_j, st_ok, c_ok, e_ok, float(np.max(E_err / np.maximum(E_bound, 1e-300))),
                  p_ok, dist.max(initial=0.0), ref["pose_bound"].max(initial=0.0), m_ok, mdist.max(initial=0.0), y_ok, n_ok,
                  cdist.max(initial=0.0), ref["flagged"].mean() if ref["flagged"].size else 0.0))
    return bool(v_ok and s_ok and j_ok and st_ok and c_ok and e_ok and p_ok and m_ok and y_ok and n_ok), report


def gap(other, ref):
    """how far another solver's outputs are from `ref` in units of ref's bounds: the largest ratio over rel, motion, E, the count (its
    bound is the number of flagged pixels; a differing count with none flagged is infinitely far) and the status"""
    worst = 0.0
    with np.errstate(all="ignore"):
        for a, b, bound in zip(other["rel"], ref["rel"], ref["pose_bound"]):
            worst = max(worst, pose_difference(a, b) / max(bound, 1e-300))
        for a, b, bound in zip(other["motion"], ref["motion"], ref["motion_bound"]):
            worst = max(worst, pose_difference(a, b) / max(bound, 1e-300))
        E_bound = ref["bound_sums"][..., 27] + 2 * EPS * np.abs(ref["info"][..., 0])
        dE = np.abs(other["info"][..., 0] - ref["info"][..., 0])
        worst = max(worst, float(np.max(np.where(dE > 0, dE / np.maximum(E_bound, 1e-300), 0.0), initial=0.0)))
        dc = np.abs(other["info"][..., 1] - ref["info"][..., 1])
        worst = max(worst, float(np.max(np.where(dc > 0, dc / np.maximum(ref["nflag"], 1e-300), 0.0), initial=0.0)))
        if not np.array_equal(other["info"][..., 3], ref["info"][..., 3]):
            worst = np.inf
    return worst


def as_got(ref):
    """a reference's own outputs in the form motion_matches takes (for holding one reference against another)"""
    return dict(rel=ref["rel"], motion=ref["motion"], info=ref["info"].astype(np.float32), residual=ref["residual"].astype(np.float32),
                jac=ref["jac"].astype(np.float32), system=ref["system"], centroid=ref["centroid"])


def reduction_check(system, info_row, centroid, residual, jac, weight, X, pose_i, huber=0.0):
    """the reduction alone: H, b, E, count and the centroid from a solver's OWN residual [ht,wd,2] / jac [ht,wd,2,6] (fp32), the edge's
    weights [ht,wd] and the camera-i points X [ht,wd,3] (fp64, from the fp32 depths) against its system [27], info row and centroid.
    The terms are formed in fp64 from the fp32 r and J, so the bound is the terms' own roundings (K_TERM EPS |term|; a's K_A, k's 2 and
    rho's 2 for E; K_X for the points) plus the tree's TREE_DEPTH EPS sum |terms| and E's rounding to fp32; a pixel with |a - huber|
    within K_A EPS a counts with both branches of k; the count is exact.  Returns (ok, worst err / bound)."""
    r = np.asarray(residual, np.float32).astype(np.float64).reshape(-1, 2)
    J = np.asarray(jac, np.float32).astype(np.float64).reshape(-1, 2, 6)
    w = np.asarray(weight, np.float32).astype(np.float64).reshape(-1)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    v = ~np.isnan(r).any(1)
    r, J, w, X = r[v], J[v], w[v], X[v]
    a, h = np.sqrt((r * r).sum(1)), np.float64(np.float32(huber))
    with np.errstate(all="ignore"):
        quad = (h == 0) | (a <= h)
        near = (h > 0) & (np.abs(a - h) <= K_A * EPS * a)
        k = np.where(quad, 1.0, h / np.where(a > 0, a, 1.0))
        rho = np.where(quad, a * a, h * (2 * a - h))
        E_k = np.where(quad, 0.0, (K_A + 2) * EPS * k) + np.where(near, np.abs(1.0 - h / np.where(a > 0, a, 1.0)), 0.0)
        E_rho = (2 * K_A + 2) * EPS * np.abs(rho) + np.where(near, np.abs(a * a - h * (2 * a - h)), 0.0)
    wk = w * k
    aJ = np.abs(J)
    tH = np.stack([wk * (J[:, :, i] * J[:, :, j]).sum(1) for i, j in _IJ], 1)
    mH = np.stack([(aJ[:, :, i] * aJ[:, :, j]).sum(1) for i, j in _IJ], 1)
    tb = wk[:, None] * (J * r[:, :, None]).sum(1)
    mb = (aJ * np.abs(r)[:, :, None]).sum(1)
    terms = np.concatenate([tH, tb, (w * rho)[:, None]], 1)
    mag = np.concatenate([wk[:, None] * mH, wk[:, None] * mb, (w * rho)[:, None]], 1)
    own = np.concatenate([(K_TERM * EPS * wk + w * E_k)[:, None] * mH, (K_TERM * EPS * wk + w * E_k)[:, None] * mb,
                          (w * E_rho + EPS * w * rho)[:, None]], 1)
    want = terms.sum(0)
    bound = own.sum(0) + TREE_DEPTH * EPS * mag.sum(0)
    bound[27] += 2 * EPS * abs(want[27])
    err = np.abs(np.concatenate([np.asarray(system, np.float64), [np.float64(info_row[0])]]) - want)
    ok = bool(np.all(err <= bound)) and int(info_row[1]) == int(v.sum())
    with np.errstate(all="ignore"):
        worst = float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))
    cnt = int(v.sum())
    Gi = np.asarray(pose_i, np.float64)
    mean = X.sum(0) / cnt if cnt else np.zeros(3)
    cw = R.rotation(pose_inv(Gi)[3:]) @ (mean - Gi[:3]) if cnt else np.zeros(3)
    cb = ((K_X + TREE_DEPTH) * EPS * np.abs(X).sum() / max(cnt, 1) * np.sqrt(3.0) + (K_RETR + 2) * EPS * (1.0 + np.abs(Gi[:3]).sum() + np.abs(mean).sum())) if cnt else 0.0
    cerr = float(np.linalg.norm(np.asarray(centroid, np.float64) - cw))
    ok = ok and cerr <= cb
    if cb > 0:
        worst = max(worst, cerr / cb)
    return ok, worst
