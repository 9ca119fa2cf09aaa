"""The plain dense bundle adjustment (pvo_ba) against fp64: regimes, the reduced pose system and its error bound, admission of a case.

Everything the calibration tests' yardstick already has is reused from tests/calib_reference.py: the closed-form fp64 Jacobians
(`pixel_jacobians`), the fp64 assembly (`fields(..., assembly="fp64")`), the step (`step` with free_mask = 0 is the plain step), and
the comparison with a bound derived from the case's own sensitivity (`sensitivity`, `within`, `relchange`, `floors`).  Added here:

    regime_window      window_general's recipe with ONE property changed per regime (REGIMES), on any graph (GRAPHS)
    reduced_system     (S, rhs): the undamped A - E Q E^T and its right-hand side in fp64 - the first half of rgbd_reference.gn_step
    reduced_abs        the same sums with every addend replaced by its magnitude: T, what a summation error is relative to
    decode_sys         the device's 64-bit fixed-point system -> fp64
    sys_bound          (n_add + 16) 2^-24 T + n_fix 2^-29 per entry, n_add and n_fix read off pvo_amd/csrc/ba_assemble.h and ba_schur.h (see n_add) for the form
                       of pvo_ba_local's launch rule that the window reaches
    launch_form        that form, as a predicate over the graph (frame_rows, frame_paths): every GPU test asserts the one it claims
    case / admission   a (graph, regime, damping) triple with its fp64 step, s_case and the conditions it must meet to be used on the GPU
The sensor-depth prior and stereo edges ride on the same kernels: reduced_system, reduced_abs, sys_bound / n_add take the prior
(sens, alpha, prior=True), frame_blocks / frame_rows / fix_addends count a stereo edge's row block as ba_schur_body does - every one of
them is what it was for a window without either.  Their windows, fields, mutations and cases are tests/ba_rider_reference.py's.

ADMISSION (tests/test_ba_fp64_host.py asserts it for every name in ADMITTED, tests/test_ba_fp64_gpu.py runs exactly those):
  * 4 s_case <= 2e-3 for dx and for dz - the cap of tests/test_ba_calib_gpu.py; a case this sensitive is replaced, not loosened;
  * in `behind` no pixel of any edge has fp64 |Z - MIN_DEPTH| < 1e-3, so that the fp32 and the fp64 mask coincide (the generator
    nudges the starting disparities until the count is 0);
  * the fp32 restatement (fields(..., assembly="oracle") -> step) lies within HALF of the bound 4 s_case + floors, and its reduced
    system within sys_bound of the fp64 one - room for a device that sums in another order.

Regimes and cases LEFT OUT, by that rule or by the issue's trials (no cap is raised for any of them):
  * a far scene (disparities ~0.01): s_case(dz) = 0 under the floor while the fp32 restatement is above it - no bound to hold to;
  * fx = 725 / 8 on a 9 x 12 map (a 7 degree field of view): s_case(dx) = 4e-3;
  * the S-A sized window (10 x 30 x 101, radius 3): s_case(dx) = 1.0e-3, four times that misses the cap;
  * `light` (weights and eta x 2^-10) under either damping: the reduced entries (7e-2) lie under ep, s_case(dz) = 0 under the
    floor, and the fp32 restatement uses 0.97 - 0.99 of the bound where half is allowed;
  * `behind` on the one-chain (32 frames), global-memory (64) and blocked (40, radius 6) graphs: s_case(dx) >= 5.4e-4, 1.4e-3 and
    1.5e-3 over the seeds tried (1..30, 1..9, 1..9) - the backward chain's scale is barely held; `behind` runs on the dense solve
    at 5 and 29 free poses and on the partitioned one (seeds 8 and 27 of the 29- and 39-pose chains, the ones that meet the cap);
  * `control` under the GLOBAL damping at 29 / 31 / 39 free poses (s_case(dx) 5.7e-4, 2.0e-3, 5.2e-4) and on the blocked graph
    (6.4e-4): those run under (1e-4, 0.1); the global damping is held on the tiny windows, at 5 poses, at 63 poses and at S-B size;
  * `behind` at S-B size: s_case(dx) = 9e-3;
  * `behind` under the GLOBAL damping (tiny window and 5 poses): it meets the cap, but the mutation lm = 0 stays inside the bound
    (0.6 and 0.3 of it) - steps of 0.7 on which lm = 1e-5 cannot be seen; `behind` runs under (1e-4, 0.1);
  * two chained `behind` steps at seed 7: the chain's s_case(dx) = 1.1e-3; seed 9 of the same window meets the cap (3.7e-4) and
    keeps every pixel 2.7e-3 away from the mask after the first step."""
import numpy as np

import calib_reference as C
from oracle import oracle as O

DAMPINGS = {"local": (1e-4, 0.1), "global": (1e-5, 1e-2)}      # the frontend's and the global BA's (factor_graph.py: lm=1e-5, ep=1e-2)
CAP = 2e-3
NEAR = 1e-3

# regime -> the motion between frames (None: GENERAL_XI); the other changes are in regime_window
REGIMES = {
    "control": None,
    "rotation_only": (1e-3, 5e-4, 1e-3, 0.02, 0.03, 0.01),      # Jz is tiny: Q ~ 1 / eta
    "big_rotation": (0.05, 0.02, 0.02, 0.1, 0.25, 0.15),        # steps of ~0.4
    "sideways": (0.3, 0.1, 0.0, 0.0, 0.02, 0.0),
    "behind": (0.0, 0.0, -0.35, 0.0, 0.0, 0.0),                 # ground-truth disparities 0.5 - 2.5: some Z < MIN_DEPTH
    "sparse_weights": None,                                     # half the weights exactly 0, a quarter x 1e-3
    "eta_wide": None,                                           # eta = 10^U(-6, 0) per pixel
    "heavy": None,                                              # weights and eta x 2^26
    "light": None,                                              # weights and eta x 2^-10
}


CLOSURE_WEIGHT = 0.2


def _closures(far):
    far = list(far)
    return [1] * len(far) + far, far + [1] * len(far)


# graph -> regime_window's shape arguments; the sizes at which pvo_ba_finish picks each solve form (solve_form, ba.hip) are the ones
# tests/test_geom_ba_gpu.py reaches them with
GRAPHS = {
    "tiny": dict(F=6, ht=9, wd=12, radius=2),
    "hw264": dict(F=6, ht=12, wd=22, radius=2),                 # a partial second chunk
    "hw273": dict(F=6, ht=13, wd=21, radius=2),                 # HW & 3 != 0
    "dense5": dict(F=6, ht=8, wd=10, radius=2),                 # dense matrix-core solve, 5 free poses
    "dense29": dict(F=30, ht=8, wd=10, radius=2),               # ... and its limit, 29
    "chain31": dict(F=32, ht=8, wd=10, radius=2, closures=_closures(range(18, 31))),      # a separator too wide: one chain
    "twin39": dict(F=40, ht=8, wd=10, radius=2),                # partitioned
    "gmem63": dict(F=64, ht=8, wd=10, radius=2, closures=_closures(range(52, 62))),       # envelope beyond LDS: global memory
    "blocked39": dict(F=40, ht=8, wd=10, radius=6),             # E > 8 P: dense in 48 x 48 blocks
    "sb": dict(F=8, ht=48, wd=64, radius=3),                    # S-B: 36 edges
    # `behind` on a long chain: the seeds (of 1..30 tried) at which the window meets the cap
    "dense29_s8": dict(F=30, ht=8, wd=10, radius=2, seed=8),
    "twin39_s27": dict(F=40, ht=8, wd=10, radius=2, seed=27),
    "tiny_s9": dict(F=6, ht=9, wd=12, radius=2, seed=9),        # `behind`, two chained steps: the seed (of 1..24) whose chain meets the cap
    # The windows that reach every form of pvo_ba_local's launch rule (launch_form below; LAUNCH_FORMS names the form each claims), the
    # smallest that do.  What decides a frame's branch is its ROW count - 6 per distinct free neighbour and its own pose, + 1 - so a
    # radius-2 graph (31 rows, two row tiles) reaches schur_pass only, at any chunk size: staging starts at 65 rows, radius 5.
    # Maps of ~1600 pixels under one fixed frame miss the cap whatever the seed (F=30, t0=1, radius 5, 32 x 49 and 33 x 47: 4 s_case(dx)
    # = 5.2e-3 .. 7.4e-3 over seeds 1..8; seed moves it by a third, the number of fixed frames by a factor of four), so the dense
    # windows keep frames in front of the window fixed: t0 = 2 (win29 1.52e-3 at seed 7, 1.48e-3 at seed 4; win29_odd 1.62e-3, 1.52e-3),
    # t0 = 3 for the wide window (mixed26: 2.9e-3 at t0 = 1, 2.5e-3 at 2, 1.35e-3 at 3).  `behind` on win29: 4 s_case(dx) = 0.15 .. 1.2
    # over seeds 1..8 - no seed comes near the cap; it stays with the windows listed above.
    "win29": dict(F=31, ht=32, wd=49, radius=5, t0=2),          # 7 chunks x 30 = 210 workgroups, P = 29: 19 frames of 67 rows staged, 12 on schur_pass
    "win29_odd": dict(F=31, ht=33, wd=47, radius=5, t0=2),      # HW = 1551, HW & 3 != 0: the non-vector loads of the same form
    # 20 free poses behind 10 fixed frames, 10 chunks x 21; frame 0 - ten frames in front of t0, beyond the 8 staging slots - sees 11
    # free poses (67 rows): it fits the LDS but has no slot, schur_rowpass_lds straight into the system, beside 10 staged frames
    "front10": dict(F=30, ht=48, wd=49, radius=5, t0=10, closures=([0] * 11, list(range(10, 21)))),
    # 8 chunks x 26; radius 9: 9 middle frames hold 109 - 115 rows, too many for the LDS segment (107), and stream; 14 are staged
    "mixed26": dict(F=28, ht=36, wd=50, radius=9, t0=3),
    # 7 chunks x 31 = 217 workgroups, P = 30: 512-pixel chunks, 1568 = 3 x 512 + 32 leaves a partial last chunk; radius 5: 20 frames of
    # five row tiles on schur_rowpass over the four z-slices, 11 on schur_pass.  Seed 7 meets the cap (1.86e-3)
    "c512": dict(F=31, ht=32, wd=49, radius=5),
    "c512_odd": dict(F=31, ht=33, wd=47, radius=5, seed=4),     # the non-vector variant; seed 4 (1.73e-3; seed 7: 1.91e-3, 1, 2, 3, 5: 2.05e-3 .. 2.7e-3)
    # 17 chunks x 64 = 1088 workgroups: 1024-pixel chunks (4160 = 4 x 1024 + 64).  63 free poses on maps of 4160 pixels are ~50 times
    # stiffer than gmem63's against the same ep, and the chain's far end floats: 4 s_case(dx) = 6.5e-3 (local) / 6.6e-2 (global) at
    # weight 1, whatever the seed (1..8), t0 (2, 3, 5: 5.5e-3 .. 6.1e-3), radius (1: 7.9e-3, 3: 8.3e-3) or closures (7.5e-3 .. 1.1e-2).
    # Weights and eta x 2^-8 put the entries where gmem63's are (1.81e-3; 2^-7: 2.7e-3, 2^-6: 3.7e-3), and gmem63's closures bring frame 1
    # to 13 row blocks - five row tiles: schur_rowpass at 1024 pixels beside schur_pass - at 1.53e-3
    "c1024": dict(F=64, ht=64, wd=65, radius=2, closures=_closures(range(52, 62)), scale=2.0 ** -8),
}
# graph -> the form of the launch rule its tests claim (asserted against launch_form before anything runs on the GPU)
LAUNCH_FORMS = {"tiny": "fused256", "hw264": "fused256", "hw273": "fused256", "sb": "fused256", "blocked39": "fused256",
                "win29": "window_staged", "win29_odd": "window_staged", "front10": "window_direct", "mixed26": "window_mixed",
                "c512": "chunk512", "c512_odd": "chunk512", "c1024": "chunk1024"}


def regime_window(name, seed=7, F=6, ht=9, wd=12, radius=2, t0=1, closures=None, scale=None):
    """calib_reference.window_general's recipe (the same draws in the same order: `control` IS window_general) with the one change
    the regime names; closures = (ii, jj) appends edges to the radius graph, with CLOSURE_WEIGHT of the recipe's weight (the
    loop-closure edges of tests/test_geom_ba_gpu.py carry 0.2 rand: a wide-baseline edge at full weight makes the window's step
    too sensitive to admit, s_case(dx) = 1.9e-3 at 32 frames); scale: weights and eta times it (a power of two).  Same dict."""
    import torch
    import rgbd_reference as R
    from pvo_amd.geom.se3 import SE3
    g = torch.Generator().manual_seed(seed)
    intr = torch.tensor([wd * 0.625, wd * 0.7, wd / 2.0 - 0.3, ht / 2.0 + 0.4])
    xi = torch.tensor(REGIMES[name] or C.GENERAL_XI)
    poses_gt = torch.stack([SE3.exp(k * xi).data for k in range(F)], 0)
    lo, span = (0.5, 2.0) if name == "behind" else (0.2, 0.8)
    low = torch.rand(1, 1, 6, 8, generator=g) * span + lo
    disps_gt = torch.nn.functional.interpolate(low, size=(ht, wd), mode="bilinear", align_corners=True)[0, 0][None].repeat(F, 1, 1)
    ii, jj = R.radius_graph(F, radius)
    if closures is not None:
        ii, jj = np.concatenate([ii, np.asarray(closures[0], np.int64)]), np.concatenate([jj, np.asarray(closures[1], np.int64)])
    ii, jj = torch.as_tensor(ii), torch.as_tensor(jj)
    E = ii.shape[0]
    c, _ = O.reproject(poses_gt.numpy(), disps_gt.numpy(), intr[None].repeat(F, 1).numpy(), ii.numpy(), jj.numpy())
    target = torch.from_numpy(c) + 0.1 * torch.randn(E, ht, wd, 2, generator=g)
    weight = torch.rand(E, ht, wd, 2, generator=g) + 0.5
    poses0 = torch.stack([poses_gt[max(k - 1, 0)] for k in range(F)], 0)
    disps0 = torch.ones(F, ht, wd) + 0.2 * torch.rand(F, ht, wd, generator=g)
    K = int(np.unique(np.concatenate([np.arange(t0, F), ii.numpy()])).shape[0])
    eta = torch.full((K, ht, wd), 1e-4) + 0.01 * torch.rand(K, ht, wd, generator=g)
    # the regime's own draws come after the recipe's
    if name == "sparse_weights":
        u = torch.rand(E, ht, wd, 2, generator=g)
        weight = torch.where(u < 0.5, torch.zeros_like(weight), torch.where(u < 0.75, weight * 1e-3, weight))
    if name == "eta_wide":
        eta = 10.0 ** (-6.0 * torch.rand(K, ht, wd, generator=g))
    if closures is not None:
        weight[E - len(closures[0]):] *= CLOSURE_WEIGHT
    if name in ("heavy", "light") or scale is not None:
        k = scale if scale is not None else (2.0 ** 26 if name == "heavy" else 2.0 ** -10)
        weight, eta = weight * k, eta * k
    s = dict(intr=intr, poses=poses0, disps=disps0, target=target.permute(0, 3, 1, 2).contiguous(),
             weight=weight.permute(0, 3, 1, 2).contiguous(), eta=eta, ii=ii.contiguous(), jj=jj.contiguous(), t0=t0, t1=F)
    # no pixel on the fence between the fp32 and the fp64 mask: in `behind`, and wherever a long loop-closure edge looks backwards
    # (a window without such pixels - every tiny regime but `behind` - is left as drawn)
    for _ in range(64):
        near = np.abs(edge_depths(s) - C.MIN_DEPTH) < NEAR
        if not near.any():
            break
        d = s["disps"].reshape(F, -1)
        for e, x in zip(*np.nonzero(near)):
            d[int(ii[e]), int(x)] += 2.0 ** -6
    assert near_count(s) == 0
    return s


def edge_depths(s):
    """Z of every edge's pixels in the target frame, fp64 from the stored fp32 operands [E,HW] (pixel_jacobians' expression)"""
    a = C.scene_args(s)
    poses, disps = a[0].astype(np.float64), a[1].astype(np.float64)
    fx, fy, cx, cy = (float(v) for v in a[2].astype(np.float64))
    F, ht, wd = disps.shape
    v_, u_ = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
    px, py = (u_.reshape(-1) - cx) / fx, (v_.reshape(-1) - cy) / fy
    Z = np.zeros((len(a[6]), ht * wd))
    for e, (i, j) in enumerate(zip(a[6], a[7])):
        Rm, t = C.rel_pose(poses[int(i)], poses[int(j)])
        Z[e] = Rm[2, 0] * px + Rm[2, 1] * py + Rm[2, 2] + disps[int(i)].reshape(-1) * t[2]
    return Z


def near_count(s):
    return int((np.abs(edge_depths(s) - C.MIN_DEPTH) < NEAR).sum())


def masked_fraction(s):
    return float((edge_depths(s) < C.MIN_DEPTH).mean())


# ------------------------------------------------------------------------------------------------ the reduced system
def _reduce(f, eta, ii, jj, t0, t1, magnitudes=False, q_from=None, stats=None, sens=None, alpha=C.ALPHA, disps=None):
    """calib_reference.step up to its damping line -> (A [6P,6P], b [6P]).  magnitudes: the fields are sums of magnitudes and the
    Schur part is ADDED (every addend of A - E Q E^T by its absolute value); q_from: the Cii that Q is formed from.
    sens, alpha, disps: the sensor-depth prior (calib_reference.prior_terms); under `magnitudes` its addend joins w by its magnitude"""
    ii, jj = np.asarray(ii, np.int64), np.asarray(jj, np.int64)
    Hs, vs, Eii, Eij, Cii, bz = (f[k] for k in C.FIELDS[:6])
    HW, E, P = Cii.shape[1], ii.shape[0], t1 - t0
    n6 = 6 * P
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
    kidx = {int(fr): k for k, fr in enumerate(kx)}
    Cq = Cii if q_from is None else q_from
    Cs, w, Ei = np.zeros((K, HW)), np.zeros((K, HW)), np.zeros((P, 6, HW))
    for e in range(E):
        k = kidx[int(ii[e])]
        Cs[k] += Cq[e]; w[k] += bz[e]
        if 0 <= int(ii[e]) - t0 < P:
            Ei[int(ii[e]) - t0] += Eii[e]
    eta = np.asarray(eta, np.float64).reshape(-1, HW)
    add = np.broadcast_to(eta, (K, HW)).copy() if eta.shape[0] == 1 else eta.copy()
    assert add.shape == (K, HW)
    if sens is not None:
        add, w2 = C.prior_terms(add, w, disps, kx, np.bincount(ii, minlength=np.asarray(disps).shape[0])[kx], sens, alpha)
        w = w + np.abs(w2 - w) if magnitudes else w2
    Q = 1.0 / (Cs + add)
    rows = [[] for _ in range(K)]
    for p in range(P):
        rows[kidx[t0 + p]].append((p, Ei[p]))
    for e in range(E):
        rows[kidx[int(ii[e])]].append((int(jj[e]) - t0, Eij[e]))
    sign = 1.0 if magnitudes else -1.0
    if stats is not None:
        stats["largest"] = max(float(np.abs(Hs).max()), float(np.abs(vs).max()))
    for k in range(K):
        live = [(p, M) for p, M in rows[k] if 0 <= p < P]
        if not live:
            continue
        M = np.concatenate([m_ for _, m_ in live], 0)
        S = (M * Q[k]) @ M.T
        v = M @ (Q[k] * w[k])
        if stats is not None:                                                  # (a frame's Schur sums: no chunk's addend is larger while HW <= 256)
            stats["largest"] = max(stats.get("largest", 0.0), float(np.abs(S).max()), float(np.abs(v).max()))
        for x, (pa, _) in enumerate(live):
            b[blk(pa)] += sign * v[6 * x:6 * x + 6]
            for y, (pb, _) in enumerate(live):
                A[blk(pa), blk(pb)] += sign * S[6 * x:6 * x + 6, 6 * y:6 * y + 6]
    return A, b


def reduced_system(f, s, stats=None, sens=None, alpha=C.ALPHA):
    """(S [6P,6P], rhs [6P]) of the window `s` from the assembled fields `f`: the undamped A - E Q E^T and v - E Q w in fp64.
    stats (a dict) receives "largest": the largest magnitude of one fixed-point addend (an edge's pose sums, a frame's Schur sums);
    sens, alpha: the sensor-depth prior, as calib_reference.step's"""
    a = C.scene_args(s)
    return _reduce(f, a[5], a[6], a[7], a[8], a[9], stats=stats, sens=sens, alpha=alpha, disps=a[1])


def reduced_abs(f, s, sens=None, alpha=C.ALPHA, mags=None):
    """T = (T_S, T_rhs): reduced_system's sums with every addend replaced by its absolute value, for the pose part (per edge,
    residual row and pixel: |w Ja Jb|, |w r Ja|) and the Schur part (|E| Q |E|^T and |E| Q |w| with |E|, |w| the per-frame sums of
    per-row magnitudes |w Jz J|, |w r Jz|; Q itself, a sum of non-negative terms, is the one of `f`).
    sens, alpha: the sensor-depth prior - |alpha (d - s)| joins |w|; mags: the magnitude fields, where abs_fields' are not the window's
    (tests/ba_rider_reference.py: a stereo edge's)"""
    a = C.scene_args(s)
    m = abs_fields(s) if mags is None else mags
    return _reduce(m, a[5], a[6], a[7], a[8], a[9], magnitudes=True, q_from=f["Cii"], sens=sens, alpha=alpha, disps=a[1])


def abs_fields(s):
    """the assembled fields of the window with every per-pixel addend replaced by its magnitude (reduced_abs)"""
    a = C.scene_args(s)
    J = C.pixel_jacobians(a[0], a[1], a[2], a[3], a[4], a[6], a[7])
    w, r, Ji, Jj, Jz = J["w"], np.abs(J["r"]), np.abs(J["Ji"]), np.abs(J["Jj"]), np.abs(J["Jz"])
    es = lambda spec, *ops: np.einsum(spec, *ops, optimize=True)
    return dict(Hs=np.stack([es("ecx,ecax,ecbx->eab", w, A, B) for A, B in ((Ji, Ji), (Ji, Jj), (Jj, Ji), (Jj, Jj))]),
                vs=np.stack([es("ecx,ecx,ecax->ea", w, r, A) for A in (Ji, Jj)]),
                Eii=es("ecx,ecx,ecax->eax", w, Jz, Ji), Eij=es("ecx,ecx,ecax->eax", w, Jz, Jj),
                Cii=es("ecx,ecx,ecx->ex", w, Jz, Jz), bz=es("ecx,ecx,ecx->ex", w, r, Jz))


def block_support(s):
    """[P,P] bool, lower block triangle: the 6 x 6 blocks of the reduced system some addend reaches - the diagonal, the pose pairs an
    edge joins, and the pairs of poses that meet in one depth frame's rows (the frame's own pose and its out-edges' targets)"""
    ii, jj, t0, t1 = s["ii"].numpy(), s["jj"].numpy(), s["t0"], s["t1"]
    P = t1 - t0
    sup = np.eye(P, dtype=bool)
    by_frame = {}
    for i, j in zip(ii, jj):
        by_frame.setdefault(int(i), {int(i) - t0}).add(int(j) - t0)
    for ps in by_frame.values():
        ps = [p for p in ps if 0 <= p < P]
        for a in ps:
            for b in ps:
                sup[max(a, b), min(a, b)] = True
    return sup


def fix_addends(s):
    """n_fix per block (S [P,P]) and per pose (rhs [P]): the fixed-point addends behind an entry - one per edge that reaches it (the
    assembly's chunk sums are added in fp64 and quantised once per edge, the deal rows of ba_schur_body: `val += part[...]` in double,
    then __double2ll_rn) and, per depth frame whose rows hold both poses, what frame_paths counts for the frame's path: one per pixel
    chunk of the launch's size (256, 512 or 1024: every chunk's tile-pair sum goes through scatter_tile's fix_add, in schur_pass,
    schur_rowpass and schur_rowpass_lds without part_out alike), or ONE for a staged frame - its chunks' fp32 sums are added in fp64
    by ba_schur_reduce_kernel (`v += static_cast<double>(a[u])`: exact to 2^-53, nothing at the 2^-24 scale of the bound) and that
    sum is quantised once.  Per PAIR OF ROW BLOCKS (frame_blocks): beyond 64 out-edges nothing is merged, and an entry of block
    (a, b) gets one addend per pair of row blocks that map to a and to b.
    A STEREO edge under a baseline is NO addend, in either part: ba_assemble_kernel writes its `part` slab as 0.0f, the deal rows add
    the zeros in double and __double2ll_rn(0.0 * kFix) is the integer 0 - added, but exact; and every tile pair that one of its zero
    Eij rows enters is a chain of fp32 products with an exact 0 operand, +0 or -0, whose negation scatter_tile quantises to 0."""
    ii, jj, t0, t1 = s["ii"].numpy(), s["jj"].numpy(), s["t0"], s["t1"]
    P = t1 - t0
    stereo = float(s.get("baseline", 0.0)) > 0
    paths = frame_paths(s)
    nS, nr = np.zeros((P, P)), np.zeros(P)
    for i, j in zip(ii, jj):
        pi, pj = int(i) - t0, int(j) - t0
        if stereo and pi == pj:
            continue
        for p in (pi, pj):
            if 0 <= p < P:
                nS[p, p] += 1; nr[p] += 1
        if 0 <= pi < P and 0 <= pj < P:
            nS[max(pi, pj), min(pi, pj)] += 1
    for fr, blocks in frame_blocks(s).items():
        mult = {}
        for p, zero in blocks:
            if not zero:
                mult[p] = mult.get(p, 0) + 1
        chunks = paths[fr][2]
        assert chunks > 0 or not blocks
        for a in mult:
            nr[a] += chunks * mult[a]
            for b in mult:
                if a >= b:
                    nS[a, b] += chunks * mult[a] * mult[b]
    return nS, nr


# ------------------------------------------------------------------------------------------------ the launch rule
# pvo_ba_local's size rules (ba.hip, "pixels per workgroup" down to the Schur launch) and ba_schur_body's per-frame branches, restated
# as predicates over the GRAPH: every GPU test asserts the form it claims before it runs, so a rule change fails the test instead of
# moving it onto another kernel.  The constants, by their names in ba_schur.h, ba_workspace.h and ba.hip:
FAST_TILES = 4            # kFastTiles: up to 4 row tiles (64 rows) take schur_pass, all tile pairs in one pass
STAGE_PAIRS = 36          # kSchurStagePairs: tile pairs a staged frame may have (8 row tiles)
STAGE_FRONT = 8           # kSchurStageFront: the frames in front of t0 that have a staging slot (schur_stage_slot)
ROWS_LDS_FLOATS = 110 * 1024 // 4      # kSchurRowsLds: the dynamic LDS of the dense-window form
LDS_ROW_PAD = 4           # kLdsRowPad
DENSE_MAX_POSES = 29      # kDenseMaxPoses
FORM_NAMES = ("fused256", "window_staged", "window_mixed", "window_direct", "chunk512", "chunk1024")


BALLOT_EDGES = 64         # ba_schur_body builds the row table by ballot (and merges edges that share a target) up to 64 out-edges


def frame_blocks(s):
    """depth frame -> the 6-row blocks of its M in ba_schur_body's row table (ba_schur.h, `if (in_lds && deg_all <= 64)` down to
    `nrows_s = r` of the sequential walk), as a list of (window pose, zero): the frame's own pose first if it is free (kRowEi), then
      up to 64 out-edges (the ballot path)   one block per DISTINCT free target pose, in the order of each target's first edge: edges
                                             that share a target are led by the first and read their summed rows from Mrg (s_merged);
      beyond (the sequential walk)           one block per out-edge with a free target, nothing merged.
    A STEREO edge (i, i) has s_pose = jj[e] - t0 = pself: the frame's own pose is its target, so with pself free it is a leader like
    any other and adds a SECOND block of six rows whose rowout entries are the own-pose block's, 6 pself + n - six more rows for the
    frame, which can carry it over a row tile onto another path.  zero: the block's rows are exact zeros - a stereo edge's Eij under a
    baseline (s["baseline"] > 0; ba_assemble_kernel stores 0.0f).  Only another stereo edge of the same frame shares that target: the
    two merge into one block (0 + 0 in Mrg).  Without a baseline an edge (i, i) is an identity edge with rows of its own, not zero."""
    ii, jj, t0, t1 = s["ii"].numpy(), s["jj"].numpy(), s["t0"], s["t1"]
    stereo = float(s.get("baseline", 0.0)) > 0
    out = {}
    for fr in np.unique(np.concatenate([np.arange(t0, t1), ii])):
        fr = int(fr)
        tg = [int(j) for i, j in zip(ii, jj) if int(i) == fr and t0 <= int(j) < t1]
        if len([1 for i in ii if int(i) == fr]) <= BALLOT_EDGES:
            tg = list(dict.fromkeys(tg))
        blocks = [(fr - t0, False)] if t0 <= fr < t1 else []
        out[fr] = blocks + [(j - t0, stereo and j == fr) for j in tg]
    return out


def frame_rows(s):
    """depth frame -> rows of its M in ba_schur_body's row table: 6 per block of frame_blocks - its own pose if that is free, each
    DISTINCT free target pose of its out-edges (every such edge beyond 64 out-edges), a stereo edge's target, the frame's own pose,
    among them - and the w row if there is any row at all"""
    return {fr: (6 * len(b) + 1 if b else 0) for fr, b in frame_blocks(s).items()}


def frame_paths(s):
    """depth frame -> (path, chunk, n_fix): which branch of ba_schur_body sums the frame's tile pairs, the pixels per workgroup, and the
    fixed-point addends the frame puts behind one entry.  Paths:
      "none"    no rows (a source frame in front of the window whose targets are all fixed);
      "pass"    T = ceil(rows / 16) <= kFastTiles: schur_pass, one addend per chunk;
      "staged"  dense window, T > kFastTiles, the frame's rows fit the dynamic LDS (rows (256 + kLdsRowPad) + 256 <= kSchurRowsLds / 4,
                that is rows <= 107; T (T + 1) / 2 <= kSchurStagePairs then holds by itself: T <= 7) and the frame has a staging slot
                (t0 - kSchurStageFront <= frame < t1): schur_rowpass_lds -> spart -> ba_schur_reduce_kernel, ONE addend per frame;
      "lds"     the same without a slot: schur_rowpass_lds straight into the system, one addend per chunk;
      "stream"  T > kFastTiles otherwise: schur_rowpass from global memory (in a dense window: rows > 107), one addend per chunk"""
    F, ht, wd = s["disps"].shape
    t0, t1 = s["t0"], s["t1"]
    P, HW = t1 - t0, ht * wd
    wg = ((HW + 255) // 256) * min(F, P + 1)
    dense = P <= DENSE_MAX_POSES and wg > 192
    pix = 256 if (wg <= 192 or dense) else (512 if wg <= 1024 else 1024)
    chunks = (HW + pix - 1) // pix
    out = {}
    for fr, rows in frame_rows(s).items():
        T = (rows + 15) // 16
        if rows == 0:
            out[fr] = ("none", pix, 0)
        elif T <= FAST_TILES:
            out[fr] = ("pass", pix, chunks)
        elif dense and rows * (256 + LDS_ROW_PAD) + 256 <= ROWS_LDS_FLOATS:
            assert T * (T + 1) // 2 <= STAGE_PAIRS
            slot = t0 - STAGE_FRONT <= fr < t1
            out[fr] = ("staged", pix, 1) if slot else ("lds", pix, chunks)
        else:
            out[fr] = ("stream", pix, chunks)
    return out


def launch_form(s):
    """the form of pvo_ba_local's Schur launch the window reaches, one of FORM_NAMES.  With chunks = ceil(HW / 256), frames = min(F, P + 1),
    wg = chunks * frames (the rule reads the map size and the pose window only):
      fused256        wg <= 192: 256-pixel chunks, the depth phase fused into the Schur kernel, four z-slices;
      a dense window  wg > 192 and P <= 29: 256-pixel chunks, ONE slice, ba_depth_kernel in front, the dynamic LDS segment, and per frame
                      (frame_paths) staged | lds | stream | pass.  Named by what its frames of more than kFastTiles row tiles do:
        window_staged   all of them are staged (and there is one);
        window_mixed    some are staged and some too wide for the LDS stream their rows: both in one launch;
        window_direct   some are staged and some - more than kSchurStageFront frames in front of t0 - go from LDS straight to the system;
      chunk512        P > 29, 192 < wg <= 1024: 512-pixel chunks, depth kernel in front, four z-slices;
      chunk1024       P > 29, wg > 1024."""
    F, ht, wd = s["disps"].shape
    P, HW = s["t1"] - s["t0"], ht * wd
    wg = ((HW + 255) // 256) * min(F, P + 1)
    if wg <= 192:
        return "fused256"
    if P > DENSE_MAX_POSES:
        return "chunk512" if wg <= 1024 else "chunk1024"
    kinds = {p for p, _, _ in frame_paths(s).values()}
    if "staged" not in kinds:
        return "window_unstaged"      # (no test claims it: a dense window none of whose frames has more than four row tiles)
    if "lds" in kinds:
        return "window_direct"
    return "window_mixed" if "stream" in kinds else "window_staged"


def max_out_degree(s):
    return int(np.bincount(s["ii"].numpy()).max())


# fp32 additions behind one fixed-point addend, read off pvo_amd/csrc/ba_workspace.h and ba_schur.h:
ASSEMBLE_CHUNK = 512      # kChunkA = 256 kPPT, kPPT = 2 pixels per thread (ba_workspace.h)
SCHUR_CHUNK = 256         # kSchurPix (ba_schur.h); pvo_ba_local keeps 256-pixel chunks while (HW / 256) (P + 1) <= 192, and in a dense window


def schur_chunk(s):
    """pixels per workgroup of the window's Schur launch (pvo_ba_local's `pix`): 256, 512 or 1024"""
    return next(iter(frame_paths(s).values()))[1]


def n_add(deg, pix=SCHUR_CHUNK, prior=False):
    """the longest chain of fp32 additions behind one fixed-point addend, for a window whose frames have at most `deg` out-edges and
    whose Schur launch takes `pix` pixels per workgroup (the functions named are those the 256-pixel form was first derived from; the
    other forms are read off the same functions):
      pose part   2 kPPT = 4 per thread (two pixels, rows u and v: pixel_terms, ba_assemble.h) + 6 steps of the wave's reduce-scatter
                  + 2 across the four waves (both in ba_assemble_kernel) = 12; the chunks of an edge are then added in fp64
                  (the deal rows of ba_schur_body, ba_schur.h);
      Schur part  64 per wave - a quarter of a 256-pixel chunk, 16 MFMAs of K = 4 (schur_pass, ba_schur.h) - + 2 across the waves
                  (schur_pass's end) = 66, on operands that are sums over the frame's out-edges themselves: Ei on either side, or w
                  (deg - 1 each, depth_pixel in ba_schur.h), C + eta (deg, depth_pixel), the division and the product E Q (2).
      512 / 1024  schur_pass<T, VEC4, PIX> and schur_rowpass<CNT, VEC4, PIX> are templates over the chunk: a wave owns PIX / 4 pixels
                  (pix_base = blockIdx.x PIX + wave PIX / 4) and walks them in PIX / 64 steps of four MFMAs of K = 4 - one product per pixel
                  added to the accumulator, a chain of PIX / 4 = 128 / 256 - then the same (w0 + w1) + (w2 + w3) across the waves:
                  PIX / 4 + 2.  The z-slices of the 512 / 1024 grids deal whole ROW TILES over workgroups (ti by the snake in
                  ba_schur_body); every tile pair is still one workgroup's chain, so they add nothing.  The operands are those of the
                  256-pixel form: ba_depth_kernel runs depth_pixel itself.
      dense window   schur_rowpass_lds<CNT, 256>: the same chain from LDS, 64 + 2 per chunk; a staged frame's chunk sums then meet in
                  fp64 (ba_schur_reduce_kernel), which lengthens no fp32 chain - see fix_addends for what it does to n_fix.
      the prior   (prior=True) depth_pixel's `wp = pr.alpha * (disps[fx] - s)` and `ww - wp`: the product and the subtraction from w,
                  2 more on the w operand (a fused multiply-add would make them 1).  The difference d - s itself is exact where
                  s / 2 <= d <= 2 s (Sterbenz), which tests/ba_rider_reference.py's sensor maps hold by construction (s within 10 %
                  of d) and assert.  C + (m ? alpha : eta) is the same one addition.
      stereo      a stereo edge (i, i) is one of the frame's out-edges: `deg` counts it (max_out_degree does), its Cii and bz are one
                  more addend of C and w each.  stereo_pixel_terms (ba_assemble.h) forms them as pixel_terms does - wu Jz Jz, then
                  `cii += wv * Jz * Jz` - so the per-pixel products stay under the same 16 units; its Eii / Eij are stored zeros."""
    return max(12, pix // 4 + 2 + 2 * (deg - 1) + deg + 2 + (2 if prior else 0))


def sys_bound(s, T, prior=False):
    """per entry of (S, rhs): (n_add + 16) 2^-24 T + n_fix 2^-29.  16 units cover the per-pixel products - the 2^-20 relative
    perturbation s_case is defined with; 2^-29 is half a unit of the 2^-28 fixed-point grid (fix_add, ba_workspace.h).
    prior: T holds the sensor-depth prior's addend (reduced_abs with sens) and n_add its roundings"""
    TS, Tr = T
    nS, nr = fix_addends(s)
    k = (n_add(max_out_degree(s), schur_chunk(s), prior) + 16) * 2.0 ** -24
    return k * TS + np.kron(nS, np.ones((6, 6))) * 2.0 ** -29, k * Tr + np.repeat(nr, 6) * 2.0 ** -29


def decode_sys(sys, P):
    """the device's fixed-point system, int64 [(6P)^2 + 6P] (row-major S, then rhs; units of 2^-28) -> (S [6P,6P], rhs [6P]) in fp64.
    Only the LOWER BLOCK TRIANGLE of `sys` is ever written - confirmed in the code: pose_block_scatter adds an edge's (i, j) block at
    (max, min) only (ba_assemble.h) and scatter_tile keeps an entry only if its block row is not above its block column
    (ba_schur.h); inside a diagonal block both triangles are written.  So S is read from the lower block triangle and mirrored;
    the words above it are not read here: tests/test_ba_fp64_gpu.py asserts that they are 0."""
    v = np.asarray(sys.cpu().numpy() if hasattr(sys, "cpu") else sys, np.int64)
    n6 = 6 * P
    S = v[:n6 * n6].astype(np.float64).reshape(n6, n6) * 2.0 ** -28
    low = np.kron(np.tril(np.ones((P, P))), np.ones((6, 6))) > 0
    strict = np.kron(np.tril(np.ones((P, P)), -1), np.ones((6, 6))) > 0
    L = np.where(low, S, 0.0)
    return L + np.where(strict, S, 0.0).T, v[n6 * n6:n6 * n6 + n6].astype(np.float64) * 2.0 ** -28


def lower_blocks(P):
    """[6P,6P] bool: the entries of the lower block triangle"""
    return np.kron(np.tril(np.ones((P, P))), np.ones((6, 6))) > 0


# ------------------------------------------------------------------------------------------------ cases
_windows, _cases = {}, {}


def window_of(graph, regime):
    """-> (window, fp64 fields); built once, shared, never modified"""
    if (graph, regime) not in _windows:
        s = regime_window(regime, **GRAPHS[graph])
        a = C.scene_args(s)
        _windows[(graph, regime)] = (s, C.fields(a[0], a[1], a[2], a[3], a[4], a[6], a[7], assembly="fp64"))
    return _windows[(graph, regime)]


def case(graph, regime, damping):
    """-> dict(s, f [fp64 fields], base [the fp64 step], sc [s_case], lm, ep); once per triple"""
    key = (graph, regime, damping)
    if key not in _cases:
        s, f = window_of(graph, regime)
        lm, ep = DAMPINGS[damping]
        base = C.scene_step(s, lm, ep, 0.1, 0, f)
        _cases[key] = dict(s=s, f=f, base=base, sc=C.sensitivity(s, base, f, lm, ep, 0.1, 0), lm=lm, ep=ep)
    return _cases[key]


def share(name, got, c, frac=1.0):
    """-> (inside, share): `got` against the case's fp64 step on dx or dz, unit by unit, within frac (4 s_case + floors); share = the
    largest |difference| / bound over the units"""
    base, rel = c["base"][name], 4 * c["sc"][name]
    intr = c["s"]["intr"].numpy()
    if not np.isfinite(np.asarray(got, np.float64)).all():
        return False, float("inf")
    a, b = C.units(name, got), C.units(name, base)
    d, m, fl = np.abs(a - b).max(1), np.abs(b).max(1), C.floors(name, base, intr)
    bound = rel * m + fl
    ok, _ = C.within(name, got, base, rel, intr)
    sh = float((d / np.where(bound > 0, bound, 1.0)).max())
    return bool(ok and np.all(d <= frac * bound)), sh


def restatement(c):
    """the fp32 restatement's step for the case: fields(..., assembly="oracle") -> step"""
    a = C.scene_args(c["s"])
    f = C.fields(a[0], a[1], a[2], a[3], a[4], a[6], a[7], assembly="oracle")
    return f, C.scene_step(c["s"], c["lm"], c["ep"], 0.1, 0, f)


def mutations(c):
    """name -> the fp64 step of a deliberately wrong variant of the case, each of a kind the 1e-4 tolerance of the fp32 oracle tests
    lets through: Eij x 1.001, the ij blocks of Hs x 1.001 (Hs[1] and its mirror Hs[2]), lm = 0, the last pixel of Cii / bz zeroed"""
    s, f, lm, ep = c["s"], c["f"], c["lm"], c["ep"]
    step = lambda g, lm_=lm: C.scene_step(s, lm_, ep, 0.1, 0, g)
    Hs = f["Hs"].copy()
    Hs[1] *= 1.001
    Hs[2] = np.swapaxes(Hs[1], 1, 2)
    Cz, bz = f["Cii"].copy(), f["bz"].copy()
    Cz[:, -1], bz[:, -1] = 0.0, 0.0
    return dict(Eij=step(dict(f, Eij=f["Eij"] * 1.001)), Hs_ij=step(dict(f, Hs=Hs)), lm0=step(f, 0.0), last_pixel=step(dict(f, Cii=Cz, bz=bz)))


def unmasked_step(c):
    """the case's step with MIN_DEPTH disabled: every pixel counts, whatever its Z"""
    a = C.scene_args(c["s"])
    keep = C.MIN_DEPTH
    C.MIN_DEPTH = -np.inf
    try:
        f = C.fields(a[0], a[1], a[2], a[3], a[4], a[6], a[7], assembly="fp64")
    finally:
        C.MIN_DEPTH = keep
    return C.scene_step(c["s"], c["lm"], c["ep"], 0.1, 0, f)


_chains = {}


def chain(graph, regime, damping, iters=2):
    """`iters` chained fp64 steps (poses and depths pass through fp32 between them, as the device's do) with the chain's own
    sensitivity: every step's fields perturbed, four seeded draws -> case's dict"""
    key = (graph, regime, damping, iters)
    if key not in _chains:
        s, _ = window_of(graph, regime)
        a = C.scene_args(s)
        lm, ep = DAMPINGS[damping]
        base = C.ba_calib(*a, iters, lm, ep, 0.1, 0, assembly="fp64")
        sc = dict(dx=0.0, dz=0.0)
        for seed in (0, 10, 20, 30):
            r = C.ba_calib(*a, iters, lm, ep, 0.1, 0, perturb_seed=seed, assembly="fp64")
            for k in sc:
                sc[k] = max(sc[k], C.relchange(k, r[k], base[k], a[2]))
        mid = C.ba_calib(*a, iters - 1, lm, ep, 0.1, 0, assembly="fp64")      # the state the last step starts from
        import torch
        near = near_count(dict(s, poses=torch.from_numpy(mid["poses"]), disps=torch.from_numpy(mid["disps"])))
        _chains[key] = dict(s=s, base=base, sc=sc, lm=lm, ep=ep, near_mid=near)
    return _chains[key]


FIX_LIMIT = 3.0e10      # fix_add's range check per addend (ba_workspace.h); the sums live in int64 units of 2^-28: |sum| < 2^35


def overflow_window():
    """the `control` window with weights and eta times 2^k, k chosen BY THE REFERENCE such that the largest fp64 diagonal entry of S
    lies in [2^35, 2^36) - beyond what the fixed-point sum can hold - while every single addend stays below fix_add's limit
    -> (window, k, largest diagonal entry, largest addend)"""
    for k in range(20, 40):
        s = regime_window("control", scale=2.0 ** k, **GRAPHS["tiny"])
        a = C.scene_args(s)
        st = {}
        S, _ = reduced_system(C.fields(a[0], a[1], a[2], a[3], a[4], a[6], a[7], assembly="fp64"), s, st)
        d = float(np.diag(S).max())
        if 2.0 ** 35 <= d < 2.0 ** 36:
            assert st["largest"] < FIX_LIMIT
            return s, k, d, st["largest"]
    raise AssertionError("no scale puts the diagonal into [2^35, 2^36)")


# ------------------------------------------------------------------------------------------------ what runs on the GPU
# (graph, regime, damping) triples that meet the admission rule; tests/test_ba_fp64_host.py asserts it for every one of them.
TINY = [("tiny", r, d) for r in REGIMES if r != "light" for d in DAMPINGS if (r, d) != ("behind", "global")]
SHAPES = [(g, "control", d) for g in ("hw264", "hw273") for d in DAMPINGS]
# cut C under every solve form, at the graph that selects it (GRAPHS): the global BA's damping where the case meets the cap under it
FORMS = [("dense5", "control", "global"), ("dense5", "behind", "local"),
         ("dense29", "control", "local"), ("dense29_s8", "behind", "local"),
         ("chain31", "control", "local"),
         ("twin39", "control", "local"), ("twin39_s27", "behind", "local"),
         ("gmem63", "control", "global"),
         ("blocked39", "control", "local"),
         ("sb", "control", "global")]
# ... and under every form of the launch rule (LAUNCH_FORMS): cut A and cut C
LAUNCHES = [(g, "control", "local") for g in ("win29", "win29_odd", "front10", "mixed26", "c512", "c512_odd", "c1024")]
ADMITTED = TINY + SHAPES + FORMS + LAUNCHES
TWO_STEPS = [("tiny", "control", "local"), ("tiny_s9", "behind", "local")]
