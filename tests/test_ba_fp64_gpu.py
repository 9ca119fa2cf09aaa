"""The plain dense bundle adjustment on the GPU (pvo_ba and its split entry points) against fp64 - tests/ba_reference.py on top of
tests/calib_reference.py, qualified and admitted case by case in tests/test_ba_fp64_host.py.  Three cuts and the failure contract:

  A  the reduced system   ba_plan + ba_local -> the 64-bit fixed-point `sys`, entry by entry within the summation bound
                          (n_add + 16) 2^-24 T + n_fix 2^-29 of ba_reference.sys_bound; exact zeros outside the structural support;
  B  the solve alone      ba_finish(motion_only) on a hand-written, badly scaled `sys` under every solve form: within the rounding of
                          the fp32 output plus Higham's forward bound for a Cholesky solve, at condition numbers up to ~1e8;
  C  the whole step       db.ba: dx per pose and dz per depth frame within 4 s_case + floors of the fp64 step (calib_reference.within),
                          every regime under both dampings, every solve form, S-B size, two chained steps;
  the failure contract    include/pvo_hip.h under pvo_ba: a poisoned operand is a status and a zero pose update, never a wrong one.

Nothing here compares the device with itself, except the two repeatability assertions (a second ba_local, a call after a rejected
one).  Every test prints the device's share of its bound (profiles/r15_ba_fp64.txt;
profiles/r23_ba_launch_forms.txt for the windows of ba_reference.LAUNCHES, one per form of pvo_ba_local's launch rule - each of them
asserts the form it claims before it runs)."""
import ctypes

import numpy as np
import pytest
import torch

import ba_reference as B
import calib_reference as C
from oracle import oracle as O

pytestmark = pytest.mark.gpu

_id = lambda t: "-".join(t)


def _operands(s, cuda, **over):
    d = lambda t: t.to(cuda).contiguous().clone()
    return dict(poses=d(s["poses"]), disps=d(s["disps"]), intr=d(s["intr"]), target=d(over.get("target", s["target"])),
                weight=d(over.get("weight", s["weight"])), eta=d(over.get("eta", s["eta"])), ii=d(s["ii"]), jj=d(s["jj"]))


def _ba(o, s, iters, lm, ep):
    """db.ba on the operands `o` (poses and disps are updated in place) -> (dx, dz, status)"""
    from pvo_amd import droid_backends as db
    st = torch.full((4,), -1, dtype=torch.int32, device=o["disps"].device)
    dx, dz = db.ba(o["poses"], o["disps"], o["intr"], o["target"], o["weight"], o["eta"], o["ii"], o["jj"], s["t0"], s["t1"], iters, lm, ep, False,
                   status=st)
    return dx, dz, st


def _ba_on(ws, o, s, iters, lm, ep):
    """pvo_ba on a workspace of the caller's (db.ba runs on one cached per device) -> (dx, dz, status)"""
    from pvo_amd import _lib, droid_backends as db
    F, ht, wd = o["disps"].shape
    dev = o["disps"].device
    K, P = o["eta"].shape[0], s["t1"] - s["t0"]
    dx = torch.zeros(P, 6, device=dev)
    dz = torch.zeros(K, ht * wd, device=dev)
    st = torch.full((4,), -1, dtype=torch.int32, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        db.check(_lib.load().pvo_ba(p(o["poses"]), p(o["disps"]), p(o["intr"]), p(o["target"]), p(o["weight"]), p(o["eta"]), p(o["ii"]), p(o["jj"]),
                                    o["ii"].shape[0], F, ht, wd, K, s["t0"], s["t1"], iters, lm, ep, 0, p(dx), p(dz), K, p(st), p(ws), ws.numel(),
                                    ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ba")
    return dx, dz, st


def _workspace(s, cuda):
    from pvo_amd import droid_backends as db
    F, ht, wd = s["disps"].shape
    return db.ba_workspace(s["ii"].shape[0], s["t1"] - s["t0"], F, ht * wd, cuda)


n64 = lambda t: t.detach().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ A: the reduced system
_CUT_A = sorted({(g, r) for g, r, _ in B.TINY + B.SHAPES}) + [(g, r) for g, r, _ in B.LAUNCHES]      # the 256-pixel fused form, then every other


@pytest.mark.parametrize("graph,regime", _CUT_A, ids=["-".join(k) for k in _CUT_A])
def test_reduced_system_matches_fp64_within_the_summation_bound(cuda, graph, regime):
    from pvo_amd import droid_backends as db
    s, f = B.window_of(graph, regime)
    F, ht, wd = s["disps"].shape
    P, HW = s["t1"] - s["t0"], ht * wd
    form = B.launch_form(s)
    assert form == B.LAUNCH_FORMS[graph]                                       # the form n_add and fix_addends count for (ba_reference.frame_paths)
    S, rhs = B.reduced_system(f, s)
    bS, br = B.sys_bound(s, B.reduced_abs(f, s))
    o = _operands(s, cuda)
    ws = _workspace(s, cuda)
    n6 = 6 * P
    words = []
    for _ in range(2):                                                         # the second on a zeroed sys: the same int64 words
        sysw = torch.zeros(n6 * n6 + n6, dtype=torch.int64, device=cuda)
        db.ba_plan(o["ii"], o["jj"], F, HW, o["eta"].shape[0], s["t0"], s["t1"], ws)
        db.ba_local(o["poses"], o["disps"], o["intr"], o["target"], o["weight"], o["eta"], o["ii"], o["jj"], s["t0"], s["t1"], False, sysw, ws)
        words.append(sysw.cpu().numpy())
    assert np.array_equal(words[0], words[1])
    raw = words[0][:n6 * n6].reshape(n6, n6)
    low = B.lower_blocks(P)
    sup = np.kron(B.block_support(s), np.ones((6, 6))) > 0
    assert not raw[~low].any()                                                 # only the lower block triangle is ever written
    assert not raw[low & ~sup].any()                                           # ... and of it only the structural support
    Sd, rd = B.decode_sys(words[0], P)
    eS, er = np.abs(Sd - S), np.abs(rd - rhs)
    sel = low & sup
    sh_S, sh_r = float((eS[sel] / bS[sel]).max()), float((er / br).max())
    print("%s-%s [%s]: reduced system, device's share of the bound S %.3f rhs %.3f (largest entry %.2e)" % (graph, regime, form, sh_S, sh_r, np.abs(S).max()))
    assert np.all(eS[sel] <= bS[sel]) and np.all(er <= br)
    assert raw[sel].any() and np.abs(Sd).max() > 0.5 * np.abs(S).max()


# ------------------------------------------------------------------------------------------------ B: the solve alone
# graph -> the partition ba_last_partition must report (None: the dense solve keeps none)
_SOLVE_FORMS = {"dense5": None, "dense29": None, "chain31": "one chain", "twin39": "split", "gmem63": "one chain", "blocked39": "one chain"}
_scaled = {}


def _scaled_system(graph, target, damping):
    """D S D of the graph's `control` system, D = diag(d0 10^(a u + shift)), u uniform in [-1, 1], with a (or, where Jacobi's scaling d0
    - a diagonal of 100 - is already worse conditioned than asked, the common shift towards the damping's ep I) bisected until the
    DAMPED matrix has a 2-norm condition number of about `target`; quantised to the 2^-28 grid, so that both sides read the same
    numbers -> (int64 words, damped matrix, rhs, kappa)"""
    key = (graph, target, damping)
    if key in _scaled:
        return _scaled[key]
    s, f = B.window_of(graph, "control")
    if graph not in _scaled:
        _scaled[graph] = B.reduced_system(f, s)
    S, rhs = _scaled[graph]
    n = S.shape[0]
    lm, ep = (float(np.float32(v)) for v in B.DAMPINGS[damping])               # the device widens its float arguments
    d0 = 10.0 / np.sqrt(np.diag(S))
    u = np.random.default_rng(n + int(np.log10(target))).uniform(-1.0, 1.0, n)

    def build(a, shift):
        D = d0 * 10.0 ** (a * u + shift)
        M = np.rint((D[:, None] * S * D[None, :]) * 2.0 ** 28) * 2.0 ** -28
        M = np.tril(M) + np.tril(M, -1).T
        Md = M.copy()
        v = np.diag(M)
        Md[np.diag_indices(n)] = v + (ep + lm * v)                               # ba_prepare_kernel's expression (ba_solve.h)
        ev = np.linalg.eigvalsh(Md)
        return M, Md, np.rint(D * rhs * 2.0 ** 28) * 2.0 ** -28, float(ev[-1] / ev[0])
    if build(0.0, 0.0)[3] < target:                                            # spread the scales until the target is reached
        lo, hi = 0.0, 5.0
        for _ in range(12):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if build(mid, 0.0)[3] < target else (lo, mid)
        M, Md, b, kappa = build(lo, 0.0)
    else:                                                                      # no diagonal scaling conditions it better than Jacobi's: shrink D
        lo, hi = -4.0, 0.0                                                     # as a whole, towards the damping's ep I
        for _ in range(12):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if build(0.0, mid)[3] < target else (lo, mid)
        M, Md, b, kappa = build(0.0, lo)
    assert np.abs(M).max() < 2.0 ** 34 and np.abs(b).max() < 2.0 ** 34
    low = B.lower_blocks(n // 6)
    words = np.concatenate([np.where(low, M * 2.0 ** 28, 0.0).reshape(-1), b * 2.0 ** 28]).astype(np.int64)
    _scaled[key] = (words, Md, b, kappa)
    return _scaled[key]


@pytest.mark.parametrize("damping", sorted(B.DAMPINGS))
@pytest.mark.parametrize("graph", sorted(_SOLVE_FORMS))
def test_pose_solve_alone_matches_an_fp64_cholesky_at_every_conditioning(cuda, graph, damping):
    """|dx - x| per pose <= 2^-23 max|x_pose| + (3 n + 1) 2^-53 kappa_2 |x|_2: the rounding of the fp32 output (twice half a unit) plus
    the forward error of a Cholesky solve - Higham, Accuracy and Stability of Numerical Algorithms (2nd ed.), Theorem 10.4: the
    computed solution solves (A + dA) x = b with |dA| <= gamma_(3n+1) |R^T| |R|, so |x^ - x| / |x| <~ gamma_(3n+1) kappa_2 with
    | |R^T| |R| | taken as |A| (eq. 10.7 bounds it by n |A|, attained for no matrix of this kind).  kappa_2 from numpy on the damped
    matrix.  The reference is numpy's Cholesky in fp64, itself checked against its residual in long double."""
    from pvo_amd import droid_backends as db
    s, _ = B.window_of(graph, "control")
    F, ht, wd = s["disps"].shape
    P, HW, E = s["t1"] - s["t0"], ht * wd, s["ii"].shape[0]
    n = 6 * P
    lm, ep = B.DAMPINGS[damping]
    ii, jj = s["ii"].to(cuda), s["jj"].to(cuda)
    ws = _workspace(s, cuda)
    db.ba_plan(ii, jj, F, HW, 1, s["t0"], s["t1"], ws)
    for target in (1e2, 1e5, 1e8):
        words, Md, b, kappa = _scaled_system(graph, target, damping)
        L = np.linalg.cholesky(Md)
        x = np.linalg.solve(L.T, np.linalg.solve(L, b))
        ld = np.longdouble
        res = b.astype(ld) - Md.astype(ld) @ x.astype(ld)
        assert float(np.abs(res).max()) <= (3 * n + 1) * 2.0 ** -53 * float((np.abs(Md) @ np.abs(x)).max()) * n
        sysw = torch.from_numpy(words).to(cuda)
        poses, disps = s["poses"].to(cuda).clone(), s["disps"].to(cuda).clone()
        st = torch.full((4,), -1, dtype=torch.int32, device=cuda)
        dx, _ = db.ba_finish(poses, disps, sysw, ii, jj, s["t0"], s["t1"], lm, ep, True, ws, status=st)
        assert int(st[0]) == 0 and not bool(sysw.any())                          # accepted; sys is left zeroed for the next step
        got, want = n64(dx), x.reshape(P, 6)
        bound = 2.0 ** -23 * np.abs(want).max(1) + (3 * n + 1) * 2.0 ** -53 * kappa * np.linalg.norm(x)
        err = np.abs(got - want).max(1)
        print("%s %s: kappa %.1e (asked %.0e), device's share of the bound %.3f (fp32 part alone: %.3f)" % (
            graph, damping, kappa, target, float((err / bound).max()), float((err / (2.0 ** -23 * np.abs(want).max(1))).max())))
        assert np.all(err <= bound) and np.isfinite(got).all()
        assert torch.equal(disps, s["disps"].to(cuda))                           # motion only
        want_form = _SOLVE_FORMS[graph]
        if want_form is not None:
            m, sp = db.ba_last_partition(E, P, F, HW, cuda, workspace=ws)
            assert (m > 0 and sp > m) if want_form == "split" else (m, sp) == (0, 0)
    assert (P <= 29) == (_SOLVE_FORMS[graph] is None) and (E > 8 * P) == (graph == "blocked39")      # solve_form's rule (ba.hip)


# ------------------------------------------------------------------------------------------------ C: the whole step
def _assert_step(name, c, dx, dz, st):
    s, base = c["s"], c["base"]
    assert st.tolist() == [0, len(base["kx"]), 0, 0]
    ok_x, sh_x = B.share("dx", n64(dx), c)
    ok_z, sh_z = B.share("dz", n64(dz), c)
    print("%s: s_case dx %.2e dz %.2e; device's share of the bound dx %.3f dz %.3f" % (name, c["sc"]["dx"], c["sc"]["dz"], sh_x, sh_z))
    assert 4 * max(c["sc"]["dx"], c["sc"]["dz"]) <= B.CAP
    assert ok_x and ok_z


@pytest.mark.parametrize("key", B.TINY + B.FORMS + B.LAUNCHES, ids=_id)
def test_one_step_matches_the_fp64_step_within_its_own_sensitivity(cuda, key):
    c = B.case(*key)
    s, base = c["s"], c["base"]
    if key in B.LAUNCHES:
        assert B.launch_form(s) == B.LAUNCH_FORMS[key[0]]
    o = _operands(s, cuda)
    dx, dz, st = _ba(o, s, 1, c["lm"], c["ep"])
    _assert_step(_id(key), c, dx, dz, st)
    # the retraction: depths += dz on the rows of kx, poses by the pose retraction of the device's own dx
    F = s["disps"].shape[0]
    kx = torch.from_numpy(base["kx"]).to(cuda)
    d0 = s["disps"].to(cuda).reshape(F, -1)[kx]
    # (disps + Q (...) may be one fused multiply-add: against fl(d0 + fl(dz)) that is half a unit of dz and half a unit of the sum on
    # one side, half a unit of the sum on the other - under 2^-22 of the largest of the three, pixel by pixel; dz reaches 4 d0 here)
    d1 = o["disps"].reshape(F, -1)[kx]
    assert bool(((d1 - (d0 + dz)).abs() <= 2.0 ** -22 * torch.maximum(torch.maximum(d0.abs(), dz.abs()), d1.abs())).all())
    assert float((d1 - d0).abs().max()) > 1e-3
    want = O.pose_retr(s["poses"].numpy(), dx.cpu().numpy(), s["t0"], s["t1"])
    assert np.abs(o["poses"].cpu().numpy() - want).max() <= 4e-6               # (the oracle's retraction of the device's dx: fp32 rounding)
    if key[0].startswith("twin39"):
        from pvo_amd import droid_backends as db
        ht, wd = s["disps"].shape[1:]
        m, sp = db.ba_last_partition(s["ii"].shape[0], s["t1"] - s["t0"], F, ht * wd, cuda)
        assert m > 0 and sp > m


@pytest.mark.parametrize("key", B.TWO_STEPS, ids=_id)
def test_two_iterations_match_two_chained_fp64_steps(cuda, key):
    c = B.chain(*key)
    o = _operands(c["s"], cuda)
    dx, dz, st = _ba(o, c["s"], 2, c["lm"], c["ep"])
    _assert_step(_id(key) + " x2", c, dx, dz, st)


# ------------------------------------------------------------------------------------------------ the failure contract
_EDGE, _PIX = 9, 40      # the poisoned edge of the tiny window (3 -> 1: its source frame lies inside the window) and its pixel


def _poisoned(s, kind):
    e = _EDGE if s["ii"].shape[0] < 30 else int(torch.nonzero(s["ii"] == 20)[0])
    tg, wt = s["target"].clone(), s["weight"].clone()
    E, _, ht, wd = tg.shape
    if kind == "nan_target":
        tg.view(E, 2, -1)[e, 0, _PIX] = float("nan")
    elif kind == "inf_weight":
        wt.view(E, 2, -1)[e, 1, _PIX] = float("inf")
    else:                                                                      # finite: 1e-3 x 1e20 x J^2 is an addend beyond 3e10
        wt.view(E, 2, -1)[e, 0, _PIX] = 1e20
    return e, tg, wt


@pytest.mark.parametrize("kind", ["nan_target", "inf_weight", "huge_weight"])
def test_a_poisoned_operand_is_a_status_a_zero_pose_update_and_a_depth_only_step(cuda, kind):
    """include/pvo_hip.h, pvo_ba: the pose step is rejected (status[0] = 1, dx = 0, poses keep their bytes) and the depths take the
    step of dx = 0, dz = Q w - finite on every frame whose own out-edges are clean, and there the fp64 Q w within its rounding error:
    w = sum over the frame's deg out-edges and both residual rows of wgt r Jz, with r = target - proj a DIFFERENCE of fp32 numbers
    of the size of the image (16 units of |target| + |proj| for the projection's arithmetic, beside (deg + 16) units of |r| for the
    products and the sum), and (deg + 18) units of the result for C, the division and the product:
        2^-24 (Q sum wgt |Jz| ((deg + 16) |r| + 16 (|proj| + |target|)) + (deg + 18) |Q w|).
    The fp32 restatement (the oracle's assembly) uses 0.47 of it, the device 0.65 (profiles/r15_ba_fp64.txt)."""
    c = B.case("tiny", "control", "local")
    s, f = c["s"], c["f"]
    e, tg, wt = _poisoned(s, kind)
    o = _operands(s, cuda, target=tg, weight=wt)
    dx, dz, st = _ba(o, s, 1, c["lm"], c["ep"])
    K = len(c["base"]["kx"])
    assert st.tolist() == [1, K, 0, 0]
    assert not bool(dx.any()) and torch.equal(o["poses"], s["poses"].to(cuda))
    src = int(s["ii"][e])
    kx = c["base"]["kx"]
    clean = np.array([int(fr) != src for fr in kx])
    F, ht, wd = s["disps"].shape
    got = n64(dz)
    assert np.isfinite(got[clean]).all() and bool(torch.isfinite(o["disps"][torch.from_numpy(kx[clean]).to(cuda)]).all())
    pix = np.arange(ht * wd) != _PIX
    assert np.isfinite(got[~clean][:, pix]).all()                              # ... and the poisoned frame's other pixels
    # the depth-only step on the clean frames against fp64
    ii = s["ii"].numpy()
    a = C.scene_args(s)
    J = C.pixel_jacobians(a[0], a[1], a[2], a[3], a[4], a[6], a[7])
    tgt = np.asarray(a[3], np.float64).reshape(len(ii), 2, -1)
    eta = s["eta"].numpy().astype(np.float64).reshape(K, -1)
    worst = 0.0
    for k, fr in enumerate(kx):
        if not clean[k]:
            continue
        es = np.nonzero(ii == fr)[0]
        deg = len(es)
        Q = 1.0 / (f["Cii"][es].sum(0) + eta[k])
        ref = Q * f["bz"][es].sum(0)
        wj = J["w"][es] * np.abs(J["Jz"][es])
        bound = 2.0 ** -24 * (Q * (wj * ((deg + 16) * np.abs(J["r"][es]) + 16 * (np.abs(J["proj"][es]) + np.abs(tgt[es])))).sum((0, 1))
                              + (deg + 18) * np.abs(ref))
        err = np.abs(got[k] - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound)
        assert float(np.abs(ref).max()) > 1e-3                                 # (a step, not a zero)
    print("%s: status %s; depth-only step on the clean frames, device's share of the bound %.3f" % (kind, st.tolist(), worst))
    d0 = s["disps"].to(cuda).reshape(F, -1)
    sel = torch.from_numpy(kx[clean]).to(cuda)
    assert float((o["disps"].reshape(F, -1)[sel] - (d0[sel] + dz[torch.from_numpy(np.nonzero(clean)[0]).to(cuda)])).abs().max()) <= 2.0 ** -22 * float(d0.max())


@pytest.mark.parametrize("graph", ["tiny", "twin39"])
def test_the_call_after_a_rejected_one_returns_the_bytes_of_a_fresh_workspace(cuda, graph):
    """meta[4] and `sys` are left clean: a short window (the dense solve) and 39 free poses (the envelope solve's loaders)"""
    c = B.case(graph, "control", "local")
    s = c["s"]
    _, tg, _ = _poisoned(s, "nan_target")
    used, fresh = _workspace(s, cuda), _workspace(s, cuda)
    bad = _operands(s, cuda, target=tg)
    _, _, st = _ba_on(used, bad, s, 2, c["lm"], c["ep"])
    assert int(st[0]) == 1
    outs = []
    for ws in (used, fresh):
        o = _operands(s, cuda)
        dx, dz, st = _ba_on(ws, o, s, 2, c["lm"], c["ep"])
        assert st.tolist() == [0, len(c["base"]["kx"]), 0, 0]
        outs.append((o["poses"], o["disps"], dx, dz))
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and bool(outs[0][2].any())


def test_a_rejected_step_leaves_the_planned_workspace_clean_for_the_chained_next_step(cuda):
    """the split entry points as the frontend chains them: ba_local(sys_is_zero=True) after a ba_finish that rejected its step, on the
    SAME plan - no ba_plan in between resets meta[4], no memset clears sys"""
    from pvo_amd import droid_backends as db
    c = B.case("tiny", "control", "local")
    s = c["s"]
    F, ht, wd = s["disps"].shape
    P, HW, K = s["t1"] - s["t0"], ht * wd, len(c["base"]["kx"])
    _, tg, _ = _poisoned(s, "nan_target")

    def step(o, sysw, ws, clean):
        st = torch.full((4,), -1, dtype=torch.int32, device=cuda)
        db.ba_local(o["poses"], o["disps"], o["intr"], o["target"], o["weight"], o["eta"], o["ii"], o["jj"], s["t0"], s["t1"], False, sysw, ws,
                    sys_is_zero=clean)
        dx, dz = db.ba_finish(o["poses"], o["disps"], sysw, o["ii"], o["jj"], s["t0"], s["t1"], c["lm"], c["ep"], False, ws, dz_rows=K, status=st)
        return dx, dz, st

    outs = []
    for poison_first in (True, False):
        ws = _workspace(s, cuda)
        sysw = torch.zeros((6 * P) ** 2 + 6 * P, dtype=torch.int64, device=cuda)
        o = _operands(s, cuda)
        db.ba_plan(o["ii"], o["jj"], F, HW, K, s["t0"], s["t1"], ws)
        if poison_first:
            _, _, st = step(_operands(s, cuda, target=tg), sysw, ws, True)
            assert int(st[0]) == 1 and not bool(sysw.any())
        dx, dz, st = step(o, sysw, ws, True)
        assert int(st[1]) == K and int(st[2]) == 0
        outs.append((o["poses"], o["disps"], dx, dz))
    assert all(torch.equal(a, b) for a, b in zip(*outs)) and bool(outs[0][2].any())
    ok_x, sh_x = B.share("dx", n64(outs[0][2]), c)
    assert ok_x


def test_a_sum_beyond_the_fixed_point_range_is_a_status_never_a_wrong_step(cuda):
    """weights and eta scaled until the fp64 diagonal of S reaches [2^35, 2^36) with every addend below fix_add's 3e10: no addend is
    flagged, the 64-bit sum wraps.  The device must report it (status[0] = 1, zero update) - it must never return status 0 with a step
    outside the bound of the fp64 step"""
    s, k, d, largest = B.overflow_window()
    o = _operands(s, cuda)
    lm, ep = B.DAMPINGS["local"]
    dx, dz, st = _ba(o, s, 1, lm, ep)
    print("overflow zone (x 2^%d, diagonal %.3e, largest addend %.3e): status %s, max |dx| %.3e" % (k, d, largest, st.tolist(), float(dx.abs().max())))
    assert int(st[0]) == 1
    assert not bool(dx.any()) and torch.equal(o["poses"], s["poses"].to(cuda))
