"""Online intrinsics calibration on the GPU (pvo_ba_calib) against the tests' own fp64 yardstick (tests/calib_reference.py, qualified
in tests/test_ba_calib_host.py).

Tolerance: the method of tests/test_ba_sigma_gpu.py, not a fixed number.  Per case the yardstick's assembled fields - the border's
Hci, Hcj, Hcc, vc, gc included - are perturbed by independent relative 2^-20 u, u in [-1, 1], with four seeded draws; s_case is the
largest relative change of dx, of dc and of dz, each separately; the device must be within 4 s_case of the unperturbed yardstick on
that quantity, and a case is only admitted with 4 s_case <= 2e-3.  The comparison (calib_reference.relchange / within) is
|a - b| <= rel |b| + floor per UNIT: dc per component, dx per pose (its 6-vector on its own largest entry), dz per depth frame (the
map on its own largest entry) - inside a pose or a map the entries change sign and cross 0.  Floors: dc[n] 2^-24 |c[n]|, half a unit
in the last place of the fp32 parameter it is added to; dx and dz 2^-20 of the quantity's largest magnitude, the size of the
perturbation itself.

Shapes: the smallest that reach each path - see _CASES."""
import ctypes

import numpy as np
import pytest
import torch

import calib_reference as C
import rgbd_reference as R

pytestmark = pytest.mark.gpu

LM, EP, EP_C = 1e-4, 0.1, 0.1

# name -> window; built once, shared, never modified
_CASES = {
    "1_partial_chunk": lambda: R.window(311, 5, 12, 22, radius=2, t0=1),              # HW = 264: a partial second chunk
    "2_hw_not_mult_4": lambda: R.window(312, 5, 13, 21, t0=2),                        # HW = 273, HW & 3 != 0
    "3_front_frames": lambda: R.window(313, 12, 9, 12, radius=3, t0=4),               # frames whose rows are all fixed poses
    "5_p31": lambda: R.window(315, 32, 9, 12, radius=2, t0=1),                        # beyond the 29-pose dense solve of pvo_ba
    "6_p64": lambda: R.window(319, 65, 8, 8, radius=2, t0=1),                         # the limit
    # rotation about all three axes and a y translation: the windows above move in x, z and about y only, which makes half of G_ij and
    # the whole fy column of Jc exact zeros
    "7_general_motion": lambda: C.window_general(320, 6, 9, 12, radius=2, t0=1),
}
_cache = {}


def _case(name, free_mask=15):
    """-> (window, fields, yardstick step, s_case)"""
    if (name, free_mask) not in _cache:
        if name not in _cache:
            s = _CASES[name]()
            a = C.scene_args(s)
            _cache[name] = (s, C.fields(a[0], a[1], a[2], a[3], a[4], a[6], a[7]))
        s, f = _cache[name]
        base = C.scene_step(s, LM, EP, EP_C, free_mask, f)
        _cache[(name, free_mask)] = (s, f, base, C.sensitivity(s, base, f, LM, EP, EP_C, free_mask))
    return _cache[(name, free_mask)]


def _operands(s, cuda, pad=0, target=None, weight=None):
    d = lambda t: t.to(cuda).contiguous().clone()
    poses, disps = s["poses"], s["disps"]
    if pad:                                                                    # frames no edge names, behind the window
        poses = torch.cat([poses, poses[-1:].expand(pad, -1)], 0)
        disps = torch.cat([disps, disps[-1:].expand(pad, -1, -1)], 0)
    return dict(poses=d(poses), disps=d(disps), intrinsics=d(s["intr"]), targets=d(s["target"] if target is None else target),
                weights=d(s["weight"] if weight is None else weight), eta=d(s["eta"]), ii=d(s["ii"]), jj=d(s["jj"]), t0=s["t0"], t1=s["t1"])


def _call(o, iterations=1, lm=LM, ep=EP, ep_c=EP_C, free_mask=15):
    """-> (dx, dz, dc, status); poses, disps, intrinsics of `o` are updated in place"""
    from pvo_amd import droid_backends as db
    st = torch.full((4,), -1, dtype=torch.int32, device=o["disps"].device)
    dx, dz, dc = db.ba_calib(iterations=iterations, lm=lm, ep=ep, ep_c=ep_c, free_mask=free_mask, status=st, **o)
    return dx, dz, dc, st


def _assert_matches(name, got, base, sc, intr):
    """got = (dx, dz, dc) of the device; each within 4 s_case of the yardstick's, unit by unit"""
    n = lambda t: t.detach().cpu().numpy().astype(np.float64)
    intr = intr.numpy()
    print("%s: s_case dx %.2e dc %.2e dz %.2e" % (name, sc["dx"], sc["dc"], sc["dz"]))
    assert 4 * max(sc.values()) <= 2e-3                                        # a case this sensitive is replaced, not loosened
    ok_x, e_x = C.within("dx", n(got[0]), base["dx"], 4 * sc["dx"], intr)
    ok_z, e_z = C.within("dz", n(got[1]), base["dz"], 4 * sc["dz"], intr)
    ok_c, e_c = C.within("dc", n(got[2]), base["dc"], 4 * sc["dc"], intr)
    print("%s: device against the yardstick dx %.2e dc %.2e dz %.2e; dc device %s yardstick %s" % (name, e_x, e_c, e_z, n(got[2]), base["dc"]))
    assert ok_x and ok_z and ok_c


@pytest.mark.parametrize("name", sorted(_CASES))
def test_one_step_matches_the_yardstick_within_its_own_sensitivity(cuda, name):
    s, f, base, sc = _case(name)
    assert not base["rejected"]
    o = _operands(s, cuda)
    dx, dz, dc, st = _call(o)
    assert st.tolist() == [0, len(base["kx"]), 0, 0]
    _assert_matches(name, (dx, dz, dc), base, sc, s["intr"])
    assert float(dc.abs().max()) > 0
    # the retraction: c += dc in fp32, depths += dz on the rows of kx, poses by the pose retraction of dx
    assert torch.equal(o["intrinsics"], s["intr"].to(cuda) + dc)
    F = s["disps"].shape[0]
    kx = torch.from_numpy(base["kx"]).to(cuda)
    d0 = s["disps"].to(cuda).reshape(F, -1)[kx]
    assert float((o["disps"].reshape(F, -1)[kx] - (d0 + dz)).abs().max()) <= 2.0 ** -22 * float(d0.max())      # (disps + Q (...) may be one fused multiply-add)
    from oracle import oracle as O
    want = O.pose_retr(s["poses"].numpy(), dx.cpu().numpy(), s["t0"], s["t1"])
    assert np.abs(o["poses"].cpu().numpy() - want).max() <= 4e-6               # (the oracle's retraction of the device's dx: fp32 rounding)
    if name == "5_p31":
        assert s["t1"] - s["t0"] == 31
    if name == "6_p64":
        assert s["t1"] - s["t0"] == 64
    if name == "7_general_motion":                                             # every component is observed and moves, fy included
        assert float(np.abs(base["dc"]).min()) > 1e-4 and float(dc.abs().min()) > 1e-4
    # the same call on cloned operands: the same bytes
    o2 = _operands(s, cuda)
    dx2, dz2, dc2, _ = _call(o2)
    assert all(torch.equal(a, b) for a, b in ((o["poses"], o2["poses"]), (o["disps"], o2["disps"]), (o["intrinsics"], o2["intrinsics"]),
                                              (dc, dc2), (dx, dx2), (dz, dz2)))


def test_65_window_poses_are_refused_as_unsupported(cuda):
    from pvo_amd import _lib, droid_backends as db
    z = lambda *sh, **k: torch.zeros(*sh, device=cuda, **k)
    with pytest.raises(db.PvoHipError, match="at most 64 window poses"):
        db.ba_calib(z(67, 7), z(67, 8, 8), z(4), z(2, 2, 8, 8), z(2, 2, 8, 8), z(67, 8, 8), z(2, dtype=torch.long), z(2, dtype=torch.long),
                    1, 66, 1, LM, EP)
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ws, cws = z(1 << 20, dtype=torch.uint8), z(1 << 20, dtype=torch.uint8)
    args = lambda t1: (p(z(67, 7)), p(z(67, 8, 8)), p(z(4)), p(z(2, 2, 8, 8)), p(z(2, 2, 8, 8)), p(z(67, 8, 8)), p(z(2, dtype=torch.long)),
                       p(z(2, dtype=torch.long)), 2, 67, 8, 8, 67, 1, t1, 1, LM, EP, EP_C, 15, None, None, 0, None, None,
                       p(ws), ws.numel(), p(cws), cws.numel(), None)
    assert lib.pvo_ba_calib(*args(66)) == 4                                     # PVO_EUNSUPPORTED: P = 65
    assert lib.pvo_ba_calib(*args(1)) == 4                                      # ... and P = 0
    bad = list(args(5))
    bad[19] = 16
    assert lib.pvo_ba_calib(*bad) == 1                                          # PVO_EINVAL: free_mask outside [0, 15]
    bad[19], bad[18] = 15, -1.0
    assert lib.pvo_ba_calib(*bad) == 1                                          # ... ep_c < 0


@pytest.mark.parametrize("free_mask", [15, 3, 0])
def test_held_parameters_keep_their_bytes_and_mask_0_is_the_plain_step(cuda, free_mask):
    name = "7_general_motion"    # (every free component is observed: none is exempt)
    s, f, base, sc = _case(name, free_mask)
    o = _operands(s, cuda)
    dx, dz, dc, st = _call(o, free_mask=free_mask)
    assert st.tolist()[0] == 0
    _assert_matches("%s mask %d" % (name, free_mask), (dx, dz, dc), base, sc, s["intr"])
    intr0 = s["intr"].to(cuda)
    for n in range(4):
        if (free_mask >> n) & 1:
            assert float(dc[n]) != 0.0
        else:
            assert float(dc[n]) == 0.0 and torch.equal(o["intrinsics"][n], intr0[n])
    if free_mask == 0:                                                         # rgbd_reference.gn_step, the step of pvo_ba
        a = C.scene_args(s)
        _, _, dz_ref, _ = R.gn_step(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], LM, EP)
        assert np.array_equal(dz_ref, base["dz"])
        from pvo_amd import droid_backends as db
        o2 = _operands(s, cuda)
        dx2, dz2 = db.ba(o2["poses"], o2["disps"], o2["intrinsics"], o2["targets"], o2["weights"], o2["eta"], o2["ii"], o2["jj"],
                         s["t0"], s["t1"], 1, LM, EP, False)
        ok, e = C.within("dx", dx.cpu().numpy(), dx2.cpu().numpy().astype(np.float64), 4 * sc["dx"], s["intr"].numpy())
        print("mask 0 against pvo_ba: dx %.2e" % e)
        assert ok


def test_two_iterations_match_two_yardstick_steps(cuda):
    name = "7_general_motion"    # (on 1_partial_chunk one pose barely moves in the second step: 4 s_case = 1.2e-2 on it, not admitted)
    s = _case(name)[0]
    a = C.scene_args(s)
    base = C.ba_calib(*a, 2, LM, EP, EP_C, 15)
    sc = dict(dx=0.0, dc=0.0, dz=0.0)
    for seed in (0, 10, 20, 30):                                                # every step's fields perturbed, four seeded draws
        r = C.ba_calib(*a, 2, LM, EP, EP_C, 15, perturb_seed=seed)
        for k in sc:
            sc[k] = max(sc[k], C.relchange(k, r[k], base[k], a[2]))
    o = _operands(s, cuda)
    dx, dz, dc, st = _call(o, iterations=2)
    assert st.tolist()[0] == 0
    _assert_matches(name + " x2", (dx, dz, dc), base, sc, s["intr"])
    # intrinsics after two steps (both pass through fp32 between the steps): each component within the two steps' dc tolerance and
    # floor, plus one rounding of the fp32 sum per step
    got, ref = o["intrinsics"].cpu().numpy().astype(np.float64), base["intr"].astype(np.float64)
    tol = 2 * (4 * sc["dc"] * np.abs(base["dc"]) + C.floors("dc", base["dc"], a[2])) + 2 * 2.0 ** -23 * np.abs(ref)
    assert np.all(np.abs(got - ref) <= tol)


def _unchanged(o, s, cuda):
    return (torch.equal(o["poses"], s["poses"].to(cuda)) and torch.equal(o["disps"], s["disps"].to(cuda))
            and torch.equal(o["intrinsics"], s["intr"].to(cuda)))


def test_a_system_that_is_not_positive_definite_is_a_status_and_changes_nothing(cuda):
    s = _case("1_partial_chunk")[0]
    o = _operands(s, cuda, weight=torch.zeros_like(s["weight"]))
    dx, dz, dc, st = _call(o, lm=0.0, ep=0.0, ep_c=0.0)
    assert int(st[0]) == 1 and _unchanged(o, s, cuda)
    assert not bool(dx.any()) and not bool(dz.any()) and not bool(dc.any())


def test_a_step_that_would_make_fx_negative_is_a_status_and_changes_nothing(cuda):
    """targets stretched threefold about the principal point, fx alone free and undamped: the yardstick's step is dfx ~ -200 on
    fx = 13.75 and it rejects for that reason (no other test fires)"""
    s = _case("1_partial_chunk")[0]
    a = C.scene_args(s)
    J = C.pixel_jacobians(a[0], a[1], a[2], a[3], a[4], a[6], a[7])
    E, _, ht, wd = s["target"].shape
    cx = float(s["intr"][2])
    tg = s["target"].clone().reshape(E, 2, ht * wd)
    tg[:, 0] = torch.from_numpy(cx + 3.0 * (J["proj"][:, 0] - cx)).float()
    tg = tg.reshape(E, 2, ht, wd)
    ref = C.gn_step_calib(a[0], a[1], a[2], tg.numpy(), a[4], a[5], a[6], a[7], a[8], a[9], LM, EP, 0.0, 1)
    assert ref["rejected"] and ref["reason"] == "focal"
    o = _operands(s, cuda, target=tg)
    dx, dz, dc, st = _call(o, ep_c=0.0, free_mask=1)
    assert st.tolist() == [1, len(ref["kx"]), 0, 0] and _unchanged(o, s, cuda)
    assert not bool(dx.any()) and not bool(dz.any()) and not bool(dc.any())
    # the same operands with the damping on: accepted
    o = _operands(s, cuda, target=tg)
    _, _, dc, st = _call(o, free_mask=1)
    assert int(st[0]) == 0 and float(dc[0]) < 0 and float(o["intrinsics"][0]) > 0


def test_frames_that_no_edge_names_keep_their_bytes(cuda):
    s = _case("2_hw_not_mult_4")[0]
    F = s["disps"].shape[0]
    o, op = _operands(s, cuda), _operands(s, cuda, pad=2)
    got, gotp = _call(o), _call(op)
    assert torch.equal(op["poses"][F:], s["poses"][-1:].expand(2, -1).to(cuda)) and torch.equal(op["disps"][F:], s["disps"][-1:].expand(2, -1, -1).to(cuda))
    assert torch.equal(op["poses"][:F], o["poses"]) and torch.equal(op["disps"][:F], o["disps"]) and torch.equal(op["intrinsics"], o["intrinsics"])
    assert all(torch.equal(a, b) for a, b in zip(got, gotp))
    # frame 0 and 1 lie in front of the window (t0 = 2): their poses are fixed
    assert torch.equal(o["poses"][:2], s["poses"][:2].to(cuda)) and not torch.equal(o["poses"][2:], s["poses"][2:].to(cuda))


def test_ba_after_calibration_on_the_same_workspace_gives_the_bits_of_ba_alone(cuda):
    from pvo_amd import droid_backends as db
    s = _case("1_partial_chunk")[0]

    def run(first):
        if first:
            _call(_operands(s, cuda), iterations=2)
        o = _operands(s, cuda)
        st = torch.zeros(4, dtype=torch.int32, device=cuda)
        dx, dz = db.ba(o["poses"], o["disps"], o["intrinsics"], o["targets"], o["weights"], o["eta"], o["ii"], o["jj"], s["t0"], s["t1"], 2, LM, EP,
                       False, status=st)
        assert st.tolist()[0] == 0
        return o["poses"], o["disps"], dx, dz

    alone = run(False)
    after = run(True)
    assert all(torch.equal(a, b) for a, b in zip(alone, after)) and not torch.equal(alone[1], s["disps"].to(cuda))


def test_the_call_is_capturable_and_replays_to_the_same_bytes(cuda):
    s = _case("1_partial_chunk")[0]
    o = _operands(s, cuda)
    want = _operands(s, cuda)
    _call(want)                                                                # (also sizes the cached workspaces before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = _call(o)
    torch.cuda.current_stream().wait_stream(side)
    for k in ("poses", "disps", "intrinsics"):                                 # capture ran nothing
        assert torch.equal(o[k], _operands(s, cuda)[k])
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o[k], want[k]) for k in ("poses", "disps", "intrinsics")) and int(out[3][0]) == 0


# ------------------------------------------------------------------------------------------------ through the frontend
def _plane_run(cuda, **over):
    """the short synthetic stream of tests/test_ba_sigma_gpu.py's closed loop on a Droid built from default_args(**over); the stand-in
    operator takes the network's place in its frontend"""
    from pvo_amd import droid_backends as db
    from pvo_amd.droid import Droid, default_args
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.synthetic import OracleFlowOperator, PlaneScene, run_sequence
    from test_cvx_upsample_gpu import _MaskedOracleOperator
    scene = PlaneScene(ht=24, wd=32, n_frames=14, seed=0)
    torch.manual_seed(0)
    droid = Droid(default_args(device=str(cuda), image_size=[scene.ht * 8, scene.wd * 8], buffer=32, upsample=True, **over))
    assert droid.frontend.opt_intr is bool(over.get("opt_intr", False))         # the switch reaches the frontend Droid builds
    op = _MaskedOracleOperator(OracleFlowOperator(scene, droid.video, lambda p, d, k, i, j: db.reproject(p, d, k, i, j)[0]))
    droid.frontend = DroidFrontend(op, droid.video, device=cuda, warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20,
                                   frontend_radius=2, frontend_nms=1, upsample=True, opt_intr=droid.frontend.opt_intr,
                                   opt_intr_free=droid.frontend.opt_intr_free)
    # ... and in its backend: the two global bundle adjustments of Droid.terminate follow the tracked sequence
    from argparse import Namespace
    from pvo_amd.backend import DroidBackend
    be = DroidBackend(Namespace(update=op), droid.video, Namespace(device=str(cuda), backend_radius=2, backend_nms=3, backend_thresh=15.0,
                                                                  beta=0.3, backend_corr="alt"))
    before, after, frames = run_sequence(scene, droid.video, droid.frontend, op, backend=be, backend_steps=(2, 3))
    return droid, scene, before, after, frames


def test_closed_loop_with_opt_intr_runs_through_the_global_ba_and_off_is_bit_identical(cuda):
    d0, scene, before0, after0, frames0 = _plane_run(cuda)                       # never mentions the option
    d1, _, before1, after1, frames1 = _plane_run(cuda, opt_intr=False)
    d2, _, before2, after2, frames2 = _plane_run(cuda, opt_intr=True)
    n = d0.video.counter
    assert frames1 == frames0 and torch.equal(before1, before0) and torch.equal(after1, after0)
    assert torch.equal(d1.video.disps[:n], d0.video.disps[:n]) and not torch.equal(after0, before0)
    assert torch.equal(d1.video.intrinsics, d0.video.intrinsics) and not d0.video.calibrated and not d1.video.calibrated
    assert d0.video.calibrated_dev is None and d1.video.calibrated_dev is None
    init = scene.intr.to(cuda)
    assert torch.equal(d0.video.intrinsics[:n], init.expand(n, 4))
    v = d2.video
    intr = v.intrinsics
    print("closed loop: %d keyframes, intrinsics %s -> %s" % (v.counter, init.tolist(), intr[0].tolist()))
    assert v.calibrated and bool(v.calibrated_dev) and len(frames2) >= 9        # keyframes were appended after the first calibration (warmup 8)
    assert bool(torch.isfinite(intr).all()) and float(intr[0, :2].min()) > 0 and float(intr.min()) > 0
    assert torch.equal(intr, intr[0:1].expand_as(intr)) and not torch.equal(intr[0], init)
    # after the global bundle adjustments, which read the calibrated rows
    assert bool(torch.isfinite(before2).all()) and bool(torch.isfinite(after2).all()) and not torch.equal(after2, before2)
    assert bool(torch.isfinite(v.disps[:v.counter]).all())
    # the item form on the calibrated video (what the trajectory filler writes per frame): the caller's vector is not stored
    k = v.counter
    v[k] = (float(k), None, v.poses[k - 1], None, init * 1.5)
    assert torch.equal(v.intrinsics[k], intr[0]) and torch.equal(d2.get_intrinsics(), 8.0 * intr[0])
