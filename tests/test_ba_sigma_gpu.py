"""Depth and pose uncertainty on the GPU (pvo_ba_sigma / pvo_ba_uncertainty) against the tests' own fp64 yardstick
(tests/sigma_reference.py, qualified in tests/test_ba_sigma_host.py).

Tolerance: not a fixed number.  Per case the yardstick's assembled fields (Hs, Eii, Eij, Cii) are perturbed by independent relative
2^-20 u, u in [-1, 1] - the 1e-6 to which tests/test_kernel_text_goldens.py holds the device's assembled sums - with four seeded
draws; s_case is the largest relative change of var_pose, of var_cond and of diag(pose_cov), each separately.  The device must be
within 4 s_case of the unperturbed yardstick on that quantity (var_pose: plus an absolute floor of 1e-12 max(var_cond), since it can
be exactly 0); 4, because the device's fp32 pixel terms differ from the oracle's by systematic rounding while the draws are
incoherent.  A case is only admitted with 4 s_case <= 2e-3.

Shapes: the smallest that reach each path - see _CASES."""
import numpy as np
import pytest
import torch

import rgbd_reference as R
import sigma_reference as G
import stereo_reference as S

pytestmark = pytest.mark.gpu

B = 0.1
LM, EP = 1e-4, 0.1


def _fan(n, fixed=0):
    """n out-edges of frame 0: the first `fixed` to frame 1, the rest alternating between the two frames behind it"""
    first = 2 if fixed else 1
    return np.zeros(n, np.int64), np.array([1] * fixed + [first + (e & 1) for e in range(n - fixed)], np.int64)


# name -> (window, yardstick kwargs); built once, shared, never modified
_CASES = {
    "1_partial_chunk": lambda: (R.window(311, 5, 12, 22, radius=2, t0=1), {}),                  # HW = 264: a partial second chunk
    "2_hw_not_mult_4": lambda: (R.window(312, 5, 13, 21, t0=2), {}),                            # HW = 273, HW & 3 != 0
    "3_front_frames": lambda: (R.window(313, 12, 9, 12, radius=3, t0=4), {}),                   # frames 0: every row a fixed pose
    "4_stereo_prior": lambda: (S.window(314, 6, 9, 12, B, range(6)), dict(baseline=B, sens="own")),
    "5_p31": lambda: (R.window(315, 32, 9, 12, radius=2, t0=1), {}),                            # beyond the 29-pose dense solve
    # deg > 255: rows from global memory.  200 of frame 0's 260 out-edges go to frame 1 in FRONT of the window (t0 = 2), 60 to the two
    # window frames: the elimination kernel of pvo_ba_local admits at most 169 out-edges to free poses per depth frame (its row
    # table, status word 3) - 260 edges 0 -> 1, 0 -> 2 with both poses free are refused, see the test of that below
    "6_deg260": lambda: (R.window(316, 4, 8, 8, t0=2, ii=_fan(260, 200)[0], jj=_fan(260, 200)[1]), {}),
    "7_p0": lambda: (R.window(317, 5, 9, 12, t0=5), {}),                                        # t0 == t1: no pose system
}
_cache = {}


def _case(name):
    """-> (window, kwargs, yardstick, s_case)"""
    if name not in _cache:
        s, kw = _CASES[name]()
        kw = dict(kw)
        if kw.get("sens") == "own":
            kw["sens"] = s["sens"].numpy()
        f = G.scene_fields(s, kw.get("baseline", 0.0))
        base = G.scene_schur(s, f, LM, EP, **kw)
        _cache[name] = (s, kw, base, G.sensitivity(s, base, LM, EP, f=f, **kw))
    return _cache[name]


def _operands(s, cuda, kw, pad=0, weight=None):
    d = lambda t: t.to(cuda).contiguous()
    poses, disps = s["poses"], s["disps"]
    sens = None if kw.get("sens") is None else s["sens"]
    if pad:                                                                    # frames no edge names, behind the window
        poses = torch.cat([poses, poses[-1:].expand(pad, -1)], 0)
        disps = torch.cat([disps, disps[-1:].expand(pad, -1, -1)], 0)
        sens = None if sens is None else torch.cat([sens, torch.zeros(pad, *sens.shape[1:])], 0)
    return dict(poses=d(poses), disps=d(disps), intrinsics=d(s["intr"]), targets=d(s["target"]),
                weights=d(s["weight"] if weight is None else weight), eta=d(s["eta"]), ii=d(s["ii"]), jj=d(s["jj"]), t0=s["t0"], t1=s["t1"],
                lm=LM, ep=EP, disps_sens=None if sens is None else d(sens), stereo_baseline=kw.get("baseline", 0.0))


SENTINEL = -7.0


def _outputs(o):
    return (torch.full_like(o["disps"], SENTINEL), torch.full_like(o["disps"], SENTINEL),
            torch.full((4,), -1, dtype=torch.int32, device=o["disps"].device))


def _one_call(o, **over):
    from pvo_amd import droid_backends as db
    vc, vp, st = _outputs(o)
    cov = db.ba_uncertainty(var_cond=vc, var_pose=vp, status=st, **dict(o, **over))
    return cov, vc, vp, st


def _split(o, want_pose=True):
    """plan + recorders + local + sigma on a private workspace -> (cov, var_cond, var_pose, status, sys, workspace)"""
    from pvo_amd import droid_backends as db
    F, ht, wd = o["disps"].shape
    E, P, HW = o["ii"].shape[0], o["t1"] - o["t0"], ht * wd
    ws = db.ba_workspace(E, P, F, HW, o["disps"].device)
    sys = torch.zeros(max((6 * P) ** 2 + 6 * P, 8), dtype=torch.int64, device=o["disps"].device)
    db.ba_plan(o["ii"], o["jj"], F, HW, o["eta"].shape[0], o["t0"], o["t1"], ws)
    if o["disps_sens"] is not None:
        db.ba_depth_prior(ws, E, P, F, HW, o["disps_sens"])
    if o["stereo_baseline"]:
        db.ba_stereo(ws, E, P, F, HW, o["stereo_baseline"])
    db.ba_local(o["poses"], o["disps"], o["intrinsics"], o["targets"], o["weights"], o["eta"], o["ii"], o["jj"], o["t0"], o["t1"], False, sys, ws)
    vc, vp, st = _outputs(o)
    before = [t.clone() for t in (o["poses"], o["disps"], sys)]
    cov = db.ba_sigma(sys, ws, o["ii"], o["jj"], o["disps"], o["t0"], o["t1"], o["lm"], o["ep"], vc, vp if want_pose else None, st)
    assert all(torch.equal(a, b) for a, b in zip(before, (o["poses"], o["disps"], sys)))      # nothing of poses, disps, sys is modified
    return cov, vc, vp, st, sys, ws


@pytest.mark.parametrize("name", sorted(_CASES))
def test_variances_and_pose_covariance_match_the_yardstick_within_its_own_sensitivity(cuda, name):
    s, kw, base, sc = _case(name)
    F, ht, wd = s["disps"].shape
    P, kx = s["t1"] - s["t0"], base["kx"]
    print("%s: s_case var_pose %.2e var_cond %.2e diag(pose_cov) %.2e" % (name, sc["var_pose"], sc["var_cond"], sc["cov_diag"]))
    assert 4 * max(sc.values()) <= 2e-3                                        # a case this sensitive is replaced, not loosened
    o = _operands(s, cuda, kw)
    cov, vc, vp, st = _one_call(o)
    assert st.tolist()[:3] == [0, len(kx), 0]
    got_c, got_p = vc.cpu().numpy().reshape(F, -1)[kx], vp.cpu().numpy().reshape(F, -1)[kx]
    floor = 1e-12 * float(base["var_cond"].max())
    ok_c, e_c = G.within(got_c, base["var_cond"], 4 * sc["var_cond"])
    ok_p, e_p = G.within(got_p, base["var_pose"], 4 * sc["var_pose"], floor)
    covn = cov.cpu().numpy().reshape(6 * P, 6 * P)
    ok_d, e_d = G.within(np.diag(covn), np.diag(base["pose_cov"]), 4 * sc["cov_diag"])
    print("%s: device against the yardstick var_pose %.2e var_cond %.2e diag(pose_cov) %.2e" % (name, e_p, e_c, e_d))
    assert ok_c and ok_p and ok_d
    assert float(vp[kx].min()) >= 0.0 and bool(torch.isfinite(vp[kx]).all())
    assert torch.equal(cov.reshape(6 * P, 6 * P), cov.reshape(6 * P, 6 * P).t())      # symmetric bit for bit (the product writes both)
    if name == "3_front_frames":                                               # frame 0 sees 1, 2, 3 - all in front of the window
        assert s["t0"] == 4 and torch.equal(vp[0], torch.zeros_like(vp[0])) and float(vp[4].min()) > 0
    if name == "5_p31":
        assert P == 31
    if name == "6_deg260":
        assert int((s["ii"] == 0).sum()) == 260 and float(vp[0].min()) > 0 and list(kx) == [0, 2, 3]
        assert torch.equal(vp[1], torch.full_like(vp[1], SENTINEL)) and torch.equal(vc[1], torch.full_like(vc[1], SENTINEL))
    if name == "7_p0":
        assert P == 0 and cov.numel() == 0 and torch.equal(vp, torch.zeros_like(vp))
    # the same call twice: the same bytes
    cov2, vc2, vp2, _ = _one_call(o)
    assert torch.equal(cov, cov2) and torch.equal(vc, vc2) and torch.equal(vp, vp2)


@pytest.mark.parametrize("name", ["1_partial_chunk", "3_front_frames", "4_stereo_prior", "7_p0"])
def test_one_call_form_equals_plan_recorders_local_sigma_and_nothing_is_modified(cuda, name):
    s, kw, _, _ = _case(name)
    o = _operands(s, cuda, kw)
    cov, vc, vp, st = _one_call(o)
    cov2, vc2, vp2, st2, _, _ = _split(o)                                      # (asserts poses, disps, sys unchanged by pvo_ba_sigma)
    assert torch.equal(cov, cov2) and torch.equal(vc, vc2) and torch.equal(vp, vp2) and torch.equal(st, st2)
    # the conditional variance alone, by a second call without var_pose: the same bits, and var_pose's buffer is not touched
    _, vc3, vp3, _, _, ws = _split(o, want_pose=False)
    assert torch.equal(vc3, vc) and torch.equal(vp3, torch.full_like(vp3, SENTINEL))
    # ... and they are the bits of the workspace's Q = 1 / (C + add), read out of the workspace pvo_ba_local left
    F, ht, wd = o["disps"].shape
    kx = torch.from_numpy(np.asarray(_case(name)[2]["kx"])).to(cuda)
    Q = _workspace_q(ws, o["ii"].shape[0], o["t1"] - o["t0"], F, ht * wd, len(kx))
    assert torch.equal(vc.reshape(F, -1)[kx], Q) and bool(torch.isfinite(Q).all()) and float(Q.min()) > 0


def _workspace_q(ws, E, P, F, HW, K):
    """rows [0, K) of Q in a BA workspace: the regions in front of it as the library carves them (pvo_amd/csrc/ba_workspace.h, `carve`: the
    plan's int tables, Eii, Eij, Cii, bz, Ei; every region padded to 256 bytes, the base aligned to 256)"""
    from pvo_amd import droid_backends as db
    up = lambda n: (n + 255) & ~255
    off = sum(up(4 * n) for n in (F + 1, F + 1, F + 2, E + 1, 16, P + 1, E * 6 * HW, E * 6 * HW, E * HW, E * HW, P * 6 * HW))
    rest = sum(up(4 * n) for n in (min(F, P + E) * HW,))                      # Q itself
    assert off + rest < db.ba_workspace_bytes(E, P, F, HW)
    base = (-ws.data_ptr()) % 256
    return ws[base + off: base + off + 4 * K * HW].view(torch.float32).reshape(K, HW).clone()


def test_rows_of_frames_outside_the_depth_frames_keep_their_bytes(cuda):
    s, kw, base, _ = _case("2_hw_not_mult_4")
    F = s["disps"].shape[0]
    cov, vc, vp, _ = _one_call(_operands(s, cuda, kw))
    covp, vcp, vpp, _ = _one_call(_operands(s, cuda, kw, pad=2))
    assert list(base["kx"]) == list(range(F))
    assert torch.equal(vcp[F:], torch.full_like(vcp[F:], SENTINEL)) and torch.equal(vpp[F:], torch.full_like(vpp[F:], SENTINEL))
    assert torch.equal(vcp[:F], vc) and torch.equal(vpp[:F], vp) and torch.equal(covp, cov)


def test_ba_after_uncertainty_on_the_same_workspace_gives_the_bits_of_ba_alone(cuda):
    from pvo_amd import droid_backends as db
    s, kw, _, _ = _case("4_stereo_prior")

    def run(first):
        o = _operands(s, cuda, kw)
        if first:
            _one_call(o)
        lm, ep = o.pop("lm"), o.pop("ep")
        st = torch.zeros(4, dtype=torch.int32, device=cuda)
        db.ba(o.pop("poses"), o["disps"], o.pop("intrinsics"), o.pop("targets"), o.pop("weights"), o.pop("eta"), o.pop("ii"), o.pop("jj"),
              o.pop("t0"), o.pop("t1"), 2, lm, ep, False, status=st, disps_sens=o["disps_sens"], stereo_baseline=o["stereo_baseline"])
        assert st.tolist()[0] == 0
        return o["disps"]

    alone = run(False)
    assert torch.equal(run(True), alone) and not torch.equal(alone, s["disps"].to(cuda))


def test_a_system_that_is_not_positive_definite_is_a_status_not_a_fault(cuda):
    s, kw, base, _ = _case("1_partial_chunk")
    o = _operands(s, cuda, kw, weight=torch.zeros_like(s["weight"]))
    cov, vc, vp, st = _one_call(o, lm=0.0, ep=0.0)
    P = s["t1"] - s["t0"]
    assert int(st[0]) == 1
    assert bool(torch.isfinite(vc).all()) and float(vc.min()) > 0              # 1 / eta
    assert bool(torch.isinf(vp).all()) and float(vp.min()) > 0                 # every frame is in kx
    c = cov.reshape(6 * P, 6 * P)
    eye = torch.eye(6 * P, dtype=torch.bool, device=cuda)
    assert bool(torch.isinf(c[eye]).all()) and float(c[eye].min()) > 0 and float(c[~eye].abs().max()) == 0.0


def test_a_frame_with_more_free_neighbours_than_the_elimination_admits_is_a_status(cuda):
    """260 edges 0 -> 1, 0 -> 2 with both poses free: pvo_ba_local's row table holds 169 free neighbours of one depth frame and flags
    the overflow in status word 3; the system it leaves is incomplete, so the uncertainty reports failure instead of numbers"""
    s = R.window(318, 3, 8, 8, t0=1, ii=_fan(260)[0], jj=_fan(260)[1])
    cov, vc, vp, st = _one_call(_operands(s, cuda, {}))
    assert st.tolist() == [1, 3, 0, 1]
    assert bool(torch.isinf(vp).all()) and bool(torch.isfinite(vc).all()) and bool(torch.isinf(torch.diagonal(cov.reshape(12, 12))).all())


def test_more_than_64_window_poses_are_refused(cuda):
    from pvo_amd import droid_backends as db
    z = lambda *sh, **k: torch.zeros(*sh, device=cuda, **k)
    with pytest.raises(db.PvoHipError, match="at most 64 window poses"):
        db.ba_uncertainty(z(66, 7), z(66, 8, 8), z(4), z(2, 2, 8, 8), z(2, 2, 8, 8), z(66, 8, 8), z(2, dtype=torch.long), z(2, dtype=torch.long),
                          1, 66, LM, EP)


# ------------------------------------------------------------------------------------------------ through the factor graph and the frontend
def test_factor_graph_uncertainty_reads_the_operands_of_the_last_updates_bundle_adjustment(cuda):
    import bench
    from pvo_amd import droid_backends as db
    from test_chained_updates import structured_operator
    video, graph = bench.make_window(cuda, seed=3)                             # S-B: 8 keyframes of 48 x 64
    structured_operator(graph.update_op, 0.1)
    for _ in range(2):
        graph.update(None, None, use_inactive=True)
    assert video.disps_var_cond is None and video.disps_var_pose is None and video.poses_cov is None      # off: none of the three exists
    poses, disps = video.poses.clone(), video.disps.clone()
    cov = graph.uncertainty(None, None, use_inactive=True)
    assert torch.equal(video.poses, poses) and torch.equal(video.disps, disps)  # read only
    # the operands the composed path (FactorGraph.update without the native update) hands to DepthVideo.ba
    ht, wd = graph.ht, graph.wd
    t0, t1 = max(1, min(graph._ii_h) + 1), max(max(graph._ii_h), max(graph._jj_h)) + 1
    assert not any((i >= t0 - 3) and (j >= t0 - 3) for i, j in zip(graph._ii_inac_h, graph._jj_inac_h))      # a fresh window: no inactive edge
    src = sorted(set(graph._ii_h))
    assert src == sorted(set(src) | set(range(t0, t1)))                        # one eta row per depth frame on either path
    eta = 0.2 * graph.damping[torch.tensor(src, device=cuda)] + 1e-7
    target = graph.target_cam.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
    weight = graph.weight.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
    vc, vp = torch.full_like(video.disps, float("inf")), torch.full_like(video.disps, float("inf"))
    want = db.ba_uncertainty(video.poses, video.disps, video.intrinsics[0], target, weight, eta, graph.ii, graph.jj, t0, t1, 1e-4, 0.1,
                             var_cond=vc, var_pose=vp)
    P = t1 - t0
    assert P >= 5 and torch.equal(cov, want) and torch.equal(video.disps_var_cond, vc) and torch.equal(video.disps_var_pose, vp)
    assert bool(torch.isfinite(vc[src]).all()) and bool(torch.isfinite(vp[src]).all()) and float(vp[src].max()) > 0
    assert torch.equal(video.poses_cov[t0:t1], torch.stack([want[p, :, p, :] for p in range(P)]))
    assert bool(torch.isinf(video.poses_cov[0].diagonal()).all())              # frame 0's pose is fixed: never estimated


def _plane_run(cuda, uncertainty):
    """the short synthetic stream of the system tests on a Droid built from default_args(uncertainty=...), tracking with
    args.upsample (so that the full-resolution map exists); the stand-in operator takes the network's place in its frontend"""
    from pvo_amd import droid_backends as db
    from pvo_amd.droid import Droid, default_args
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.synthetic import OracleFlowOperator, PlaneScene, run_sequence
    from test_cvx_upsample_gpu import _MaskedOracleOperator
    scene = PlaneScene(ht=24, wd=32, n_frames=14, seed=0)
    torch.manual_seed(0)
    droid = Droid(default_args(device=str(cuda), image_size=[scene.ht * 8, scene.wd * 8], buffer=32, upsample=True, uncertainty=uncertainty))
    assert droid.frontend.uncertainty is bool(uncertainty)                      # the switch reaches the frontend Droid builds
    op = _MaskedOracleOperator(OracleFlowOperator(scene, droid.video, lambda p, d, k, i, j: db.reproject(p, d, k, i, j)[0]))
    droid.frontend = DroidFrontend(op, droid.video, device=cuda, warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20,
                                   frontend_radius=2, frontend_nms=1, upsample=True, uncertainty=droid.frontend.uncertainty)
    poses, frames = run_sequence(scene, droid.video, droid.frontend, op)
    return droid, poses, frames


def test_closed_loop_with_uncertainty_keeps_the_trajectory_and_filters_the_map(cuda):
    d0, poses0, frames0 = _plane_run(cuda, False)
    d1, poses1, frames1 = _plane_run(cuda, True)
    v0, v1 = d0.video, d1.video
    assert v0.disps_var_cond is None and v0.disps_var_pose is None and v0.poses_cov is None      # off: nothing is allocated
    with pytest.raises(RuntimeError, match="uncertainty"):
        d0.get_uncertainty()
    n = v1.counter
    assert frames1 == frames0 and len(frames1) == 14 and torch.equal(poses1, poses0) and torch.equal(v1.disps[:n], v0.disps[:n])
    assert torch.equal(v1.disps_up[:n], v0.disps_up[:n])
    sigma, vc, vp, pc = d1.get_uncertainty()
    assert sigma.shape == vc.shape == vp.shape == v1.disps[:n].shape and pc.shape == (n, 6, 6) and pc.dtype == torch.float64
    assert torch.equal(sigma, torch.sqrt(vc + vp))
    assert bool(torch.isfinite(sigma).all()) and float(sigma.min()) > 0        # every keyframe has been estimated
    assert bool(torch.isfinite(pc[1:]).all())
    rel = sigma / v1.disps[:n]
    bound = float(rel.flatten().kthvalue(int(0.7 * rel.numel())).values)       # keeps about 70 % of the cells
    whole, part = d1.get_map(thresh=0.05), d1.get_map(thresh=0.05, max_rel_sigma=bound)
    nw, npart = int(whole["frame_start"][-1]), int(part["frame_start"][-1])
    print("closed loop: %d keyframes, relative sigma in [%.3f, %.3f], map %d points, %d with sigma / disp <= %.3f"
          % (n, float(rel.min()), float(rel.max()), nw, npart, bound))
    assert 0 < npart < nw and "sigma" not in whole and part["sigma"].shape == (npart,)
    key = lambda m: set(map(tuple, m["src"].tolist()))
    assert key(part) < key(whole)                                              # a subset of the unfiltered map
    f, k = part["src"][:, 0].long(), part["src"][:, 1].long()
    assert torch.equal(part["sigma"], sigma.reshape(n, -1)[f, k])
    assert bool((part["sigma"] <= bound * v1.disps[:n].reshape(n, -1)[f, k]).all())
    dropped = torch.tensor(sorted(key(whole) - key(part)), device=cuda).long()
    assert bool((rel.reshape(n, -1)[dropped[:, 0], dropped[:, 1]] > bound).all())
    # full resolution: the mask and each point's sigma are those of its 1/8 cell (y // 8, x // 8)
    fw, fp = d1.get_map(thresh=0.05, full_res=True), d1.get_map(thresh=0.05, full_res=True, max_rel_sigma=bound)
    nfw, nfp = int(fw["frame_start"][-1]), int(fp["frame_start"][-1])
    assert 0 < nfp < nfw and key(fp) < key(fw)
    f, k = fp["src"][:, 0].long(), fp["src"][:, 1].long()
    y, x = (k // v1.wd) // 8, (k % v1.wd) // 8
    assert torch.equal(fp["sigma"], sigma[f, y, x]) and bool((rel[f, y, x] <= bound).all())
    gone = torch.tensor(sorted(key(fw) - key(fp)), device=cuda).long()
    assert bool((rel[gone[:, 0], (gone[:, 1] // v1.wd) // 8, (gone[:, 1] % v1.wd) // 8] > bound).all())
