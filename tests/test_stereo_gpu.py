"""Stereo tracking on the GPU: fixed-baseline edges (i, i) in the native bundle adjustment against the tests' own fp64 yardstick
(tests/stereo_reference.py, qualified in tests/test_stereo_host.py), the phantom-frame equivalence on the device, the bit
identities that guard "off means untouched", two virtual ranks, the reprojection kernels with a baseline, stereo edges inside the
native update (native, sharded and no-riders doors), and the closed loop through DepthVideo / DroidFrontend / the backend.

Shapes: 9 x 12 (HW = 108: one partial assembly chunk) and 30 x 101 (HW = 3030: no multiple of 256, six assembly chunks, HW & 3 != 0).
Stereo edges against fp64 within derived bounds, in every launch form and row-table branch: tests/test_ba_riders_fp64_gpu.py."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import rgbd_reference as R
import stereo_reference as S
from test_stereo_host import BASELINE

pytestmark = pytest.mark.gpu

B = 0.1                   # the BA cases' baseline


def _only_stereo_out_edge(F, radius, frame):
    ii, jj = R.radius_graph(F, radius)
    keep = ii != frame
    return ii[keep], jj[keep]


# name -> window; built once, shared, never modified
_CASES = {
    "a": lambda: S.window(201, 6, 9, 12, B, range(6)),                                        # radius 2 + every frame's stereo edge, t0 = 1
    "b": lambda: S.window(202, 5, 30, 101, B, (0, 2, 4)),                                     # frame 0: pose fixed, depth optimised
    "c": lambda: S.window(203, 5, 9, 12, B, (1, 4), ii=_only_stereo_out_edge(5, 2, 4)[0], jj=_only_stereo_out_edge(5, 2, 4)[1]),
    "d": lambda: S.window(204, 5, 9, 12, B, range(5), eta_rows=1),                            # a single broadcast eta row
}
_cache = {}


def _case(name):
    if name not in _cache:
        s = _CASES[name]()
        _cache[name] = (s, S.reference(s, 2))
    return _cache[name]


def _ba(s, cuda, iters, baseline="own", motion_only=False, edges=None, sens=None, lm=1e-4, ep=0.1):
    from pvo_amd import droid_backends as db
    d = lambda t: t.to(cuda)
    poses, disps = d(s["poses"].clone()), d(s["disps"].clone())
    status = torch.zeros(4, dtype=torch.int32, device=cuda)
    e = slice(None) if edges is None else edges
    kw = {} if baseline is None else {"stereo_baseline": s["baseline"] if isinstance(baseline, str) else baseline}
    if sens is not None:
        kw["disps_sens"] = d(sens).contiguous()
    db.ba(poses, disps, d(s["intr"]), d(s["target"][e].contiguous()), d(s["weight"][e].contiguous()), None if motion_only else d(s["eta"]),
          d(s["ii"][e].contiguous()), d(s["jj"][e].contiguous()), s["t0"], s["t1"], iters, lm, ep, motion_only, status=status, **kw)
    st = status.cpu()
    assert int(st[0]) == 0 and int(st[2]) == 0
    return poses, disps


@pytest.mark.parametrize("name", sorted(_CASES))
def test_ba_with_stereo_edges_matches_the_yardstick(cuda, name):
    s, (want_p, want_d) = _case(name)
    ns = s["n_stereo"]
    assert s["ii"][:ns].tolist() == s["jj"][:ns].tolist() and bool((s["ii"][ns:] != s["jj"][ns:]).all())
    poses, disps = _ba(s, cuda, 2)
    ep, ed = np.abs(poses.cpu().numpy() - want_p).max(), np.abs(disps.cpu().numpy() - want_d).max()
    plain_p, plain_d = _ba(s, cuda, 2, baseline=None)                          # the same edges as identity edges
    moved = float((plain_d - disps).abs().max())
    print("%s (%d frames of %d x %d, %d stereo of %d edges): against the yardstick poses %.2e disps %.2e; the stereo term moves a depth by up to %.3f"
          % ((name,) + tuple(s["disps"].shape) + (ns, s["ii"].shape[0], ep, ed, moved)))
    assert ep < 1e-4 and ed < 1e-4
    assert moved > 1e-3                                                         # the term is in the kernels, not a no-op
    if name == "b":                                                             # frame 0: its pose is fixed, its depth moves
        assert s["t0"] == 1 and torch.equal(poses[0].cpu(), s["poses"][0]) and not torch.equal(disps[0].cpu(), s["disps"][0])
    if name == "c":                                                             # frame 4's only out-edge is its stereo edge
        assert s["ii"].tolist().count(4) == 1 and not torch.equal(disps[4].cpu(), s["disps"][4])
        assert float((plain_d[4].cpu() - s["disps"][4]).abs().max()) < 1e-4     # (as an identity edge it constrains nothing: Jz ~ 0)
        assert float((disps[4].cpu() - s["disps"][4]).abs().max()) > 1e-2
    if name == "d":
        assert s["eta"].shape[0] == 1


def test_stereo_together_with_the_sensor_depth_prior_applies_both_terms(cuda):
    s, _ = _case("a")
    sens = s["sens"]
    want_p, want_d = S.reference(s, 2, sens=sens.numpy())
    poses, disps = _ba(s, cuda, 2, sens=sens)
    ep, ed = np.abs(poses.cpu().numpy() - want_p).max(), np.abs(disps.cpu().numpy() - want_d).max()
    print("stereo + RGB-D: against the yardstick poses %.2e disps %.2e" % (ep, ed))
    assert ep < 1e-4 and ed < 1e-4
    assert not torch.equal(disps, _ba(s, cuda, 2)[1]) and not torch.equal(disps, _ba(s, cuda, 2, baseline=None, sens=sens)[1])


def test_stereo_edges_are_ordinary_edges_to_phantom_right_cameras_on_the_device(cuda):
    from pvo_amd import droid_backends as db
    from test_stereo_host import _phantom_case
    s, poses2, disps2, jj2 = _phantom_case(F=4, ht=9, wd=12, b=B, seed=22)
    F = 4
    d = lambda t: t.to(cuda)
    _, got = _ba(s, cuda, 2)
    p2, d2 = d(poses2.clone()), d(disps2.clone())
    status = torch.zeros(4, dtype=torch.int32, device=cuda)
    db.ba(p2, d2, d(s["intr"]), d(s["target"]), d(s["weight"]), d(s["eta"]), d(s["ii"]), d(jj2.contiguous()), 2 * F, 2 * F, 2, 1e-4, 0.1, False,
          status=status)
    assert int(status[0]) == 0 and int(status[2]) == 0
    gap = float((got - d2[:F]).abs().max())
    moved = float((got.cpu() - s["disps"]).abs().max())
    print("stereo edges vs phantom frames, both through pvo_ba: depths differ by %.2e (the steps move them by up to %.3f)" % (gap, moved))
    assert gap < 1e-4 and moved > 1e-2


@pytest.mark.parametrize("name", ["a", "b"])
def test_bit_identities(cuda, name):
    from pvo_amd import droid_backends as db
    s, _ = _case(name)
    ns, E = s["n_stereo"], s["ii"].shape[0]
    d = lambda t: t.to(cuda)
    # motion-only: stereo edges appended behind the graph's edges add exactly nothing
    order = torch.cat([torch.arange(ns, E), torch.arange(ns)])
    pm, dm = _ba(s, cuda, 2, motion_only=True, edges=order)
    p0, d0 = _ba(s, cuda, 2, motion_only=True, edges=torch.arange(ns, E), baseline=None)
    assert torch.equal(pm, p0) and torch.equal(dm, d0) and torch.equal(dm.cpu(), s["disps"]) and not torch.equal(pm.cpu(), s["poses"])
    # baseline 0.0 passed explicitly is no argument, with the (i, i) edges present: they stay identity edges
    pz, dz = _ba(s, cuda, 2, baseline=0.0)
    pn, dn = _ba(s, cuda, 2, baseline=None)
    assert torch.equal(pz, pn) and torch.equal(dz, dn)
    # the same BA twice: the same bits
    p1, d1 = _ba(s, cuda, 2)
    p2, d2 = _ba(s, cuda, 2)
    assert torch.equal(p1, p2) and torch.equal(d1, d2) and not torch.equal(d1, dn)
    # the one-call form = plan + recorder + pvo_ba_local / pvo_ba_finish; the next plan resets the baseline
    F, ht, wd = s["disps"].shape
    P = s["t1"] - s["t0"]
    ws = db.ba_workspace(E, P, F, ht * wd, cuda)
    sysb = torch.zeros((6 * P) ** 2 + 6 * P, dtype=torch.int64, device=cuda)
    ii, jj = d(s["ii"]), d(s["jj"])

    def split(baseline, clear=False):
        poses, disps = d(s["poses"].clone()), d(s["disps"].clone())
        db.ba_plan(ii, jj, F, ht * wd, s["eta"].shape[0], s["t0"], s["t1"], ws)
        if baseline:
            db.ba_stereo(ws, E, P, F, ht * wd, baseline)
        if clear:
            db.ba_stereo(ws, E, P, F, ht * wd, 0.0)
        for _ in range(2):
            db.ba_local(poses, disps, d(s["intr"]), d(s["target"]), d(s["weight"]), d(s["eta"]), ii, jj, s["t0"], s["t1"], False, sysb, ws)
            db.ba_finish(poses, disps, sysb, ii, jj, s["t0"], s["t1"], 1e-4, 0.1, False, ws)
        return poses, disps
    a = split(s["baseline"])
    assert torch.equal(a[0], p1) and torch.equal(a[1], d1)
    b = split(0.0)                                                              # the same workspace, planned again: identity edges
    assert torch.equal(b[0], pn) and torch.equal(b[1], dn)
    c = split(s["baseline"], clear=True)
    assert torch.equal(c[0], pn) and torch.equal(c[1], dn)


def test_two_virtual_ranks_with_stereo_edges(cuda):
    """12 keyframes of 9 x 12, the edges |i - j| <= 3 plus every frame's stereo edge, as two edge shards by source keyframe that take
    turns on the device, each with the baseline behind its plan: poses and the depth maps a rank owns are the whole graph's, bit for bit"""
    from pvo_amd import droid_backends as db
    from pvo_amd.parallel import local_eta_rows, partition_by_source
    s = S.window(2121, 12, 9, 12, B, range(12), radius=3)
    d = lambda t: t.to(cuda)
    whole_p, whole_d = _ba(s, cuda, 2)
    owner, _ = partition_by_source(s["ii"].tolist(), 2)
    F, ht, wd = s["disps"].shape
    P = s["t1"] - s["t0"]
    shards = []
    for r in range(2):
        m = torch.tensor([o == r for o in owner])
        rows = local_eta_rows(s["ii"].tolist(), s["ii"][m].tolist(), s["t0"], s["t1"])
        sh = dict(ii=d(s["ii"][m].contiguous()), jj=d(s["jj"][m].contiguous()), target=d(s["target"][m].contiguous()),
                  weight=d(s["weight"][m].contiguous()), eta=d(s["eta"][rows].contiguous()), poses=d(s["poses"].clone()),
                  disps=d(s["disps"].clone()), owned=sorted(set(s["ii"][m].tolist())))
        assert bool((sh["ii"] == sh["jj"]).any())                               # each rank holds stereo edges
        E = sh["ii"].shape[0]
        sh["ws"] = db.ba_workspace(E, P, F, ht * wd, cuda)
        sh["sys"] = torch.zeros((6 * P) ** 2 + 6 * P, dtype=torch.int64, device=cuda)
        db.ba_plan(sh["ii"], sh["jj"], F, ht * wd, sh["eta"].shape[0], s["t0"], s["t1"], sh["ws"])
        db.ba_stereo(sh["ws"], E, P, F, ht * wd, B)
        shards.append(sh)
    assert shards[0]["owned"] and shards[1]["owned"] and not set(shards[0]["owned"]) & set(shards[1]["owned"])
    for _ in range(2):
        for sh in shards:
            db.ba_local(sh["poses"], sh["disps"], d(s["intr"]), sh["target"], sh["weight"], sh["eta"], sh["ii"], sh["jj"],
                        s["t0"], s["t1"], False, sh["sys"], sh["ws"])
        total = shards[0]["sys"] + shards[1]["sys"]
        for sh in shards:
            db.ba_finish(sh["poses"], sh["disps"], total.clone(), sh["ii"], sh["jj"], s["t0"], s["t1"], 1e-4, 0.1, False, sh["ws"])
            sh["sys"].zero_()
    assert torch.equal(shards[0]["poses"], shards[1]["poses"]) and torch.equal(shards[0]["poses"], whole_p)
    for sh, other in ((shards[0], shards[1]), (shards[1], shards[0])):
        assert torch.equal(sh["disps"][sh["owned"]], whole_d[sh["owned"]])
        assert torch.equal(sh["disps"][other["owned"]], d(s["disps"])[other["owned"]])      # ... and a map it does not own stays (dz = 0)
    assert not torch.equal(whole_d, _ba(s, cuda, 2, baseline=None)[1])


# ------------------------------------------------------------------------------------------------ reprojection
def _coord_bound(want, ht, wd):
    """fewer than eight fp32 roundings on values of the size of the image or the coordinate: 8 * 2^-24 * max(wd, ht, |coord|)"""
    return 8.0 * 2.0 ** -24 * np.maximum(max(wd, ht), np.abs(want))


@pytest.mark.parametrize("ht,wd", [(9, 12), (30, 101)])
def test_reproject_with_a_baseline(cuda, ht, wd):
    from pvo_amd import droid_backends as db
    from pvo_amd.geom.se3 import SE3
    g = torch.Generator().manual_seed(ht * wd)
    F, b = 5, 0.37
    poses = SE3.exp(0.05 * torch.randn(F, 6, generator=g)).data.contiguous()
    disps = 0.2 + torch.rand(F, ht, wd, generator=g)
    intr = torch.tensor([wd * 0.9, wd * 0.85, wd / 2.0 + 0.25, ht / 2.0 - 0.5]).repeat(F, 1)
    ii = torch.tensor([0, 1, 1, 2, 3, 4, 4, 0])
    jj = torch.tensor([1, 1, 0, 2, 1, 4, 3, 0])
    st = (ii == jj)
    d = lambda t: t.to(cuda)
    c1, v1 = db.reproject(d(poses), d(disps), d(intr), d(ii), d(jj), baseline=b)
    c0, v0 = db.reproject(d(poses), d(disps), d(intr), d(ii), d(jj))
    assert torch.equal(c1[~st], c0[~st]) and torch.equal(v1[~st], v0[~st])      # ordinary edges: the bits of the call without baseline
    want, _ = S.reproject(poses.numpy(), disps.numpy(), intr.numpy(), ii.numpy(), jj.numpy(), b)
    got = c1.cpu().numpy().astype(np.float64)
    err = np.abs(got - want)[st.numpy()]
    bound = _coord_bound(want, ht, wd)[st.numpy()]
    print("%d x %d: stereo edges against the fp64 closed form: max error %.2e px (bound there %.2e)" % (ht, wd, err.max(), bound[err == err.max()].max()))
    assert bool((err <= bound).all())
    assert bool((v1[st] == 1.0).all())                                          # `valid` keeps its rule: Z = 1 on both sides
    assert float(np.abs(got - c0.cpu().numpy())[st.numpy()].max()) > 1.0        # (an identity edge reprojects a pixel onto itself)
    # with the motion features in one pass: bit-identical to the two separate calls (the rule of pvo_reproject_motion)
    E = ii.numel()
    target = d(20.0 * torch.randn(1, E, ht, wd, 2, generator=g))
    ddy = d(torch.randn(1, E, ht, wd, 2, generator=g))
    raw = d(4.0 * torch.randn(1, E, ht, wd, 2, generator=g))
    for dtype in (torch.float16, torch.bfloat16):
        m0 = db.graph_motion(target, c1[None].contiguous(), ddy, raw, dtype)
        c2, v2, m2 = db.reproject_motion(d(poses), d(disps), d(intr), d(ii), d(jj), target, ddy, raw, dtype, baseline=b)
        assert torch.equal(c2, c1) and torch.equal(v2, v1) and torch.equal(m0.view(torch.int16), m2.view(torch.int16))
        c3, v3, m3 = db.reproject_motion(d(poses), d(disps), d(intr), d(ii), d(jj), target, ddy, raw, dtype)
        assert torch.equal(c3, c0) and torch.equal(v3, v0)


# ------------------------------------------------------------------------------------------------ inside the native update
def _window(cuda, stereo, zero_flow_head=False, baseline=BASELINE):
    """bench.make_window's S-B window; stereo: right maps from a seeded generator and one stereo edge per keyframe"""
    import bench
    from test_chained_updates import structured_operator
    video, graph = bench.make_window(cuda, seed=3)
    structured_operator(graph.update_op, 0.1)
    if zero_flow_head:
        with torch.no_grad():
            graph.update_op.delta[2].weight.zero_(); graph.update_op.delta[2].bias.zero_()
    if stereo:
        n = graph.nkf
        g = torch.Generator().manual_seed(17)
        video.ensure_fmaps_right()[:n] = torch.randn(n, video.ht // 8, video.wd // 8, 128, generator=g).half().to(cuda)
        video.stereo_baseline = baseline
        graph.add_factors(list(range(n)), list(range(n)))
        assert graph._ii_h[-n:] == graph._jj_h[-n:] == list(range(n))
    return video, graph


def _updates(cuda, stereo, door="native", n=2, **kw):
    from pvo_amd.parallel import ShardedBA
    video, graph = _window(cuda, stereo, **kw)
    sb = ShardedBA(communicate=False) if door == "sharded" else None
    for _ in range(n):
        if sb is None:
            graph.update(None, None, use_inactive=True)
        else:
            graph._update_fused(None, None, 2, True, 1e-7, False, sharded=sb)
    torch.cuda.synchronize()
    return video, graph


def test_target_of_a_stereo_edge_is_the_closed_form_reprojection(cuda):
    """the flow-revision head zeroed: after one update target_cam = the in-update reprojection of the state the update found"""
    video, graph = _window(cuda, True, zero_flow_head=True)
    n, ht, wd = graph.nkf, graph.ht, graph.wd
    poses0, disps0 = video.poses.clone(), video.disps.clone()
    graph.update(None, None, use_inactive=True)
    torch.cuda.synchronize()
    ii, jj = np.array(graph._ii_h), np.array(graph._jj_h)
    want, _ = S.reproject(poses0.cpu().numpy(), disps0.cpu().numpy(), video.intrinsics.cpu().numpy(), ii, jj, BASELINE)
    got = graph.target_cam[0].cpu().numpy().astype(np.float64)
    st = ii == jj
    err, bound = np.abs(got - want)[st], _coord_bound(want, ht, wd)[st]
    print("target_cam of the %d stereo edges after one update against the closed form: max error %.2e px" % (int(st.sum()), err.max()))
    assert int(st.sum()) == n and bool((err <= bound).all())
    u = np.arange(wd, dtype=np.float64)
    assert np.abs(want[st][..., 0] - (u[None, None, :] - 40.0 * BASELINE * disps0[:n].cpu().numpy())).max() < 1e-9      # u - fx b d
    assert not torch.equal(video.disps, disps0)                                 # (and the BA behind it ran)


def test_stereo_edges_inside_the_native_update(cuda):
    from pvo_amd import droid_backends as db
    v1, g1 = _updates(cuda, True)
    v0, g0 = _updates(cuda, False)
    n = g1.nkf
    assert v0.fmaps_right is None and len(g1._ii_h) == len(g0._ii_h) + n
    moved = float((v1.disps[:n] - v0.disps[:n]).abs().max())
    print("two native updates with one stereo edge per keyframe: depths differ from the window without them by up to %.4f" % moved)
    assert moved > 1e-4 and not torch.equal(v1.poses, v0.poses)
    assert bool(torch.isfinite(v1.disps).all()) and bool(torch.isfinite(v1.poses).all())
    # the same kernels behind the other door: the edge-sharded entry points with ba_stereo
    v2, g2 = _updates(cuda, True, door="sharded")
    assert torch.equal(v2.poses, v1.poses) and torch.equal(v2.disps, v1.disps)
    assert torch.equal(g2.net, g1.net) and torch.equal(g2.target_cam, g1.target_cam) and torch.equal(g2.weight, g1.weight)
    # the debug form without riders: the same bits
    db.debug_config("no_riders", True)
    try:
        v3, g3 = _updates(cuda, True)
    finally:
        db.debug_config("no_riders", False)
    assert torch.equal(v3.poses, v1.poses) and torch.equal(v3.disps, v1.disps)
    # baseline 0 on a video with right maps is off: the (i, i) edges are identity edges of a monocular video
    v4, g4 = _updates(cuda, True, baseline=0.0)
    assert not torch.equal(v4.disps, v1.disps) and g4._rig_baseline() == 0.0


# ------------------------------------------------------------------------------------------------ closed loop
def _closed_loop(cuda, scene, kw, b, backend_steps=None):
    from pvo_amd import droid_backends as db
    from pvo_amd.backend import DroidBackend
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.synthetic import OracleFlowOperator
    from test_stereo_host import run_stereo_sequence
    video = DepthVideo(image_size=(scene.ht * 8, scene.wd * 8), buffer=scene.n + 8, device=cuda)
    video.stereo_baseline = b if b > 0 else video.stereo_baseline
    # the oracle operator's targets: the reprojection kernel itself on the TRUE poses and depths - with the baseline a stereo edge's
    # target is the true u - fx b d_true
    op = OracleFlowOperator(scene, video, lambda p, d, k, i, j: db.reproject(p, d, k, i, j, **({"baseline": b} if b > 0 else {}))[0])
    fe = DroidFrontend(op, video, device=cuda, **kw)
    poses, frames = run_stereo_sequence(scene, video, fe, op, b > 0)
    if backend_steps:
        be = DroidBackend(Namespace(update=op), video,
                          Namespace(device=str(cuda), backend_radius=2, backend_nms=3, backend_thresh=15.0, beta=0.3, backend_corr="alt"))
        for steps in backend_steps:
            be(steps)
        poses = video.poses[:video.counter].detach().cpu().clone()
    return video, fe, poses, frames


def test_closed_loop_through_the_real_video_and_frontend_is_metric(cuda):
    """the scene, baseline and thresholds of the CPU loop (tests/test_stereo_host.py), through DepthVideo / DroidFrontend / HIP kernels"""
    from pvo_amd.synthetic import PlaneScene
    from test_rgbd_host import metric_figures
    scene = PlaneScene(ht=24, wd=32, n_frames=14, seed=0)
    kw = dict(warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20, frontend_radius=2, frontend_nms=1)
    v1, fe1, poses1, frames1 = _closed_loop(cuda, scene, kw, BASELINE)
    v0, _, poses0, frames0 = _closed_loop(cuda, scene, kw, 0.0)
    stereo, mono = metric_figures(poses1, frames1, scene), metric_figures(poses0, frames0, scene)
    for name, f, fr in (("stereo", stereo, frames1), ("monocular", mono, frames0)):
        print("%s: ATE-RMSE without alignment %.5f of the path, aligned %.2e, path scale %.4f, %d keyframes" % ((name,) + f + (len(fr),)))
    assert v0.fmaps_right is None and v1.has_stereo
    assert frames1 == frames0 and len(frames1) == 14                            # the same keyframes as the monocular run
    pairs = list(zip(fe1.graph._ii_h, fe1.graph._jj_h)) + list(zip(fe1.graph._ii_inac_h, fe1.graph._jj_inac_h))
    assert sorted(p for p in pairs if p[0] == p[1]) == [(k, k) for k in range(14)]
    assert stereo[0] <= 0.005 and abs(stereo[2] - 1.0) < 0.01                   # metric without alignment
    assert mono[0] > 0.1


def test_closed_loop_with_keyframe_removal_and_global_ba_keeps_the_scale(cuda):
    """30 x 101 maps, every third frame barely moves: rm_keyframe runs on a stereo video (the right map moves with its frame), then two
    backend passes on the alt-corr path, which must not rescale a metric map"""
    from pvo_amd.synthetic import PlaneScene
    from test_rgbd_host import metric_figures
    scene = PlaneScene(ht=30, wd=101, n_frames=26, seed=0, step=0.06, pattern=(1.0, 1.0, 0.15))
    kw = dict(warmup=8, keyframe_thresh=0.6, frontend_thresh=16.0, frontend_window=25, frontend_radius=2, frontend_nms=1)
    video, fe, poses, frames = _closed_loop(cuda, scene, kw, BASELINE, backend_steps=(2, 3))
    n = video.counter
    assert fe.keyframes_removed >= 4 and n == len(frames) >= 16
    # the right maps followed their frames through the removals (run_stereo_sequence fills frame k's with k + 1)
    assert [float(video.fmaps_right[k, 0, 0, 0]) for k in range(n)] == [float(f + 1) for f in frames]
    ratio = float((video.disps[:n].cpu() / scene.disps[frames]).median())
    figs = metric_figures(poses, frames, scene)
    print("after two backend passes: median disps / truth %.4f; ATE-RMSE without alignment %.5f of the path, scale %.4f, %d removed"
          % (ratio, figs[0], figs[2], fe.keyframes_removed))
    assert abs(ratio - 1.0) < 0.01
