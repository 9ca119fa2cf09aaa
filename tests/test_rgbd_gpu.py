"""RGB-D tracking on the GPU: the sensor-depth prior in the native bundle adjustment (both homes of the depth phase, every launch
form) against the tests' own dense reference (tests/rgbd_reference.py, qualified in tests/test_rgbd_host.py), its bit identities,
two virtual ranks, the prior inside the native update, the ingest kernel, and the closed loop through DepthVideo and DroidFrontend.

Which form of the launch rule (ba.hip, pvo_ba_local) a shape reaches, with chunks = ceil(HW / 256) and frames = min(F, P + 1):
  chunks x frames <= 192                          256-pixel chunks, the depth phase FUSED into the Schur kernel
  above that, P <= 29 (a dense window)            256-pixel chunks, ba_depth_kernel in front
  above that, P > 29                              512- (up to 1024 workgroups) or 1024-pixel chunks, ba_depth_kernel in front
The prior against fp64 within derived bounds, in each of the six launch forms: tests/test_ba_riders_fp64_gpu.py."""
from argparse import Namespace

import numpy as np
import pytest
import torch

import ba_reference as B
import rgbd_reference as R

pytestmark = pytest.mark.gpu


def _form(s):
    """ba_reference.launch_form, the one statement of the launch rule, under the names this module asserts"""
    form = B.launch_form(s)
    return {"fused256": "fused", "chunk512": "depth kernel, 512", "chunk1024": "depth kernel, 1024"}.get(form, "depth kernel, dense window")


def _no_out_edges(F, radius, frame):
    ii, jj = R.radius_graph(F, radius)
    keep = ii != frame
    return ii[keep], jj[keep]


# name -> (window, the form it must reach); built once, shared, never modified
_CASES = {
    "a": lambda: R.window(101, 5, 12, 22),                                      # HW = 264: a multiple of 4, a partial second chunk
    "b": lambda: R.window(102, 5, 13, 21),                                      # HW = 273: HW & 3 != 0
    "c": lambda: R.window(103, 17, 30, 101),                                    # 12 chunks x 17 frames > 192, P = 16
    "d": lambda: R.window(104, 32, 30, 60),                                     # 8 chunks x 32 frames > 192, P = 31
    "e": lambda: R.window(105, 6, 12, 16, t0=2),                                # frames 0, 1: sources in front of the window, measured
    "f": lambda: R.window(106, 5, 12, 16, ii=_no_out_edges(5, 2, 4)[0], jj=_no_out_edges(5, 2, 4)[1]),   # frame 4: no out-edge
}
_FORMS = {"a": "fused", "b": "fused", "c": "depth kernel, dense window", "d": "depth kernel, 512", "e": "fused", "f": "fused"}
_cache = {}


def _case(name):
    if name not in _cache:
        s = _CASES[name]()
        _cache[name] = (s, R.reference(s, 2))
    return _cache[name]


def _ba(s, cuda, iters, sens="own", eta=None, lm=1e-4, ep=0.1):
    from pvo_amd import droid_backends as db
    d = lambda t: t.to(cuda)
    poses, disps = d(s["poses"].clone()), d(s["disps"].clone())
    status = torch.zeros(4, dtype=torch.int32, device=cuda)
    kw = {} if sens is None else {"disps_sens": d(s["sens"] if isinstance(sens, str) else sens).contiguous()}
    db.ba(poses, disps, d(s["intr"]), d(s["target"]), d(s["weight"]), d(s["eta"] if eta is None else eta), d(s["ii"]), d(s["jj"]),
          s["t0"], s["t1"], iters, lm, ep, False, status=status, **kw)
    st = status.cpu()
    assert int(st[0]) == 0 and int(st[2]) == 0
    return poses, disps


@pytest.mark.parametrize("name", sorted(_CASES))
def test_ba_prior_matches_the_dense_reference(cuda, name):
    s, (want_p, want_d) = _case(name)
    assert _form(s) == _FORMS[name]
    meas = s["sens"] > 0
    frac = float(meas.float().mean())
    rel = float(((s["sens"] - s["disps"]).abs() / s["disps"])[meas].max())
    assert 0.6 < frac < 0.8 and 0.05 < rel <= 0.1001 and float(s["weight"].min()) >= 0.5 and float(s["weight"].max()) <= 1.5
    poses, disps = _ba(s, cuda, 2)
    ep, ed = np.abs(poses.cpu().numpy() - want_p).max(), np.abs(disps.cpu().numpy() - want_d).max()
    plain_p, plain_d = _ba(s, cuda, 2, sens=None)
    moved = float((plain_d - disps).abs().max())
    print("%s (%s): against the reference poses %.2e disps %.2e; the prior moves a depth by up to %.3f" % (name, _form(s), ep, ed, moved))
    assert ep < 1e-4 and ed < 1e-4
    assert moved > 1e-3                                                         # the term is in the kernels, not a no-op
    if name == "e":                                                             # the frames in front of the window follow their sensor
        assert s["t0"] == 2 and bool((s["ii"] < 2).any())
        for f in (0, 1):
            gap = lambda dd: float((dd[f].cpu() - s["sens"][f]).abs()[meas[f]].mean())
            assert gap(disps) < gap(plain_d)
    if name == "f":                                                             # dz = 0 for the frame without out-edges, measured or not
        assert not bool((s["ii"] == 4).any()) and bool(meas[4].any())
        assert torch.equal(disps[4].cpu(), s["disps"][4]) and not torch.equal(disps[3].cpu(), s["disps"][3])


@pytest.mark.parametrize("name", ["a", "c"])
def test_bit_identities(cuda, name):
    from pvo_amd import droid_backends as db
    s, _ = _case(name)
    d = lambda t: t.to(cuda)
    # an all-zero map is no map
    p0, d0 = _ba(s, cuda, 2, sens=None)
    pz, dz = _ba(s, cuda, 2, sens=torch.zeros_like(s["sens"]))
    assert torch.equal(p0, pz) and torch.equal(d0, dz)
    # residual exactly 0, one step: eta' = where(sens > 0, alpha, eta)
    s0 = dict(s, sens=torch.where(s["sens"] > 0, s["disps"], torch.zeros_like(s["disps"])))
    pr, dr = _ba(s0, cuda, 1)
    pe, de = _ba(s0, cuda, 1, sens=None, eta=R.swapped_eta(s0))
    assert torch.equal(pr, pe) and torch.equal(dr, de)
    assert not torch.equal(dr, _ba(s0, cuda, 1, sens=None)[1])
    # two identical calls repeat
    p1, d1 = _ba(s, cuda, 2)
    p2, d2 = _ba(s, cuda, 2)
    assert torch.equal(p1, p2) and torch.equal(d1, d2) and not torch.equal(d1, d0)
    # the prior is the plan's: set behind pvo_ba_plan it acts on every later pvo_ba_local, the next pvo_ba_plan clears it
    F, ht, wd = s["disps"].shape
    E, P = s["ii"].shape[0], s["t1"] - s["t0"]
    ws = db.ba_workspace(E, P, F, ht * wd, cuda)
    sysb = torch.zeros((6 * P) ** 2 + 6 * P, dtype=torch.int64, device=cuda)
    ii, jj, sens = d(s["ii"]), d(s["jj"]), d(s["sens"]).contiguous()

    def split(prior, clear=False):
        poses, disps = d(s["poses"].clone()), d(s["disps"].clone())
        db.ba_plan(ii, jj, F, ht * wd, s["eta"].shape[0], s["t0"], s["t1"], ws)
        if prior:
            db.ba_depth_prior(ws, E, P, F, ht * wd, sens)
        if clear:
            db.ba_depth_prior(ws, E, P, F, ht * wd, None)
        for _ in range(2):
            db.ba_local(poses, disps, d(s["intr"]), d(s["target"]), d(s["weight"]), d(s["eta"]), ii, jj, s["t0"], s["t1"], False, sysb, ws)
            db.ba_finish(poses, disps, sysb, ii, jj, s["t0"], s["t1"], 1e-4, 0.1, False, ws)
        return poses, disps
    a = split(True)
    assert torch.equal(a[0], p1) and torch.equal(a[1], d1)
    b = split(False)                                                            # the same workspace, planned again: today's results
    assert torch.equal(b[0], p0) and torch.equal(b[1], d0)
    c = split(True, clear=True)                                                 # NULL clears it too
    assert torch.equal(c[0], p0) and torch.equal(c[1], d0)


def test_two_virtual_ranks_with_the_prior(cuda):
    """S-20 size (64 keyframes of 48 x 64, the 372 edges |i - j| <= 3) as two edge shards by source keyframe that take turns on the
    device, each with the prior behind its plan: poses and the depth maps a rank owns are the whole graph's, bit for bit"""
    from pvo_amd import droid_backends as db
    from pvo_amd.parallel import local_eta_rows, partition_by_source
    s = R.window(2020, 64, 48, 64, radius=3)
    assert s["ii"].shape[0] == 372
    d = lambda t: t.to(cuda)
    whole_p, whole_d = _ba(s, cuda, 2)
    owner, _ = partition_by_source(s["ii"].tolist(), 2)
    F, ht, wd = s["disps"].shape
    P = s["t1"] - s["t0"]
    sens = d(s["sens"]).contiguous()
    shards = []
    for r in range(2):
        m = torch.tensor([o == r for o in owner])
        rows = local_eta_rows(s["ii"].tolist(), s["ii"][m].tolist(), s["t0"], s["t1"])
        sh = dict(ii=d(s["ii"][m].contiguous()), jj=d(s["jj"][m].contiguous()), target=d(s["target"][m].contiguous()),
                  weight=d(s["weight"][m].contiguous()), eta=d(s["eta"][rows].contiguous()), poses=d(s["poses"].clone()),
                  disps=d(s["disps"].clone()), owned=sorted(set(s["ii"][m].tolist())))
        E = sh["ii"].shape[0]
        sh["ws"] = db.ba_workspace(E, P, F, ht * wd, cuda)
        sh["sys"] = torch.zeros((6 * P) ** 2 + 6 * P, dtype=torch.int64, device=cuda)
        db.ba_plan(sh["ii"], sh["jj"], F, ht * wd, sh["eta"].shape[0], s["t0"], s["t1"], sh["ws"])
        db.ba_depth_prior(sh["ws"], E, P, F, ht * wd, sens)
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
    assert not torch.equal(whole_d, _ba(s, cuda, 2, sens=None)[1])


# ------------------------------------------------------------------------------------------------ inside the native update
def _window(cuda, size):
    import bench
    from test_chained_updates import structured_operator
    if size == "sb":
        video, graph = bench.make_window(cuda, seed=3)
    else:                                                              # a real frontend window: 26 keyframes of 30 x 101
        video, graph = bench.make_window(cuda, seed=3, H8=30, W8=101, NKF=26, buffer=32, intr=(60.0, 60.0, 50.5, 15.0))
    structured_operator(graph.update_op, 0.1)
    return video, graph


def _updates(cuda, size, sens_value, door="native", motion_only=False, n=2):
    from pvo_amd.parallel import ShardedBA
    video, graph = _window(cuda, size)
    if sens_value is not None:
        g = torch.Generator().manual_seed(9)
        sens = video.ensure_disps_sens()                               # before the first plan: a persistent buffer of the video
        sens[:] = torch.where(torch.rand(sens.shape, generator=g) < 0.7, torch.tensor(sens_value), torch.tensor(0.0)).to(cuda)
        video.has_sensor_depth = True
    sb = ShardedBA(communicate=False) if door == "sharded" else None
    for _ in range(n):
        if sb is None:
            graph.update(None, None, use_inactive=True, motion_only=motion_only)
        else:
            graph._update_fused(None, None, 2, True, 1e-7, motion_only, sharded=sb)
    torch.cuda.synchronize()
    return video, graph


@pytest.mark.parametrize("size", ["sb", "window"])
def test_inside_the_native_update(cuda, size):
    from pvo_amd import droid_backends as db
    S = 1.3                                                            # the measured inverse depth; the window's depths start at 1
    v1, g1 = _updates(cuda, size, S)
    v0, g0 = _updates(cuda, size, None)
    n = g1.nkf
    assert v0.disps_sens is None and not torch.equal(v1.disps, v0.disps) and not torch.equal(v1.poses, v0.poses)
    src = sorted(set(g1._ii_h))
    meas = (v1.disps_sens[src] > 0)
    gap1, gap0 = float((v1.disps[src] - S).abs()[meas].mean()), float((v0.disps[src] - S).abs()[meas].mean())
    print("%s: mean |disp - sensor| on measured pixels %.4f with the map, %.4f without (0.3 at the start)" % (size, gap1, gap0))
    assert gap1 < 0.3 and gap1 < gap0                                  # measured pixels move towards the sensor
    # the same kernels behind the other door: the edge-sharded entry points with ba_depth_prior
    v2, g2 = _updates(cuda, size, S, door="sharded")
    assert torch.equal(v2.poses, v1.poses) and torch.equal(v2.disps, v1.disps)
    assert torch.equal(g2.net, g1.net) and torch.equal(g2.target_cam, g1.target_cam) and torch.equal(g2.weight, g1.weight)
    # the debug form without riders: the same bits
    db.debug_config("no_riders", True)
    try:
        v3, g3 = _updates(cuda, size, S)
    finally:
        db.debug_config("no_riders", False)
    assert torch.equal(v3.poses, v1.poses) and torch.equal(v3.disps, v1.disps)
    # a motion-only update has no depth phase: the map changes nothing
    vm1, _ = _updates(cuda, size, S, motion_only=True, n=1)
    vm0, _ = _updates(cuda, size, None, motion_only=True, n=1)
    assert torch.equal(vm1.poses, vm0.poses) and torch.equal(vm1.disps, vm0.disps)
    assert n >= 8


# ------------------------------------------------------------------------------------------------ ingest
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("ht,wd", [(48, 64), (44, 60), (240, 808)])
def test_depth_sense_equals_the_host_formulation(cuda, ht, wd, dtype):
    from pvo_amd import droid_backends as db
    from pvo_amd.depth_video import DepthVideo
    g = torch.Generator().manual_seed(ht + wd)
    depth = (torch.rand(ht, wd, generator=g) * 20 + 0.05)
    bad = torch.rand(ht, wd, generator=g)
    depth[bad < 0.05] = 0.0
    depth[(bad >= 0.05) & (bad < 0.1)] = -1.5
    depth[(bad >= 0.1) & (bad < 0.15)] = float("nan")
    depth[(bad >= 0.15) & (bad < 0.2)] = float("inf")
    depth[(bad >= 0.2) & (bad < 0.22)] = -float("inf")
    depth = depth.to(dtype)
    want = DepthVideo.sense_depth_host(depth)
    assert want.shape == (ht // 8, wd // 8) and 0.1 < float((want == 0).float().mean()) < 0.4
    guard = torch.full((ht // 8 + 2, wd // 8), -3.0, device=cuda)       # the rows around the output stay as they were
    db.depth_sense(depth.to(cuda), guard[1:-1])
    assert torch.equal(guard[1:-1].cpu(), want)
    assert bool((guard[0] == -3.0).all()) and bool((guard[-1] == -3.0).all())
    # ... and through DepthVideo.append, from the device and from the host
    v = DepthVideo(image_size=(ht, wd), buffer=3, device=cuda)
    z = torch.zeros(128, ht // 8, wd // 8, dtype=torch.half, device=cuda)
    v.append(0.0, None, None, torch.ones(4, device=cuda), z, z, z, depth=depth.to(cuda))
    v.append(1.0, None, None, torch.ones(4, device=cuda), z, z, z, depth=depth)
    assert torch.equal(v.disps_sens[0].cpu(), want) and torch.equal(v.disps_sens[1].cpu(), want) and not v.disps_sens[2].any()


# ------------------------------------------------------------------------------------------------ closed loop
def _closed_loop(cuda, scene, kw, depth, backend_steps=None):
    from pvo_amd import droid_backends as db
    from pvo_amd.backend import DroidBackend
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.synthetic import OracleFlowOperator
    from test_rgbd_host import run_rgbd_sequence
    video = DepthVideo(image_size=(scene.ht * 8, scene.wd * 8), buffer=scene.n + 8, device=cuda)
    op = OracleFlowOperator(scene, video, lambda p, d, k, i, j: db.reproject(p, d, k, i, j)[0])
    fe = DroidFrontend(op, video, device=cuda, **kw)
    if depth is not None:                                               # every other image is already on the device: both ingest paths
        depth = [x.to(cuda) if k % 2 == 0 else x for k, x in enumerate(depth)]
    poses, frames = run_rgbd_sequence(scene, video, fe, op, depth)
    if backend_steps:
        be = DroidBackend(Namespace(update=op), video,
                          Namespace(device=str(cuda), backend_radius=2, backend_nms=3, backend_thresh=15.0, beta=0.3, backend_corr="alt"))
        for steps in backend_steps:
            be(steps)
        poses = video.poses[:video.counter].detach().cpu().clone()
    return video, fe, poses, frames


def test_closed_loop_through_the_real_video_and_frontend_is_metric(cuda):
    from pvo_amd.synthetic import PlaneScene
    from test_rgbd_host import depth_images, metric_figures, sensor_map
    scene = PlaneScene(ht=24, wd=32, n_frames=14, seed=0)
    kw = dict(warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20, frontend_radius=2, frontend_nms=1)
    v1, _, poses1, frames1 = _closed_loop(cuda, scene, kw, list(depth_images(sensor_map(scene))))
    v0, _, poses0, frames0 = _closed_loop(cuda, scene, kw, None)
    rgbd, mono = metric_figures(poses1, frames1, scene), metric_figures(poses0, frames0, scene)
    for name, f, fr in (("rgbd", rgbd, frames1), ("monocular", mono, frames0)):
        print("%s: ATE-RMSE without alignment %.5f of the path, aligned %.2e, path scale %.4f, %d keyframes" % ((name,) + f + (len(fr),)))
    assert v0.disps_sens is None and v1.has_sensor_depth
    assert frames1 == frames0 and len(frames1) == 14                    # the same keyframes as the monocular run
    assert rgbd[0] <= 0.005 and abs(rgbd[2] - 1.0) < 0.01               # metric without alignment
    assert abs(rgbd[1] - mono[1]) < 1e-3
    assert mono[0] > 0.1


def test_closed_loop_with_keyframe_removal_and_global_ba_keeps_the_scale(cuda):
    """30 x 101 maps, every third frame barely moves: rm_keyframe runs with sensor depth (the map moves with its frame), then two
    backend passes, which must not rescale a metric map"""
    from pvo_amd.synthetic import PlaneScene
    from test_rgbd_host import depth_images, metric_figures, sensor_map
    scene = PlaneScene(ht=30, wd=101, n_frames=26, seed=0, step=0.06, pattern=(1.0, 1.0, 0.15))
    kw = dict(warmup=8, keyframe_thresh=0.6, frontend_thresh=16.0, frontend_window=25, frontend_radius=2, frontend_nms=1)
    sens = sensor_map(scene)
    video, fe, poses, frames = _closed_loop(cuda, scene, kw, list(depth_images(sens)), backend_steps=(2, 3))
    n = video.counter
    assert fe.keyframes_removed >= 4 and n == len(frames) >= 16
    # the sensor rows followed their frames through the removals
    want = torch.where(sens[frames] > 0, 1.0 / (1.0 / sens[frames].clamp(min=1e-6)), torch.zeros_like(sens[frames]))
    assert torch.equal(video.disps_sens[:n].cpu(), want)
    ratio = float((video.disps[:n].cpu() / scene.disps[frames]).median())
    figs = metric_figures(poses, frames, scene)
    print("after two backend passes: median disps / truth %.4f; ATE-RMSE without alignment %.5f of the path, scale %.4f, %d removed"
          % (ratio, figs[0], figs[2], fe.keyframes_removed))
    assert abs(ratio - 1.0) < 0.01
