"""RGB-D tracking, the parts that need no GPU: the C ABI of the three new entry points, the tests' own dense reference of the
bundle adjustment with the sensor-depth prior (tests/rgbd_reference.py) qualified against the oracle, the host logic (ingest,
rm_keyframe, the frontend's seeding, the backend's normalisation, the switch, the plan hook) on a CPU DepthVideo with the native
calls stubbed, and the closed loop on the CPU: sensor depth makes the trajectory metric."""
import ctypes
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

import rgbd_reference as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pvo_ba_depth_prior", "pvo_ba_prior", "pvo_depth_sense")


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    from pvo_amd import _lib
    header = open(os.path.join(ROOT, "include", "pvo_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in include/pvo_hip.h"
        assert hasattr(lib, name), name + " is not exported by libpvo_hip.so"
        assert name in _lib.SIGNATURES, name + " is not bound by pvo_amd._lib"
    loaded = _lib.load()
    assert loaded.pvo_version() == _lib.PVO_ABI_VERSION == 106               # the ABI version and pvo_graph_update_args stay
    # argument checks are host code: they answer without a device
    assert loaded.pvo_ba_depth_prior(None, 1 << 20, 4, 3, 4, 16, 16, 0.05, None) == 1                # NULL workspace: PVO_EINVAL
    assert loaded.pvo_ba_depth_prior(256, 16, 4, 3, 4, 16, 16, 0.05, None) == 3                      # workspace too small: PVO_EWORKSPACE
    assert loaded.pvo_ba_depth_prior(256, 1 << 30, 4, 3, 4, 16, 16, 0.0, None) == 1                  # a map with alpha = 0
    assert loaded.pvo_depth_sense(16, 16, 16, 16, _lib.PVO_BF16, None) == 4                          # odd dtype: PVO_EUNSUPPORTED
    assert loaded.pvo_depth_sense(16, 16, 16, 16, 7, None) == 4
    assert loaded.pvo_depth_sense(None, 16, 16, 16, _lib.PVO_F32, None) == 1                         # NULL image
    assert loaded.pvo_depth_sense(16, 16, -1, 16, _lib.PVO_F32, None) == 1
    assert loaded.pvo_depth_sense(None, None, 7, 64, _lib.PVO_F32, None) == 0                        # no lattice row: nothing to do
    assert loaded.pvo_ba_prior(*([None] * 8), 4, 4, 4, 4, 4, 1, 4, -1, 1e-4, 0.1, 0, None, None, 0, None, None, 0, None, 0.05, None) == 1
    assert loaded.pvo_ba_prior(*([None] * 8), 4, 4, 4, 4, 4, 1, 4, 1, 1e-4, 0.1, 0, None, None, 0, None, 256, 1 << 30, 16, -1.0, None) == 1


# ------------------------------------------------------------------------------------------------ the reference qualifies
def _small():
    s = R.window(11, 5, 12, 16, radius=2, t0=1, measured=0.7, residual=0.0)
    assert s["ii"].shape[0] == 14
    return s


def test_reference_without_a_sensor_map_is_the_oracles_ba():
    s = _small()
    n = lambda t: t.numpy()
    want = O.ba(n(s["poses"]), n(s["disps"]), n(s["intr"]), n(s["target"]), n(s["weight"]), n(s["eta"]), n(s["ii"]), n(s["jj"]),
                1, 5, 2, 1e-4, 0.1)
    poses, disps = R.reference(s, 2, sens=None)
    ep, ed = np.abs(poses - want["poses"]).max(), np.abs(disps - want["disps"]).max()
    print("reference vs oracle.ba, no sensor map: poses %.2e disps %.2e" % (ep, ed))
    assert ep < 1e-5 and ed < 1e-5
    poses0, disps0 = R.reference(s, 2, sens=np.zeros_like(n(s["sens"])))        # an all-zero map is no map
    assert np.array_equal(poses0, poses) and np.array_equal(disps0, disps)


def test_reference_with_a_residual_zero_map_is_the_oracles_ba_under_the_swapped_eta():
    """sens == disps on ~70 % of the pixels: the residual is exactly 0, so the term only replaces eta by alpha there.  One step: after
    it the depths have moved and the residual is no longer 0."""
    s = _small()
    n = lambda t: t.numpy()
    assert 0.6 < float((s["sens"] > 0).float().mean()) < 0.8 and torch.equal(s["sens"][s["sens"] > 0], s["disps"][s["sens"] > 0])
    eta2 = R.swapped_eta(s)
    want = O.ba(n(s["poses"]), n(s["disps"]), n(s["intr"]), n(s["target"]), n(s["weight"]), n(eta2), n(s["ii"]), n(s["jj"]),
                1, 5, 1, 1e-4, 0.1)
    poses, disps = R.reference(s, 1)
    ep, ed = np.abs(poses - want["poses"]).max(), np.abs(disps - want["disps"]).max()
    print("reference vs oracle.ba(eta'), residual-zero map: poses %.2e disps %.2e" % (ep, ed))
    assert ep < 1e-5 and ed < 1e-5
    plain = R.reference(s, 1, sens=None)
    assert np.abs(plain[1] - disps).max() > 1e-3                                # ... and the swap is not a no-op


def test_reference_keeps_a_frame_without_out_edges():
    """the deg > 0 rule: frame 4 of the window has in-edges only - its depth map stays although it carries measurements"""
    ii, jj = R.radius_graph(5, 2)
    keep = ii != 4
    s = R.window(12, 5, 12, 16, t0=1, ii=ii[keep], jj=jj[keep], residual=0.1)
    poses, disps = R.reference(s, 2)
    assert np.array_equal(disps[4], s["disps"][4].numpy()) and np.abs(disps[3] - s["disps"][3].numpy()).max() > 1e-3


# ------------------------------------------------------------------------------------------------ host logic
def _depth_image(ht, wd, seed=0):
    g = torch.Generator().manual_seed(seed)
    d = torch.rand(ht, wd, generator=g) * 4 + 0.5
    d[3, 3], d[3, 11], d[11, 3], d[11, 11], d[19, 19] = 0.0, -1.0, float("nan"), float("inf"), -float("inf")
    return d


def _lattice_reference(d):
    h8, w8 = d.shape[0] // 8, d.shape[1] // 8
    out = torch.zeros(h8, w8)
    for y in range(h8):
        for x in range(w8):
            v = float(d[8 * y + 3, 8 * x + 3])
            out[y, x] = (torch.tensor(1.0) / torch.tensor(v)) if (v > 0 and np.isfinite(v)) else 0.0
    return out


@pytest.mark.parametrize("ht,wd", [(48, 64), (44, 60)])
def test_ingest_samples_the_lattice_and_zeroes_invalid_values(ht, wd):
    from pvo_amd.depth_video import DepthVideo
    v = DepthVideo(image_size=(ht, wd), buffer=4, device="cpu")
    assert v.disps_sens is None and v.has_sensor_depth is False
    d = _depth_image(ht, wd)
    z = torch.zeros(128, ht // 8, wd // 8, dtype=torch.half)
    v.append(0.0, None, None, torch.ones(4), z, z, z)                           # a keyframe without depth: nothing is allocated
    assert v.disps_sens is None and v.has_sensor_depth is False
    v.append(1.0, None, None, torch.ones(4), z, z, z, depth=d)
    assert v.has_sensor_depth is True and v.disps_sens.shape == v.disps.shape == (4, ht // 8, wd // 8)
    want = _lattice_reference(d)
    assert torch.equal(v.disps_sens[1], want) and not v.disps_sens[0].any()
    assert want[0, 0] == 0 and want[0, 1] == 0 and want[1, 0] == 0 and want[1, 1] == 0 and want[2, 2] == 0 and int((want > 0).sum()) == want.numel() - 5
    v.append(2.0, None, None, torch.ones(4), z, z, z, depth=d.half())           # a 16-bit image
    assert torch.equal(v.disps_sens[2], _lattice_reference(d.half().float()))
    v.disps_sens[3] = 7.0                                                       # (a stale row, as rm_keyframe leaves one)
    v.append(3.0, None, None, torch.ones(4), z, z, z)
    assert not v.disps_sens[3].any()
    # upstream's item form
    v[1] = (1.0, None, None, None, None, None, z, z, None, 2 * d)
    assert torch.equal(v.disps_sens[1], _lattice_reference(2 * d))
    with pytest.raises(ValueError):
        v.append(4.0, None, None, torch.ones(4), z, z, z, depth=torch.ones(ht + 8, wd))


def test_rm_keyframe_moves_the_sensor_map():
    from test_cvx_upsample_host import _host_graph
    v, fg, _, _ = _host_graph(False)
    fg.corr = None
    fg.ii_inac = fg.jj_inac = torch.zeros(0, dtype=torch.long)
    sens = v.ensure_disps_sens()
    sens[:] = torch.arange(6, dtype=torch.float)[:, None, None]
    v.has_sensor_depth = True
    fg.rm_factors = lambda mask, store=False: None
    fg.rm_keyframe(2)
    assert [float(sens[k, 0, 0]) for k in range(6)] == [0.0, 1.0, 3.0, 3.0, 4.0, 5.0]
    v2, fg2, _, _ = _host_graph(False)                                         # without a map there is nothing to move
    fg2.corr = None
    fg2.ii_inac = fg2.jj_inac = torch.zeros(0, dtype=torch.long)
    fg2.rm_factors = lambda mask, store=False: None
    fg2.rm_keyframe(2)
    assert v2.disps_sens is None


def test_frontend_seeds_the_new_keyframe_before_the_first_update():
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.frontend import DroidFrontend
    v = DepthVideo(image_size=(40, 56), buffer=8, device="cpu")
    v.counter = 5
    g = torch.Generator().manual_seed(3)
    v.disps[:] = torch.rand(8, 5, 7, generator=g) + 0.5
    sens = v.ensure_disps_sens()
    sens[:] = torch.where(torch.rand(8, 5, 7, generator=g) < 0.6, torch.rand(8, 5, 7, generator=g) + 2.0, torch.zeros(8, 5, 7))
    v.has_sensor_depth = True
    fe = DroidFrontend(lambda *a, **k: None, v, device="cpu")
    fe.t1, fe.is_initialized = 4, True
    before = v.disps.clone()
    log = []
    fe.graph.corr = None
    fe.graph.add_proximity_factors = lambda *a, **k: log.append(("prox", v.disps.clone()))
    fe.graph.update = lambda *a, **k: log.append(("update", v.disps.clone()))
    v.distance = lambda *a, **k: torch.tensor([1.0])
    fe._update_begin()
    assert [n for n, _ in log] == ["prox"] + ["update"] * 4
    assert torch.equal(log[0][1], before)                                      # after add_proximity_factors ...
    want = before.clone()
    want[4] = torch.where(sens[4] > 0, sens[4], before[4])
    assert torch.equal(log[1][1], want) and not torch.equal(want, before)      # ... before the first update, the new keyframe only
    # without sensor depth the frontend leaves the depths alone
    v.has_sensor_depth = False
    v.disps[:] = before
    log.clear()
    fe.t1 = 4
    fe._update_begin()
    assert torch.equal(log[1][1], before)


def test_backend_skips_normalize_exactly_when_the_video_holds_sensor_depth():
    from pvo_amd.backend import DroidBackend
    from pvo_amd.depth_video import DepthVideo
    v = DepthVideo(image_size=(40, 56), buffer=8, device="cpu")
    v.counter = 4
    calls = []
    v.normalize = lambda: calls.append("normalize")
    be = DroidBackend(Namespace(update=None), v, Namespace(device="cpu", backend_radius=2, backend_nms=3, backend_thresh=15.0, beta=0.3))
    graph = Namespace(_ii_h=[], clear_edges=lambda: None)
    be._connect_all = lambda keep=None: (graph, ([], []))
    be(2)
    assert calls == ["normalize"]
    v.has_sensor_depth = True
    be(2)
    assert calls == ["normalize"]


def test_the_switch_off_ignores_depth_and_allocates_nothing():
    from pvo_amd.droid import Droid, default_args
    assert default_args().rgbd is False
    torch.manual_seed(0)
    image = torch.randint(0, 255, (3, 32, 48), dtype=torch.uint8)
    depth = torch.rand(32, 48) + 1.0
    intr = torch.tensor([30.0, 30.0, 24.0, 16.0])
    for rgbd in (False, True):
        droid = Droid(default_args(device="cpu", image_size=[32, 48], buffer=4, half_update=False, rgbd=rgbd))
        assert droid.filterx.use_depth is rgbd
        seen = []
        real = droid.video.append
        droid.video.append = lambda *a, **k: (seen.append(dict(k)), real(*a, **k))[1]
        droid.filterx.track_vo(0.0, image, depth, intr)
        droid.filterx.track_vo(1.0, image, None, intr)                         # a frame without depth in an RGB-D run
        assert ("depth" in seen[0]) is rgbd and "depth" not in seen[1]
        if rgbd:
            assert droid.video.has_sensor_depth and torch.equal(droid.video.disps_sens[0], 1.0 / depth[3::8, 3::8])
            assert not droid.video.disps_sens[1].any()
        else:
            assert droid.video.disps_sens is None and droid.video.has_sensor_depth is False


def test_factor_graph_sets_the_prior_after_a_replan_and_not_otherwise(monkeypatch):
    from pvo_amd import droid_backends as db
    from test_cvx_upsample_host import _host_graph
    v, fg, _, _ = _host_graph(False)
    log = []
    monkeypatch.setattr(db, "ba_workspace_bytes", lambda *a: 64)
    monkeypatch.setattr(db, "ba_plan", lambda ii, jj, F, HW, K, t0, t1, ws: log.append(("plan", K)))
    monkeypatch.setattr(db, "ba_depth_prior", lambda ws, E, P, F, HW, sens, alpha=0.05: log.append(("prior", E, P, F, HW, sens.data_ptr(), alpha)))
    ii, jj = fg.ii, fg.jj
    fg._ba_plan(ii, jj, 1, 4, False, 0, 3)
    assert log == [("plan", 3)]                                                # no sensor depth: today's plan, nothing else
    fg._ba_plan(ii, jj, 1, 4, False, 0, 3)
    assert log == [("plan", 3)]                                                # cached
    sens = v.ensure_disps_sens()                                               # allocated before the plan: a persistent buffer
    v.has_sensor_depth = True
    fg._ba_plan(ii, jj, 1, 4, False, 0, 3)                                     # the flag came up: a re-plan, the prior behind it
    assert log[1:] == [("plan", 3), ("prior", 5, 3, 6, 35, sens.data_ptr(), 0.05)]
    fg._ba_plan(ii, jj, 1, 4, False, 0, 3)
    assert len(log) == 3                                                       # same edge set: neither
    fg._version += 1                                                           # an edge-set change
    fg._ba_plan(ii, jj, 1, 4, False, 0, 3)
    assert [x[0] for x in log[3:]] == ["plan", "prior"]
    fg._ba_plan(ii, jj, 1, 4, True, 0, 3)                                      # a motion-only plan carries no prior
    assert log[5:] == [("plan", -1)]


def test_sharded_ba_sets_the_prior_behind_its_plan():
    from pvo_amd.parallel import ShardedBA
    log = []

    class Backend:
        def ba_workspace(self, *a): return torch.zeros(8)
        def ba_plan(self, *a): log.append("plan")
        def ba_depth_prior(self, ws, E, P, F, HW, sens, alpha): log.append(("prior", None if sens is None else sens.data_ptr(), alpha))
        def ba_local(self, *a, **k): log.append("local")
        def ba_finish(self, *a, **k): log.append("finish"); return torch.zeros(2, 6), None
    sb = ShardedBA(backend=Backend(), communicate=False)
    poses, disps = torch.zeros(4, 7), torch.ones(4, 3, 5)
    sens = torch.ones(4, 3, 5)
    a = (poses, disps, torch.ones(4), torch.zeros(3, 2, 3, 5), torch.zeros(3, 2, 3, 5), torch.ones(3, 3, 5), torch.tensor([1, 2, 3]), torch.tensor([2, 3, 1]), 1, 3)
    sb.ba(*a, itrs=1, plan_key="k")
    assert log == ["plan", "local", "finish"]                                  # no map: no call the CPU backends lack
    sb.ba(*a, itrs=1, plan_key="k", disps_sens=sens)
    assert log[3:] == [("prior", sens.data_ptr(), 0.05), "local", "finish"]
    sb.ba(*a, itrs=1, plan_key="k", disps_sens=sens)
    assert log[6:] == ["local", "finish"]                                      # same plan, same map: nothing to set
    sb.ba(*a, itrs=1, plan_key="k2", disps_sens=sens)
    assert log[8:] == ["plan", ("prior", sens.data_ptr(), 0.05), "local", "finish"]
    sb.ba(*a, itrs=1, plan_key="k2")
    assert log[12:] == [("prior", None, 0.05), "local", "finish"]              # the map went away: cleared


# ------------------------------------------------------------------------------------------------ closed loop
def sensor_map(scene, missing=0.3, seed=5):
    """scene.disps with `missing` of the pixels zeroed by a seeded draw and columns 0-2 blank"""
    g = torch.Generator().manual_seed(seed)
    s = torch.where(torch.rand(scene.disps.shape, generator=g) < missing, torch.zeros_like(scene.disps), scene.disps)
    s[..., :3] = 0
    return s


def depth_images(sens):
    """full-resolution depth images whose [3::8, 3::8] lattice is 1 / sens (0 = no measurement)"""
    n, h, w = sens.shape
    d = torch.zeros(n, 8 * h, 8 * w)
    d[:, 3::8, 3::8] = torch.where(sens > 0, 1.0 / sens.clamp(min=1e-6), torch.zeros_like(sens))
    return d


def run_rgbd_sequence(scene, video, frontend, operator, depth):
    """pvo_amd.synthetic.run_sequence with a depth image per frame"""
    dev = video.poses.device
    h, w = scene.ht, scene.wd
    g = torch.Generator().manual_seed(1)
    for k in range(scene.n):
        slot = video.counter
        operator.bind(slot, k)
        video.append(float(k), None if k else scene.poses[0].to(dev), None, scene.intr.to(dev),
                     torch.randn(h, w, 128, generator=g).half().to(dev),
                     torch.zeros(128, h, w, dtype=torch.half, device=dev), torch.zeros(128, h, w, dtype=torch.half, device=dev),
                     **({"depth": depth[k]} if depth is not None else {}))
        frontend()
        if video.counter <= slot:
            operator.frame_of.pop(slot, None)
            operator.bind(video.counter - 1, k)
    frames = [operator.frame_of.get(s, s) for s in range(video.counter)]
    return video.poses[:video.counter].detach().cpu().clone(), frames


def metric_figures(poses, frames, scene):
    """(ATE-RMSE without alignment / path length, ATE-RMSE after Sim(3) alignment, estimated / true path scale)"""
    from pvo_amd.trajectory import ate_rmse, camera_centres
    gt = camera_centres(scene.poses[frames].numpy())
    est = camera_centres(poses.numpy())
    length = np.linalg.norm(np.diff(gt, axis=0), axis=1).sum()
    scale = np.linalg.norm(np.diff(est, axis=0), axis=1).sum() / length
    return ate_rmse(est, gt, align=False) / length, ate_rmse(est, gt), scale


def test_closed_loop_on_the_cpu_is_metric_with_sensor_depth():
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.synthetic import OracleFlowOperator, PlaneScene
    from test_synthetic_vo import OracleVideo, _oracle_reproject

    class RefVideo(OracleVideo):
        """OracleVideo with DepthVideo's sensor map (its own ingest) and `ba` answered by the dense reference"""
        def __init__(self, ht, wd, buffer):
            super().__init__(ht, wd, buffer)
            self.disps_sens, self.has_sensor_depth, self.sensor_alpha = None, False, R.ALPHA

        def append(self, tstamp, pose, disp, intrinsics, *unused, depth=None):
            if depth is not None:
                if self.disps_sens is None:
                    self.disps_sens = torch.zeros_like(self.disps)
                self.disps_sens[self.counter] = DepthVideo.sense_depth_host(depth)
                self.has_sensor_depth = True
            super().append(tstamp, pose, disp, intrinsics)

        def ba(self, target, weight, eta, ii, jj, t0=1, t1=None, itrs=2, lm=1e-4, ep=0.1, motion_only=False):
            assert not motion_only
            p, d = R.ba(self.poses.numpy(), self.disps.numpy(), self.intrinsics[0].numpy(), target.numpy(), weight.numpy(), eta.numpy(),
                        ii.numpy(), jj.numpy(), t0, t1, itrs, lm, ep, self.disps_sens.numpy() if self.has_sensor_depth else None)
            self.poses.copy_(torch.from_numpy(p)); self.disps.copy_(torch.from_numpy(d).clamp(min=0.001))

    scene = PlaneScene(ht=24, wd=32, n_frames=14, seed=0)
    kw = dict(warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20, frontend_radius=2, frontend_nms=1)
    out = {}
    for name, depth in (("monocular", None), ("rgbd", depth_images(sensor_map(scene)))):
        ov = RefVideo(scene.ht, scene.wd, buffer=32)
        op = OracleFlowOperator(scene, ov, _oracle_reproject)
        fe = DroidFrontend(op, ov, device="cpu", **kw)
        fe.graph.corr_impl = "none"
        fe.graph.corr = type("NoVolumes", (), {"__call__": lambda self, coords, **kw: None})()
        poses, frames = run_rgbd_sequence(scene, ov, fe, op, depth)
        out[name] = metric_figures(poses, frames, scene) + (len(frames),)
        print("%s: ATE-RMSE without alignment %.5f of the path, aligned %.2e, path scale %.4f, %d keyframes" % ((name,) + out[name]))
    assert out["rgbd"][3] == out["monocular"][3] == 14
    assert out["rgbd"][0] <= 0.005                                             # metric: within 0.5 % of the path length, no alignment
    assert abs(out["rgbd"][2] - 1.0) < 0.01
    assert out["monocular"][0] > 0.1                                           # (the monocular run is defined up to scale only)
    assert abs(out["rgbd"][1] - out["monocular"][1]) < 1e-3
