"""Stereo tracking, the parts that need no GPU: the C ABI of the new entry points and the grown pvo_graph_update_args, the tests' own
fp64 yardstick of the bundle adjustment with stereo edges (tests/stereo_reference.py) qualified before anything is held to it, the
host logic (right feature maps in DepthVideo, which edges the factor graph requests and what it correlates them against,
rm_keyframe, the motion filter, the switch, the backend's normalisation, the plan hooks, tools/vo_stereo.py) on CPU tensors with
the native calls stubbed, and the closed loop on the CPU: a stereo run is metric.

The closed loop decides the baseline of the GPU closed loop (tests/test_stereo_gpu.py imports BASELINE from here)."""
import ctypes
import os
import re
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import rgbd_reference as R
import stereo_reference as S
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pvo_ba_stereo", "pvo_ba_rig", "pvo_reproject_rig", "pvo_reproject_motion_rig", "pvo_graph_update_rig")
BASELINE = 0.1            # the closed loops' baseline: see test_closed_loop_on_the_cpu_is_metric_with_stereo_edges


# ------------------------------------------------------------------------------------------------ C ABI
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
    assert re.search(r"#define\s+PVO_ABI_VERSION\s+106\b", header)
    # argument checks are host code: they answer without a device
    assert loaded.pvo_ba_stereo(None, 1 << 20, 4, 3, 4, 16, 0.1, None) == 1                          # NULL workspace: PVO_EINVAL
    assert loaded.pvo_ba_stereo(256, 16, 4, 3, 4, 16, 0.1, None) == 3                                # workspace too small: PVO_EWORKSPACE
    assert loaded.pvo_ba_stereo(256, 1 << 30, 4, 3, 4, 16, -0.1, None) == 1                          # a negative baseline
    assert loaded.pvo_ba_stereo(256, 1 << 30, 4, 3, 4, 16, float("nan"), None) == 1
    assert loaded.pvo_ba_stereo(256, 1 << 30, 4, 3, 4, 16, float("inf"), None) == 1
    assert loaded.pvo_reproject_rig(*([16] * 7), 2, 4, 4, -1.0, None) == 1
    assert loaded.pvo_reproject_rig(*([None] * 7), 0, 4, 4, 0.1, None) == 0                          # no edge: nothing to do
    assert loaded.pvo_reproject_motion_rig(*([16] * 11), 2, 4, 4, _lib.PVO_F16, float("nan"), None) == 1
    assert loaded.pvo_ba_rig(*([None] * 8), 4, 4, 4, 4, 4, 1, 4, 1, 1e-4, 0.1, 0, None, None, 0, None, 256, 1 << 30, None, 0.05, -0.5, None) == 1


def test_graph_update_args_stay_and_the_baseline_is_an_argument_of_its_own_entry_point():
    from pvo_amd import _lib
    lib = _lib.load()
    a = _lib.GraphUpdateArgs
    assert lib.pvo_graph_update_args_size() == ctypes.sizeof(a)
    names = [f[0] for f in a._fields_]
    assert names[-3:] == ["want_upsample", "disps_up", "up_frames"] and "stereo_baseline" not in names      # the struct is pinned
    assert _lib.SIGNATURES["pvo_graph_update_rig"][1] == _lib.SIGNATURES["pvo_graph_update"][1][:-1] + [ctypes.c_float, ctypes.c_void_p]
    # argument checks are host code: they answer without a device
    w, u = _lib.UpdateWeights(), a()
    for bad in (-0.1, float("nan"), float("inf")):
        assert lib.pvo_graph_update_rig(ctypes.byref(w), ctypes.byref(u), None, 0, bad, None) == 1           # PVO_EINVAL
    assert lib.pvo_graph_update_rig(None, None, None, 0, 0.1, None) == 1


# ------------------------------------------------------------------------------------------------ the yardstick qualifies
def test_yardstick_without_a_stereo_edge_is_the_rgbd_yardstick_exactly():
    s = R.window(11, 5, 12, 16, radius=2, t0=1)
    n = lambda t: t.numpy()
    a = (n(s["poses"]), n(s["disps"]), n(s["intr"]), n(s["target"]), n(s["weight"]), n(s["eta"]), n(s["ii"]), n(s["jj"]), 1, 5, 1e-4, 0.1)
    want = R.gn_step(*a, sens=None)
    for b in (0.0, 0.1):                                                         # (no edge (i, i) in the graph: the baseline is inert)
        got = S.gn_step(*a, baseline=b)
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
    # identity edges (i, i) with baseline 0 stay ordinary edges: the oracle's assembly for all of them
    ii, jj = S.with_stereo_edges(n(s["ii"]), n(s["jj"]), [1, 3])
    s2 = R.window(11, 5, 12, 16, t0=1, ii=ii, jj=jj)
    a2 = (n(s2["poses"]), n(s2["disps"]), n(s2["intr"]), n(s2["target"]), n(s2["weight"]), n(s2["eta"]), ii, jj, 1, 5, 1e-4, 0.1)
    assert all(np.array_equal(x, y) for x, y in zip(S.gn_step(*a2, baseline=0.0), R.gn_step(*a2, sens=None)))
    assert not np.array_equal(S.gn_step(*a2, baseline=0.1)[1], R.gn_step(*a2, sens=None)[1])
    # ... and the sensor-depth prior rides along unchanged
    sens = n(s["sens"])
    assert all(np.array_equal(x, y) for x, y in zip(S.gn_step(*a, baseline=0.1, sens=sens), R.gn_step(*a, sens=sens)))


def _phantom_case(F=4, ht=12, wd=16, b=0.1, seed=21):
    """depth-only window (t0 == t1, P == 0): the stereo edges (i, i) of every frame, and the same constraints as ordinary edges
    (i, F + i) to appended phantom frames whose pose is T_b o G_i"""
    s = S.window(seed, F, ht, wd, b, range(F), ii=np.zeros(0, np.int64), jj=np.zeros(0, np.int64), t0=F)
    assert s["ii"].tolist() == s["jj"].tolist() == list(range(F)) and s["t0"] == s["t1"] == F and s["eta"].shape[0] == F
    poses2 = torch.cat([s["poses"], s["poses"]]).clone()
    poses2[F:, 0] -= b                                                           # T_b o G_i: the same rotation, t_i + (-b, 0, 0)
    disps2 = torch.cat([s["disps"], torch.ones_like(s["disps"])])
    jj2 = s["jj"] + F
    return s, poses2, disps2, jj2


def test_yardstick_stereo_edges_are_ordinary_edges_to_phantom_right_cameras():
    s, poses2, disps2, jj2 = _phantom_case()
    F = s["disps"].shape[0]
    n = lambda t: t.numpy()
    want = O.ba(n(poses2), n(disps2), n(s["intr"]), n(s["target"]), n(s["weight"]), n(s["eta"]), n(s["ii"]), n(jj2), 2 * F, 2 * F, 2, 1e-4, 0.1)
    poses, disps = S.reference(s, 2)
    gap = np.abs(disps - want["disps"][:F]).max()
    moved = np.abs(disps - n(s["disps"])).max()
    print("stereo edges vs phantom frames through oracle.ba: depths differ by %.2e (the step moves them by up to %.3f)" % (gap, moved))
    assert np.array_equal(poses, n(s["poses"])) and gap < 1e-5 and moved > 1e-2
    assert np.array_equal(want["disps"][F:], n(disps2)[F:])                      # (the phantom frames have no out-edge)


def test_yardstick_jz_is_the_finite_difference_of_the_projection():
    intr, b = np.array([20.0, 19.0, 8.0, 6.0]), 0.37
    g = np.random.default_rng(3)
    u, v, d = g.uniform(0, 16, 50), g.uniform(0, 12, 50), g.uniform(0.1, 2.0, 50)
    h = 1e-4
    pu1, pv1 = S.stereo_project(u, v, d + h, intr, b)
    pu0, pv0 = S.stereo_project(u, v, d - h, intr, b)
    ju, jv = S.stereo_jz(intr, b)
    assert np.abs((pu1 - pu0) / (2 * h) - ju).max() < 1e-8 and np.abs((pv1 - pv0) / (2 * h) - jv).max() < 1e-8
    pu, pv = S.stereo_project(u, v, d, intr, b)
    assert np.allclose(pu, u - intr[0] * b * d, atol=1e-12) and np.allclose(pv, v, atol=1e-12)      # u_right = u - fx b d, v_right = v
    # ... and the terms are what that Jacobian gives
    disp = g.uniform(0.3, 1.5, (4, 5)).astype(np.float32)
    tgt, wgt = g.uniform(0, 5, (2, 4, 5)).astype(np.float32), g.uniform(0.5, 1.5, (2, 4, 5)).astype(np.float32)
    C, w = S.stereo_terms(disp, intr, tgt, wgt, b)
    vv, uu = np.meshgrid(np.arange(4.0), np.arange(5.0), indexing="ij")
    ru = tgt[0].astype(np.float64) - (uu - intr[0] * b * disp.astype(np.float64))
    assert np.allclose(C, (0.001 * wgt[0].astype(np.float64) * ju * ju).reshape(-1), rtol=1e-12)
    assert np.allclose(w, (0.001 * wgt[0].astype(np.float64) * ru * ju).reshape(-1), rtol=1e-9, atol=1e-15)


# ------------------------------------------------------------------------------------------------ host logic
def _video(ht=5, wd=7, buffer=8):
    from pvo_amd.depth_video import DepthVideo
    v = DepthVideo(image_size=(ht * 8, wd * 8), buffer=buffer, device="cpu")
    v.reproject = lambda ii, jj: (torch.zeros(1, len(ii), ht, wd, 2), torch.ones(1, len(ii), ht, wd, 1))
    v.reproject_into = lambda ii, jj, dst: dst.zero_()
    return v


def _fill(v, n, stereo=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    h, w = v.ht // 8, v.wd // 8
    z = torch.zeros(128, h, w, dtype=torch.half)
    for k in range(n):
        kw = {"right_fmap": torch.randn(h, w, 128, generator=g).half()} if stereo else {}
        v.append(float(k), None, None, torch.ones(4), torch.randn(h, w, 128, generator=g).half(), z, z, **kw)


def test_append_takes_the_right_map_in_both_layouts_and_allocates_on_first_use():
    v = _video()
    h, w = 5, 7
    g = torch.Generator().manual_seed(1)
    z = torch.zeros(128, h, w, dtype=torch.half)
    f = torch.randn(h, w, 128, generator=g).half()
    v.append(0.0, None, None, torch.ones(4), f, z, z)
    assert v.fmaps_right is None and v.has_stereo is False and v.stereo_baseline == 0.1 and v.rig_baseline() == 0.0
    r_cl = torch.randn(h, w, 128, generator=g).half()
    v.append(1.0, None, None, torch.ones(4), f, z, z, right_fmap=r_cl)                           # channels-last
    assert v.has_stereo is True and v.fmaps_right.shape == v.fmaps.shape and v.fmaps_right.dtype == torch.half
    assert torch.equal(v.fmaps_right[1], r_cl) and not v.fmaps_right[0].any() and v.rig_baseline() == 0.1
    r_cf = torch.randn(128, h, w, generator=g).half()
    v.append(2.0, None, None, torch.ones(4), f.permute(2, 0, 1), z, z, right_fmap=r_cf)           # the reference's [128,h,w]
    assert torch.equal(v.fmaps_right[2], r_cf.permute(1, 2, 0)) and torch.equal(v.fmaps[2], f)
    v.fmaps_right[3] = 7.0                                                                        # (a stale row, as rm_keyframe leaves one)
    v.append(3.0, None, None, torch.ones(4), f, z, z)
    assert not v.fmaps_right[3].any()
    v.stereo_baseline = 0.0                                                                       # b == 0 is off
    assert v.has_stereo is False and v.rig_baseline() == 0.0 and v._rig_kw("baseline") == {}
    with pytest.raises(ValueError):
        v.append(4.0, None, None, torch.ones(4), f, z, z, right_fmap=torch.zeros(64, h, w).half())


class _RecordingCorr:
    """stands in for the correlation block: records the feature rows every add_factors hands over"""
    log = []

    def __init__(self, fmap1, fmap2, channels_last=False):
        assert channels_last
        self.n = fmap1.shape[1]
        _RecordingCorr.log.append((fmap1[0].clone(), fmap2[0].clone()))

    def cat(self, other):
        self.n += other.n
        return self

    def __getitem__(self, idx):
        return self


def _graph(v, monkeypatch, max_factors=-1):
    from pvo_amd import factor_graph
    from pvo_amd.factor_graph import FactorGraph
    _RecordingCorr.log = []
    monkeypatch.setattr(factor_graph, "CorrBlock", _RecordingCorr)
    return FactorGraph(v, lambda *a, **k: None, device="cpu", max_factors=max_factors)


def test_neighborhood_factors_request_one_stereo_edge_per_keyframe_in_front_and_correlate_it_against_the_right_map(monkeypatch):
    v = _video()
    _fill(v, 5)
    fg = _graph(v, monkeypatch)
    fg.add_neighborhood_factors(0, 5, r=2)
    E = len(fg._ii_h)
    assert list(zip(fg._ii_h, fg._jj_h))[:5] == [(k, k) for k in range(5)]                        # in front of the other edges
    assert sum(i == j for i, j in zip(fg._ii_h, fg._jj_h)) == 5 and E == 5 + 14
    f1, f2 = _RecordingCorr.log[0]
    for e, (i, j) in enumerate(zip(fg._ii_h, fg._jj_h)):
        assert torch.equal(f1[e], v.fmaps[i])
        assert torch.equal(f2[e], v.fmaps_right[i] if i == j else v.fmaps[j])
    assert not torch.equal(v.fmaps_right[0], v.fmaps[0])
    fg.add_neighborhood_factors(0, 5, r=2)                                                        # all of them exist: nothing is added
    assert len(fg._ii_h) == E and len(_RecordingCorr.log) == 1
    # aged into the inactive list they are not requested again
    fg.rm_factors([i == j for i, j in zip(fg._ii_h, fg._jj_h)], store=True)
    assert sorted(zip(fg._ii_inac_h, fg._jj_inac_h)) == [(k, k) for k in range(5)] and all(i != j for i, j in zip(fg._ii_h, fg._jj_h))
    fg.add_neighborhood_factors(0, 5, r=2)
    assert len(fg._ii_h) == E - 5 and len(_RecordingCorr.log) == 1


def test_without_a_right_view_no_stereo_edge_is_requested_and_identity_edges_keep_the_left_map(monkeypatch):
    v = _video()
    _fill(v, 5, stereo=False)
    fg = _graph(v, monkeypatch)
    fg.add_neighborhood_factors(0, 5, r=2)
    assert v.fmaps_right is None and len(fg._ii_h) == 14 and all(i != j for i, j in zip(fg._ii_h, fg._jj_h))
    fg.add_factors([2], [2])                                                                      # an (i, i) edge stays an identity edge
    f1, f2 = _RecordingCorr.log[-1]
    assert torch.equal(f1[0], v.fmaps[2]) and torch.equal(f2[0], v.fmaps[2])
    # a stereo video with baseline 0 is off too
    v2 = _video()
    _fill(v2, 4)
    v2.stereo_baseline = 0.0
    fg2 = _graph(v2, monkeypatch)
    fg2.add_neighborhood_factors(0, 4, r=1)
    assert all(i != j for i, j in zip(fg2._ii_h, fg2._jj_h))
    fg2.add_factors([1], [1])
    assert torch.equal(_RecordingCorr.log[-1][1][0], v2.fmaps[1])


@pytest.mark.parametrize("native", [True, False])
def test_proximity_factors_request_one_stereo_edge_per_keyframe(monkeypatch, native):
    v = _video(buffer=12)
    _fill(v, 7)
    v.distance = lambda ii, jj, beta=0.3, bidirectional=True: torch.as_tensor(3.0 * np.abs(np.asarray(ii) - np.asarray(jj)), dtype=torch.float)
    fg = _graph(v, monkeypatch)
    fg.native_select = native
    fg.add_proximity_factors(2, 0, rad=2, nms=1, thresh=7.0)
    pairs = list(zip(fg._ii_h, fg._jj_h))
    assert pairs[:5] == [(k, k) for k in range(2, 7)]                                             # the keyframes of [t0, t), in front
    assert sum(i == j for i, j in pairs) == 5 and len(pairs) > 5                                  # one each (the other edges follow the reference's rules)
    plain = _video(buffer=12)
    _fill(plain, 7, stereo=False)
    plain.distance = v.distance
    fg0 = _graph(plain, monkeypatch)
    fg0.native_select = native
    fg0.add_proximity_factors(2, 0, rad=2, nms=1, thresh=7.0)
    assert pairs[5:] == list(zip(fg0._ii_h, fg0._jj_h))                                           # the other edges are the monocular run's
    # the next keyframe: only ITS stereo edge is new; the aged ones wait in the inactive list and are not requested twice
    fg = _graph(v, monkeypatch)
    fg.native_select = native
    fg.add_proximity_factors(2, 0, rad=2, nms=1, thresh=7.0)
    fg.rm_factors([(i == j and i < 4) for i, j in zip(fg._ii_h, fg._jj_h)], store=True)
    g = torch.Generator().manual_seed(5)
    z = torch.zeros(128, 5, 7, dtype=torch.half)
    v.append(7.0, None, None, torch.ones(4), torch.randn(5, 7, 128, generator=g).half(), z, z, right_fmap=torch.randn(5, 7, 128, generator=g).half())
    before = len(fg._ii_h)
    fg.add_proximity_factors(3, 0, rad=2, nms=1, thresh=7.0)
    new = list(zip(fg._ii_h, fg._jj_h))[before:]
    assert [p for p in new if p[0] == p[1]] == [(7, 7)] and new[0] == (7, 7)
    everything = list(zip(fg._ii_h, fg._jj_h)) + list(zip(fg._ii_inac_h, fg._jj_inac_h))
    assert sorted(p for p in everything if p[0] == p[1]) == [(k, k) for k in range(2, 8)]


def test_rm_keyframe_moves_the_right_map(monkeypatch):
    v = _video()
    _fill(v, 5)
    v.counter = 5
    fg = _graph(v, monkeypatch)
    fg.add_neighborhood_factors(0, 5, r=1)
    right = v.fmaps_right.clone()
    fg.rm_keyframe(2)
    assert torch.equal(v.fmaps_right[2], right[3]) and torch.equal(v.fmaps_right[1], right[1]) and torch.equal(v.fmaps[2], v.fmaps[3])
    # (frame 2's stereo edge went with it; frame 3's is now (2, 2))
    assert sorted(p for p in zip(fg._ii_h, fg._jj_h) if p[0] == p[1]) == [(0, 0), (1, 1), (2, 2), (3, 3)]
    plain = _video()
    _fill(plain, 5, stereo=False)
    fg0 = _graph(plain, monkeypatch)
    fg0.add_neighborhood_factors(0, 5, r=1)
    fg0.rm_keyframe(2)
    assert plain.fmaps_right is None


def test_video_passes_the_baseline_exactly_when_it_is_a_stereo_video(monkeypatch):
    from pvo_amd import depth_video
    from pvo_amd.depth_video import DepthVideo
    log = []

    class Db:
        @staticmethod
        def reproject(poses, disps, intr, ii, jj, out=None, **kw):
            log.append(("reproject", dict(kw)))
            return torch.zeros(len(ii), 5, 7, 2), torch.zeros(len(ii), 5, 7, 1)

        @staticmethod
        def ba(*a, **kw):
            log.append(("ba", dict(kw)))
    monkeypatch.setattr(depth_video, "db", Db)
    v = DepthVideo(image_size=(40, 56), buffer=4, device="cpu")
    ii = jj = torch.tensor([0, 1])
    t = torch.zeros(2, 2, 5, 7)
    v.reproject(ii, jj); v.reproject_into(ii, jj, torch.zeros(2, 5, 7, 2)); v.ba(t, t, torch.ones(2, 5, 7), ii, jj, 1, 2)
    assert log == [("reproject", {}), ("reproject", {}), ("ba", {})]                             # a monocular video: today's calls
    del log[:]
    v.ensure_fmaps_right()
    v.stereo_baseline = 0.25
    v.reproject(ii, jj); v.reproject_into(ii, jj, torch.zeros(2, 5, 7, 2)); v.ba(t, t, torch.ones(2, 5, 7), ii, jj, 1, 2)
    v.ba(t, t, None, ii, jj, 1, 2, motion_only=True)
    assert log == [("reproject", {"baseline": 0.25}), ("reproject", {"baseline": 0.25}), ("ba", {"stereo_baseline": 0.25}),
                   ("ba", {"stereo_baseline": 0.25})]
    # stereo together with RGB-D: both terms apply
    del log[:]
    v.ensure_disps_sens(); v.has_sensor_depth = True
    v.ba(t, t, torch.ones(2, 5, 7), ii, jj, 1, 2)
    assert set(log[0][1]) == {"disps_sens", "alpha", "stereo_baseline"}


def test_factor_graph_sets_the_baseline_after_a_replan_and_not_otherwise(monkeypatch):
    from pvo_amd import droid_backends as db
    from test_cvx_upsample_host import _host_graph
    v, fg, _, _ = _host_graph(False)
    log = []
    monkeypatch.setattr(db, "ba_workspace_bytes", lambda *a: 64)
    monkeypatch.setattr(db, "ba_plan", lambda ii, jj, F, HW, K, t0, t1, ws: log.append(("plan", K)))
    monkeypatch.setattr(db, "ba_stereo", lambda ws, E, P, F, HW, b: log.append(("stereo", E, P, F, HW, b)))
    ii, jj = fg.ii, fg.jj
    fg._ba_plan(ii, jj, 1, 4, False, 0, 3)
    assert log == [("plan", 3)]                                                # no right view: today's plan, nothing else
    v.ensure_fmaps_right()
    fg._ba_plan(ii, jj, 1, 4, False, 0, 3)                                     # the video became a stereo video: a re-plan, the baseline behind it
    assert log[1:] == [("plan", 3), ("stereo", 5, 3, 6, 35, 0.1)]
    fg._ba_plan(ii, jj, 1, 4, False, 0, 3)
    assert len(log) == 3                                                       # cached
    v.stereo_baseline = 0.4
    fg._ba_plan(ii, jj, 1, 4, False, 0, 3)
    assert log[3:] == [("plan", 3), ("stereo", 5, 3, 6, 35, 0.4)]
    fg._ba_plan(ii, jj, 1, 4, True, 0, 3)                                      # a motion-only plan carries it too: stereo edges must add nothing
    assert log[5:] == [("plan", -1), ("stereo", 5, 3, 6, 35, 0.4)]
    v.stereo_baseline = 0.0
    fg._ba_plan(ii, jj, 1, 4, False, 0, 3)
    assert log[7:] == [("plan", 3)]


def test_sharded_ba_sets_the_baseline_behind_its_plan():
    from pvo_amd.parallel import ShardedBA
    log = []

    class Backend:
        def ba_workspace(self, *a): return torch.zeros(8)
        def ba_plan(self, *a): log.append("plan")
        def ba_stereo(self, ws, E, P, F, HW, b): log.append(("stereo", b))
        def ba_local(self, *a, **k): log.append("local")
        def ba_finish(self, *a, **k): log.append("finish"); return torch.zeros(2, 6), None
    sb = ShardedBA(backend=Backend(), communicate=False)
    a = (torch.zeros(4, 7), torch.ones(4, 3, 5), torch.ones(4), torch.zeros(3, 2, 3, 5), torch.zeros(3, 2, 3, 5), torch.ones(3, 3, 5),
         torch.tensor([1, 2, 3]), torch.tensor([2, 3, 1]), 1, 3)
    sb.ba(*a, itrs=1, plan_key="k")
    assert log == ["plan", "local", "finish"]                                  # no baseline: no call the CPU backends lack
    sb.ba(*a, itrs=1, plan_key="k", stereo_baseline=0.1)
    assert log[3:] == [("stereo", 0.1), "local", "finish"]
    sb.ba(*a, itrs=1, plan_key="k", stereo_baseline=0.1)
    assert log[6:] == ["local", "finish"]                                      # same plan, same baseline: nothing to set
    sb.ba(*a, itrs=1, plan_key="k2", stereo_baseline=0.1)
    assert log[8:] == ["plan", ("stereo", 0.1), "local", "finish"]             # a fresh plan has lost it
    sb.ba(*a, itrs=1, plan_key="k2")
    assert log[12:] == [("stereo", 0.0), "local", "finish"]                    # gone: cleared


def test_backend_skips_normalize_on_a_stereo_video():
    from pvo_amd.backend import DroidBackend
    from pvo_amd.depth_video import DepthVideo
    v = DepthVideo(image_size=(40, 56), buffer=8, device="cpu")
    v.counter = 4
    calls = []
    v.normalize = lambda: calls.append("normalize")
    be = DroidBackend(Namespace(update=None), v, Namespace(device="cpu", backend_radius=2, backend_nms=3, backend_thresh=15.0, beta=0.3))
    be._connect_all = lambda keep=None: (Namespace(_ii_h=[], clear_edges=lambda: None), ([], []))
    be(2)
    assert calls == ["normalize"]
    v.ensure_fmaps_right()
    be(2)
    assert calls == ["normalize"]                                              # the baseline fixes the scale
    v.stereo_baseline = 0.0
    be(2)
    assert calls == ["normalize"] * 2


def test_the_switch_off_ignores_the_right_image_and_allocates_nothing():
    from pvo_amd.droid import Droid, default_args
    assert default_args().stereo is False and default_args().stereo_baseline == 0.1
    torch.manual_seed(0)
    image = torch.randint(0, 255, (3, 32, 48), dtype=torch.uint8)
    right = torch.randint(0, 255, (3, 32, 48), dtype=torch.uint8)
    intr = torch.tensor([30.0, 30.0, 24.0, 16.0])
    for stereo in (False, True):
        droid = Droid(default_args(device="cpu", image_size=[32, 48], buffer=4, half_update=False, stereo=stereo, stereo_baseline=0.54))
        assert droid.filterx.use_stereo is stereo and droid.video.stereo_baseline == 0.54
        seen, encoded = [], []
        real = droid.video.append
        droid.video.append = lambda *a, **k: (seen.append(dict(k)), real(*a, **k))[1]
        feats = droid.filterx._features_g
        droid.filterx._features_g = lambda img: (encoded.append(img.clone()), feats(img))[1]
        droid.filterx.track_vo(0.0, image, None, intr, right=right)
        droid.filterx.track_vo(1.0, image, None, intr)                         # a frame without a right view in a stereo run
        assert ("right_fmap" in seen[0]) is stereo and "right_fmap" not in seen[1]
        assert len(encoded) == (3 if stereo else 2)                            # the right image costs one more fnet pass, for its keyframe only
        if stereo:
            assert droid.video.has_stereo and torch.equal(encoded[1].cpu(), right)
            want = feats(right.to(droid.filterx.device))[0].movedim(0, -1)
            assert torch.equal(droid.video.fmaps_right[0].float(), want.float().to(droid.video.fmaps_right.dtype).float())
            assert not torch.equal(droid.video.fmaps_right[0], droid.video.fmaps[0]) and not droid.video.fmaps_right[1].any()
        else:
            assert droid.video.fmaps_right is None and droid.video.has_stereo is False


def test_motion_filter_encodes_the_right_image_of_keyframes_only():
    from pvo_amd.droid import Droid, default_args
    torch.manual_seed(1)
    droid = Droid(default_args(device="cpu", image_size=[32, 48], buffer=4, half_update=False, stereo=True))
    f = droid.filterx
    intr = torch.tensor([30.0, 30.0, 24.0, 16.0])
    image = torch.randint(0, 255, (3, 32, 48), dtype=torch.uint8)
    right = torch.randint(0, 255, (3, 32, 48), dtype=torch.uint8)
    encoded = []
    feats = f._features_g
    f._features_g = lambda img: (encoded.append(1), feats(img))[1]
    # (the captured frame graph - encoder, 1-edge volume, operator - needs the device: a stand-in hands back a map and the motion test's scalar)
    mag, frame_inputs = [0.0], []
    f._frame_g = lambda img, *ref: (frame_inputs.append(img.clone()), (torch.randn(1, 128, 4, 6), torch.tensor([mag[0]])))[1]
    assert f.track(0.0, image, None, intr, right=right) is True                # the first frame: a keyframe
    assert len(encoded) == 2 and droid.video.fmaps_right[0].any() and not frame_inputs
    n = len(encoded)
    assert f.track(1.0, image, None, intr, right=right) is False               # nothing moved: no keyframe
    assert len(encoded) == n and f._right is None and droid.video.counter == 1     # its right view was never looked at
    mag[0] = 100.0
    assert f.track(2.0, image, None, intr, right=right) is True
    assert len(encoded) == n + 1 and droid.video.fmaps_right[1].any()          # (the left map came from the frame graph)
    assert all(torch.equal(x.cpu(), image) for x in frame_inputs)              # the frame graph and the motion test read the left view only


def test_vo_stereo_pairs_left_and_right_images_and_passes_right(tmp_path):
    tools = os.path.join(ROOT, "tools")
    sys.path.insert(0, tools)
    try:
        import vo_stereo
    finally:
        sys.path.remove(tools)
    a = vo_stereo.parse_args(["--datapath", "x", "--right_dir", "r", "--baseline", "0.54", "--buffer", "64"])
    assert a.stereo is True and a.stereo_baseline == 0.54 and a.right_dir == "r" and a.buffer == 64
    assert vo_stereo.parse_args(["--datapath", "x", "--no_stereo"]).stereo is False
    assert vo_stereo.parse_args(["--datapath", "x", "--right_dir", "r"]).stereo_baseline == 0.1
    # the pairing: left frame t goes with the t-th right image (sorted), read, resized and cropped like the left one
    from PIL import Image
    left_dir = tmp_path / "seq" / vo_stereo.test_vo.SPLIT["val"] / "frames" / "rgb" / "Camera_0"
    right_dir = tmp_path / "right"
    left_dir.mkdir(parents=True); right_dir.mkdir()
    g = np.random.default_rng(0)
    for t in range(3):
        Image.fromarray(g.integers(0, 255, (30, 50, 3), dtype=np.uint8)).save(str(left_dir / ("rgb_%05d.jpg" % t)))
        Image.fromarray(g.integers(0, 255, (30, 50, 3), dtype=np.uint8)).save(str(right_dir / ("rgb_%05d.jpg" % t)))
    size = [20, 37]                                                            # (resized, then cropped to 16 x 32)
    lefts = [im for _, im, _, _ in vo_stereo.test_vo.image_stream(str(tmp_path / "seq"), size, "val", False)]
    as_left = []                                                               # the right files through the LEFT images' reader
    for t in range(3):
        os.replace(str(right_dir / ("rgb_%05d.jpg" % t)), str(left_dir / ("zz_%05d.jpg" % t)))
    both = [im for _, im, _, _ in vo_stereo.test_vo.image_stream(str(tmp_path / "seq"), size, "val", False)]
    as_left = both[3:]
    for t in range(3):
        os.replace(str(left_dir / ("zz_%05d.jpg" % t)), str(right_dir / ("rgb_%05d.jpg" % t)))
    tracked = []
    droid = Namespace(track=lambda t, image, intrinsics=None, segments=None, right=None: tracked.append((t, image, right)))
    vo_stereo.track_pairs(droid, Namespace(datapath=str(tmp_path / "seq"), right_dir=str(right_dir), image_size=size, segm_filter=False, stereo=True))
    assert [x[0] for x in tracked] == [0, 1, 2] and tracked[0][1].shape == (3, 16, 32)
    for t in range(3):
        assert torch.equal(tracked[t][1], lefts[t]) and torch.equal(tracked[t][2], as_left[t]) and tracked[t][2].dtype == lefts[t].dtype
    assert not torch.equal(tracked[0][2], tracked[0][1])
    with pytest.raises(SystemExit):
        vo_stereo.track_pairs(droid, Namespace(datapath=str(tmp_path / "seq"), right_dir=None, image_size=size, segm_filter=False, stereo=True))


# ------------------------------------------------------------------------------------------------ closed loop
def run_stereo_sequence(scene, video, frontend, operator, stereo):
    """pvo_amd.synthetic.run_sequence with a right feature map per keyframe (its content is not read: the operator is the oracle)"""
    dev = video.poses.device
    h, w = scene.ht, scene.wd
    g = torch.Generator().manual_seed(1)
    for k in range(scene.n):
        slot = video.counter
        operator.bind(slot, k)
        left = torch.randn(h, w, 128, generator=g).half().to(dev)
        z = torch.zeros(128, h, w, dtype=torch.half, device=dev)
        video.append(float(k), None if k else scene.poses[0].to(dev), None, scene.intr.to(dev), left, z, z,
                     **({"right_fmap": torch.full((h, w, 128), float(k + 1), dtype=torch.half, device=dev)} if stereo else {}))
        frontend()
        if video.counter <= slot:
            operator.frame_of.pop(slot, None)
            operator.bind(video.counter - 1, k)
    frames = [operator.frame_of.get(s, s) for s in range(video.counter)]
    return video.poses[:video.counter].detach().cpu().clone(), frames


def _cpu_loop(scene, kw, b):
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.synthetic import OracleFlowOperator
    from test_synthetic_vo import OracleVideo

    class RefVideo(OracleVideo):
        """OracleVideo with DepthVideo's stereo state; `ba` is the fp64 yardstick, `reproject` the oracle's plus the closed form"""
        def __init__(self, ht, wd, buffer):
            super().__init__(ht, wd, buffer)
            self.fmaps_right, self.stereo_baseline = None, b

        has_stereo = property(lambda self: self.fmaps_right is not None and self.stereo_baseline > 0)

        def _b(self):
            return self.stereo_baseline if self.has_stereo else 0.0

        def append(self, tstamp, pose, disp, intrinsics, *unused, right_fmap=None):
            if right_fmap is not None:
                if self.fmaps_right is None:
                    self.fmaps_right = torch.zeros(self.poses.shape[0], 1, 1, 1)
                self.fmaps_right[self.counter] = float(right_fmap.reshape(-1)[0])
            super().append(tstamp, pose, disp, intrinsics)

        def reproject(self, ii, jj):
            c, val = S.reproject(self.poses.numpy(), self.disps.numpy(), self.intrinsics.numpy(), np.asarray(ii), np.asarray(jj), self._b())
            return torch.from_numpy(c).float()[None], torch.from_numpy(val)[None]

        def ba(self, target, weight, eta, ii, jj, t0=1, t1=None, itrs=2, lm=1e-4, ep=0.1, motion_only=False):
            assert not motion_only
            p, d = S.ba(self.poses.numpy(), self.disps.numpy(), self.intrinsics[0].numpy(), target.numpy(), weight.numpy(), eta.numpy(),
                        ii.numpy(), jj.numpy(), t0, t1, itrs, lm, ep, self._b())
            self.poses.copy_(torch.from_numpy(p)); self.disps.copy_(torch.from_numpy(d).clamp(min=0.001))

    ov = RefVideo(scene.ht, scene.wd, buffer=32)
    # the oracle operator's targets: a stereo edge's is the TRUE right-view pixel u - fx b d_true (the closed form on the true depths)
    rp = lambda p, d, k, i, j: torch.from_numpy(S.reproject(p.numpy(), d.numpy(), k.numpy(), i.numpy(), j.numpy(), b)[0]).float()
    op = OracleFlowOperator(scene, ov, rp)
    fe = DroidFrontend(op, ov, device="cpu", **kw)
    fe.graph.corr_impl = "none"
    fe.graph.corr = type("NoVolumes", (), {"__call__": lambda self, coords, **kw: None})()
    poses, frames = run_stereo_sequence(scene, ov, fe, op, b > 0)
    return ov, fe, poses, frames


def test_closed_loop_on_the_cpu_is_metric_with_stereo_edges():
    """PlaneScene(24, 32, 14 frames, seed 0) through the real DroidFrontend / FactorGraph with the BA answered by the fp64 yardstick.
    This run decides the baseline of the closed loops: the smallest of 0.1, 0.2, 0.4, 0.8 at which the YARDSTICK stays within the
    RGB-D tests' thresholds (unaligned ATE <= 0.5 % of the path, |scale - 1| < 0.01).  Chosen: BASELINE = 0.1, the default.
    The yardstick's own figures are printed by this test and recorded in DESIGN.md section 4, *Stereo*."""
    from pvo_amd.synthetic import PlaneScene
    from test_rgbd_host import metric_figures
    scene = PlaneScene(ht=24, wd=32, n_frames=14, seed=0)
    kw = dict(warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20, frontend_radius=2, frontend_nms=1)
    out = {}
    for name, b in (("monocular", 0.0), ("stereo", BASELINE)):
        ov, fe, poses, frames = _cpu_loop(scene, kw, b)
        out[name] = metric_figures(poses, frames, scene) + (len(frames),)
        print("%s (b = %.2f): ATE-RMSE without alignment %.5f of the path, aligned %.2e, path scale %.4f, %d keyframes" % ((name, b) + out[name]))
        pairs = list(zip(fe.graph._ii_h, fe.graph._jj_h)) + list(zip(fe.graph._ii_inac_h, fe.graph._jj_inac_h))
        st = sorted(p for p in pairs if p[0] == p[1])
        if b > 0:
            assert st == [(k, k) for k in range(ov.counter)]                   # one stereo edge per keyframe, none twice
            assert [float(ov.fmaps_right[k]) for k in range(ov.counter)] == [float(f + 1) for f in frames]
        else:
            assert not st and ov.fmaps_right is None
    assert out["stereo"][3] == out["monocular"][3] == 14
    assert out["stereo"][0] <= 0.005                                           # metric: within 0.5 % of the path length, no alignment
    assert abs(out["stereo"][2] - 1.0) < 0.01
    assert out["monocular"][0] > 0.1                                           # (the monocular run is defined up to scale only)
