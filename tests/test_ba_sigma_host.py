"""Depth and pose uncertainty, the parts that need no GPU: the tests' own fp64 yardstick (tests/sigma_reference.py) qualified before
anything is held to it - its two routes against each other, symmetry and definiteness, the reductions to the conditional variance,
the monotonicity of the sensor prior and the stereo term, a unit-right-hand-side solve of the full damped system - and the host side
of the feature: the C ABI of the new entry points, the argument checks, the PLY writer's optional column and the reject-mask logic."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rgbd_reference as R
import sigma_reference as G
import stereo_reference as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pvo_ba_sigma", "pvo_ba_uncertainty")

# name -> (window, kwargs of the yardstick); built once, shared, never modified
_SCENES = {
    "5x12x22": lambda: (R.window(301, 5, 12, 22), {}),
    "5x13x21": lambda: (R.window(302, 5, 13, 21, t0=2), {}),
    "6x9x12": lambda: (R.window(303, 6, 9, 12), {}),
    "8x12x22": lambda: (R.window(304, 8, 12, 22), {}),
}
_cache = {}


def _scene(name):
    if name not in _cache:
        s, kw = _SCENES[name]()
        f = G.scene_fields(s, **kw)
        _cache[name] = (s, f, G.scene_schur(s, f, **kw))
    return _cache[name]


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("name", sorted(_SCENES))
def test_schur_and_dense_routes_agree(name):
    s, f, a = _scene(name)
    b = G.scene_dense(s, f)
    e_var = G.relmax(a["var_cond"] + a["var_pose"], b["var_total"])
    e_cov = G.relmax(np.diag(a["pose_cov"]), np.diag(b["pose_cov"]))
    e_off = float(np.abs(a["pose_cov"] - b["pose_cov"]).max() / np.abs(b["pose_cov"]).max())
    print("%s: schur vs dense, depth variances %.2e, pose diagonal %.2e, pose block %.2e; var_pose / var_cond in [%.2e, %.2e]"
          % (name, e_var, e_cov, e_off, float((a["var_pose"] / a["var_cond"]).min()), float((a["var_pose"] / a["var_cond"]).max())))
    assert e_var < 1e-10 and e_cov < 1e-10 and e_off < 1e-10


@pytest.mark.parametrize("name", sorted(_SCENES))
def test_pose_covariance_is_symmetric_positive_definite_and_var_pose_is_not_negative(name):
    _, _, a = _scene(name)
    cov = a["pose_cov"]
    assert np.array_equal(cov, cov.T)
    assert float(np.linalg.eigvalsh(cov).min()) > 0
    assert float(a["var_pose"].min()) >= 0 and float(a["var_cond"].min()) > 0
    assert float(a["var_pose"].max()) > 0                                     # (not vacuous)


def test_depth_only_window_and_fixed_pose_frames_reduce_to_the_conditional_variance():
    s, f, _ = _scene("6x9x12")
    z = dict(s, t0=6, t1=6)                                                   # t0 == t1: no pose is free
    a = G.scene_schur(z, f)
    assert a["pose_cov"].shape == (0, 0) and not a["var_pose"].any()
    assert list(a["kx"]) == list(range(6)) and a["var_cond"].shape == (6, 108)
    # source frames in front of the window: with t0 = 4 and radius 2, frame 0's and 1's targets are all < t0
    w = dict(s, t0=4)
    b = G.scene_schur(w, f)
    assert list(b["kx"]) == list(range(6))
    assert not b["var_pose"][0].any() and not b["var_pose"][1].any()          # exact zeros
    assert b["var_pose"][2].min() > 0 and b["var_pose"][4].min() > 0          # frame 2 sees pose 4; frame 4 is a window frame
    d = G.scene_dense(w, f)
    assert G.relmax(b["var_cond"] + b["var_pose"], d["var_total"]) < 1e-10


def test_sensor_prior_and_stereo_edges_never_increase_the_conditional_variance():
    s, f, a = _scene("6x9x12")
    sens = s["sens"].numpy()
    p = G.scene_schur(s, f, sens=sens)
    kx = a["kx"]
    m = (sens.reshape(6, -1)[kx] > 0)
    alpha_over_eta = G.ALPHA > float(s["eta"].max())                          # the prior replaces eta by a LARGER alpha where measured
    assert alpha_over_eta
    assert np.all(p["var_cond"] <= a["var_cond"]) and np.all(p["var_cond"][m] < a["var_cond"][m])
    assert np.array_equal(p["var_cond"][~m], a["var_cond"][~m])
    # a stereo edge on every frame, against the same edges as identity edges (baseline 0)
    st = S.window(305, 6, 9, 12, 0.1, range(6))
    with_b, without = G.scene_schur(st, baseline=0.1), G.scene_schur(st, baseline=0.0)
    assert np.all(with_b["var_cond"] <= without["var_cond"]) and np.all(with_b["var_cond"] < without["var_cond"] * 0.999)
    both = G.scene_schur(st, baseline=0.1, sens=st["sens"].numpy())
    assert np.all(both["var_cond"] <= with_b["var_cond"])
    d = G.scene_dense(st, baseline=0.1, sens=st["sens"].numpy())
    assert G.relmax(both["var_cond"] + both["var_pose"], d["var_total"]) < 1e-10


def test_unit_right_hand_side_on_one_depth_variable_reproduces_its_marginal_variance():
    s, f, a = _scene("5x12x22")
    F, ht, wd = s["disps"].shape
    H, kx = G.full_information(f, s["eta"].numpy(), s["ii"].numpy(), s["jj"].numpy(), s["t0"], s["t1"], F, ht * wd, 1e-4, 0.1)
    n6, HW = 6 * (s["t1"] - s["t0"]), ht * wd
    total = a["var_cond"] + a["var_pose"]
    for k, x in ((0, 0), (1, 131), (2, HW - 1), (4, 77)):
        e = np.zeros(H.shape[0])
        e[n6 + k * HW + x] = 1.0
        z = np.linalg.solve(H, e)
        assert abs(z[n6 + k * HW + x] - total[k, x]) <= 1e-10 * total[k, x], (k, x)
        # moving the variable by a finite step against the information matrix: the restoring gradient is H z = e, i.e. 1 at
        # the variable and 0 everywhere else
        assert np.abs(H @ z - e).max() < 1e-9


# ------------------------------------------------------------------------------------------------ C ABI and argument checks
def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    from pvo_amd import _lib
    header = open(os.path.join(ROOT, "include", "pvo_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in include/pvo_hip.h"
        assert hasattr(lib, name), name + " is not exported by libpvo_hip.so"
        assert name in _lib.SIGNATURES, name + " is not bound by pvo_amd._lib"
    loaded = _lib.load()
    assert loaded.pvo_version() == _lib.PVO_ABI_VERSION == 106               # new symbols only
    assert re.search(r"#define\s+PVO_ABI_VERSION\s+106\b", header)
    # the one-call form takes pvo_ba_rig's operands with the three outputs in place of iterations / dx_out / dz_out
    rig, unc = _lib.SIGNATURES["pvo_ba_rig"][1], _lib.SIGNATURES["pvo_ba_uncertainty"][1]
    assert unc[:15] == rig[:15] and unc[15:17] == rig[16:18] and unc[-7:] == rig[-7:] and len(unc) == len(rig) - 2
    # argument checks are host code: they answer without a device
    big = 1 << 30
    sigma = lambda ws=256, nbytes=big, E=4, P=3, F=4, ht=4, wd=4, t0=1, sys=256, cov=256: \
        loaded.pvo_ba_sigma(sys, ws, nbytes, 256, 256, E, P, F, ht, wd, t0, 1e-4, 0.1, cov, None, None, None, None)
    assert sigma(ws=None) == 1                                                # NULL workspace: PVO_EINVAL
    assert sigma(nbytes=16) == 3                                              # PVO_EWORKSPACE
    assert sigma(P=65, F=70) == 4                                             # beyond the frontend's window: PVO_EUNSUPPORTED
    assert sigma(P=-1) == 1 and sigma(P=4) == 1                               # the window must fit the buffer
    assert sigma(E=0) == 1                                                    # nothing assembled
    assert sigma(sys=None) == 1 and sigma(cov=None) == 1                      # with a free pose both are needed
    unc_call = lambda t0=1, t1=4, F=4, alpha=0.05, b=0.0, ws=256: loaded.pvo_ba_uncertainty(
        *([256] * 8), 4, F, 4, 4, 4, t0, t1, 1e-4, 0.1, 256, None, None, None, ws, big, 256, alpha, b, None)
    assert unc_call(t1=70, F=70) == 4
    assert unc_call(b=-0.1) == 1 and unc_call(alpha=0.0) == 1 and unc_call(ws=None) == 1 and unc_call(t0=3, t1=2) == 1


def test_python_argument_checks_speak_the_reference_language():
    from pvo_amd import droid_backends as db
    import droid_backends as top
    assert top.ba_sigma is db.ba_sigma and top.ba_uncertainty is db.ba_uncertainty
    z = torch.zeros
    ok = dict(poses=z(4, 7), disps=z(4, 4, 4), intrinsics=z(4), targets=z(3, 2, 4, 4), weights=z(3, 2, 4, 4), eta=z(4, 4, 4),
              ii=z(3, dtype=torch.long), jj=z(3, dtype=torch.long), t0=1, t1=4, lm=1e-4, ep=0.1)
    bad = dict(ok, targets=z(3, 2, 4, 8)[..., ::2])
    with pytest.raises(RuntimeError, match="targets must be contiguous"):
        db.ba_uncertainty(**bad)
    with pytest.raises(RuntimeError, match="needs device tensors"):           # there is no CPU fallback
        db.ba_uncertainty(**ok)
    with pytest.raises(RuntimeError, match="ii must be contiguous"):
        db.ba_sigma(z(400, dtype=torch.long), z(16, dtype=torch.uint8), z(6, dtype=torch.long)[::2], ok["jj"], ok["disps"], 1, 4, 1e-4, 0.1)


# ------------------------------------------------------------------------------------------------ host-side plumbing
def test_write_ply_with_and_without_sigma(tmp_path):
    from pvo_amd.handoff import write_ply
    g = np.random.default_rng(5)
    xyz = g.standard_normal((7, 3)).astype(np.float32)
    rgb = g.integers(0, 255, (7, 4), dtype=np.uint8)
    label = g.integers(0, 9, 7).astype(np.int32)
    sigma = g.uniform(0.01, 0.2, 7).astype(np.float32)
    # the default file: byte for byte the layout it always had, built here by hand
    a = tmp_path / "a.ply"
    assert write_ply(str(a), xyz, rgb, label) == 7
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty int label\nend_header\n")
    body = b"".join(xyz[k].tobytes() + rgb[k, :3].tobytes() + label[k].tobytes() for k in range(7))
    assert a.read_bytes() == header.encode("ascii") + body
    b = tmp_path / "b.ply"
    assert write_ply(str(b), xyz, rgb, label, sigma=None) == 7 and b.read_bytes() == a.read_bytes()
    # with the column: one more property, one more float per record, the round trip
    c = tmp_path / "c.ply"
    assert write_ply(str(c), torch.from_numpy(xyz), rgb, label, sigma=torch.from_numpy(sigma)) == 7
    raw = c.read_bytes()
    head, rest = raw.split(b"end_header\n", 1)
    assert head.decode("ascii") == header.replace("end_header\n", "property float sigma\n")
    rec = np.frombuffer(rest, dtype=np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("label", "<i4"),
                                              ("sigma", "<f4")]))
    assert rec.shape == (7,) and np.array_equal(rec["sigma"], sigma) and np.array_equal(rec["x"], xyz[:, 0]) and np.array_equal(rec["label"], label)


def test_max_rel_sigma_builds_the_reject_mask_and_gathers_each_points_sigma():
    from pvo_amd.depth_video import DepthVideo
    disps = torch.tensor([[[1.0, 2.0, 0.5], [1.0, 1.0, 4.0]]]).repeat(2, 1, 1)              # [2, 2, 3]
    sigma = torch.tensor([[[0.05, 0.3, 0.04], [float("inf"), 0.1, float("nan")]]]).repeat(2, 1, 1)
    m = DepthVideo.rel_sigma_reject(sigma, disps, 0.1)
    # sigma / disp = .05, .15, .08 / inf, .1, nan: above the bound, never estimated and NaN are rejected; exactly on it stays
    assert m.dtype == torch.bool and m[0].tolist() == [[False, True, False], [True, False, True]]
    own = torch.zeros(2, 1, 2, 3, dtype=torch.uint8)
    own[1, 0, 0, 0] = 1
    both = DepthVideo.rel_sigma_reject(sigma, disps, 0.1, own)
    assert both[0].tolist() == m[0].tolist() and both[1, 0, 0].item() is True and both[1].sum() == m[1].sum() + 1
    # the map's src = (keyframe, pixel of the map the points were taken from): the 1/8 lattice ...
    src = torch.tensor([[0, 0], [1, 4], [1, 5]], dtype=torch.int32)
    s = torch.arange(12, dtype=torch.float).reshape(2, 2, 3)
    assert DepthVideo.gather_sigma(s, src, 3, 1).tolist() == [0.0, 10.0, 11.0]
    # ... or the full-resolution map, whose pixel (y, x) lies in cell (y // 8, x // 8)
    full = torch.tensor([[0, 7], [0, 8], [1, 8 * 24 + 23], [1, 15 * 24 + 16]], dtype=torch.int32)
    assert DepthVideo.gather_sigma(s, full, 3, 8).tolist() == [0.0, 1.0, 11.0, 11.0]


def test_video_allocates_the_variances_on_first_use_and_they_travel_with_their_keyframe():
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.droid import default_args
    from test_cvx_upsample_host import _host_graph
    assert default_args().uncertainty is False and default_args(uncertainty=True).uncertainty is True
    v = DepthVideo(image_size=(40, 56), buffer=6, device="cpu")
    z = torch.zeros(128, 5, 7, dtype=torch.half)
    v.append(0.0, None, None, torch.ones(4), z, z, z)
    assert v.disps_var_cond is None and v.disps_var_pose is None and v.poses_cov is None      # off: nothing is allocated
    with pytest.raises(RuntimeError, match="no uncertainty"):
        v.map_points(max_rel_sigma=0.1)
    vc, vp, pc = v.ensure_uncertainty()
    assert v.ensure_uncertainty()[0] is vc                                                    # once
    assert vc.shape == vp.shape == v.disps.shape and pc.shape == (6, 6, 6) and pc.dtype == torch.float64
    assert bool(torch.isinf(vc).all()) and bool(torch.isinf(vp).all())
    assert bool(torch.isinf(pc.diagonal(dim1=1, dim2=2)).all()) and float(torch.nan_to_num(pc, posinf=0.0).abs().max()) == 0.0
    vc[:] = torch.arange(6, dtype=torch.float)[:, None, None]; vp[:] = 10 + vc; pc[:] = 20 + torch.arange(6, dtype=torch.float64)[:, None, None]
    v.append(1.0, None, None, torch.ones(4), z, z, z)                                         # a new keyframe in slot 1: its old estimate goes
    assert bool(torch.isinf(vc[1]).all()) and bool(torch.isinf(vp[1]).all()) and float(vc[2, 0, 0]) == 2.0
    assert bool(torch.isinf(pc[1].diagonal()).all()) and float(pc[1, 0, 1]) == 0.0
    v[3] = (3.0, None, None, torch.full((5, 7), 2.0), None)                                   # a new depth map through the item form
    assert bool(torch.isinf(vc[3]).all()) and float(vc[4, 0, 0]) == 4.0
    v[4] = (4.0, None, None, None, None)                                                      # nothing of the depth changes: the estimate stays
    assert float(vc[4, 0, 0]) == 4.0
    # rm_keyframe: the rows move down with their frame
    v2, fg, _, _ = _host_graph(False)
    fg.corr = None
    fg.ii_inac = fg.jj_inac = torch.zeros(0, dtype=torch.long)
    fg.rm_factors = lambda mask, store=False: None
    c2, p2, k2 = v2.ensure_uncertainty()
    c2[:] = torch.arange(6, dtype=torch.float)[:, None, None]; p2[:] = 10 + c2; k2[:] = torch.arange(6, dtype=torch.float64)[:, None, None]
    fg.rm_keyframe(2)
    for buf, off in ((c2, 0.0), (p2, 10.0), (k2, 0.0)):
        assert [float(buf[k].reshape(-1)[0]) - off for k in range(6)] == [0.0, 1.0, 3.0, 3.0, 4.0, 5.0]


def test_frontend_asks_once_per_keyframe_after_its_last_update_and_a_sharded_run_refuses():
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.parallel import ShardedBA
    calls = []

    class Graph:
        _ii_h = [0]
        def update(self, *a, **k): calls.append("u")
        def uncertainty(self, *a, **k): calls.append(("s", a, k))
        def rm_keyframe(self, ix): calls.append("rm")

    class Video:
        counter = 5
        poses, disps, dirty = torch.zeros(8, 7), torch.ones(8, 2, 2), torch.zeros(8, dtype=torch.bool)

    for on in (False, True):
        for drop in (False, True):
            del calls[:]
            fe = DroidFrontend.__new__(DroidFrontend)
            fe.video, fe.graph, fe.uncertainty, fe.iters2, fe.t1 = Video(), Graph(), on, 2, 5
            fe.update_pending, fe._dist, fe.keyframe_decision, fe.count, fe.keyframes_removed = True, torch.tensor(1.0), (lambda c, d: drop), 1, 0
            fe._update_finish()
            if drop:
                assert calls == ["rm"]                                     # a dropped keyframe has no last update
            elif on:
                assert calls[:2] == ["u", "u"] and len(calls) == 3 and calls[2][0] == "s" and calls[2][2] == {"use_inactive": True}
            else:
                assert calls == ["u", "u"]                                 # off: the launch sequence is what it was
    with pytest.raises(NotImplementedError, match="uncertainty"):
        ShardedBA(communicate=False).uncertainty()


def test_factor_graph_skips_a_window_beyond_the_limit_and_refuses_an_edge_sharded_run():
    from pvo_amd.parallel import ShardedBA
    from test_cvx_upsample_host import _host_graph
    v, fg, _, _ = _host_graph(False)
    fg.corr = None
    fg._ii_h, fg._jj_h = [0, 1], [70, 2]                                      # t0 = 1, t1 = 71: 70 window poses
    assert fg.uncertainty(None, None, use_inactive=True) is None
    assert v.disps_var_cond is None                                           # not estimated: nothing allocated, nothing raised
    with pytest.raises(NotImplementedError, match="edge-sharded"):
        fg.uncertainty(None, None, sharded=ShardedBA(communicate=False))
