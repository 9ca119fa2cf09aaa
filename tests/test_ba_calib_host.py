"""Online intrinsics calibration, host side: the yardstick of tests/test_ba_calib_gpu.py (tests/calib_reference.py) is qualified
against autograd and against the full normal equations, and the Python layers' bookkeeping is checked with the native call stubbed.
No GPU is needed: the argument checks of the library are host code."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import calib_reference as C
import rgbd_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pvo_ba_calib_workspace_bytes", "pvo_ba_calib")
LM, EP, EP_C = 1e-4, 0.1, 0.1


# ------------------------------------------------------------------------------------------------ the yardstick against autograd
def _tiny():
    """4 frames of 4 x 6 (reverse mode is slow beyond that), radius-2 graph, window [1, 4), GENERAL motion - rotation about all three
    axes, translation along all three: no entry of G_ij and no column of Jc is an exact zero; quaternions normalised in fp64, for which
    the closed forms are exact"""
    s = C.window_general(411, 4, 4, 6, radius=2, t0=1)
    a = list(C.scene_args(s))
    poses = a[0].astype(np.float64)
    poses[:, 3:] /= np.linalg.norm(poses[:, 3:], axis=1, keepdims=True)
    a[0] = poses
    return s, a


def _rot_t(q):
    x, y, z, w = q
    return torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)]),
                        torch.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)]),
                        torch.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)])])


def _hat(p):
    z = torch.zeros((), dtype=p.dtype)
    return torch.stack([torch.stack([z, -p[2], p[1]]), torch.stack([p[2], z, -p[0]]), torch.stack([-p[1], p[0], z])])


def _project(xi, disps, c, poses, ii, jj, ht, wd):
    """the projection of every edge's pixels, [E,2,HW], as a function of the tangents xi [F,6] (pose f <- exp(xi_f) pose f, with exp to
    second order: exact first derivatives at 0), the inverse depths [F,HW] and c = (fx, fy, cx, cy) - plain torch, fp64"""
    fx, fy, cx, cy = c
    v_, u_ = torch.meshgrid(torch.arange(ht, dtype=torch.float64), torch.arange(wd, dtype=torch.float64), indexing="ij")
    px, py = (u_.reshape(-1) - cx) / fx, (v_.reshape(-1) - cy) / fy
    Xi = torch.stack([px, py, torch.ones_like(px)])
    Rs, ts = [], []
    for f in range(poses.shape[0]):
        K = _hat(xi[f, 3:])
        Rx = torch.eye(3, dtype=torch.float64) + K + 0.5 * K @ K
        Rf = _rot_t(poses[f, 3:])
        Rs.append(Rx @ Rf); ts.append(Rx @ poses[f, :3] + xi[f, :3])
    out = []
    for i, j in zip(ii, jj):
        Rij = Rs[j] @ Rs[i].T
        tij = ts[j] - Rij @ ts[i]
        X = Rij @ Xi + tij[:, None] * disps[i][None]
        out.append(torch.stack([fx * X[0] / X[2] + cx, fy * X[1] / X[2] + cy]))
    return torch.stack(out)


_auto = {}


def _autograd():
    """-> (window, operands, closed-form Jacobians, autograd's (J_xi [E,2,HW,F,6], J_d [E,2,HW,F,HW], J_c [E,2,HW,4])); once"""
    if not _auto:
        s, a = _tiny()
        F, ht, wd = s["disps"].shape
        ii, jj = [int(v) for v in a[6]], [int(v) for v in a[7]]
        poses = torch.from_numpy(a[0])
        d0 = torch.from_numpy(a[1].astype(np.float64)).reshape(F, -1)
        c0 = torch.from_numpy(a[2].astype(np.float64))
        fn = lambda xi, d, c: _project(xi, d, c, poses, ii, jj, ht, wd)
        J = torch.autograd.functional.jacobian(fn, (torch.zeros(F, 6, dtype=torch.float64), d0, c0))
        cf = C.pixel_jacobians(a[0], a[1], a[2], a[3], a[4], a[6], a[7])
        assert np.abs(fn(torch.zeros(F, 6, dtype=torch.float64), d0, c0).numpy() - cf["proj"]).max() < 1e-12
        assert float(cf["w"].min()) > 0                                         # every pixel in front of the camera: no masked row
        live = [e for e in range(len(ii)) if not np.array_equal(a[0][ii[e]], a[0][jj[e]])]      # (frames 0 and 1 start from one pose)
        assert len(live) >= 8 and all(float(np.abs(cf["Jc"][e]).max(2).min()) > 1e-3 for e in live)      # every column of Jc, fy's included, is compared at non-zero values
        for e in live[:2]:
            Rm, t = C.rel_pose(a[0][ii[e]], a[0][jj[e]])
            assert float(np.abs(Rm).min()) > 1e-4 and float(np.abs(t).min()) > 1e-4      # ... and every entry of G_ij
        _auto.update(s=s, a=a, cf=cf, J=[t.numpy() for t in J], ii=ii, jj=jj)
    return _auto


def test_closed_form_jacobians_equal_autograd():
    A = _autograd()
    cf, (Jx, Jd, Jc), ii, jj = A["cf"], A["J"], A["ii"], A["jj"]
    E, _, HW = cf["r"].shape
    F = Jx.shape[3]
    assert E <= 12 and F <= 4 and HW <= 24
    worst = dict(Ji=0.0, Jj=0.0, Jz=0.0, Jc=0.0, other=0.0)
    for e in range(E):
        i, j = ii[e], jj[e]
        worst["Ji"] = max(worst["Ji"], np.abs(np.moveaxis(Jx[e, :, :, i, :], 2, 1) - cf["Ji"][e]).max())
        worst["Jj"] = max(worst["Jj"], np.abs(np.moveaxis(Jx[e, :, :, j, :], 2, 1) - cf["Jj"][e]).max())
        diag = Jd[e, :, np.arange(HW), i, np.arange(HW)].T                       # [2, HW]: pixel x depends on depth x of frame i alone
        worst["Jz"] = max(worst["Jz"], np.abs(diag - cf["Jz"][e]).max())
        worst["Jc"] = max(worst["Jc"], np.abs(np.moveaxis(Jc[e], 2, 1) - cf["Jc"][e]).max())
        rest_x = np.delete(Jx[e], [i, j], axis=2)
        off = Jd[e].copy()
        off[:, np.arange(HW), i, np.arange(HW)] = 0.0
        worst["other"] = max(worst["other"], np.abs(rest_x).max() if rest_x.size else 0.0, np.abs(off).max())
    print("closed form against autograd:", {k: "%.1e" % v for k, v in worst.items()})
    assert max(worst.values()) <= 1e-12


def test_schur_route_equals_the_full_normal_equations():
    A = _autograd()
    s, a, cf, (Jx, Jd, Jc) = A["s"], A["a"], A["cf"], A["J"]
    F, ht, wd = s["disps"].shape
    HW, t0, t1 = ht * wd, s["t0"], s["t1"]
    P, E = t1 - t0, len(A["ii"])
    f = C.fields(a[0], a[1], a[2], a[3], a[4], a[6], a[7], assembly="fp64")
    for free_mask in (15, 3, 5):
        got = C.step(f, a[0], a[1], a[2], a[5], a[6], a[7], t0, t1, LM, EP, EP_C, free_mask)
        assert not got["rejected"]
        kx = got["kx"]
        K = len(kx)
        free = [n for n in range(4) if (free_mask >> n) & 1]
        # unknowns: [6P poses | free intrinsics | K HW depths]; rows: every edge, residual row and pixel, from AUTOGRAD's Jacobian
        cols = [Jx[:, :, :, t0:t1, :].reshape(E * 2 * HW, 6 * P), Jc.reshape(E * 2 * HW, 4)[:, free],
                Jd[:, :, :, kx, :].reshape(E * 2 * HW, K * HW)]
        Jf = np.concatenate(cols, 1)
        w, r = cf["w"].reshape(-1), cf["r"].reshape(-1)
        H = Jf.T @ (Jf * w[:, None])
        g = Jf.T @ (w * r)
        n6, nc = 6 * P, len(free)
        eta = np.asarray(a[5], np.float64).reshape(K, HW)
        H[np.arange(n6), np.arange(n6)] += EP + LM * got["S_diag"]               # the same damping, added to the reduced diagonal
        H[np.arange(n6, n6 + nc), np.arange(n6, n6 + nc)] += EP_C + LM * got["Scc_diag"][free]
        H[np.arange(n6 + nc, H.shape[0]), np.arange(n6 + nc, H.shape[0])] += eta.reshape(-1)
        z = np.linalg.solve(H, g)
        dx, dc = z[:n6].reshape(P, 6), z[n6:n6 + nc]
        ex = np.abs(got["dx"] - dx).max() / np.abs(dx).max()
        ec = np.abs(got["dc"][free] - dc).max() / np.abs(dc).max()
        print("mask %d: Schur route against the full system dx %.1e dc %.1e" % (free_mask, ex, ec))
        assert ex <= 1e-9 and ec <= 1e-9


def test_mask_0_reproduces_gn_step_exactly_and_a_held_parameter_does_not_move():
    s = R.window(311, 5, 12, 22, radius=2, t0=1)
    a = C.scene_args(s)
    f = C.fields(a[0], a[1], a[2], a[3], a[4], a[6], a[7])
    poses, disps, dz, kx = R.gn_step(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], LM, EP)
    m0 = C.step(f, a[0], a[1], a[2], a[5], a[6], a[7], a[8], a[9], LM, EP, EP_C, 0)
    assert np.array_equal(m0["poses"], poses) and np.array_equal(m0["disps"], disps) and np.array_equal(m0["dz"], dz)
    assert np.array_equal(m0["kx"], kx) and not m0["dc"].any() and np.array_equal(m0["intr"], a[2])
    for free_mask in (3, 5, 10, 15):
        r = C.step(f, a[0], a[1], a[2], a[5], a[6], a[7], a[8], a[9], LM, EP, EP_C, free_mask)
        for n in range(4):
            if (free_mask >> n) & 1:
                assert r["intr"][n] == np.float32(a[2][n]) + np.float32(r["dc"][n])
            else:
                assert r["dc"][n] == 0.0 and r["intr"][n].tobytes() == a[2][n].tobytes()
        assert not np.array_equal(r["dx"], m0["dx"])                           # the border reaches the poses
    # two steps: the second starts from the first's fp32 state
    one = C.ba_calib(*a, 1, LM, EP, EP_C, 15)
    two = C.ba_calib(*a, 2, LM, EP, EP_C, 15)
    again = C.gn_step_calib(one["poses"], one["disps"], one["intr"], a[3], a[4], a[5], a[6], a[7], a[8], a[9], LM, EP, EP_C, 15)
    assert np.array_equal(two["disps"], again["disps"]) and np.array_equal(two["intr"], again["intr"])


def test_an_identity_edge_has_no_intrinsics_jacobian():
    s = R.window(412, 3, 4, 6, ii=[0, 1, 1], jj=[1, 1, 2], t0=1)
    a = C.scene_args(s)
    J = C.pixel_jacobians(a[0], a[1], a[2], a[3], a[4], a[6], a[7])
    assert np.abs(J["Jc"][1]).max() <= 1e-15 and np.abs(J["Jc"][2]).max() > 1e-3      # (frames 0 and 1 start from the same pose: edge 0 is an identity too)


# ------------------------------------------------------------------------------------------------ C ABI and argument checks
def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    from pvo_amd import _lib
    header = open(os.path.join(ROOT, "include", "pvo_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), name + " is not declared in include/pvo_hip.h"
        assert hasattr(lib, name), name + " is not exported by libpvo_hip.so"
        assert name in _lib.SIGNATURES, name + " is not bound by pvo_amd._lib"
    loaded = _lib.load()
    assert loaded.pvo_version() == _lib.PVO_ABI_VERSION                       # new symbols only: the ABI version stays
    # pvo_ba's operands with ep_c / free_mask behind ep, dc_out behind dz_rows and the second workspace behind the first
    ba, cal = _lib.SIGNATURES["pvo_ba"][1], _lib.SIGNATURES["pvo_ba_calib"][1]
    assert cal[:18] == ba[:18] and cal[18:20] == [ctypes.c_float, ctypes.c_int] and cal[20:23] == ba[19:22] and cal[24:27] == ba[22:25]
    assert len(cal) == len(ba) + 4
    assert loaded.pvo_ba_calib_workspace_bytes(-1, 3, 4, 16) == 0
    small, big = loaded.pvo_ba_calib_workspace_bytes(4, 3, 5, 16), loaded.pvo_ba_calib_workspace_bytes(40, 30, 50, 160)
    assert 0 < small < big and small >= 4 * 4 * 4 * 16 + 8 * 18 * 18             # gc and S_d^-1 at least
    # argument checks are host code: they answer without a device
    huge = 1 << 30
    call = lambda E=4, F=5, t0=1, t1=4, it=1, ep_c=0.1, mask=15, ws=256, nb=huge, cws=256, cnb=huge, intr=256: loaded.pvo_ba_calib(
        256, 256, intr, 256, 256, 256, 256, 256, E, F, 4, 4, 4, t0, t1, it, 1e-4, 0.1, ep_c, mask, None, None, 0, None, None, ws, nb, cws, cnb, None)
    assert call(t1=70, F=70) == 4 and call(t0=1, t1=66, F=70) == 4              # P = 69, 65: PVO_EUNSUPPORTED
    assert call(t0=2, t1=2) == 4                                               # P = 0 likewise
    assert call(E=0) == 1 and call(ep_c=-0.1) == 1 and call(ep_c=float("nan")) == 1
    assert call(mask=16) == 1 and call(mask=-1) == 1 and call(it=-1) == 1
    assert call(ws=None) == 1 and call(cws=None) == 1 and call(intr=None) == 1
    assert call(nb=16) == 3 and call(cnb=16) == 3                              # PVO_EWORKSPACE, either workspace
    assert call(t0=3, t1=2) == 1 and call(t1=6) == 1                           # the window must fit the buffer


def test_python_argument_checks_speak_the_reference_language():
    from pvo_amd import droid_backends as db
    import droid_backends as top
    assert top.ba_calib is db.ba_calib and db.BA_CALIB_MAX_POSES == 64
    z = torch.zeros
    ok = dict(poses=z(4, 7), disps=z(4, 4, 4), intrinsics=z(4), targets=z(3, 2, 4, 4), weights=z(3, 2, 4, 4), eta=z(4, 4, 4),
              ii=z(3, dtype=torch.long), jj=z(3, dtype=torch.long), t0=1, t1=4, iterations=1, lm=1e-4, ep=0.1)
    with pytest.raises(RuntimeError, match="targets must be contiguous"):
        db.ba_calib(**dict(ok, targets=z(3, 2, 4, 8)[..., ::2]))
    with pytest.raises(RuntimeError, match="needs device tensors"):           # there is no CPU fallback
        db.ba_calib(**ok)


# ------------------------------------------------------------------------------------------------ host-side plumbing
def _stub_backend(monkeypatch, log, accept=True):
    """db.ba_calib replaced: records its operands and, like an accepted step, moves intrinsics (row 0's storage) in place"""
    from pvo_amd import droid_backends as db

    def ba_calib(poses, disps, intrinsics, targets, weights, eta, ii, jj, t0, t1, iterations, lm, ep, ep_c=0.1, free_mask=15, status=None):
        log.append(dict(intrinsics=intrinsics, ptr=intrinsics.data_ptr(), targets=targets, weights=weights, eta=eta, ii=ii, jj=jj, t0=t0, t1=t1,
                        iterations=iterations, lm=lm, ep=ep, ep_c=ep_c, free_mask=free_mask))
        if accept:
            intrinsics += torch.tensor([1.0, 2.0, 0.5, 0.25])
        return [torch.zeros(t1 - t0, 6), torch.zeros(1, 1), torch.tensor([1.0, 2.0, 0.5, 0.25])]
    monkeypatch.setattr(db, "ba_calib", ba_calib)


def test_video_writes_every_row_in_place_and_keeps_the_calibrated_vector(monkeypatch):
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.droid import default_args
    assert default_args().opt_intr is False and default_args().opt_intr_free == "all" and default_args(opt_intr=True).opt_intr is True
    log = []
    _stub_backend(monkeypatch, log)
    z = torch.zeros(128, 5, 7, dtype=torch.half)
    guess = torch.tensor([40.0, 40.0, 28.0, 20.0])

    def fill(v):
        for k in range(3):
            v.append(float(k), None, None, guess, z, z, z)
        v[3] = (3.0, None, None, None, guess * 1.5)

    plain = DepthVideo(image_size=(40, 56), buffer=6, device="cpu")
    fill(plain)                                                                # an uncalibrated video: the caller's vectors, as ever
    assert not plain.calibrated and torch.equal(plain.intrinsics[:3], guess.expand(3, 4)) and torch.equal(plain.intrinsics[3], guess * 1.5)
    assert torch.equal(plain.intrinsics[4:], torch.zeros(2, 4))
    v = DepthVideo(image_size=(40, 56), buffer=6, device="cpu")
    fill(v)
    ptr, buf = v.intrinsics.data_ptr(), v.intrinsics
    E = 2
    tg, wt, eta = torch.zeros(E, 2, 5, 7), torch.ones(E, 2, 5, 7), torch.ones(3, 5, 7)
    ii, jj = torch.tensor([1, 2]), torch.tensor([2, 1])
    out = v.ba_calib(tg, wt, eta, ii, jj, 1, 3, itrs=3, ep_c=0.2, free="focal")
    assert len(out) == 4 and out[3].dtype == torch.int32 and out[3].numel() == 4
    call = log[0]
    assert call["ptr"] == ptr and call["intrinsics"].shape == (4,)             # it runs on intrinsics[0], the buffer's own storage
    assert (call["iterations"], call["ep_c"], call["free_mask"], call["t0"], call["t1"]) == (3, 0.2, 3, 1, 3)
    want = guess + torch.tensor([1.0, 2.0, 0.5, 0.25])
    assert v.intrinsics is buf and v.intrinsics.data_ptr() == ptr              # copy_, never rebinding
    assert v.calibrated and torch.equal(v.intrinsics, want.expand(6, 4))       # every row of the buffer
    v.ba_calib(tg, wt, eta, ii, jj, 1, 3)
    assert log[1]["free_mask"] == 15 and log[1]["iterations"] == 2 and torch.equal(v.intrinsics, (want + torch.tensor([1.0, 2.0, 0.5, 0.25])).expand(6, 4))
    want = v.intrinsics[0].clone()
    v.append(4.0, None, None, guess, z, z, z)                                  # slot 3 (counter): the stream's stale guess is not written
    v[5] = (5.0, None, None, None, guess)
    v[0:2] = (torch.zeros(2), None, None, None, guess.expand(2, 4))
    assert torch.equal(v.intrinsics, want.expand(6, 4)) and v.intrinsics.data_ptr() == ptr
    assert bool(v.calibrated_dev)
    # every step rejected (row 0 does not move): rows and flag stay, the caller's vectors are still written - decided on the device
    _stub_backend(monkeypatch, log, accept=False)
    r = DepthVideo(image_size=(40, 56), buffer=6, device="cpu")
    fill(r)
    rows = r.intrinsics.clone()
    r.ba_calib(tg, wt, eta, ii, jj, 1, 3)
    assert r.calibrated and not bool(r.calibrated_dev) and torch.equal(r.intrinsics, rows)      # row 3's own vector included
    r.append(4.0, None, None, guess * 2, z, z, z)
    r[5] = (5.0, None, None, None, guess * 3)
    assert torch.equal(r.intrinsics[4], guess * 2) and torch.equal(r.intrinsics[5], guess * 3)
    _stub_backend(monkeypatch, log)                                            # ... and an accepted step later calibrates it
    r.ba_calib(tg, wt, eta, ii, jj, 1, 3)
    assert bool(r.calibrated_dev) and torch.equal(r.intrinsics, (guess + torch.tensor([1.0, 2.0, 0.5, 0.25])).expand(6, 4))
    with pytest.raises(ValueError, match="free"):
        v.ba_calib(tg, wt, eta, ii, jj, 1, 3, free="cx")
    v.has_sensor_depth = True
    with pytest.raises(NotImplementedError, match="sensor-depth prior or stereo"):
        v.ba_calib(tg, wt, eta, ii, jj, 1, 3)


def test_droid_refuses_opt_intr_with_rgbd_or_stereo_when_it_is_built():
    from pvo_amd.droid import Droid, default_args
    for over in (dict(rgbd=True), dict(stereo=True)):
        with pytest.raises(ValueError, match="opt_intr together with"):
            Droid(default_args(device="cpu", opt_intr=True, **over))
    with pytest.raises(ValueError, match="opt_intr_free"):
        Droid(default_args(device="cpu", opt_intr=True, opt_intr_free="cx"))


def test_factor_graph_calibrate_hands_over_the_operands_of_uncertainty(monkeypatch):
    from pvo_amd.parallel import ShardedBA
    from test_cvx_upsample_host import _host_graph
    v, fg, _, _ = _host_graph(False)
    fg.corr = None
    got = {}
    v.uncertainty = lambda *a, **k: got.__setitem__("unc", (a, k))
    v.ba_calib = lambda *a, **k: got.__setitem__("cal", (a, k)) or "done"
    fg.damping[:] = torch.rand_like(fg.damping)
    fg._last_EP = 1e-5
    fg.uncertainty(None, None, use_inactive=True)
    assert fg.calibrate(None, None, use_inactive=True, itrs=3, ep_c=0.3, free="focal") == "done"
    (ua, uk), (ca, ck) = got["unc"], got["cal"]
    assert len(ua) == len(ca) == 7 and ua[5:] == ca[5:] == (2, 4)              # t0 / t1 by the same rule
    assert all(torch.equal(x, y) for x, y in zip(ua[:5], ca[:5]))              # target, weight, eta, ii, jj
    assert ca[0].shape == (5, 2, 5, 7) and ca[2].shape == (3, 5, 7) and uk == dict(lm=1e-4, ep=0.1)
    assert ck == dict(itrs=3, lm=1e-4, ep=0.1, ep_c=0.3, free="focal")
    # beyond 64 poses: None, and nothing is done
    got.clear()
    fg._ii_h, fg._jj_h = [0, 1], [70, 2]
    assert fg.calibrate(None, None, use_inactive=True) is None and not got and not v.calibrated
    with pytest.raises(NotImplementedError, match="edge-sharded"):
        fg.calibrate(None, None, sharded=ShardedBA(communicate=False))
    with pytest.raises(NotImplementedError, match="calibration"):
        ShardedBA(communicate=False).calibrate()


def test_frontend_calibrates_after_the_last_update_and_before_the_uncertainty():
    from pvo_amd.frontend import DroidFrontend
    calls = []

    class Graph:
        _ii_h = [0]
        def update(self, *a, **k): calls.append("u")
        def uncertainty(self, *a, **k): calls.append(("s", a, k))
        def calibrate(self, *a, **k): calls.append(("c", a, k))
        def rm_keyframe(self, ix): calls.append("rm")
        def add_neighborhood_factors(self, *a, **k): pass
        def add_proximity_factors(self, *a, **k): pass

    class Video:
        counter = 5
        poses, disps, dirty = torch.zeros(8, 7), torch.ones(8, 2, 2), torch.zeros(8, dtype=torch.bool)

    for on, unc in ((False, False), (False, True), (True, False), (True, True)):
        for drop in (False, True):
            del calls[:]
            fe = DroidFrontend.__new__(DroidFrontend)
            fe.video, fe.graph, fe.uncertainty, fe.iters2, fe.t1 = Video(), Graph(), unc, 2, 5
            fe.opt_intr, fe.opt_intr_free = on, "focal"
            fe.update_pending, fe._dist, fe.keyframe_decision, fe.count, fe.keyframes_removed = True, torch.tensor(1.0), (lambda c, d: drop), 1, 0
            fe._update_finish()
            kinds = [c if isinstance(c, str) else c[0] for c in calls]
            assert kinds == (["rm"] if drop else ["u", "u"] + (["c"] if on else []) + (["s"] if unc else []))
            if on and not drop:
                assert calls[2][1:] == ((None, None), {"use_inactive": True, "free": "focal"})
        # initialisation: after its last update
        del calls[:]
        fe = DroidFrontend.__new__(DroidFrontend)
        fe.video, fe.graph, fe.uncertainty, fe.opt_intr, fe.opt_intr_free, fe.frontend_thresh = Video(), Graph(), unc, on, "all", 16.0
        fe._initialize()
        kinds = [c if isinstance(c, str) else c[0] for c in calls]
        assert kinds == ["u"] * 20 + (["c"] if on else []) + (["s"] if unc else [])
        if on:
            assert calls[20][1:] == ((1,), {"use_inactive": True, "free": "all"})
