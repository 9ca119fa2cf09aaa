"""Map export on the device: pvo_map_points (pvo_amd/csrc/map_points.hip) against tests/map_reference.py fed the votes of
pvo_depth_filter on the same device - the same arithmetic, so the selection is held to EQUALITY - and its points against the fp64
evaluation under the bound derived in map_reference.py; capacity, gathers, bad pixels, determinism, and the system path
(DepthVideo.map_points / Droid.get_map)."""
import numpy as np
import pytest
import torch

import map_reference as M

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _ix_cases(nf):
    """all frames | output follows ix, not frame order ([6,0,3]; on a scene with fewer than 7 frames its last, first and middle
    frame) | a single frame | frame ids -1 and nframes mixed in, which contribute nothing"""
    order = [6, 0, 3] if nf > 6 else [nf - 1, 0, nf // 2]
    return {"all": list(range(nf)), "order": order, "single": [nf - 1], "invalid": [nf - 1, -1, 0, nf, nf // 2]}


_scenes, _runs = {}, {}


def _scene(cuda, name):
    if name not in _scenes:
        nf, ht, wd, noise = M.SCENES[name]
        poses, disps, intr = M.scene(M.SEED, nf, ht, wd, noise)
        _scenes[name] = (poses, disps, intr, poses.to(cuda), disps.to(cuda), intr.to(cuda))
    return _scenes[name]


def _votes(cuda, poses_d, disps_d, intr_d, ix, th):
    """[len(ix),ht,wd] numpy: pvo_depth_filter's votes for the frame ids of ix that are in range, 0 for the others"""
    from pvo_amd import droid_backends as db
    nf, ht, wd = disps_d.shape
    ok = [b for b, f in enumerate(ix) if 0 <= f < nf]
    v = np.zeros((len(ix), ht, wd), np.float32)
    if ok:
        ix_ok = torch.tensor([ix[b] for b in ok], dtype=torch.long, device=cuda)
        v[ok] = db.depth_filter(poses_d, disps_d, intr_d, ix_ok, torch.full((len(ok),), th, device=cuda)).cpu().numpy()
    return v


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _run(cuda, name, th, case):
    """(native result as numpy, reference) of one scene / threshold / ix case, computed once"""
    from pvo_amd import droid_backends as db
    key = (name, th, case)
    if key not in _runs:
        poses, disps, intr, poses_d, disps_d, intr_d = _scene(cuda, name)
        ix = _ix_cases(disps.shape[0])[case]
        got = _host(db.map_points(poses_d, disps_d, intr_d, torch.tensor(ix, dtype=torch.long, device=cuda),
                                  torch.full((len(ix),), th, device=cuda)))
        ref = M.map_reference(poses.numpy(), disps.numpy(), intr.numpy(), ix, _votes(cuda, poses_d, disps_d, intr_d, ix, th))
        _runs[key] = (got, ref)
    return _runs[key]


def _assert_selection(got, ref):
    assert np.array_equal(got["frame_start"], ref["frame_start"])
    assert int(got["frame_start"][-1]) == ref["total"] == len(got["src"]) == len(got["xyz"])
    assert np.array_equal(got["src"], ref["src"])
    assert np.array_equal(got["rgba"][:, 3], ref["alpha"])


CASES = [(n, th, c) for n in M.SCENES for th in M.THRESHOLDS for c in ("all", "order", "single", "invalid")]


@pytest.mark.parametrize("name,th,case", CASES)
def test_selection_is_exact(cuda, name, th, case):
    got, ref = _run(cuda, name, th, case)
    print("%s thresh %g ix %s: %d points, frame_start %s" % (name, th, case, ref["total"], ref["frame_start"].tolist()))
    _assert_selection(got, ref)
    assert np.array_equal(got["rgba"][:, :3], np.zeros((ref["total"], 3), np.uint8))       # no images: colour 0
    if case in ("all", "order"):
        assert ref["total"] > 0
    if name == "9x12x3" and case == "all":
        assert ref["frame_start"].tolist()[:3] == [0, 0, 0]                               # two empty frames in front


@pytest.mark.parametrize("name,th", [(n, th) for n in M.SCENES for th in M.THRESHOLDS])
def test_points_are_within_the_derived_bound(cuda, name, th):
    """|xyz - fp64| <= K_POINT * 2^-24 * (|t|_1 + |Xc|_1) per component (map_reference.py); the bound itself is tighter than the
    rtol 1e-5 / atol 1e-5 the iproj tests grant on this scene family"""
    for case in ("all", "order"):
        got, ref = _run(cuda, name, th, case)
        _assert_selection(got, ref)
        err = np.abs(got["xyz"].astype(np.float64) - ref["xyz"])
        ratio = (err / ref["bound"][:, None]).max()
        print("%s thresh %g ix %s: %d points, max error %.3e, max error / bound %.3f, max bound %.3e"
              % (name, th, case, ref["total"], err.max(), ratio, ref["bound"].max()))
        assert np.all(ref["bound"][:, None] <= 1e-5 + 1e-5 * np.abs(ref["xyz"]))
        assert np.all(err <= ref["bound"][:, None])


def test_more_workgroups_than_scan_threads(cuda):
    """5 frames of 240 x 240: 5 * 225 = 1125 per-workgroup counts, so every thread of the one-workgroup scan owns MORE than one
    (the scenes above stop at 60).  frame_start, the selection and the points against the reference."""
    from pvo_amd import droid_backends as db
    nf, ht, wd, th = 5, 240, 240, 0.2
    assert nf * -(-ht * wd // 256) > 1024
    poses, disps, intr = M.scene(M.SEED, nf, ht, wd, 0.02)
    poses_d, disps_d, intr_d = poses.to(cuda), disps.to(cuda), intr.to(cuda)
    ix = [3, 0, 4, 1, 2]
    got = _host(db.map_points(poses_d, disps_d, intr_d, torch.tensor(ix, dtype=torch.long, device=cuda), torch.full((nf,), th, device=cuda)))
    ref = M.map_reference(poses.numpy(), disps.numpy(), intr.numpy(), ix, _votes(cuda, poses_d, disps_d, intr_d, ix, th))
    print("240x240x5: %d points, frame_start %s" % (ref["total"], ref["frame_start"].tolist()))
    _assert_selection(got, ref)
    assert ref["total"] > 0
    err = np.abs(got["xyz"].astype(np.float64) - ref["xyz"])
    assert np.all(err <= ref["bound"][:, None])


def _buffers(cuda, cap, N, label=False):
    fill = lambda nbytes, dt: torch.full((cap, nbytes), SENTINEL, dtype=torch.uint8, device=cuda).view(dt)
    out = {"xyz": fill(12, torch.float32), "rgba": fill(4, torch.uint8), "src": fill(8, torch.int32),
           "frame_start": torch.full((N + 1,), -7, dtype=torch.int32, device=cuda)}
    if label:
        out["label"] = fill(4, torch.int32).reshape(cap)
    return out


def _into(cuda, name, th, cap_rows, capacity):
    """pvo_map_points on sentinel-filled buffers of cap_rows rows, told that they hold `capacity` rows; returns their bytes"""
    from pvo_amd import _lib, droid_backends as db
    poses, disps, intr, poses_d, disps_d, intr_d = _scene(cuda, name)
    nf = disps.shape[0]
    out = _buffers(cuda, cap_rows, nf)
    view = {k: (v if k == "frame_start" else v[:capacity]) for k, v in out.items()}
    db.map_points_into(_lib.MapPointsArgs(), poses_d, disps_d, intr_d, torch.arange(nf, device=cuda), torch.full((nf,), th, device=cuda), view)
    return {k: v.cpu().numpy().view(np.uint8).reshape(v.shape[0], -1) if k != "frame_start" else v.cpu().numpy() for k, v in out.items()}


def test_capacity_drops_the_tail_and_touches_nothing_beyond(cuda):
    name, th = "13x17x7", 0.2
    got, ref = _run(cuda, name, th, "all")
    total, fs = ref["total"], ref["frame_start"]
    full = _into(cuda, name, th, total + 9, total + 9)
    assert np.array_equal(full["frame_start"], fs)
    assert np.array_equal(full["src"][:total].view(np.int32), ref["src"]) and np.all(full["src"][total:] == SENTINEL)
    assert np.array_equal(full["xyz"][:total].view(np.float32), got["xyz"])
    for cap in (total - 1, 0, int(fs[3]) + 5):
        assert 0 <= cap < total and (cap == 0 or cap == total - 1 or fs[3] < cap < fs[4])
        part = _into(cuda, name, th, total + 9, cap)
        assert np.array_equal(part["frame_start"], fs)                  # unchanged: the total is not clamped
        for k in ("xyz", "rgba", "src"):
            assert np.all(part[k][cap:] == SENTINEL), (cap, k)          # nothing at an index >= capacity
            assert np.array_equal(part[k][:cap], full[k][:cap]), (cap, k)


def test_two_calls_give_identical_bytes(cuda):
    for name, th, cap in (("30x101x5", 0.2, 5000), ("24x40x8", 0.05, 10 ** 4)):
        a, b = _into(cuda, name, th, cap + 3, cap), _into(cuda, name, th, cap + 3, cap)
        assert a["frame_start"][-1] > 0
        for k in a:
            assert np.array_equal(a[k], b[k]), (name, k)


def _gather_case(cuda, ht, wd, ih, iw, stride, offset, lh, lw, div, th=0.2, nf=7, seed=11):
    poses, disps, intr = M.scene(seed, nf, ht, wd, 0.02)
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (nf, 3, ih, iw), generator=g).to(torch.uint8)
    labels = torch.randint(0, 1000, (nf, lh, lw), generator=g).to(torch.int32)
    reject = torch.zeros(nf, lh, lw, dtype=torch.bool)
    reject[1::2, : max(1, lh // 2), 1:] = True                          # a block of cells in every second frame
    return poses, disps, intr, images, labels, reject


@pytest.mark.parametrize("shape", ["eighth", "full"])
def test_colours_labels_and_rejected_cells(cuda, shape):
    """eighth: an 8 x 8 map coloured from a 64 x 64 image at [3::8, 3::8], labels and reject at the map's resolution;
    full: a 16 x 24 map coloured pixel for pixel (stride 1, offset 0), labels and reject 2 x 3 with label_div = 8"""
    from pvo_amd import droid_backends as db
    ht, wd, ih, iw, s, o, lh, lw, div = (8, 8, 64, 64, 8, 3, 8, 8, 1) if shape == "eighth" else (16, 24, 16, 24, 1, 0, 2, 3, 8)
    poses, disps, intr, images, labels, reject = _gather_case(cuda, ht, wd, ih, iw, s, o, lh, lw, div)
    d = lambda t: t.to(cuda)
    nf, th = disps.shape[0], 0.2
    ix = list(range(nf))
    votes = _votes(cuda, d(poses), d(disps), d(intr), ix, th)
    args = (d(poses), d(disps), d(intr), torch.arange(nf, device=cuda), torch.full((nf,), th, device=cuda))
    for rej in (None, reject):
        got = _host(db.map_points(*args, images=d(images), img_stride=s, img_offset=o, labels=d(labels), label_div=div,
                                  reject=None if rej is None else d(rej)))
        ref = M.map_reference(poses.numpy(), disps.numpy(), intr.numpy(), ix, votes, images=images.numpy(), img_stride=s, img_offset=o,
                              labels=labels.numpy(), label_div=div, reject=None if rej is None else rej.numpy())
        _assert_selection(got, ref)
        assert ref["total"] > 20
        assert np.array_equal(got["rgba"][:, :3], ref["rgb"]) and np.array_equal(got["label"], ref["label"])
        if rej is not None:
            f, k = got["src"][:, 0], got["src"][:, 1]
            assert not rej.numpy()[f, (k // wd) // div, (k % wd) // div].any() and ref["total"] < total_before
        total_before = ref["total"]
    # reject alone (no labels) uses its own grid
    got = _host(db.map_points(*args, reject=d(reject), label_div=div))
    ref = M.map_reference(poses.numpy(), disps.numpy(), intr.numpy(), ix, votes, reject=reject.numpy(), label_div=div)
    _assert_selection(got, ref)
    assert "label" not in got


def test_out_of_bounds_strides_are_refused_before_any_launch(cuda):
    from pvo_amd import _lib, droid_backends as db
    poses, disps, intr, images, labels, reject = _gather_case(cuda, 8, 8, 64, 64, 8, 3, 8, 8, 1)
    d = lambda t: t.to(cuda)
    nf = disps.shape[0]
    base = (d(poses), d(disps), d(intr), torch.arange(nf, device=cuda), torch.full((nf,), 0.2, device=cuda))

    def refused(**kw):
        a = _lib.MapPointsArgs()
        if "images" in kw:
            im = d(kw["images"])
            a.images, a.IH, a.IW, a.img_stride, a.img_offset = im.data_ptr(), im.shape[2], im.shape[3], kw.get("s", 8), kw.get("o", 3)
        if "labels" in kw:
            lab = d(kw["labels"])
            a.labels, a.LH, a.LW, a.label_div = lab.data_ptr(), lab.shape[1], lab.shape[2], kw["div"]
        out = _buffers(cuda, 16, nf)
        with pytest.raises(_lib.PvoHipError, match="status 1"):                           # PVO_EINVAL
            db.map_points_into(a, *base, out)
        torch.cuda.synchronize()
        assert np.all(out["frame_start"].cpu().numpy() == -7)                              # nothing ran: not even frame_start
        assert np.all(out["xyz"].view(torch.uint8).cpu().numpy() == SENTINEL)

    refused(images=images[:, :, :59].contiguous())               # 8 * 7 + 3 = 59 >= IH = 59
    refused(images=images[:, :, :, :59].contiguous())  # the same for the width
    refused(images=images, s=9)                       # 9 * 7 + 3 = 66 >= 64
    refused(images=images, o=8)                       # 8 * 7 + 8 = 64 >= 64
    refused(images=images, s=0)
    refused(labels=labels[:, :7].contiguous(), div=1)  # (8 - 1) / 1 = 7 >= LH = 7
    refused(labels=labels[:, :, :7].contiguous(), div=1)
    refused(labels=labels[:, :2, :2].contiguous(), div=2)   # 7 / 2 = 3 >= 2
    refused(labels=labels, div=0)
    # and the largest stride / smallest grid that fit are accepted
    ok = db.map_points(*base, images=d(images[:, :, :60, :60].contiguous()), labels=d(labels[:, :4, :4].contiguous()), label_div=2)
    assert int(ok["frame_start"][-1]) == ok["xyz"].shape[0] > 0


def test_bad_pixels_are_never_kept_and_change_nothing_else(cuda):
    """NaN, +inf, 0 and a negative inverse depth, in exported frames that are also the neighbours other exported frames project into,
    and a frame without a positive value (mean <= 0).  Every index the kernels form stays in range: a frame id is checked against
    [0, nframes) before any use, the four taps of a vote are read only where the saturating floor of the projection (NaN -> 0) lies
    inside [0, wd-1) x [0, ht-1), and colours / labels / cells are read at indices the host bounded before the launch."""
    from pvo_amd import droid_backends as db
    nf, ht, wd, noise = M.SCENES["24x40x8"]
    poses, disps, intr = M.scene(M.SEED, nf, ht, wd, noise)
    disps = disps.clone()
    bad = {2: [(5, 7, 0.0), (6, 8, -0.25), (11, 20, 0.0), (12, 21, -1.0)], 4: [(9, 13, float("nan")), (10, 30, float("nan"))],
           5: [(7, 19, float("inf"))]}
    for f, cells in bad.items():
        for y, x, v in cells:
            disps[f, y, x] = v
    disps[7] = -disps[7]
    disps[7, 3, 4] = 0.0                                                # frame 7: no positive value, mean < 0
    th, ix = 0.2, list(range(nf))
    poses_d, disps_d, intr_d = poses.to(cuda), disps.to(cuda), intr.to(cuda)
    got = _host(db.map_points(poses_d, disps_d, intr_d, torch.arange(nf, device=cuda), torch.full((nf,), th, device=cuda)))
    torch.cuda.synchronize()
    ref = M.map_reference(poses.numpy(), disps.numpy(), intr.numpy(), ix, _votes(cuda, poses_d, disps_d, intr_d, ix, th))
    _assert_selection(got, ref)
    per = np.diff(got["frame_start"])
    print("points per frame with planted pixels:", per.tolist())
    assert per[4] == 0 and per[5] == 0 and per[7] == 0                  # mean NaN, mean inf, mean <= 0: nothing exported
    assert per[2] > 0 and per[0] > 0 and per[1] > 0 and per[3] > 0 and per[6] > 0
    kept = set(map(tuple, got["src"].tolist()))
    for f, cells in bad.items():
        for y, x, _ in cells:
            assert (f, y * wd + x) not in kept
    assert np.isfinite(got["xyz"]).all()
    assert np.all(np.abs(got["xyz"].astype(np.float64) - ref["xyz"]) <= ref["bound"][:, None])
    # the clean scene differs only where the rule says so: frames 0 and 1 have the neighbours -/- and 3, 4, 5 ... of which only
    # frame 0's neighbours 3, 4, 5 hold planted pixels; their own disps are untouched, so their points are a subset of the clean run's
    clean, _ = _run(cuda, "24x40x8", th, "all")
    clean_kept = set(map(tuple, clean["src"].tolist()))
    assert {p for p in kept if p[0] in (0, 1, 3, 6)} <= clean_kept


def test_empty_calls_write_frame_start(cuda):
    from pvo_amd import droid_backends as db
    poses, disps, intr, poses_d, disps_d, intr_d = _scene(cuda, "13x17x7")
    out = db.map_points(poses_d, disps_d, intr_d, torch.zeros(0, dtype=torch.long, device=cuda), torch.zeros(0, device=cuda))
    assert out["frame_start"].tolist() == [0] and out["xyz"].shape == (0, 3)
    out = db.map_points(poses_d, disps_d[:, :0].contiguous(), intr_d, torch.arange(3, device=cuda), torch.full((3,), 0.2, device=cuda))
    assert out["frame_start"].tolist() == [0, 0, 0, 0] and out["xyz"].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ system
_tracked = {}


def _track(cuda):
    """the short synthetic stream of the system tests (pvo_amd.synthetic: plane scene, ground-truth flow operator, upsampling masks
    as tests/test_cvx_upsample_gpu.py builds them) on a Droid that stores images and tracks with args.upsample"""
    if "droid" not in _tracked:
        from pvo_amd import droid_backends as db
        from pvo_amd.droid import Droid, default_args
        from pvo_amd.frontend import DroidFrontend
        from pvo_amd.synthetic import OracleFlowOperator, PlaneScene, run_sequence
        from test_cvx_upsample_gpu import _MaskedOracleOperator
        scene = PlaneScene(ht=24, wd=32, n_frames=14, seed=0)
        torch.manual_seed(0)
        droid = Droid(default_args(device=str(cuda), image_size=[scene.ht * 8, scene.wd * 8], buffer=32, upsample=True, store_images=True))
        assert droid.video.images is not None and droid.video.images.dtype == torch.uint8
        op = _MaskedOracleOperator(OracleFlowOperator(scene, droid.video, lambda p, d, k, i, j: db.reproject(p, d, k, i, j)[0]))
        droid.frontend = DroidFrontend(op, droid.video, device=cuda, warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20,
                                       frontend_radius=2, frontend_nms=1, upsample=True)
        run_sequence(scene, droid.video, droid.frontend, op)
        g = torch.Generator().manual_seed(3)                            # (run_sequence feeds feature maps, not images: give the frames content)
        n, v = droid.video.counter, droid.video
        v.images[:n] = torch.randint(0, 256, (n, 3, v.ht, v.wd), generator=g).to(torch.uint8).to(cuda)
        v.segms[:n] = torch.randint(0, 40, (n, 1, v.ht // 8, v.wd // 8), generator=g).to(torch.int32).to(cuda)
        _tracked["droid"] = droid
    return _tracked["droid"]


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_get_map_is_the_native_call_on_the_videos_buffers(cuda):
    from pvo_amd import droid_backends as db
    droid = _track(cuda)
    v, n = droid.video, droid.video.counter
    th = 0.05
    m = droid.get_map(thresh=th)
    ix, tt = torch.arange(n, device=cuda), torch.full((n,), th, device=cuda)
    want = db.map_points(v.poses, v.disps, v.intrinsics[0].contiguous(), ix, tt, images=v.images, img_stride=8, img_offset=3,
                         labels=v.segms, label_div=1)
    _same(m, want)
    total = int(m["frame_start"][-1])
    print("1/8 map: %d of %d candidate pixels" % (total, n * v.disps.shape[1] * v.disps.shape[2]))
    assert total > 0 and m["xyz"].shape == (total, 3) and bool(torch.isfinite(m["xyz"]).all())
    src = m["src"].long()
    y, x = src[:, 1] // v.disps.shape[2], src[:, 1] % v.disps.shape[2]
    for c in range(3):                                                  # BGR planes -> RGB
        assert torch.equal(m["rgba"][:, c], v.images[src[:, 0], 2 - c, 8 * y + 3, 8 * x + 3])
    assert torch.equal(m["label"], v.segms[src[:, 0], 0, y, x])
    # the selection is the reference rule on pvo_depth_filter's votes
    votes = db.depth_filter(v.poses, v.disps, v.intrinsics[0].contiguous(), ix, tt).cpu().numpy()
    ref = M.map_reference(v.poses.cpu().numpy(), v.disps.cpu().numpy(), v.intrinsics[0].cpu().numpy(), list(range(n)), votes)
    assert ref["total"] == total and np.array_equal(ref["src"], m["src"].cpu().numpy())
    # a reject mask and an explicit frame list go through
    rej = torch.zeros(v.segms.shape[0], v.ht // 8, v.wd // 8, dtype=torch.bool, device=cuda)
    rej[:, :, : v.wd // 16] = True
    m2 = droid.get_map(thresh=th, ix=[n - 1, 2], reject=rej)
    assert 0 < int(m2["frame_start"][-1]) < total and bool((m2["src"][:, 1] % (v.wd // 8) >= v.wd // 16).all())
    assert m2["src"][0, 0].item() == n - 1 and m2["src"][-1, 0].item() == 2


def test_get_map_full_resolution(cuda):
    from pvo_amd import droid_backends as db
    droid = _track(cuda)
    v, n = droid.video, droid.video.counter
    th = 0.05
    m = droid.get_map(thresh=th, full_res=True)
    ix, tt = torch.arange(n, device=cuda), torch.full((n,), th, device=cuda)
    want = db.map_points(v.poses, v.disps_up, (8.0 * v.intrinsics[0]).contiguous(), ix, tt, images=v.images, img_stride=1, img_offset=0,
                         labels=v.segms, label_div=8)
    _same(m, want)
    total = int(m["frame_start"][-1])
    assert v.disps_up.shape[1] * v.disps_up.shape[2] == 8 * 8 * v.disps.shape[1] * v.disps.shape[2]       # 64 x the candidates
    print("full-resolution map: %d of %d candidate pixels" % (total, n * v.ht * v.wd))
    assert total > int(droid.get_map(thresh=th)["frame_start"][-1])
    src = m["src"].long()
    y, x = src[:, 1] // v.wd, src[:, 1] % v.wd
    assert torch.equal(m["label"], v.segms[src[:, 0], 0, y // 8, x // 8])
    assert torch.equal(m["rgba"][:, 0], v.images[src[:, 0], 2, y, x])
    # without the full-resolution depths the request is refused, as get_depth(convex=True) is
    from pvo_amd.depth_video import DepthVideo
    with pytest.raises(RuntimeError, match="upsample"):
        DepthVideo(image_size=(64, 64), buffer=4, device=cuda).map_points(full_res=True)


def test_get_map_dirty_only_exports_the_dirty_frames_and_clears_them(cuda):
    from pvo_amd import droid_backends as db
    droid = _track(cuda)
    v, n = droid.video, droid.video.counter
    v.dirty[:n] = False
    v.dirty[[1, 4, 5]] = True
    v.dirty[n + 1] = True                                               # (beyond the counter: not a keyframe, stays as it is)
    m = droid.get_map(thresh=0.05, dirty_only=True)
    ix = torch.tensor([1, 4, 5], device=cuda)
    want = db.map_points(v.poses, v.disps, v.intrinsics[0].contiguous(), ix, torch.full((3,), 0.05, device=cuda), images=v.images,
                         labels=v.segms)
    _same(m, want)
    assert sorted(set(m["src"][:, 0].tolist())) == [1, 4, 5]
    assert not bool(v.dirty[:n].any()) and bool(v.dirty[n + 1])
    again = droid.get_map(thresh=0.05, dirty_only=True)
    assert again["frame_start"].tolist() == [0] and again["xyz"].shape == (0, 3) and again["rgba"].shape == (0, 4)
    v.dirty[n + 1] = False


def test_map_without_stored_images_has_no_colours(cuda):
    from pvo_amd.depth_video import DepthVideo
    poses, disps, intr, poses_d, disps_d, intr_d = _scene(cuda, "13x17x7")
    nf, ht, wd = disps.shape
    v = DepthVideo(image_size=(ht * 8, wd * 8), buffer=nf, device=cuda)
    assert v.images is None
    v.poses[:], v.disps[:], v.intrinsics[:] = poses_d, disps_d, intr_d
    v.counter = nf
    m = v.map_points(thresh=0.2)
    got, ref = _run(cuda, "13x17x7", 0.2, "all")
    assert np.array_equal(m["src"].cpu().numpy(), ref["src"]) and not bool(m["rgba"][:, :3].any())
