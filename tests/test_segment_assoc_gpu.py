"""Segment association on the device: pvo_segment_associate (pvo_amd/csrc/segment_assoc.hip) against tests/segment_assoc_reference.py -
all six outputs held to EQUALITY (the contract is integers and exactly stated fp32) on the fixed scene at three sizes in the LDS form
(form = 1) and in the global form the call picks, at S = 48 / 128 / 160 with the labels spread over the range (the other LDS widths, and
the global form where only it exists), with and without valid and cls, on
the planted cases, with an edge whose frames do not exist; E = 0, guard bytes and the clear, capture, the binding's checks, and the
system path (Droid with args.segment_tracks)."""
import os
import sys

import numpy as np
import pytest
import torch

import segment_assoc_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
_cache = {}


def _dev(cuda, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _np(d):
    return {k: d[k].cpu().numpy() for k in R.OUTPUTS}


def _scene(size, S=R.S):
    if (size, S) not in _cache:
        sc = R.scene(*size)
        _cache[(size, S)] = sc if S == R.S else R.spread(sc, S)
    return _cache[(size, S)]


def _call(cuda, c, S, valid=None, cls=None, min_iou=R.MIN_IOU, **kw):
    from pvo_amd import droid_backends as db
    return db.segment_associate(_dev(cuda, c["labels"]), _dev(cuda, c["ii"]), _dev(cuda, c["jj"]), _dev(cuda, c["target"]), S,
                                valid=_dev(cuda, valid), cls=_dev(cuda, cls), min_iou=min_iou, **kw)


def _both(cuda, c, S, riders, **kw):
    valid, cls = (c["valid"], c["cls"]) if riders else (None, None)
    got = _np(_call(cuda, c, S, valid, cls, **kw))
    ref = R.associate(c["labels"], c["ii"], c["jj"], c["target"], S, valid=valid, cls=cls, min_iou=R.MIN_IOU)
    return got, ref


def _assert_same(got, ref, what):
    for k in R.OUTPUTS:
        assert np.array_equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()))


@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("riders", (False, True))
def test_the_lds_form_equals_the_reference(cuda, size, riders):
    got, ref = _both(cuda, _scene(size), R.S, riders, form=1)
    print(size, riders, "counted", int(ref["overlap"].sum()), "matches", int((ref["match"] >= 0).sum()))
    assert (ref["match"] >= 0).sum() >= 10
    _assert_same(got, ref, (size, riders))


@pytest.mark.parametrize("S", (48, 128, 160))
@pytest.mark.parametrize("riders", (False, True))
def test_wider_tables_equal_the_reference(cuda, S, riders):
    """S = 48 and 128: the LDS form's 64 x 64 and 128 x 128 tables; S = 160: the global form.  Labels spread over [1, S)"""
    c = _scene((9, 12), S)
    assert c["labels"].max() > S // 2
    for form in ((0, 1) if S <= 128 else (0,)):
        got, ref = _both(cuda, c, S, riders, form=form)
        _assert_same(got, ref, (S, riders, form))
    base = R.run(_scene((9, 12)), valid=c["valid"] if riders else None, cls=_scene((9, 12))["cls"] if riders else None)
    assert np.array_equal(ref["match_n"].sum(1), base["match_n"].sum(1))       # (the same scene under other names)


@pytest.mark.parametrize("size", R.SIZES)
def test_the_global_form_equals_the_reference(cuda, size):
    """the form the call picks: one workgroup per 256 pixels, so 30 x 101 = 3030 pixels end inside a workgroup and inside a wave"""
    c = _scene(size)
    got, ref = _both(cuda, c, R.S, True)
    _assert_same(got, ref, size)


@pytest.mark.parametrize("form", (0, 1))
def test_several_pixels_per_thread(cuda, form):
    """50 edges of 60 x 160: the counting grid would be 1900 workgroups at one pixel per thread, so a thread takes two (the call keeps
    the grid at two workgroups per compute unit or above) and a workgroup's 512-pixel chunk ends inside the frame's 9600"""
    key = ("per", 60, 160)
    if key not in _cache:
        sc = R.scene(60, 160, edges=R.EDGES * 10)
        _cache[key] = (sc, R.associate(sc["labels"], sc["ii"], sc["jj"], sc["target"], R.S, valid=sc["valid"], cls=sc["cls"], min_iou=R.MIN_IOU))
    sc, ref = _cache[key]
    E, P = len(sc["ii"]), 60 * 160
    assert E * -(-P // 512) >= 512 > E * -(-P // 1024)                         # the call's rule gives two pixels per thread
    got = _np(_call(cuda, sc, R.S, sc["valid"], sc["cls"], form=form))
    _assert_same(got, ref, ("per", form))
    assert np.array_equal(ref["overlap"][:5], ref["overlap"][5:10]) and (ref["match"] >= 0).sum() >= 100


@pytest.mark.parametrize("name", sorted(R.PLANTED))
def test_planted_cases(cuda, name):
    c, want = R.PLANTED[name]()
    for form in (0, 1):
        got = _np(_call(cuda, c, c["S"], c["valid"], c["cls"], c["min_iou"], form=form))
        for k, v in want.items():
            assert np.array_equal(got[k], v), (name, form, k, got[k])
        _assert_same(got, R.run(c), name)


def test_an_edge_without_frames_is_not_read(cuda):
    c = dict(_scene((9, 12)))
    c["ii"], c["jj"] = np.array([0, 5, -1, 1, 1 << 40], np.int64), np.array([1, 1, 2, 7, 0], np.int64)
    got, ref = _both(cuda, c, R.S, True)
    _assert_same(got, ref, "frames")
    assert not got["overlap"][1:].any() and not got["area_j"][1:].any() and (got["match"][1:] == -1).all() and got["overlap"][0].any()
    poisoned = dict(c, target=c["target"].copy())
    poisoned["target"][1:] = np.nan                                           # nothing of those edges is dereferenced
    _assert_same(_both(cuda, poisoned, R.S, True)[0], ref, "poisoned")


def _guarded(cuda, E, S):
    bufs, out = {}, {}
    for k in R.OUTPUTS:
        shape = (E, S, S) if k == "overlap" else (E, S)
        nbytes = int(np.prod(shape)) * 4
        bufs[k] = torch.full((256 + nbytes + 256,), SENTINEL, dtype=torch.uint8, device=cuda)
        out[k] = bufs[k][256:256 + nbytes].view(torch.int32).view(shape)
    return bufs, out


@pytest.mark.parametrize("S,form", ((R.S, 0), (R.S, 1), (128, 1), (160, 0)))
def test_guard_bytes_and_the_clear(cuda, S, form):
    """the outputs arrive poisoned and are written twice: the call clears its own tables, and writes nothing around them"""
    c = _scene((9, 12), S)
    bufs, out = _guarded(cuda, len(c["ii"]), S)
    ref = R.associate(c["labels"], c["ii"], c["jj"], c["target"], S, min_iou=R.MIN_IOU)
    for _ in range(2):
        _call(cuda, c, S, out=out, form=form)
        _assert_same(_np(out), ref, (S, form))
    for k, flat in bufs.items():
        assert bool((flat[:256] == SENTINEL).all()) and bool((flat[-256:] == SENTINEL).all()), k


def test_no_edge(cuda):
    c = _scene((9, 12))
    none = dict(c, ii=c["ii"][:0], jj=c["jj"][:0], target=c["target"][:0])
    got = _call(cuda, none, R.S)
    assert got["overlap"].shape == (0, R.S, R.S) and all(got[k].shape == (0, R.S) for k in R.OUTPUTS[1:])
    empty = dict(c, labels=np.zeros_like(c["labels"]))                         # frames with no segments
    got = _np(_call(cuda, empty, R.S))
    assert (got["match"] == -1).all() and not got["match_n"].any() and not got["overlap"][:, 1:].any() and not got["overlap"][:, :, 1:].any()
    _assert_same(got, R.run(empty, valid=None, cls=None), "empty")


@pytest.mark.parametrize("S", (R.S, 160))
def test_capture_and_replay_give_the_eager_bytes(cuda, S):
    from pvo_amd import droid_backends as db
    c = _scene((30, 101) if S == R.S else (9, 12), S)
    ops = [_dev(cuda, c[k]) for k in ("labels", "ii", "jj", "target")]
    valid, cls = _dev(cuda, c["valid"]), _dev(cuda, c["cls"])

    def run(out):
        db.segment_associate(*ops, S, valid=valid, cls=cls, min_iou=R.MIN_IOU, out=out, form=1 if S == R.S else 0)

    eager = _guarded(cuda, len(c["ii"]), S)[1]
    run(eager)
    torch.cuda.synchronize()
    out = _guarded(cuda, len(c["ii"]), S)[1]
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            run(out)
    torch.cuda.current_stream().wait_stream(side)
    assert all(bool((t.view(torch.uint8) == SENTINEL).all()) for t in out.values())               # capture ran nothing
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    _assert_same(_np(out), _np(eager), S)
    _assert_same(_np(out), R.associate(c["labels"], c["ii"], c["jj"], c["target"], S, valid=c["valid"], cls=c["cls"], min_iou=R.MIN_IOU), S)


def test_the_binding_checks_its_operands(cuda):
    from pvo_amd import droid_backends as db
    c = _scene((9, 12))
    d = {k: _dev(cuda, c[k]) for k in ("labels", "ii", "jj", "target", "valid", "cls")}
    base = dict(labels=d["labels"], ii=d["ii"], jj=d["jj"], target=d["target"], S=R.S)
    E = len(c["ii"])
    for over in (dict(labels=d["labels"].long()), dict(ii=d["ii"].int()), dict(jj=d["jj"][:2]), dict(target=d["target"].double()),
                 dict(target=d["target"][..., :1]), dict(target=d["target"].permute(0, 2, 1, 3)), dict(labels=d["labels"][0]),
                 dict(labels=d["labels"].cpu()), dict(valid=d["valid"].bool()), dict(valid=d["valid"][:2]), dict(cls=d["cls"].long()),
                 dict(cls=d["cls"][:, :4]), dict(S=0), dict(S=1025), dict(min_iou=float("nan")), dict(min_iou=-0.1), dict(labels=None),
                 dict(out=dict(overlap=torch.empty(E, R.S, R.S, dtype=torch.int32, device=cuda))),
                 dict(out={k: torch.empty((E, R.S, R.S) if k == "overlap" else (E, R.S + 1), dtype=torch.int32, device=cuda) for k in R.OUTPUTS})):
        with pytest.raises(ValueError, match="segment_associate"):
            db.segment_associate(**dict(base, **over))
    from pvo_amd import _lib
    import ctypes
    assert _lib.load().pvo_segment_assoc_args_size() == ctypes.sizeof(_lib.SegmentAssocArgs)
    with pytest.raises(_lib.PvoHipError, match="segment_associate"):
        db.segment_associate(**dict(base, form=7))
    wide = R.spread(c, 160)
    with pytest.raises(_lib.PvoHipError, match="segment_associate"):          # the LDS form ends at S = 128
        _call(cuda, wide, 160, form=1)


# ------------------------------------------------------------------------------------------------------------ the system path
TRUTH_IDS = (1, 2, 3)


def _plane_run(cuda, segment_tracks):
    """pvo_amd.synthetic's plane scene through a Droid's frontend (the oracle operator in the network's place).  Every frame brings the same
    segments - 1 on the left, 2 on the right, a 3 x 3 patch of 3, a strip of 0 - under ids permuted per FRAME, as a per-image panoptic
    network would number them: raw id = 1000 + 10 * perm_k[truth]"""
    from pvo_amd import droid_backends as db
    from pvo_amd.droid import Droid, default_args
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.synthetic import OracleFlowOperator, PlaneScene
    scene = PlaneScene(ht=24, wd=32, n_frames=12, seed=0)
    torch.manual_seed(0)
    droid = Droid(default_args(device=str(cuda), image_size=[scene.ht * 8, scene.wd * 8], buffer=32, store_segment_ids=True, store_images=True,
                               segment_tracks=segment_tracks))
    assert (droid.frontend.segment_tracks is not None) is bool(segment_tracks) and droid.frontend.segment_tracks is droid.segment_tracks
    truth = torch.ones(scene.ht, scene.wd, dtype=torch.int64)
    truth[:, 16:] = 2
    truth[:3, :3] = 3
    truth[-2:] = 0
    video = droid.video
    op = OracleFlowOperator(scene, video, lambda p, d, k, i, j: db.reproject(p, d, k, i, j)[0])
    frontend = DroidFrontend(op, video, device=cuda, warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20,
                             frontend_radius=2, frontend_nms=1)
    frontend.segment_tracks = droid.segment_tracks
    droid.frontend = frontend
    rng = np.random.RandomState(3)
    raw_of = {}                                                               # frame -> {raw id: truth id}
    g = torch.Generator().manual_seed(1)
    for k in range(scene.n):                                                  # (pvo_amd.synthetic.run_sequence, with the frame's segments)
        slot = video.counter
        op.bind(slot, k)
        perm = np.concatenate([[0], 1 + rng.permutation(3)])
        raw = torch.from_numpy(np.where(truth.numpy() > 0, 1000 + 10 * perm[truth.numpy()], 0))
        raw_of[float(k)] = {1000 + 10 * int(perm[t]): t for t in TRUTH_IDS}
        video.append(float(k), None if k else scene.poses[0].to(cuda), None, scene.intr.to(cuda),
                     torch.randn(scene.ht, scene.wd, 128, generator=g).half().to(cuda),
                     torch.zeros(128, scene.ht, scene.wd, dtype=torch.half, device=cuda), torch.zeros(128, scene.ht, scene.wd, dtype=torch.half, device=cuda),
                     segm=raw)
        frontend()
        if video.counter <= slot:
            op.frame_of.pop(slot, None)
            op.bind(video.counter - 1, k)
    n = video.counter
    return droid, video.poses[:n].detach().cpu().clone(), [op.frame_of.get(s, s) for s in range(n)], raw_of


def test_droid_keeps_segment_tracks_and_tracking_is_untouched_by_them(cuda, tmp_path):
    d0, poses0, frames0, _ = _plane_run(cuda, None)
    d1, poses1, frames1, raw_of = _plane_run(cuda, True)
    n = d1.video.counter
    assert frames1 == frames0 and torch.equal(poses1, poses0) and torch.equal(d1.video.disps[:n], d0.video.disps[:n])      # the switch changes no byte
    with pytest.raises(RuntimeError, match="segment_tracks"):
        d0.get_segment_tracks()
    table = d1.get_segment_tracks()
    stamps = d1.video.tstamp[:n].tolist()
    assert len(table) > 0 and d1.segment_tracks.observations >= 2
    assert {t for t, _, _ in table} <= set(stamps)                            # a removed keyframe's entries went with it
    by_truth = {}
    for t, rid, track in table:
        by_truth.setdefault(raw_of[t][rid], set()).add(track)
    print("segment tracks: %d keyframes, %d observations, %d entries; tracks per true segment %s" % (
        n, d1.segment_tracks.observations, len(table), {k: sorted(v) for k, v in by_truth.items()}))
    # the two halves keep one track each through every keyframe, under ids permuted per frame (the camera moves a few pixels between
    # keyframes: their IoU is far above 0.25); the 3 x 3 patch may or may not hold on
    assert len(by_truth[1]) == 1 and len(by_truth[2]) == 1 and by_truth[1] != by_truth[2]
    keyed = {(t, rid) for t, rid, _ in table}
    # the ledger sees a keyframe at the observation after its last update; a stream whose LAST step removes a keyframe leaves the newest
    # one unobserved, so it is held to the ledger only if the ledger has seen it
    seen = stamps if any(t == stamps[-1] for t, _ in keyed) else stamps[:-1]
    assert len(seen) >= n - 1 and all((t, rid) in keyed for t in seen for rid in raw_of[t])         # every segment of every observed keyframe has a track
    tm = d1.segment_tracks.track_map()
    assert tm.shape == (n, 24, 32) and tm.dtype == torch.int32 and not tm[:, -2:].any()
    m = len(seen)
    assert tm[:m, 5:20, :16].unique().tolist() == sorted(by_truth[1]) and tm[:m, 5:20, 16:].unique().tolist() == sorted(by_truth[2])
    last = d1.segment_tracks.last
    assert set(R.OUTPUTS) | {"ids", "ii", "jj"} <= set(last) and bool((last["ii"] < last["jj"]).all())
    # the labelled map by track: tsdf(panoptic=True, labels=track_map) runs, through Droid and through the export tool
    kw = dict(voxel=0.05, thresh=0.1)
    mesh = d1.get_mesh(panoptic=True, track_ids=True, **kw)
    same = d1.video.tsdf(panoptic=True, labels=tm, **kw)
    assert torch.equal(mesh["vlabel"], same["vlabel"]) and torch.equal(mesh["label"], same["label"])
    tracks = {track for _, _, track in table}
    assert set(mesh["label"].unique().tolist()) <= tracks | {0} and set(mesh["label"].unique().tolist()) & tracks
    raw = d1.get_mesh(panoptic=True, **kw)
    assert set(raw["label"].unique().tolist()) - {0} <= {rid for r in raw_of.values() for rid in r}      # without the flag: the ids as given
    with pytest.raises(ValueError):
        d1.video.tsdf(panoptic=True, labels=tm.long(), **kw)
    with pytest.raises(RuntimeError, match="segment_tracks"):
        d0.get_mesh(panoptic=True, track_ids=True, **kw)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import export_map
    import segment_tracks as tool
    args = export_map.parse_args(["--datapath", "x", "--map", "a.ply", "--voxel", "0.05", "--filter_thresh_map", "0.1", "--mesh", str(tmp_path / "m.ply"),
                                  "--panoptic", "--track_ids"])
    assert args.track_ids is True and "segments" in export_map.write_mesh(d1, args)
    per = tool.save_tracks(str(tmp_path / "t.npz"), table, tm.cpu().numpy(), stamps)
    z = np.load(str(tmp_path / "t.npz"))
    assert len(z["track"]) == len(table) and z["track_start"][-1] == len(z["track_tstamp"]) == len(z["track_pixels"])
    assert [t for t, _ in per[next(iter(by_truth[1]))]] == seen


def test_the_driver_runs_end_to_end_on_a_written_sequence(cuda, tmp_path):
    """tools/segment_tracks.py's main() over a sequence in the dataset's directory layout (a drifting texture, two segments under ids
    permuted per frame), random weights: the stream reader, the args it sets, the ledger behind the frontend, the .npz"""
    from PIL import Image
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import segment_tracks as tool
    root = tmp_path / "Scene01"
    (root / "15-deg-left" / "frames" / "rgb" / "Camera_0").mkdir(parents=True)
    (root / "15-deg-left" / "panFPN_segm").mkdir(parents=True)
    g = torch.Generator().manual_seed(0)
    n, ht, wd = 10, 60, 200
    big = torch.randint(0, 256, (3, ht, wd + 4 * n), generator=g).float()
    big = torch.nn.functional.avg_pool2d(big[None], 5, stride=1, padding=2)[0].permute(1, 2, 0).to(torch.uint8).numpy()
    rng = np.random.RandomState(1)
    for k in range(n):
        Image.fromarray(np.ascontiguousarray(big[:, 4 * k:4 * k + wd])).save(root / "15-deg-left" / "frames" / "rgb" / "Camera_0" / ("rgb_%05d.jpg" % k))
        left, right = rng.permutation(200)[:2] + 1
        seg = np.zeros((ht, wd, 3), dtype=np.uint8)
        seg[:, :100, 0], seg[:, 100:, 0] = left, right
        Image.fromarray(seg).save(root / "15-deg-left" / "panFPN_segm" / ("seg_%05d.png" % k))
    out = str(tmp_path / "tracks.npz")
    torch.manual_seed(0)
    tool.main(["--datapath", str(root), "--tracks", out, "--min-iou", "0.3", "--buffer", "16", "--warmup", "6", "--filter_thresh", "0",
               "--keyframe_thresh", "0", "--frontend_thresh", "100"])
    z = np.load(out)
    assert len(z["track"]) == len(z["tstamp"]) == len(z["raw_id"]) > 0 and (z["track"] >= 1).all()
    assert set(z["tstamp"].tolist()) <= set(float(k) for k in range(n)) and z["track_start"][-1] == len(z["track_tstamp"]) == len(z["track_pixels"])
    assert (np.unique(np.stack([z["tstamp"], z["raw_id"]]), axis=1).shape[1]) == len(z["track"])           # one track per (keyframe, raw id)
