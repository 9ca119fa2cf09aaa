"""Frame-to-model tracking on the device: pvo_tsdf_track and pvo_tsdf_sparse_track (pvo_amd/csrc/tsdf_track.hip) against
tests/tsdf_track_reference.py on the kernel's own fused volumes - an evaluation per pixel (votes held to EQUALITY, S and J to the derived
bounds on every pixel whose decisions are not within rounding of flipping), the reduction alone from the kernel's own residual / jac, one
step, ten iterations from the host test's starts, the brick call held to the BYTES of the dense call, the contract's case list, capture,
and the system path (Droid.refine_to_model)."""
import ctypes

import numpy as np
import pytest
import torch

import tsdf_track_reference as T

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
_cache = {}
OUTPUTS = ("poses", "info", "system", "residual", "jac")


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _np(d):
    return {k: t.cpu().numpy() for k, t in d.items() if t is not None}


def _same(a, b, keys=OUTPUTS):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in keys)


def _frames(cuda, size):
    """the scene at size: (numpy poses, disps, intr, weight), the same on the device"""
    if ("frames", size) not in _cache:
        host = T.scene(*size)
        _cache[("frames", size)] = (host, [_dev(cuda, a) for a in host])
    return _cache[("frames", size)]


def _volume(cuda):
    """the kernel's own fused volume of the scene: (device tsdf, wsum, the dict the reference takes)"""
    if "vol" not in _cache:
        from pvo_amd import droid_backends as db
        _, (poses, disps, intr, wgt) = _frames(cuda, T.FUSE_SIZE)
        tsdf, wsum = torch.zeros(T.DIMS, device=cuda), torch.zeros(T.DIMS, device=cuda)
        db.tsdf_integrate(tsdf, wsum, None, poses, disps, intr, torch.arange(T.NFRAMES, device=cuda), T.ORIGIN, T.VOXEL, T.TRUNC, weight=wgt)
        _cache["vol"] = (tsdf, wsum, dict(tsdf=tsdf.cpu().numpy(), wsum=wsum.cpu().numpy(), origin=T.ORIGIN, voxel=T.VOXEL))
    return _cache["vol"]


# a world of 4 x 5 x 6 bricks around the same frames, one brick wider than the dense volume on its low sides: bricks that do not exist
WORLD = ((4, 5, 6), tuple(np.float32(o) - np.float32(0.4) for o in T.ORIGIN))


def _bricks(cuda):
    if "bricks" not in _cache:
        from pvo_amd.tsdf_sparse import SparseTSDF
        _, (poses, disps, intr, wgt) = _frames(cuda, T.FUSE_SIZE)
        vol = SparseTSDF([float(v) for v in WORLD[1]], WORLD[0], T.VOXEL, T.TRUNC, colours=False, device=cuda, cap=2)
        ix = torch.arange(T.NFRAMES, device=cuda)
        vol.allocate(poses, disps, intr, ix, weight=wgt)
        vol.integrate(poses, disps, intr, ix, weight=wgt)
        _cache["bricks"] = (vol, vol.to_dense())
    return _cache["bricks"]


def _slots(size, kind):
    """(start poses [N,7] f32, ix): "three" - two starts on frame 2 around an id out of range; "outer" - the outer cameras from
    full-extent starts and an id out of range; "starts" - the host test's starts on frame 2 and the true pose"""
    poses = T.scene(*size)[0]
    xs = T.starts(6)
    if kind == "three":
        return np.stack([T.perturbed(poses[2], xs[1]), poses[0], T.perturbed(poses[2], xs[2])]), [2, 9, 2]
    if kind == "outer":
        return np.stack([T.perturbed(poses[0], xs[0]), T.perturbed(poses[4], xs[1]), poses[1], T.perturbed(poses[4], xs[2])]), [0, 4, -3, 4]
    return np.stack([T.perturbed(poses[2], x) for x in xs] + [poses[2]]), [2] * 7


def _args(kw):
    a = dict(T.PARAMS)
    a.update(kw)
    return a


def _run(cuda, size, start, ix, weight=True, disps=None, out=None, want=True, **kw):
    from pvo_amd import droid_backends as db
    tsdf, wsum, _ = _volume(cuda)
    _, (_, d, intr, wgt) = _frames(cuda, size)
    d = d if disps is None else _dev(cuda, disps)
    return db.tsdf_track(tsdf, wsum, T.ORIGIN, T.VOXEL, _dev(cuda, start), d, intr, torch.tensor(ix, dtype=torch.long, device=cuda),
                         weight=wgt if weight else None, system=want, residual=want, jac=want, out=out, **_args(kw))


def _ref(cuda, size, start, ix, weight=True, disps=None, **kw):
    (_, d, intr, wgt), _ = _frames(cuda, size)
    return T.track_reference(_volume(cuda)[2], start, d if disps is None else disps, intr, ix, weight=wgt if weight else None, **_args(kw))


def _pair(cuda, size, kind, **kw):
    key = ("pair", size, kind, tuple(sorted(kw.items())))
    if key not in _cache:
        start, ix = _slots(size, kind)
        _cache[key] = (_np(_run(cuda, size, start, ix, **kw)), _ref(cuda, size, start, ix, **kw), start, ix)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("size", T.SIZES)
def test_an_evaluation_matches_the_reference_per_pixel(cuda, size):
    flagged = pixels = 0
    for kind in ("three", "outer"):
        for band, huber in ((0.9, 0.0), (0.6, 0.3)):
            got, ref, start, ix = _pair(cuda, size, kind, iters=0, band=band, huber=huber)
            ok, report = T.track_matches(got, ref)
            print("%dx%d %s band %.1f huber %.1f: %s" % (size[0], size[1], kind, band, huber, report))
            assert ok, report
            assert np.array_equal(got["poses"].view(np.uint32), start.view(np.uint32)) and got["info"].shape == (len(ix), 1, 4)
            live = [s for s, f in enumerate(ix) if 0 <= f < T.NFRAMES]
            assert ref["votes"][live].mean() > 0.25                                              # there is something to compare
            flagged, pixels = flagged + ref["flagged"][live].sum(), pixels + ref["flagged"][live].size
    print("%dx%d: flagged share %.4f %%" % (size[0], size[1], 100.0 * flagged / pixels))
    assert flagged <= 0.01 * pixels


@pytest.mark.parametrize("size", T.SIZES)
def test_the_reduction_alone(cuda, size):
    """H, b, E and count recomputed in fp64 from the kernel's OWN residual / jac and the weights: no flags"""
    (_, _, _, wgt), _ = _frames(cuda, size)
    worst = 0.0
    for kind, kw in (("three", dict(iters=0)), ("outer", dict(iters=0, band=0.6, huber=0.3)), ("starts", dict(iters=10)), ("three", dict(iters=1))):
        got, ref, start, ix = _pair(cuda, size, kind, **kw)
        for s, f in enumerate(ix):
            if not 0 <= f < T.NFRAMES:
                assert not got["system"][s].any() and np.isnan(got["residual"][s]).all() and not got["jac"][s].any()
                assert np.array_equal(got["info"][s], np.tile(np.float32([0, 0, 0, 4]), (got["info"].shape[1], 1)))
                continue
            ok, ratio = T.reduction_check(got["system"][s], got["info"][s, -1], got["residual"][s], got["jac"][s], wgt[f], kw.get("huber", 0.0))
            worst = max(worst, ratio)
            assert ok, (kind, s, ratio)
            assert got["info"][s, -1, 1] > 0 and got["info"][s, -1, 2] == 0
    print("%dx%d: the reduction's worst error / bound %.3f" % (size[0], size[1], worst))


@pytest.mark.parametrize("size", T.SIZES)
def test_one_step(cuda, size):
    for kind in ("three", "outer"):
        got, ref, start, ix = _pair(cuda, size, kind, iters=1)
        ok, report = T.track_matches(got, ref)
        print("%dx%d %s: %s" % (size[0], size[1], kind, report))
        assert ok, report
        err = np.abs(got["info"][:, 0, 2].astype(np.float64) - ref["info"][:, 0, 2])             # max |xi| of the step taken
        print("  max|xi| %s, error %s, bound %s" % (ref["info"][:, 0, 2], err, ref["xi0_bound"]))
        assert np.all(err <= ref["xi0_bound"] + T.EPS * ref["info"][:, 0, 2])
        live = ref["info"][:, 0, 3] == 0
        assert live.sum() >= 2 and np.all(ref["info"][live, 0, 2] > 1e-3)                         # a step worth the name


@pytest.mark.parametrize("size", T.SIZES)
def test_ten_iterations_end_at_the_reference_trackers_pose(cuda, size):
    got, ref, start, ix = _pair(cuda, size, "starts", iters=10)
    ok, report = T.track_matches(got, ref)
    truth = T.scene(*size)[0][2]
    to_truth = [T.pose_difference(p, truth) for p in got["poses"]]
    print("%dx%d: %s; %.5f .. %.5f from the true pose (recorded, not asserted)" % (size[0], size[1], report, min(to_truth), max(to_truth)))
    assert ok, report
    assert np.all(got["info"][:, -1, 0] <= got["info"][:, 0, 0])
    assert np.all(got["info"][:, -1, 3] == 0) and np.all(got["info"][:, -1, 2] == 0)


# ------------------------------------------------------------------------------------------------ bricks
@pytest.mark.parametrize("size", T.SIZES)
def test_the_brick_call_gives_the_bytes_of_the_dense_call(cuda, size):
    from pvo_amd import droid_backends as db
    vol, dense = _bricks(cuda)
    assert 0 < vol.bricks < vol.grid.numel()                                                      # there are bricks that do not exist
    _, (_, disps, intr, wgt) = _frames(cuda, size)
    for kind, kw in (("three", dict(iters=10)), ("outer", dict(iters=2, band=0.6, huber=0.3)), ("starts", dict(iters=0))):
        start, ix = _slots(size, kind)
        P_, I = _dev(cuda, start), torch.tensor(ix, dtype=torch.long, device=cuda)
        opts = dict(weight=wgt, system=True, residual=True, jac=True, **_args(kw))
        sparse = _np(vol.track(P_, disps, intr, I, **opts))
        full = _np(db.tsdf_track(dense["tsdf"], dense["wsum"], vol.origin, vol.voxel, P_, disps, intr, I, **opts))
        assert _same(sparse, full), kind
        assert (sparse["info"][:, -1, 1] > 20).sum() >= 2 and (~np.isnan(sparse["residual"])).sum() > 60


# ------------------------------------------------------------------------------------------------ the contract's cases
def test_a_frame_that_looks_away_keeps_its_pose(cuda):
    size = (13, 19)
    away = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0], np.float32)
    start = np.stack([away, _slots(size, "three")[0][0]])
    got = _np(_run(cuda, size, start, [2, 2], iters=3))
    assert np.array_equal(got["info"][0], np.tile(np.float32([0, 0, 0, 1]), (4, 1)))
    assert np.array_equal(got["poses"][0].view(np.uint32), away.view(np.uint32))
    assert np.isnan(got["residual"][0]).all() and not got["jac"][0].any() and not got["system"][0].any()
    assert np.all(got["info"][1, :, 3] == 0) and not np.array_equal(got["poses"][1], start[1])


def test_iters_zero_only_evaluates_and_poses_out_may_be_poses(cuda):
    size = (24, 32)
    start, ix = _slots(size, "three")
    zero = _np(_run(cuda, size, start, ix, iters=0))
    assert np.array_equal(zero["poses"].view(np.uint32), start.view(np.uint32)) and zero["info"].shape == (3, 1, 4)
    assert np.all(zero["info"][[0, 2], 0, 1] > 100) and np.all(zero["info"][:, 0, 2] == 0)
    full = _np(_run(cuda, size, start, ix, iters=4))
    P_ = _dev(cuda, start)
    out = {"poses": P_, "info": torch.empty(3, 5, 4, device=cuda), "system": torch.empty(3, 27, dtype=torch.float64, device=cuda),
           "residual": torch.empty((3,) + size, device=cuda), "jac": torch.empty((3,) + size + (6,), device=cuda)}
    from pvo_amd import droid_backends as db
    tsdf, wsum, _ = _volume(cuda)
    _, (_, d, intr, wgt) = _frames(cuda, size)
    db.tsdf_track(tsdf, wsum, T.ORIGIN, T.VOXEL, P_, d, intr, torch.tensor(ix, dtype=torch.long, device=cuda), weight=wgt, out=out, **_args(dict(iters=4)))
    assert _same(_np(out), full)                                                                  # poses_out aliasing poses
    assert not np.array_equal(full["poses"][0], start[0])


def _guarded(cuda, N, ht, wd, rows):
    """sentinel-filled output buffers with guard bytes behind them: (flat byte buffers, the views tsdf_track takes)"""
    shapes = dict(poses=((N, 7), torch.float32), info=((N, rows, 4), torch.float32), system=((N, 27), torch.float64),
                  residual=((N, ht, wd), torch.float32), jac=((N, ht, wd, 6), torch.float32))
    bufs, out = {}, {}
    for k, (shape, dt) in shapes.items():
        nbytes = int(np.prod(shape)) * (8 if dt == torch.float64 else 4)
        bufs[k] = torch.full((nbytes + 256,), SENTINEL, dtype=torch.uint8, device=cuda)
        out[k] = bufs[k][:nbytes].view(dt).view(shape)
    return bufs, out


def _untouched(got):
    """no 4-byte word of the outputs still holds the sentinel"""
    sent = np.frombuffer(bytes([SENTINEL] * 4), np.uint32)[0]
    return all(not (got[k].view(np.uint32) == sent).any() for k in OUTPUTS)


@pytest.mark.parametrize("size", ((13, 19), (9, 12)))
def test_everything_is_written_and_nothing_else(cuda, size):
    start, ix = _slots(size, "outer")
    vol, _ = _bricks(cuda)
    _, (_, d, intr, wgt) = _frames(cuda, size)
    for sparse in (False, True):
        bufs, out = _guarded(cuda, len(ix), size[0], size[1], 4)
        if sparse:
            vol.track(_dev(cuda, start), d, intr, torch.tensor(ix, dtype=torch.long, device=cuda), weight=wgt, out=out, **_args(dict(iters=3)))
        else:
            _run(cuda, size, start, ix, out=out, iters=3)
        for k, flat in bufs.items():
            assert bool((flat[-256:] == SENTINEL).all()), k
        got = _np(out)
        assert _untouched(got)
        assert np.all(got["info"][2, :, 3] == 4) and np.array_equal(got["poses"][2].view(np.uint32), start[2].view(np.uint32))
        assert (got["info"][[0, 1, 3], -1, 1] > 20).all()


def test_optional_outputs_weights_and_determinism(cuda):
    size = (24, 32)
    start, ix = _slots(size, "three")
    full = _np(_run(cuda, size, start, ix, iters=3))
    again = _np(_run(cuda, size, start, ix, iters=3))
    assert _same(full, again)                                                                     # the same operands, the same bytes
    bare = _np(_run(cuda, size, start, ix, want=False, iters=3))
    assert set(bare) == {"poses", "info"} and _same(bare, full, ("poses", "info"))                # NULL system / residual / jac
    (_, disps, _, _), _ = _frames(cuda, size)
    from pvo_amd import droid_backends as db
    tsdf, wsum, _ = _volume(cuda)
    _, (_, d, intr, _) = _frames(cuda, size)
    P_, I = _dev(cuda, start), torch.tensor(ix, dtype=torch.long, device=cuda)
    opts = dict(system=True, residual=True, jac=True, **_args(dict(iters=3)))
    none = _np(db.tsdf_track(tsdf, wsum, T.ORIGIN, T.VOXEL, P_, d, intr, I, weight=None, **opts))
    ones = _np(db.tsdf_track(tsdf, wsum, T.ORIGIN, T.VOXEL, P_, d, intr, I, weight=torch.ones_like(d), **opts))
    assert _same(none, ones) and not _same(none, full, ("poses",))
    # min_weight above every wsum, and a volume without a cell: no pixel contributes, status 1 (4 for the id out of range)
    for got in (_np(_run(cuda, size, start, ix, iters=2, min_weight=float(wsum.max()) + 1.0)),
                _np(db.tsdf_track(tsdf[:, :1].contiguous(), wsum[:, :1].contiguous(), T.ORIGIN, T.VOXEL, P_, d, intr, I, **dict(opts, iters=2)))):
        assert np.array_equal(got["info"][:, :, 3], np.tile(np.float32([[1], [4], [1]]), (1, 3))) and not got["info"][:, :, :3].any()
        assert np.array_equal(got["poses"].view(np.uint32), start.view(np.uint32)) and np.isnan(got["residual"]).all()
        assert not got["jac"].any() and not got["system"].any()
    none = db.tsdf_track(tsdf, wsum, T.ORIGIN, T.VOXEL, P_[:0], d, intr, I[:0], **opts)
    assert none["poses"].shape == (0, 7) and none["info"].shape == (0, 4, 4)
    from pvo_amd._lib import PvoHipError
    with pytest.raises(PvoHipError, match="out lacks residual"):                                 # asked for, but no buffer for it
        db.tsdf_track(tsdf, wsum, T.ORIGIN, T.VOXEL, P_, d, intr, I, residual=True, out={"poses": torch.empty(3, 7, device=cuda),
                                                                                         "info": torch.empty(3, 11, 4, device=cuda)})
    assert none["poses"].shape == (0, 7) and none["info"].shape == (0, 4, 4)


def test_huber_holds_the_pose_against_a_displaced_block(cuda):
    """a block of 8 x 10 pixels of frame 2 lies half a truncation behind the surface: with huber = 0.2 the pose ends nearer the clean
    result than without, on the device as in the reference"""
    size = (24, 32)
    (poses, disps, intr, wgt), _ = _frames(cuda, size)
    bad = disps.copy()
    bad[2, 6:14, 8:18] = (1.0 / (1.0 / bad[2, 6:14, 8:18].astype(np.float64) + 0.5 * T.TRUNC)).astype(np.float32)
    start, ix = _slots(size, "three")[0][:1], [2]
    dist = {}
    for who, run in (("device", lambda **kw: _np(_run(cuda, size, start, ix, want=False, **kw))), ("reference", lambda **kw: _ref(cuda, size, start, ix, **kw))):
        clean = run(iters=10)["poses"][0]
        dist[who] = [T.pose_difference(run(iters=10, disps=bad, huber=h)["poses"][0], clean) for h in (0.0, 0.2)]
    print("distance from the clean result without / with huber: device %s, reference %s" % (dist["device"], dist["reference"]))
    assert dist["device"][1] < dist["device"][0] and dist["reference"][1] < dist["reference"][0]
    assert dist["device"][0] > 1e-3                                                               # the block does pull


def _raw(cuda, size=(9, 12), sparse=False):
    """a valid argument struct of the C entry point with its tensors (kept alive) and workspace"""
    from pvo_amd import _lib
    start, ix = _slots(size, "three")
    _, (_, d, intr, wgt) = _frames(cuda, size)
    t = dict(poses=_dev(cuda, start), ix=torch.tensor(ix, dtype=torch.long, device=cuda), disps=d, intr=intr,
             out=_guarded(cuda, 3, size[0], size[1], 3)[1])
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    if sparse:
        vol, _ = _bricks(cuda)
        a = _lib.TsdfSparseTrackArgs()
        a.grid, a.tsdf, a.wsum = p(vol.grid), p(vol.tsdf), p(vol.wsum)
        (a.gz, a.gy, a.gx), a.cap = vol.grid.shape, vol.tsdf.shape[0]
        origin = [float(v) for v in vol.origin]
    else:
        tsdf, wsum, _ = _volume(cuda)
        a = _lib.TsdfTrackArgs()
        a.tsdf, a.wsum = p(tsdf), p(wsum)
        a.nz, a.ny, a.nx = T.DIMS
        origin = T.ORIGIN
    a.origin[0], a.origin[1], a.origin[2] = origin
    a.voxel, a.min_weight = T.VOXEL, 1.0
    a.poses, a.disps, a.intrinsics, a.ix, a.weight = p(t["poses"]), p(d), p(intr), p(t["ix"]), None
    a.N, a.nframes, a.ht, a.wd, a.iters, a.min_count = 3, T.NFRAMES, size[0], size[1], 2, 32
    a.band, a.huber, a.lm, a.ep = 0.9, 0.0, 1e-4, 1e-6
    o = t["out"]
    a.poses_out, a.info, a.system, a.residual, a.jac = p(o["poses"]), p(o["info"]), p(o["system"]), p(o["residual"]), p(o["jac"])
    lib = _lib.load()
    need = (lib.pvo_tsdf_sparse_track_workspace_bytes if sparse else lib.pvo_tsdf_track_workspace_bytes)(3, size[0], size[1])
    t["ws"] = torch.empty(need + 64, dtype=torch.uint8, device=cuda)
    return a, t, need, (lib.pvo_tsdf_sparse_track if sparse else lib.pvo_tsdf_track)


def test_limits_and_workspace(cuda):
    OK, EINVAL, EWORKSPACE = 0, 1, 3
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    for sparse in (False, True):
        def call(ws_bytes=None, ws_off=0, **over):
            a, t, need, fn = _raw(cuda, sparse=sparse)
            for k, v in over.items():
                setattr(a, k, v)
            ws = ctypes.c_void_p(t["ws"].data_ptr() + ws_off) if ws_off >= 0 else None
            r = fn(ctypes.byref(a), ws, need if ws_bytes is None else ws_bytes, stream)
            torch.cuda.synchronize()
            return r, t
        r, t = call()
        assert r == OK and _untouched(_np(t["out"]))
        inf, nan = float("inf"), float("nan")
        bad = [dict(iters=-1), dict(iters=65), dict(band=0.0), dict(band=1.5), dict(band=nan), dict(huber=-1.0), dict(huber=inf), dict(huber=nan),
               dict(lm=-1.0), dict(lm=nan), dict(lm=inf), dict(ep=-1.0), dict(ep=nan), dict(min_count=0), dict(voxel=0.0), dict(voxel=inf),
               dict(min_weight=nan), dict(N=-1), dict(nframes=-1), dict(ht=65536, wd=32768), dict(ht=-1), dict(ht=524281, wd=1)]
        bad += [{k: None} for k in ("poses", "poses_out", "info", "disps", "intrinsics", "ix", "tsdf", "wsum")]
        bad += [dict(grid=None), dict(gz=-1), dict(cap=-1), dict(gx=(1 << 21) // 8 + 1)] if sparse else [dict(nz=-1), dict(nz=1 << 11, ny=1 << 10, nx=1 << 10)]
        for over in bad:
            r, t = call(**over)
            assert r == EINVAL, over
            assert bool(all((v.view(torch.uint8) == SENTINEL).all() for v in t["out"].values())), over      # nothing was written
        assert call(ws_bytes=call()[1]["ws"].numel() - 64 - 1)[0] == EWORKSPACE and call(ws_off=-1)[0] == EWORKSPACE
        assert call(ws_off=4)[0] == EINVAL                                                        # not 16-byte aligned
        for over in (dict(N=0), dict(ht=0), dict(wd=0)):                                          # no pixel: PVO_OK, nothing written
            r, t = call(**over)
            assert r == OK and bool(all((v.view(torch.uint8) == SENTINEL).all() for v in t["out"].values())), over
    r, t = call(cap=0)                                                                            # (sparse) no brick: no pixel contributes
    got = _np(t["out"])
    assert r == OK and np.array_equal(got["info"][:, :, 3], np.tile(np.float32([[1], [4], [1]]), (1, 3))) and np.isnan(got["residual"]).all()


def test_args_sizes_and_workspace_bytes(cuda):
    from pvo_amd import _lib
    lib = _lib.load()
    assert lib.pvo_tsdf_track_args_size() == ctypes.sizeof(_lib.TsdfTrackArgs)
    assert lib.pvo_tsdf_sparse_track_args_size() == ctypes.sizeof(_lib.TsdfSparseTrackArgs)
    for fn in (lib.pvo_tsdf_track_workspace_bytes, lib.pvo_tsdf_sparse_track_workspace_bytes):
        assert fn(0, 24, 32) == 0 and fn(3, 0, 32) == 0
        assert fn(3, 24, 32) >= 3 * 64 + 3 * 3 * 128 and fn(3, 24, 32) % 16 == 0                  # sixteen view floats and three slabs per slot
        assert fn(64, 384, 512) >= 64 * 48 * 16 * 128


def test_capture_and_replay_give_the_eager_bytes(cuda):
    size = (24, 32)
    start, ix = _slots(size, "three")
    vol, _ = _bricks(cuda)
    _, (_, d, intr, wgt) = _frames(cuda, size)
    P_, I = _dev(cuda, start), torch.tensor(ix, dtype=torch.long, device=cuda)                    # (no copy inside the capture)
    from pvo_amd import droid_backends as db
    tsdf, wsum, _ = _volume(cuda)
    kw = _args(dict(iters=3))

    def run(out_d, out_s):
        db.tsdf_track(tsdf, wsum, T.ORIGIN, T.VOXEL, P_, d, intr, I, weight=wgt, out=out_d, **kw)
        vol.track(P_, d, intr, I, weight=wgt, out=out_s, **kw)

    eager = (_guarded(cuda, 3, size[0], size[1], 4)[1], _guarded(cuda, 3, size[0], size[1], 4)[1])
    run(*eager)                                                                                   # (also sizes the cached workspace)
    torch.cuda.synchronize()
    outs = (_guarded(cuda, 3, size[0], size[1], 4)[1], _guarded(cuda, 3, size[0], size[1], 4)[1])
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            run(*outs)
    torch.cuda.current_stream().wait_stream(side)
    assert all(bool((t.view(torch.uint8) == SENTINEL).all()) for o in outs for t in o.values())   # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        assert _same(_np(o), _np(e)) and _untouched(_np(o))


def test_many_slots_loop_over_the_grid(cuda):
    """more slots than gridDim.z may have (65535): every slot gets what it gets alone"""
    from pvo_amd import droid_backends as db
    tsdf, wsum, _ = _volume(cuda)
    poses = T.scene(2, 3)[0]
    disps = _dev(cuda, T.scene(9, 12)[1][:, 3:5, 4:7])                                            # six central pixels of the 9 x 12 frames
    K = torch.tensor([9.6, 9.6, 1.5, 1.0], device=cuda)
    N = 65540
    ix = torch.arange(N, device=cuda) % (T.NFRAMES + 1)                                           # (NFRAMES itself: out of range)
    P_ = _dev(cuda, poses)[ix.clamp(max=T.NFRAMES - 1)].contiguous()
    kw = dict(iters=1, min_count=1, system=True, residual=True)
    got = _np(db.tsdf_track(tsdf, wsum, T.ORIGIN, T.VOXEL, P_, disps, K, ix, **kw))
    few = _np(db.tsdf_track(tsdf, wsum, T.ORIGIN, T.VOXEL, P_[:T.NFRAMES + 1].contiguous(), disps, K, ix[:T.NFRAMES + 1].contiguous(), **kw))
    assert (few["info"][:T.NFRAMES, 0, 1] > 0).all() and few["info"][T.NFRAMES, 0, 3] == 4
    for k in ("poses", "info", "system", "residual"):
        assert np.array_equal(got[k].view(np.uint8), np.concatenate([few[k]] * (N // (T.NFRAMES + 1) + 1))[:N].view(np.uint8)), k


# ------------------------------------------------------------------------------------------------ system
def _droid(cuda):
    """a Droid whose video holds this scene at 1/8 of 192 x 256 images: five keyframes"""
    if "droid" not in _cache:
        from pvo_amd.droid import Droid, default_args
        nf, (ht, wd) = T.NFRAMES, T.FUSE_SIZE
        _, (poses, disps, intr, _) = _frames(cuda, T.FUSE_SIZE)
        droid = Droid(default_args(device=str(cuda), image_size=[ht * 8, wd * 8], buffer=8))
        v = droid.video
        v.poses[:nf], v.disps[:nf], v.intrinsics[:nf] = poses, disps, intr
        v.counter = nf
        _cache["droid"] = droid
    return _cache["droid"]


def test_refine_to_model_pulls_a_pushed_keyframe_back(cuda):
    """keyframe 2's pose pushed off by a voxel against get_mesh's volume: refine_to_model of THAT keyframe brings its model_residual
    median back to within a factor 2 of the keyframes the call never touched (they share the volume's discretisation error, which
    dwarfs fp32 rounding).  With a quadratic loss it does not (ratio 2.4: the residuals against a fused volume are heavy-tailed, see
    Droid.REFINE_HUBER), which is why refine_to_model tracks with a Huber loss unless told otherwise; the quadratic figure is printed."""
    droid = _droid(cuda)
    v, n = droid.video, droid.video.counter
    vol = droid.get_mesh(voxel=T.VOXEL, trunc=T.TRUNC, thresh=0.1, origin=T.ORIGIN, dims=T.DIMS)
    clean = v.model_residual(vol)["median"].cpu().numpy()
    true2 = v.poses[2].clone()
    push = torch.tensor([T.VOXEL, 0.0, 0.0], device=cuda)
    try:
        v.poses[2, :3] += push
        stored = v.poses[:n].clone()
        dry = droid.refine_to_model(vol, ix=[2])                                                  # apply=False: the video is not written
        quad = droid.refine_to_model(vol, ix=[2], huber=0.0)
        assert torch.equal(v.poses[:n], stored)
        with pytest.raises(ValueError):
            droid.refine_to_model(vol, apply=True)                                                # which keyframes to overwrite: the caller says
        with pytest.raises(ValueError):
            droid.refine_to_model(vol, ix=[2, 2], apply=True)
        with pytest.raises(ValueError):
            droid.refine_to_model(vol, ix=[2], disps=v.disps[:n])
        out = droid.refine_to_model(vol, ix=[2], apply=True)
        after = v.model_residual(vol)["median"].cpu().numpy()
        moved = T.pose_difference(v.poses[2].cpu().numpy(), true2.cpu().numpy())
        kept = v.poses[:n].clone()
    finally:
        v.poses[2] = true2
    before, reported = out["before"]["median"].cpu().numpy(), out["after"]["median"].cpu().numpy()
    others = np.delete(after, 2)
    print("model_residual medians: consistent %s, keyframe 2 pushed %.5f, refined %.5f (quadratic loss: %.5f); it ends %.5f from its true "
          "pose; ratio to the median / the smallest / the largest of the untouched keyframes' %.3f / %.3f / %.3f (quadratic: %.3f to the median)"
          % (np.round(clean, 5), before[0], after[2], float(quad["after"]["median"][0]), moved, after[2] / np.median(others), after[2] / others.min(),
             after[2] / others.max(), float(quad["after"]["median"][0]) / np.median(others)))
    assert set(out) == {"ix", "poses", "info", "before", "after"} and out["info"].shape == (1, 11, 4) and out["ix"].tolist() == [2]
    assert float(out["info"][0, -1, 3]) == 0 and torch.equal(kept[2], out["poses"][0])
    assert torch.equal(kept[[0, 1, 3, 4]], stored[[0, 1, 3, 4]]) and np.array_equal(others, np.delete(clean, 2))    # the others: never touched
    assert np.allclose(reported, after[2]) and np.allclose(dry["after"]["median"].cpu().numpy(), after[2])
    assert before[0] > after[2] and before[0] > 2.0 * np.median(others)                          # the push shows, the refinement helps
    assert after[2] <= 2.0 * np.median(others)
    assert moved < 0.5 * T.VOXEL
