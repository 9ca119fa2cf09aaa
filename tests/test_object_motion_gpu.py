"""Object motion on the device: pvo_object_motion (pvo_amd/csrc/object_motion.hip) against tests/object_motion_reference.py - an
evaluation per pixel (contribution held to EQUALITY, r and J to the derived bounds on every pixel whose decisions are not within their
bound of flipping), the reduction alone from the kernel's own residual / jac, one step and eight iterations from the NULL start and from
perturbed starts, the sphere's motion against the true one, the contract's case list, capture, and the system path (Droid with
args.object_motion)."""
import ctypes

import numpy as np
import pytest
import torch

import object_motion_reference as M

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
_cache = {}
OUTPUTS = ("rel", "motion", "info", "system", "centroid", "residual", "jac")
SPHERE = (0, 3, 6)


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _np(d):
    return {k: t.cpu().numpy() for k, t in d.items() if t is not None}


def _same(a, b, keys=OUTPUTS):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in keys)


def _scene(cuda, size):
    """(the host scene, its arrays on the device, the job list)"""
    if size not in _cache:
        sc = M.scene(*size)
        dev = {k: _dev(cuda, sc[k]) for k in ("poses", "disps", "intr", "labels", "ii", "jj", "target", "weight")}
        _cache[size] = (sc, dev, M.jobs(sc))
    return _cache[size]


def _args(case="plain", **kw):
    a = dict(M.PARAMS, **M.CASES[case])
    a.update(kw)
    return a


def _start(cuda, size, start):
    sc, _, (je, _) = _scene(cuda, size)
    return M.perturbed_start(sc, je) if isinstance(start, str) else start


def _run(cuda, size, case="plain", start=None, weight="scene", want=True, out=None, jobs=None, over=None, **kw):
    from pvo_amd import droid_backends as db
    sc, d, (je, jl) = _scene(cuda, size)
    je, jl = (je, jl) if jobs is None else jobs
    d = dict(d, **(over or {}))
    s = _start(cuda, size, start)
    w = d["weight"] if isinstance(weight, str) else weight
    return db.object_motion(d["poses"], d["disps"], d["intr"], d["labels"], d["ii"], d["jj"], d["target"], _dev(cuda, je), _dev(cuda, jl),
                            weight=w, start=None if s is None else _dev(cuda, s), system=want, centroid=want, residual=want, jac=want,
                            out=out, **_args(case, **kw))


def _ref(cuda, size, case="plain", start=None, weight="scene", jobs=None, **kw):
    key = ("ref", size, case, start if start is None or isinstance(start, str) else id(start), weight if isinstance(weight, str) else None,
           None if jobs is None else tuple(map(tuple, jobs)), tuple(sorted(kw.items())))
    if key not in _cache:
        sc, _, (je, jl) = _scene(cuda, size)
        je, jl = (je, jl) if jobs is None else jobs
        _cache[key] = M.motion_reference(sc, je, jl, start=_start(cuda, size, start), weight=weight, **_args(case, **kw))
    return _cache[key]


@pytest.mark.parametrize("size", M.SIZES)
@pytest.mark.parametrize("case", sorted(M.CASES))
def test_one_evaluation_per_pixel(cuda, size, case):
    """iters = 0 from a given start: both sides evaluate the same fp32 A"""
    got, ref = _np(_run(cuda, size, case, "perturbed", iters=0)), _ref(cuda, size, case, "perturbed", iters=0)
    ok, report = M.motion_matches(got, ref)
    print(size, case, report)
    assert ref["same_start"][ref["info"][:, -1, 3] != 4].all() and ref["flagged"].mean() <= 0.01
    assert ok, report
    assert np.array_equal(got["rel"].view(np.uint32), _start(cuda, size, "perturbed").view(np.uint32))      # no step: A is the start


@pytest.mark.parametrize("size", M.SIZES)
@pytest.mark.parametrize("case", ("plain", "huber"))
def test_the_reduction_alone(cuda, size, case):
    """H, b, E, count and the centroid recomputed in fp64 from the kernel's OWN residual and jac"""
    sc, _, (je, jl) = _scene(cuda, size)
    got = _np(_run(cuda, size, case, "perturbed", iters=2))
    fx, fy, cx, cy = [np.float64(v) for v in sc["intr"]]
    vv, uu = np.meshgrid(np.arange(size[0]), np.arange(size[1]), indexing="ij")
    worst = 0.0
    for n in range(len(je) - 1):
        e = int(je[n])
        i = int(sc["ii"][e])
        z = 1.0 / sc["disps"][i].astype(np.float64)
        X = np.stack([z * (uu - cx) / fx, z * (vv - cy) / fy, z], -1)
        ok, w = M.reduction_check(got["system"][n], got["info"][n, -1], got["centroid"][n], got["residual"][n], got["jac"][n],
                                  sc["weight"][e], X, sc["poses"][i], huber=_args(case)["huber"])
        worst = max(worst, w)
        assert ok, (n, w)
    print(size, case, "reduction: worst err / bound %.3f" % worst)


@pytest.mark.parametrize("size", M.SIZES)
@pytest.mark.parametrize("case,start,iters", (("plain", None, 1), ("plain", "perturbed", 1), ("plain", None, 8), ("plain", "perturbed", 8),
                                               ("huber", "perturbed", 8), ("zcut", "perturbed", 8), ("zfar", None, 8)))
def test_steps_and_iterations(cuda, size, case, start, iters):
    got, ref = _np(_run(cuda, size, case, start, iters=iters)), _ref(cuda, size, case, start, iters=iters)
    ok, report = M.motion_matches(got, ref)
    print(size, case, start, iters, report)
    assert ok, report
    if case == "plain" and iters == 8:                                       # the sphere's motion is the true one, the plane's the identity
        Tw = M.true_motion()
        for n in SPHERE + (9,):
            d = M.pose_difference(got["motion"][n], Tw)
            print("  job %d: motion to the truth %.3e, bound %.3e" % (n, d, ref["truth_bound"][n]))
            assert got["info"][n, -1, 3] == 0 and d <= ref["truth_bound"][n]
        for n in (1, 4, 7):
            assert M.pose_difference(got["motion"][n], M.IDENTITY) <= ref["truth_bound"][n]
        # the centroid under the motion: the sphere's points move with it (the mean of the moved points is the moved mean)
        assert np.all(np.linalg.norm(got["centroid"][list(SPHERE)] - M.R.SPHERE_C, axis=1) < M.R.SPHERE_R)


def _guarded(cuda, N, ht, wd, rows):
    """sentinel-filled output buffers with guard bytes behind them: (flat byte buffers, the views object_motion takes)"""
    f32 = torch.float32
    shapes = dict(rel=((N, 7), f32), motion=((N, 7), f32), info=((N, rows, 4), f32), system=((N, 27), torch.float64), centroid=((N, 3), f32),
                  residual=((N, ht, wd, 2), f32), jac=((N, ht, wd, 2, 6), f32))
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


@pytest.mark.parametrize("size", M.SIZES)
def test_the_case_list_of_the_contract(cuda, size):
    sc, d, (je, jl) = _scene(cuda, size)
    N = len(je)
    bufs, out = _guarded(cuda, N, size[0], size[1], 4)
    _run(cuda, size, "plain", "perturbed", out=out, iters=3)
    for k, flat in bufs.items():
        assert bool((flat[-256:] == SENTINEL).all()), k                       # everything is written and nothing else
    got = _np(out)
    start = _start(cuda, size, "perturbed")
    assert _untouched(got)
    again = _np(_run(cuda, size, "plain", "perturbed", iters=3))
    assert _same(got, again)                                                  # the same operands, the same bytes
    twin = np.array(start)                                                    # two identical jobs (0 and 13, with the same start) ...
    twin[13] = twin[0]
    two = _np(_run(cuda, size, "plain", twin, iters=3))
    assert all(np.array_equal(two[k][0].view(np.uint8), two[k][13].view(np.uint8)) for k in OUTPUTS)      # ... give identical bytes
    assert np.array_equal(two["rel"][1].view(np.uint32), got["rel"][1].view(np.uint32))           # several jobs on one edge, each its own
    assert np.all(got["info"][[0, 1, 3, 4, 6, 7, 9, 10], -1, 3] == 0)
    for n in (2, 5, 8, 11):                                                   # label 7: four pixels < min_count: status 1, A unchanged
        assert np.all(got["info"][n, :, 1] == 4) and np.all(got["info"][n, :, 3] == 1) and np.all(got["info"][n, :, 2] == 0)
        assert np.array_equal(got["rel"][n].view(np.uint32), start[n].view(np.uint32))
        assert (~np.isnan(got["residual"][n]).any(-1)).sum() == 4
    assert np.all(got["info"][12, :, :2] == 0) and np.all(got["info"][12, :, 3] == 1)             # a label nobody has: count 0 ...
    assert not got["centroid"][12].any() and not got["system"][12].any() and np.isnan(got["residual"][12]).all()      # ... centroid 0
    assert np.array_equal(got["motion"][9], got["rel"][9]) and np.array_equal(got["motion"][10], got["rel"][10])      # the (2,2) edge
    n = 14                                                                    # the edge without frames: status 4 ...
    assert np.all(got["info"][n] == (0, 0, 0, 4)) and np.array_equal(got["rel"][n].view(np.uint32), start[n].view(np.uint32))
    assert np.array_equal(got["motion"][n], np.float32(M.IDENTITY)) and not got["system"][n].any() and not got["centroid"][n].any()
    assert np.isnan(got["residual"][n]).all() and not got["jac"][n].any()
    nul = _np(_run(cuda, size, "plain", None, iters=1))
    assert np.array_equal(nul["rel"][n], np.float32(M.IDENTITY)) and np.all(nul["info"][n] == (0, 0, 0, 4))
    # ... and nothing of it dereferenced: the rows it would have read are poisoned (edge 4's target and weight; frame 1 is edge 0's too)
    tgt, wgt = d["target"].clone(), d["weight"].clone()
    tgt[4], wgt[4] = float("nan"), float("nan")
    poisoned = _np(_run(cuda, size, "plain", "perturbed", over=dict(target=tgt, weight=wgt), iters=3))
    assert _same(got, poisoned)
    # an edge index outside [0, E): the same
    far = _np(_run(cuda, size, "plain", None, jobs=(np.array([0, 5, -1, 1 << 40], np.int64), np.array([2, 2, 2, 2], np.int32)), iters=2))
    assert far["info"][0, -1, 3] == 0 and np.all(far["info"][1:, :, 3] == 4) and np.array_equal(far["motion"][1:], np.tile(np.float32(M.IDENTITY), (3, 1)))
    # rel aliased to start
    s = _dev(cuda, start)
    alias = dict(_guarded(cuda, N, size[0], size[1], 4)[1], rel=s)
    from pvo_amd import droid_backends as db
    db.object_motion(d["poses"], d["disps"], d["intr"], d["labels"], d["ii"], d["jj"], d["target"], _dev(cuda, je), _dev(cuda, jl),
                     weight=d["weight"], start=s, out=alias, **_args(iters=3))
    assert _same(_np(alias), got)
    # weight NULL against a weight of ones
    none = _np(_run(cuda, size, "plain", "perturbed", weight=None, iters=3))
    ones = _np(_run(cuda, size, "plain", "perturbed", weight=torch.ones_like(d["weight"]), iters=3))
    assert _same(none, ones) and not _same(none, got, ("rel",))
    bare = _np(_run(cuda, size, "plain", "perturbed", want=False, iters=3))                      # NULL optional outputs
    assert set(bare) == {"rel", "motion", "info"} and _same(bare, got, ("rel", "motion", "info"))


@pytest.mark.parametrize("size", M.SIZES)
def test_bad_pixels_drop_exactly_those_pixels(cuda, size):
    """NaN or non-positive disps / weight / targets at chosen pixels of the sphere on edge 0"""
    sc, d, (je, jl) = _scene(cuda, size)
    clean = _np(_run(cuda, size, "plain", "perturbed", iters=0))
    ys, xs = np.nonzero(sc["labels"][1] == 2)
    pick = [(int(ys[k]), int(xs[k])) for k in np.linspace(0, len(ys) - 1, 7).astype(int)]
    disps, wgt, tgt = d["disps"].clone(), d["weight"].clone(), d["target"].clone()
    nan, inf = float("nan"), float("inf")
    disps[1, pick[0][0], pick[0][1]] = nan
    disps[1, pick[1][0], pick[1][1]] = 0.0
    disps[1, pick[2][0], pick[2][1]] = -0.5
    wgt[0, pick[3][0], pick[3][1]] = nan
    wgt[0, pick[4][0], pick[4][1]] = 0.0
    tgt[0, pick[5][0], pick[5][1], 0] = nan
    tgt[0, pick[6][0], pick[6][1], 1] = inf
    got = _np(_run(cuda, size, "plain", "perturbed", over=dict(disps=disps, weight=wgt, target=tgt), iters=0))
    gone = np.zeros(size, bool)
    for y, x in pick:
        gone[y, x] = True
    was = ~np.isnan(clean["residual"][0]).any(-1)
    now = ~np.isnan(got["residual"][0]).any(-1)
    assert was[gone].all() and np.array_equal(now, was & ~gone) and got["info"][0, 0, 1] == clean["info"][0, 0, 1] - 7
    assert np.array_equal(got["residual"][0][now].view(np.uint32), clean["residual"][0][now].view(np.uint32)) and not got["jac"][0][gone].any()
    assert np.isfinite(got["system"][0]).all() and np.isfinite(got["info"][0]).all()
    # frame 1's disps feed edge 0 and edge 4's jobs only (edge 4 has no frames); the other edges' jobs keep their bytes
    others = [n for n in range(len(je)) if je[n] not in (0,)]
    assert all(np.array_equal(got[k][others].view(np.uint8), clean[k][others].view(np.uint8)) for k in OUTPUTS)


def _raw(cuda, size):
    """a valid argument struct of the C entry point with its tensors (kept alive) and workspace"""
    from pvo_amd import _lib
    sc, d, (je, jl) = _scene(cuda, size)
    N = 3
    t = dict(je=_dev(cuda, je[:N]), jl=_dev(cuda, jl[:N]), out=_guarded(cuda, N, size[0], size[1], 3)[1])
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    a = _lib.ObjectMotionArgs()
    a.poses, a.disps, a.intrinsics, a.labels, a.ii, a.jj, a.target = (p(d[k]) for k in ("poses", "disps", "intr", "labels", "ii", "jj", "target"))
    a.weight, a.start, a.job_edge, a.job_label = None, None, p(t["je"]), p(t["jl"])
    a.N, a.E, a.nframes, a.ht, a.wd, a.iters, a.min_count = N, len(sc["ii"]), M.NFRAMES, size[0], size[1], 2, 16
    a.z_min, a.huber, a.lm, a.ep = 0.25, 0.0, 1e-4, 1e-6
    o = t["out"]
    a.rel, a.motion, a.info, a.system, a.centroid, a.residual, a.jac = (p(o[k]) for k in OUTPUTS)
    lib = _lib.load()
    need = lib.pvo_object_motion_workspace_bytes(N, size[0], size[1])
    t["ws"] = torch.empty(need + 64, dtype=torch.uint8, device=cuda)
    return a, t, need, lib.pvo_object_motion


@pytest.mark.parametrize("size", M.SIZES)
def test_limits_and_workspace(cuda, size):
    OK, EINVAL, EWORKSPACE = 0, 1, 3
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)

    def call(ws_bytes=None, ws_off=0, **over):
        a, t, need, fn = _raw(cuda, size)
        for k, v in over.items():
            setattr(a, k, v)
        ws = ctypes.c_void_p(t["ws"].data_ptr() + ws_off) if ws_off >= 0 else None
        r = fn(ctypes.byref(a), ws, need if ws_bytes is None else ws_bytes, stream)
        torch.cuda.synchronize()
        return r, t

    clean = lambda t: bool(all((v.view(torch.uint8) == SENTINEL).all() for v in t["out"].values()))
    r, t = call()
    assert r == OK and _untouched(_np(t["out"]))
    inf, nan = float("inf"), float("nan")
    bad = [dict(iters=-1), dict(iters=65), dict(z_min=0.0), dict(z_min=-1.0), dict(z_min=nan), dict(z_min=inf), dict(huber=-1.0), dict(huber=inf),
           dict(huber=nan), dict(lm=-1.0), dict(lm=nan), dict(lm=inf), dict(ep=-1.0), dict(ep=nan), dict(ep=inf), dict(min_count=0),
           dict(N=-1), dict(E=-1), dict(nframes=-1), dict(ht=-1), dict(wd=-1), dict(ht=65536, wd=32768)]
    bad += [{k: None} for k in ("poses", "disps", "intrinsics", "labels", "ii", "jj", "target", "job_edge", "job_label", "rel", "motion", "info")]
    for over in bad:
        r, t = call(**over)
        assert r == EINVAL and clean(t), over                                 # nothing was written
    assert call(ws_bytes=call()[1]["ws"].numel() - 64 - 1)[0] == EWORKSPACE and call(ws_off=-1)[0] == EWORKSPACE
    assert call(ws_off=4)[0] == EINVAL                                        # not 16-byte aligned
    assert call(ws_bytes=0, iters=-1)[0] == EINVAL                            # PVO_EINVAL comes first
    for over in (dict(N=0), dict(ht=0), dict(wd=0), dict(N=0, rel=None), dict(ht=0, target=None)):       # no job, no pixel: PVO_OK, nothing written
        r, t = call(**over)
        assert r == OK and clean(t), over
    r, t = call(E=0, ii=None, jj=None, target=None)                           # no edge: every job has status 4
    got = _np(t["out"])
    assert r == OK and np.all(got["info"][..., 3] == 4) and not got["info"][..., :3].any() and np.isnan(got["residual"]).all()
    assert np.array_equal(got["rel"], np.tile(np.float32(M.IDENTITY), (3, 1))) and np.array_equal(got["motion"], got["rel"])
    from pvo_amd import _lib
    lib = _lib.load()
    assert lib.pvo_object_motion_args_size() == ctypes.sizeof(_lib.ObjectMotionArgs)
    fn = lib.pvo_object_motion_workspace_bytes
    assert fn(0, 24, 32) == 0 and fn(3, 0, 32) == 0 and fn(3, 24, 32) >= 3 * 64 + 3 * 3 * 128 and fn(3, 24, 32) % 16 == 0


def test_the_binding_checks_its_operands(cuda):
    from pvo_amd import droid_backends as db
    size = (9, 12)
    sc, d, (je, jl) = _scene(cuda, size)
    base = dict(poses=d["poses"], disps=d["disps"], intrinsics=d["intr"], labels=d["labels"], ii=d["ii"], jj=d["jj"], target=d["target"],
                job_edge=_dev(cuda, je), job_label=_dev(cuda, jl))
    for over in (dict(labels=d["labels"].long()), dict(job_label=_dev(cuda, jl).long()), dict(ii=d["ii"].int()), dict(disps=d["disps"].double()),
                 dict(target=d["target"][..., :1]), dict(target=d["target"].permute(0, 2, 1, 3)), dict(poses=d["poses"][:, :6]),
                 dict(job_edge=_dev(cuda, je)[:3]), dict(weight=d["weight"][:2]), dict(start=d["poses"]), dict(disps=d["disps"].cpu()),
                 dict(iters=65), dict(out=dict(rel=torch.empty(2, 7, device=cuda))), dict(residual=True, out=dict(
                     rel=torch.empty(len(je), 7, device=cuda), motion=torch.empty(len(je), 7, device=cuda), info=torch.empty(len(je), 9, 4, device=cuda)))):
        with pytest.raises(ValueError):
            db.object_motion(**dict(base, **over))
    none = db.object_motion(**dict(base, job_edge=_dev(cuda, je)[:0], job_label=_dev(cuda, jl)[:0], iters=3))
    assert none["rel"].shape == (0, 7) and none["info"].shape == (0, 4, 4)


@pytest.mark.parametrize("size", M.SIZES)
def test_capture_and_replay_give_the_eager_bytes(cuda, size):
    sc, d, (je, jl) = _scene(cuda, size)
    N = len(je)
    JE, JL, S = _dev(cuda, je), _dev(cuda, jl), _dev(cuda, _start(cuda, size, "perturbed"))       # (no copy inside the capture)
    from pvo_amd import droid_backends as db
    kw = _args("huber", iters=3)

    def run(out):
        db.object_motion(d["poses"], d["disps"], d["intr"], d["labels"], d["ii"], d["jj"], d["target"], JE, JL, weight=d["weight"], start=S,
                         out=out, **kw)

    eager = _guarded(cuda, N, size[0], size[1], 4)[1]
    run(eager)                                                                # (also sizes the cached workspace)
    torch.cuda.synchronize()
    out = _guarded(cuda, N, size[0], size[1], 4)[1]
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            run(out)
    torch.cuda.current_stream().wait_stream(side)
    assert all(bool((t.view(torch.uint8) == SENTINEL).all()) for t in out.values())               # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert _same(_np(out), _np(eager)) and _untouched(_np(out))


# ------------------------------------------------------------------------------------------------------------ the system path
def _plane_run(cuda, object_motion):
    """pvo_amd.synthetic's plane scene through a Droid's frontend (the oracle operator in the network's place), every keyframe with the
    same label image: 1 on the left, 2 on the right, a 3 x 3 patch of 3 (too small), a strip of 0 (no segment)"""
    from pvo_amd import droid_backends as db
    from pvo_amd.droid import Droid, default_args
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.object_motion import ObjectTracks, graph_object_motion, _native
    from pvo_amd.synthetic import OracleFlowOperator, PlaneScene, run_sequence
    scene = PlaneScene(ht=24, wd=32, n_frames=12, seed=0)
    torch.manual_seed(0)
    droid = Droid(default_args(device=str(cuda), image_size=[scene.ht * 8, scene.wd * 8], buffer=32, object_motion=object_motion))
    assert (droid.frontend.object_tracks is not None) is bool(object_motion)                     # the switch reaches the frontend Droid builds
    lab = torch.ones(scene.ht, scene.wd, dtype=torch.int32, device=cuda)
    lab[:, 16:] = 2
    lab[:3, :3] = 3
    lab[-2:] = 0
    droid.video.segms[:, 0] = lab
    op = OracleFlowOperator(scene, droid.video, lambda p, d, k, i, j: db.reproject(p, d, k, i, j)[0])
    tracks, seen = droid.frontend.object_tracks, []
    droid.frontend = DroidFrontend(op, droid.video, device=cuda, warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20,
                                   frontend_radius=2, frontend_nms=1)
    if tracks is not None:
        def recording(ops, job_edge, job_label, **kw):
            out = _native(ops, job_edge, job_label, **kw)
            seen.append(({k: v.clone() for k, v in ops.items()}, job_edge.clone(), job_label.clone(), dict(kw), {k: v.clone() for k, v in out.items()},
                         droid.video.tstamp.clone()))
            return out
        droid.frontend.object_tracks = ObjectTracks(droid.video, min_pixels=64, solve=lambda graph, **kw: graph_object_motion(graph, native=recording, **kw))
    poses, frames = run_sequence(scene, droid.video, droid.frontend, op)
    return droid, poses, frames, seen


def test_droid_keeps_object_tracks_and_tracking_is_untouched_by_them(cuda):
    from pvo_amd import droid_backends as db
    d0, poses0, frames0, _ = _plane_run(cuda, None)
    d1, poses1, frames1, seen = _plane_run(cuda, True)
    n = d1.video.counter
    assert frames1 == frames0 and torch.equal(poses1, poses0) and torch.equal(d1.video.disps[:n], d0.video.disps[:n])      # the switch changes no byte
    with pytest.raises(RuntimeError, match="object_motion"):
        d0.get_object_tracks()
    tracks = d1.get_object_tracks()
    stamps = d1.video.tstamp[:n].tolist()
    assert sorted(tracks) == [1, 2] and len(seen) >= 2                        # label 3 is too small, 0 is no segment
    for lab in (1, 2):
        pairs = [(t["tstamp_i"], t["tstamp_j"]) for t in tracks[lab]]
        assert pairs == sorted(pairs)
        assert set(zip(stamps[:-1], stamps[1:])) <= set(pairs), (lab, pairs, stamps)              # an entry per consecutive keyframe pair
    # every entry has the bytes of a direct call on the operands the ledger saw
    latest = {}
    for ops, je, jl, kw, out, tstamp in seen:
        direct = db.object_motion(ops["poses"], ops["disps"], ops["intrinsics"], ops["labels"], ops["ii"], ops["jj"], ops["target"], je, jl, **kw)
        assert all(torch.equal(direct[k].view(torch.uint8), out[k].view(torch.uint8)) for k in ("rel", "motion", "info", "centroid"))
        ti, tj = tstamp[ops["ii"]].tolist(), tstamp[ops["jj"]].tolist()
        for k, (e, lab) in enumerate(zip(je.tolist(), jl.tolist())):
            latest[(ti[e], tj[e], lab)] = (direct["motion"][k].cpu().numpy(), direct["centroid"][k].cpu().numpy(), direct["info"][k, -1].cpu().numpy())
    count = 0
    for lab, entries in tracks.items():
        for t in entries:
            motion, centroid, info = latest[(t["tstamp_i"], t["tstamp_j"], lab)]
            assert np.array_equal(t["motion"].view(np.uint32), motion.view(np.uint32)) and np.array_equal(t["centroid"].view(np.uint32), centroid.view(np.uint32))
            assert (t["count"], t["status"]) == (int(info[1]), int(info[3])) and t["count"] >= 64
            count += 1
    # (the scene is static and the oracle's flow is the camera's plus its noise: the motions are near the identity; printed, not held)
    worst = max(M.pose_difference(t["motion"], M.IDENTITY) for e in tracks.values() for t in e)
    print("object tracks: %d keyframes, %d observations, %d entries, the static scene's motions within %.3e of the identity" % (n, len(seen), count, worst))
    assert all(t["status"] == 0 and np.isfinite(t["motion"]).all() and np.isfinite(t["centroid"]).all() for e in tracks.values() for t in e)
