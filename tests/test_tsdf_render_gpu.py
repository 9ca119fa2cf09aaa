"""Rendering a TSDF volume on the device: pvo_tsdf_render and pvo_tsdf_sparse_render (pvo_amd/csrc/tsdf_render.hip, tsdf_ray.h) against
tests/tsdf_render_reference.py on the kernel's own fused volumes - hit / miss and ids held to EQUALITY, depth, normal and colour to the
bounds derived there on every pixel whose decisions are not within rounding of flipping (at most 1 %), four deliberately wrong
references that the same check must reject, the brick render held to the BYTES of the dense render (the test of the jump over bricks that
do not exist), the contract's case list, capture, and the system path (Droid.get_renders, DepthVideo.model_residual, the export tool)."""
import os
import sys

import numpy as np
import pytest
import torch

import tsdf_reference as R
import tsdf_sparse_reference as SR
import tsdf_panoptic_reference as P
import tsdf_render_reference as V

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
Z_FAR = 2.6
_cache = {}


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _np(d):
    return {k: (None if t is None else t.cpu().numpy()) for k, t in d.items()}


def _volume(cuda, name):
    """the kernel's own fused volume of a scene of tsdf_reference with colours and panoptic ids: (device dict, numpy dict, poses)"""
    if ("vol", name) not in _cache:
        from pvo_amd import droid_backends as db
        nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
        host = R.scene(nf, ht, wd)
        poses, disps, intr, imgs, wgt = [_dev(cuda, a) for a in host[:5]]
        vol = {"tsdf": torch.zeros(dims, device=cuda), "wsum": torch.zeros(dims, device=cuda), "rgb": torch.zeros(tuple(dims) + (3,), device=cuda),
               "label": torch.zeros(dims, dtype=torch.int32, device=cuda), "lconf": torch.zeros(dims, device=cuda)}
        db.tsdf_integrate(vol["tsdf"], vol["wsum"], vol["rgb"], poses, disps, intr, torch.arange(nf, device=cuda), origin, voxel, trunc, weight=wgt,
                          images=imgs, img_stride=1, img_offset=0, label=vol["label"], lconf=vol["lconf"], labels=_dev(cuda, P.label_maps(host[5], 1)),
                          label_div=1)
        _cache[("vol", name)] = (vol, _np(vol), host[0])
    return _cache[("vol", name)]


def _views(name, which):
    poses = _volume_poses(name)
    if which == "own":
        return poses, V.OWN_SIZE
    return V.extra_views(poses), V.EXTRA_SIZE


def _volume_poses(name):
    nf, ht, wd = R.SCENES[name][:3]
    return R.scene(nf, ht, wd)[0]


def _render(cuda, name, which, rgb=True, label=True, **kw):
    """pvo_tsdf_render of the kernel's volume at the scene's views, as numpy"""
    from pvo_amd import droid_backends as db
    _, _, _, dims, origin, voxel, trunc = R.SCENES[name]
    vol = _volume(cuda, name)[0]
    poses, (ht, wd) = _views(name, which)
    args = dict(dz=V.DZ_FACTOR * voxel, z_near=0.0, z_far=Z_FAR)
    args.update(kw)
    ix = args.pop("ix", list(range(len(poses))))
    out = db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"] if rgb else None, origin, voxel, _dev(cuda, poses), _dev(cuda, V.view_intrinsics(ht, wd)),
                         torch.tensor(ix, dtype=torch.long, device=cuda), ht, wd, label=vol["label"] if label else None, **args)
    return _np(out)


def _ref(cuda, name, which, mutant=None):
    key = ("ref", name, which, mutant)
    if key not in _cache:
        _, _, _, dims, origin, voxel, trunc = R.SCENES[name]
        vol = _volume(cuda, name)[1]
        poses, (ht, wd) = _views(name, which)
        _cache[key] = V.render_reference(vol["tsdf"], vol["wsum"], vol["rgb"], vol["label"], origin, voxel, poses, V.view_intrinsics(ht, wd),
                                         range(len(poses)), ht, wd, V.DZ_FACTOR * voxel, 0.0, Z_FAR, mutant=mutant)
    return _cache[key]


def _got(cuda, name, which):
    key = ("got", name, which)
    if key not in _cache:
        _cache[key] = _render(cuda, name, which)
    return _cache[key]


def _same(a, b, keys=("depth", "normal", "rgba", "label")):
    for k in keys:
        if (a.get(k) is None) != (b.get(k) is None):
            return False
        if a.get(k) is not None and not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)):
            return False
    return True


def _all_miss(r):
    return not any(t is not None and t.view(np.uint8).any() for t in r.values())


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", list(R.SCENES))
def test_render_matches_the_reference(cuda, name):
    flagged = pixels = 0
    for which in ("own", "extra"):
        got, ref = _got(cuda, name, which), _ref(cuda, name, which)
        ok, report = V.render_matches(got, ref)
        print("%s %s: %d hits of %d pixels; %s" % (name, which, ref["hit"].sum(), ref["hit"].size, report))
        assert ok, report
        flagged, pixels = flagged + ref["flagged"].sum(), pixels + ref["flagged"].size
        assert ref["hit"][0].mean() > 0.15                                                   # there is something to compare
    assert flagged <= 0.01 * pixels
    extra = _got(cuda, name, "extra")
    assert _all_miss({k: t[1:] for k, t in extra.items()})                                    # looking away; starting inside the sphere
    own = _got(cuda, name, "own")
    hit = own["depth"] > 0
    assert own["rgba"][hit][:, :3].max() > 0 and np.all(own["rgba"][hit][:, 3] == 255)
    ids = set(np.unique(own["label"][hit]).tolist())
    assert P.SPHERE_ID in ids and P.PLANE_ID in ids
    n = np.linalg.norm(own["normal"][hit].astype(np.float64), axis=1)
    assert np.all(np.abs(n - 1.0) < 1e-5)


@pytest.mark.parametrize("mutant", V.MUTANTS)
@pytest.mark.parametrize("name", list(R.SCENES))
def test_the_check_rejects_a_wrong_reference(cuda, name, mutant):
    ok, report = V.render_matches(_got(cuda, name, "own"), _ref(cuda, name, "own", mutant=mutant))
    print(name, mutant, report)
    assert not ok


# ------------------------------------------------------------------------------------------------ bricks
def _bricks(cuda, name, world=None):
    """a SparseTSDF of a scene of tsdf_sparse_reference with colours and ids, allocated and integrated for all frames, its dense copy,
    and the scene's poses (the last one looks away).  world = (gdims, origin): another world around the same frames"""
    if ("bricks", name, world) not in _cache:
        from pvo_amd.tsdf_sparse import SparseTSDF
        nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES[name]
        if world is not None:
            gdims, origin = world
        host, ix = SR.scene(name)
        poses, disps, intr, imgs, wgt = [_dev(cuda, a) for a in host[:5]]
        vol = SparseTSDF(origin, gdims, voxel, trunc, colours=True, device=cuda, cap=2, labels=True)
        ixd = torch.tensor(ix, dtype=torch.long, device=cuda)
        vol.allocate(poses, disps, intr, ixd, weight=wgt)
        vol.integrate(poses, disps, intr, ixd, weight=wgt, images=imgs, img_stride=1, img_offset=0, labels=_dev(cuda, P.label_maps(host[5], 1)))
        _cache[("bricks", name, world)] = (vol, vol.to_dense(), host[0])
    return _cache[("bricks", name, world)]


def _both(cuda, name, poses, ix, ht, wd, visited=False, world=None, **kw):
    """(brick render, dense render over to_dense()) of the same views, numpy"""
    from pvo_amd import droid_backends as db
    vol, dense, _ = _bricks(cuda, name, world)
    args = dict(dz=V.DZ_FACTOR * vol.voxel, z_near=0.0, z_far=3.2, min_weight=1.0)
    args.update(kw)
    P_, K, I = _dev(cuda, poses), _dev(cuda, V.view_intrinsics(ht, wd)), torch.tensor(ix, dtype=torch.long, device=cuda)
    outs = []
    for _ in range(2):
        o = {"depth": torch.empty(len(ix), ht, wd, device=cuda), "normal": torch.empty(len(ix), ht, wd, 3, device=cuda),
             "rgba": torch.empty(len(ix), ht, wd, 4, dtype=torch.uint8, device=cuda), "label": torch.empty(len(ix), ht, wd, dtype=torch.int32, device=cuda)}
        if visited:
            o["visited"] = torch.empty(len(ix), ht, wd, 2, dtype=torch.int32, device=cuda)
        outs.append(o)
    vol.render(P_, K, I, ht, wd, out=outs[0], **args)
    db.tsdf_render(dense["tsdf"], dense["wsum"], dense["rgb"], vol.origin, vol.voxel, P_, K, I, ht, wd, label=dense["label"], out=outs[1], **args)
    return _np(outs[0]), _np(outs[1])


@pytest.mark.parametrize("name", list(SR.SCENES))
def test_brick_render_gives_the_bytes_of_the_dense_render(cuda, name):
    vol, dense, scene_poses = _bricks(cuda, name)
    holes = vol.bricks < vol.grid.numel()                                                     # there are bricks that do not exist
    assert vol.bricks > 0 and (holes or name != "5x24x32")                                    # (the two small worlds are all surface)
    for poses, (ht, wd) in ((scene_poses, V.OWN_SIZE), (V.extra_views(scene_poses), V.EXTRA_SIZE)):
        ix = list(range(len(poses))) + [-2, len(poses)]
        sparse, full = _both(cuda, name, poses, ix, ht, wd, visited=True)
        hits = int((full["depth"] > 0).sum())
        walked, walked_dense = int(sparse["visited"][..., 0].sum()), int(full["visited"][..., 0].sum())
        print("%s %dx%d: %d hits of %d pixels; samples examined: bricks %d, dense %d (clipped range %d)"
              % (name, ht, wd, hits, full["depth"].size, walked, walked_dense, int(full["visited"][..., 1].sum())))
        assert _same(sparse, full)
        assert hits > 0.1 * full["depth"][0].size and len(set(np.unique(full["label"]).tolist()) & {P.SPHERE_ID, P.PLANE_ID}) == 2
        assert np.array_equal(sparse["visited"][..., 1], full["visited"][..., 1])            # the same clip of the same box
        assert np.all(sparse["visited"][..., 0] <= full["visited"][..., 0]) and (walked < walked_dense or not holes)      # the jump removed samples
        assert np.all(full["visited"][..., 0] <= full["visited"][..., 1])


def test_brick_render_of_a_corridor_crosses_bricks_that_do_not_exist(cuda):
    """the 5 x 24 x 32 scene's frames in a world of 4 x 4 x 8 bricks, 3.2 m long in x, seen along x from outside it: every ray
    crosses bricks that do not exist before it meets a surface"""
    name = "5x24x32"
    world = ((4, 4, 8), (-1.613, -0.817, 0.753))
    vol, dense, scene_poses = _bricks(cuda, name, world)
    eye = np.array([-2.0, 0.02, 1.45])
    poses = np.stack([V.look_at(eye, [0.1, 0.05, 1.3], roll=0.1), V.look_at(eye + [0.0, 0.3, 0.2], [0.1, 0.05, 1.4], roll=-0.2)])
    sparse, full = _both(cuda, name, poses, [0, 1], 21, 27, visited=True, world=world, z_far=4.0)
    assert _same(sparse, full) and int((full["depth"] > 0).sum()) > 30
    share = 1.0 - sparse["visited"][..., 0].sum() / max(full["visited"][..., 0].sum(), 1)
    print("corridor: %d hits; the jump removed %.1f %% of the samples the dense walk examined" % ((full["depth"] > 0).sum(), 100 * share))
    assert vol.bricks < vol.grid.numel() and share > 0.0


def test_brick_render_of_many_views(cuda):
    """N = 543 slots (> 512, as the brick integration's tests use): the scene's frames over and over, the one that looks away and ids
    out of range among them"""
    name = "3x12x16"
    vol, dense, scene_poses = _bricks(cuda, name)
    long_ix = SR.scene(name)[1] * 90 + [2, 0, 1]
    assert len(long_ix) == 543
    sparse, full = _both(cuda, name, scene_poses, long_ix, *V.EXTRA_SIZE)
    assert _same(sparse, full)
    first = {k: t[:len(long_ix) // 90] for k, t in sparse.items()}
    assert all(_same({k: t[6 * j:6 * j + 6] for k, t in sparse.items()}, first) for j in range(1, 90))
    assert _all_miss({k: t[1] for k, t in sparse.items()}) and not _all_miss({k: t[0] for k, t in sparse.items()})      # ix[1] = -3


def test_more_views_than_the_launch_has_layers(cuda):
    """N = 65540 > 65535 slots of one pixel each: the pixel kernel's loop over slots"""
    from pvo_amd import droid_backends as db
    name = "2x9x12"
    nf, _, _, dims, origin, voxel, trunc = R.SCENES[name]
    vol = _volume(cuda, name)[0]
    ht, wd = 2, 3
    K = torch.tensor([15.2, 15.2, 1.0, 0.5], device=cuda)                                     # the 19-wide view's focal length, six central rays
    ix = torch.arange(65540, device=cuda) % (nf + 1)                                          # (nf itself: out of range)
    kw = dict(dz=V.DZ_FACTOR * voxel, z_far=Z_FAR, label=vol["label"])
    got = _np(db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, _dev(cuda, _volume_poses(name)), K, ix, ht, wd, **kw))
    few = _np(db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, _dev(cuda, _volume_poses(name)), K, ix[:nf + 1].contiguous(), ht, wd,
                             **kw))
    assert (few["depth"][:nf] > 0).all() and _all_miss({k: t[nf:] for k, t in few.items()})
    for k in ("depth", "normal", "rgba", "label"):
        assert np.array_equal(got[k].view(np.uint8), np.concatenate([few[k]] * (65540 // (nf + 1) + 1))[:65540].view(np.uint8)), k


# ------------------------------------------------------------------------------------------------ the contract's cases
def _guarded(cuda, N, ht, wd, label=True):
    """sentinel-filled output buffers with three guard rows (of the image's width) behind them"""
    def fill(per_pixel, dt):
        flat = torch.full(((N * ht + 3) * wd * per_pixel,), SENTINEL, dtype=torch.uint8, device=cuda)
        return flat, flat[:N * ht * wd * per_pixel].view(dt)
    bufs, out = {}, {}
    for k, (nbytes, dt, shape) in dict(depth=(4, torch.float32, (N, ht, wd)), normal=(12, torch.float32, (N, ht, wd, 3)),
                                       rgba=(4, torch.uint8, (N, ht, wd, 4)), label=(4, torch.int32, (N, ht, wd))).items():
        if k == "label" and not label:
            continue
        bufs[k], flat = fill(nbytes, dt)
        out[k] = flat.view(shape)
    return bufs, out


def test_every_pixel_is_written_and_nothing_else(cuda):
    from pvo_amd import droid_backends as db
    name = "5x24x32"
    _, _, _, dims, origin, voxel, trunc = R.SCENES[name]
    vol = _volume(cuda, name)[0]
    bricks, dense, scene_poses = _bricks(cuda, name)
    for which in ("own", "extra"):
        poses, (ht, wd) = _views(name, which)
        ix = list(range(len(poses))) + [99, -1]
        for sparse in (False, True):
            bufs, out = _guarded(cuda, len(ix), ht, wd)
            I, K = torch.tensor(ix, dtype=torch.long, device=cuda), _dev(cuda, V.view_intrinsics(ht, wd))
            if sparse:
                bricks.render(_dev(cuda, poses), K, I, ht, wd, dz=0.03, z_far=Z_FAR, out=out)
            else:
                db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, _dev(cuda, poses), K, I, ht, wd, dz=0.03, z_far=Z_FAR,
                               label=vol["label"], out=out)
            for k, flat in bufs.items():
                per = flat.numel() // ((len(ix) * ht + 3) * wd)
                assert bool((flat[len(ix) * ht * wd * per:] == SENTINEL).all()), k           # the guard rows
            sent32 = np.frombuffer(bytes([SENTINEL] * 4), np.uint32)[0]
            got = _np(out)
            assert not (got["depth"].view(np.uint32) == sent32).any() and not (got["normal"].view(np.uint32) == sent32).any()
            assert not (got["label"].view(np.uint32) == sent32).any() and set(np.unique(got["rgba"][..., 3]).tolist()) <= {0, 255}
            assert (got["depth"] > 0).sum() > 50
            assert _all_miss({k: t[-2:] for k, t in got.items()})                              # the ids out of range


def test_optional_outputs_and_volumes(cuda):
    from pvo_amd import droid_backends as db
    name = "3x12x16"
    _, _, _, dims, origin, voxel, trunc = R.SCENES[name]
    vol = _volume(cuda, name)[0]
    full = _got(cuda, name, "own")
    poses, (ht, wd) = _views(name, "own")
    N = len(poses)
    P_, K, I = _dev(cuda, poses), _dev(cuda, V.view_intrinsics(ht, wd)), torch.arange(N, device=cuda)
    kw = dict(dz=V.DZ_FACTOR * voxel, z_near=0.0, z_far=Z_FAR)
    # NULL normal / rgba / label leave depth's bytes unchanged
    only = {"depth": torch.full((N, ht, wd), -1.0, device=cuda)}
    db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, P_, K, I, ht, wd, out=only, **kw)
    assert np.array_equal(only["depth"].cpu().numpy().view(np.uint32), full["depth"].view(np.uint32))
    bare = _render(cuda, name, "own", normals=False, label=False)
    assert set(bare) == {"depth", "rgba"} and _same(bare, full, ("depth", "rgba"))
    # no rgb volume: (0,0,0,255) on hits, the rest unchanged
    grey = _render(cuda, name, "own", rgb=False)
    hit = full["depth"] > 0
    assert _same(grey, full, ("depth", "normal", "label")) and not grey["rgba"][hit][:, :3].any() and np.all(grey["rgba"][hit][:, 3] == 255)
    assert not grey["rgba"][~hit].any()
    # min_weight above every wsum: all miss; N = 0; a volume without a cell: all miss, whatever the buffers held
    assert _all_miss(_render(cuda, name, "own", min_weight=float(vol["wsum"].max()) + 1.0))
    none = db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, P_, K, I[:0], ht, wd, label=vol["label"], **kw)
    assert none["depth"].shape == (0, ht, wd) and none["label"].shape == (0, ht, wd)
    _, out = _guarded(cuda, N, ht, wd, label=False)
    db.tsdf_render(vol["tsdf"][:, :1].contiguous(), vol["wsum"][:, :1].contiguous(), None, origin, voxel, P_, K, I, ht, wd, out=out, **kw)
    assert _all_miss(_np(out))
    # the defaults: dz = voxel / 2 and z_far from the box give what the explicit values give
    auto = db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, P_, K, I, ht, wd, label=vol["label"])
    dz, z_near, z_far = db._render_range("t", dims, origin, voxel, P_, I, None, 0.0, None)
    same = db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, P_, K, I, ht, wd, label=vol["label"], dz=0.5 * voxel, z_far=z_far)
    assert _same(_np(auto), _np(same)) and (auto["depth"] > 0).sum() > 100
    from pvo_amd._lib import PvoHipError
    with pytest.raises(PvoHipError, match="raise dz"):
        db.tsdf_render(vol["tsdf"], vol["wsum"], None, origin, voxel, P_, K, I, ht, wd, dz=1e-6)


def test_the_same_operands_give_the_same_bytes(cuda):
    for name in ("5x24x32", "2x9x12"):
        assert _same(_render(cuda, name, "own"), _got(cuda, name, "own"))
    vol, dense, scene_poses = _bricks(cuda, "5x24x32")
    a, _ = _both(cuda, "5x24x32", scene_poses, list(range(len(scene_poses))), *V.OWN_SIZE)
    b, _ = _both(cuda, "5x24x32", scene_poses, list(range(len(scene_poses))), *V.OWN_SIZE)
    assert _same(a, b)


def test_capture_and_replay_give_the_eager_bytes(cuda):
    from pvo_amd import droid_backends as db
    name = "5x24x32"
    _, _, _, dims, origin, voxel, trunc = R.SCENES[name]
    vol = _volume(cuda, name)[0]
    bricks, dense, scene_poses = _bricks(cuda, name)
    poses, (ht, wd) = _views(name, "own")
    N = len(poses)
    P_, K, I = _dev(cuda, poses), _dev(cuda, V.view_intrinsics(ht, wd)), torch.arange(N, device=cuda)       # (no copy inside the capture)
    SP = _dev(cuda, scene_poses)
    SI = torch.arange(len(scene_poses), device=cuda)

    def run(out_d, out_s):
        db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, P_, K, I, ht, wd, dz=0.03, z_far=Z_FAR, label=vol["label"], out=out_d)
        bricks.render(SP, K, SI, ht, wd, dz=0.03, z_far=3.2, out=out_s)

    eager = (_guarded(cuda, N, ht, wd)[1], _guarded(cuda, len(scene_poses), ht, wd)[1])
    run(*eager)                                                                               # (also sizes the cached workspace)
    torch.cuda.synchronize()
    outs = (_guarded(cuda, N, ht, wd)[1], _guarded(cuda, len(scene_poses), ht, wd)[1])
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            run(*outs)
    torch.cuda.current_stream().wait_stream(side)
    assert all(bool((t.view(torch.uint8) == SENTINEL).all()) for o in outs for t in o.values())            # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        assert _same(_np(o), _np(e)) and (o["depth"] > 0).sum() > 100


# ------------------------------------------------------------------------------------------------ system
_system = {}


def _droid(cuda):
    """a Droid whose video holds tsdf_reference's analytic scene at 1/8 of 192 x 256 images with raw segment ids: five keyframes"""
    if "droid" not in _system:
        from pvo_amd.droid import Droid, default_args
        nf, ht, wd = 5, 24, 32
        host = R.scene(nf, ht, wd)
        poses, disps, intr = [_dev(cuda, a) for a in host[:3]]
        droid = Droid(default_args(device=str(cuda), image_size=[ht * 8, wd * 8], buffer=8, store_images=True, store_segment_ids=True))
        v = droid.video
        v.poses[:nf], v.disps[:nf], v.intrinsics[:nf] = poses, disps, intr
        g = torch.Generator().manual_seed(7)
        v.images[:nf] = torch.randint(0, 256, (nf, 3, ht * 8, wd * 8), generator=g).to(torch.uint8).to(cuda)
        v.segms_raw[:nf] = _dev(cuda, P.label_maps(host[5], 1))
        v.ensure_disps_up()[:nf] = disps.repeat_interleave(8, 1).repeat_interleave(8, 2)
        v.counter = nf
        _system["droid"], _system["host"] = droid, host
    return _system["droid"]


KW = dict(voxel=0.05, trunc=0.15, thresh=0.1, origin=R.SCENES["5x24x32"][4], dims=R.SCENES["5x24x32"][3])


def test_get_renders_is_the_composed_native_calls(cuda):
    from pvo_amd import droid_backends as db
    droid = _droid(cuda)
    v, n = droid.video, droid.video.counter
    host = _system["host"]
    ix = torch.arange(n, device=cuda)
    intr = v.intrinsics[0].contiguous()
    vol = droid.get_mesh(panoptic=True, keep_rgb=True, **KW)
    plain = droid.get_mesh(**KW)
    assert set(vol) == set(plain) | {"vlabel", "label", "lconf", "rgb"} and torch.equal(vol["tsdf"], plain["tsdf"])
    got = droid.get_renders(vol)
    want = db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"], KW["origin"], KW["voxel"], v.poses[:n], intr, ix, 24, 32, label=vol["label"])
    assert set(got) == {"depth", "normal", "rgba", "label"} and all(torch.equal(got[k], want[k]) for k in got)
    bare = droid.get_renders(plain, ix=[3, 1], dz=0.02, z_far=3.0, normals=False)             # no colours, no ids; chosen views
    want = db.tsdf_render(plain["tsdf"], plain["wsum"], None, KW["origin"], KW["voxel"], v.poses[:n], intr, torch.tensor([3, 1], device=cuda), 24, 32,
                          dz=0.02, z_far=3.0, normals=False)
    assert set(bare) == {"depth", "rgba"} and all(torch.equal(bare[k], want[k]) for k in bare)
    # against the closed forms, within twice what the reference's render of the reference's volume measures (test_tsdf_render_host.py)
    depth, normal, label = [got[k].cpu().numpy() for k in ("depth", "normal", "label")]
    worst_d = worst_n = 0.0
    for k in range(n):
        d, nrm, sphere = V.analytic_view(host[0][k], host[2], 24, 32)
        ok = V.interior(sphere) & (depth[k] > 0)
        worst_d = max(worst_d, np.abs(depth[k] - d)[ok].max())
        worst_n = max(worst_n, np.abs(normal[k] - nrm).max(-1)[ok].max())
        on = ok & sphere
        assert ok.sum() > 100 and on.sum() >= 25 and (label[k][on] == P.SPHERE_ID).mean() > 0.9
        assert (label[k][ok & ~sphere] == P.PLANE_ID).mean() > 0.7                            # (frame 1 calls the plane something else)
    print("system render against the closed forms: depth %.4f, normal %.4f" % (worst_d, worst_n))
    assert worst_d <= 2.0 * V.ANALYTIC_DEPTH_ERR and worst_n <= 2.0 * V.ANALYTIC_NORMAL_ERR
    # a novel pose, full resolution, and the brick volume
    novel = V.extra_views(host[0])[:1]
    got = droid.get_renders(vol, poses=novel, full_res=True, z_far=3.0)
    want = db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"], KW["origin"], KW["voxel"], _dev(cuda, novel), (8.0 * v.intrinsics[0]).contiguous(),
                          torch.arange(1, device=cuda), 192, 256, label=vol["label"], z_far=3.0)
    assert all(torch.equal(got[k], want[k]) for k in want) and (got["depth"] > 0).float().mean() > 0.1
    nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES["5x24x32"]
    sp = droid.get_mesh(panoptic=True, sparse=True, voxel=voxel, trunc=trunc, thresh=0.1, origin=origin, dims=tuple(8 * g for g in gdims))
    got = droid.get_renders(sp)
    want = db.tsdf_sparse_render(sp["volume"].volume(), v.poses[:n], intr, ix, 24, 32, label=sp["volume"].label)
    assert set(got) == {"depth", "normal", "rgba", "label"} and all(torch.equal(got[k], want[k]) for k in got)
    assert (got["depth"] > 0).float().mean() > 0.3 and int((got["label"] == P.SPHERE_ID).sum()) > 100
    with pytest.raises(ValueError):
        droid.get_renders(vol, poses=novel, ix=[0])


def test_model_residual_is_small_on_a_consistent_scene_and_sees_a_scaled_keyframe(cuda):
    """The keyframes' own depths are the closed forms, so on the consistent scene the residual is the render's distance from the closed
    form: its median stays below twice the MEAN error the host test measures (ANALYTIC_DEPTH_MEAN_ERR) over the nearest depth of the
    scene (0.9).  Frame 2 with depths 1.5 % too large, fused with equal weight among five, leaves the surface 0.3 % off and itself
    1.2 % from it: its median must reach half of that, exceed every other frame's and twice the consistent scene's."""
    droid = _droid(cuda)
    v, n = droid.video, droid.video.counter
    vol = v.tsdf(**KW)
    res = v.model_residual(vol)
    med, p90, share = [res[k].cpu().numpy() for k in ("median", "p90", "share")]
    print("consistent: median %s p90 %s share %s" % (np.round(med, 5), np.round(p90, 5), np.round(share, 3)))
    assert res["ix"].tolist() == list(range(n)) and med.shape == (n,)
    assert med.max() <= 2.0 * V.ANALYTIC_DEPTH_MEAN_ERR / 0.9 and np.all(p90 >= med)
    hits = (v.tsdf_render(vol, normals=False)["depth"] > 0).float().mean((1, 2)).cpu().numpy()
    assert np.allclose(share, hits) and share.min() > 0.1                                     # (every pixel of the scene has a depth of its own)
    true2 = v.disps[2].clone()
    try:
        v.disps[2] = true2 / 1.015                                                            # frame 2's depths 1.5 % too large
        off = v.model_residual(v.tsdf(**KW))
    finally:
        v.disps[2] = true2
    med2 = off["median"].cpu().numpy()
    print("frame 2 scaled: median %s" % np.round(med2, 5))
    assert med2[2] > 2.0 * med.max() and med2[2] >= 0.006 and med2[2] == med2.max()
    sub = v.model_residual(vol, ix=[4, 0])
    assert sub["ix"].tolist() == [4, 0] and np.array_equal(sub["median"].cpu().numpy(), med[[4, 0]])


def test_export_tool_writes_the_renders(cuda, tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import export_map
    droid = _droid(cuda)
    n = droid.video.counter
    base = ["--datapath", "x", "--map", "a.ply", "--voxel", "0.05", "--filter_thresh_map", "0.1"]
    plain, out, rd = str(tmp_path / "plain.ply"), str(tmp_path / "mesh.ply"), str(tmp_path / "renders")
    export_map.write_mesh(droid, export_map.parse_args(base + ["--mesh", plain]))
    args = export_map.parse_args(base + ["--mesh", out, "--render_dir", rd])
    assert args.render_dir == rd
    line = export_map.write_mesh(droid, args)
    assert open(plain, "rb").read() == open(out, "rb").read()                                 # the mesh is what it was
    assert "model residual" in line and "renders: depth / normal / rgba of %d keyframes at 24 x 32" % n in line
    assert sorted(os.listdir(rd)) == sorted("%s_%06d.npy" % (k, i) for k in ("depth", "normal", "rgba") for i in range(n))
    d, nrm, c = [np.load(os.path.join(rd, "%s_000002.npy" % k)) for k in ("depth", "normal", "rgba")]
    assert (d.shape, d.dtype, nrm.shape, nrm.dtype, c.shape, c.dtype) == ((24, 32), np.float32, (24, 32, 3), np.float32, (24, 32, 4), np.uint8)
    assert (d > 0).mean() > 0.3 and c[d > 0][:, :3].max() > 0
    rd2 = str(tmp_path / "renders_panoptic")
    for extra in (["--panoptic"], ["--panoptic", "--sparse"]):
        args = export_map.parse_args(base + ["--mesh", out, "--render_dir", rd2] + extra)
        export_map.write_mesh(droid, args)
        assert sorted(os.listdir(rd2)) == sorted("%s_%06d.npy" % (k, i) for k in ("depth", "normal", "rgba", "label") for i in range(n))
        lab = np.load(os.path.join(rd2, "label_000000.npy"))
        assert lab.shape == (24, 32) and lab.dtype == np.int32 and (lab == P.SPHERE_ID).sum() > 10
    with pytest.raises(SystemExit):
        export_map.parse_args(["--datapath", "x", "--map", "a.ply", "--render_dir", rd])
