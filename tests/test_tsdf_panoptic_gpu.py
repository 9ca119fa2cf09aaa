"""Panoptic surface reconstruction on the device: pvo_tsdf[_sparse]_integrate_panoptic and pvo_tsdf[_sparse]_mesh_panoptic
(pvo_amd/csrc/tsdf_fuse.h, tsdf_mesh.h, tsdf.hip, tsdf_sparse.hip) against tests/tsdf_panoptic_reference.py.  tsdf / wsum / rgb must be the BYTES the
plain calls leave; label and lconf EQUAL to the reference on every touched voxel whose decisions are not within rounding of flipping
(at most 1 % are); four deliberately wrong references that the same check must reject; split calls; bricks against the dense call;
the vertex labels EQUAL to the rule on the kernel's own volume, with the plain mesh outputs unchanged; capture and replay; the system
path (DepthVideo.tsdf(panoptic=True), the export tool)."""
import os
import sys

import numpy as np
import pytest
import torch

import tsdf_reference as R
import tsdf_sparse_reference as SR
import tsdf_panoptic_reference as P

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
_scenes, _sparse_scenes, _refs = {}, {}, {}
VARIANTS = {"colours+weight": dict(), "plain": dict(weight=False, images=False), "w_max": dict(w_max=2.25)}
CASES = [("5x24x32", 1), ("5x24x32", 8), ("3x12x16", 1), ("2x9x12", 1)]


def _dev(cuda, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _scene(cuda, name, div=1):
    """(host arrays of tsdf_reference.scene, device tensors (poses, disps, intr, images, weight), label maps host / device)"""
    if (name, div) not in _scenes:
        nf, ht, wd = R.SCENES[name][:3]
        host = R.scene(nf, ht, wd)
        lab = P.label_maps(host[5], div)
        _scenes[(name, div)] = (host, [_dev(cuda, a) for a in host[:5]], lab, _dev(cuda, lab))
    return _scenes[(name, div)]


def _ref(name, div, weight=True, w_max=0.0, mutant=None, ix=None):
    key = (name, div, weight, w_max, mutant, None if ix is None else tuple(ix))
    if key not in _refs:
        nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
        poses, disps, intr, imgs, wgt, hit = R.scene(nf, ht, wd)
        _refs[key] = P.integrate_panoptic_reference(dims, origin, voxel, trunc, poses, disps, intr, list(range(nf)) if ix is None else ix,
                                                    P.label_maps(hit, div), div, weight=wgt if weight else None, w_max=w_max,
                                                    mutant=mutant, check=mutant is None)
    return _refs[key]


def _zeros(cuda, dims, images=True):
    return {"tsdf": torch.zeros(dims, device=cuda), "wsum": torch.zeros(dims, device=cuda),
            "rgb": torch.zeros(tuple(dims) + (3,), device=cuda) if images else None,
            "label": torch.zeros(dims, dtype=torch.int32, device=cuda), "lconf": torch.zeros(dims, device=cuda)}


def _fuse(cuda, name, div, ix, weight=True, images=True, w_max=0.0, vol=None, panoptic=True):
    from pvo_amd import droid_backends as db
    nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
    host, (poses, disps, intr, imgs, wgt), lab, lab_d = _scene(cuda, name, div)
    vol = _zeros(cuda, dims, images) if vol is None else vol
    pan = dict(label=vol["label"], lconf=vol["lconf"], labels=lab_d, label_div=div) if panoptic else {}
    db.tsdf_integrate(vol["tsdf"], vol["wsum"], vol["rgb"], poses, disps, intr, torch.tensor(ix, dtype=torch.long, device=cuda), origin, voxel,
                      trunc, weight=wgt if weight else None, images=imgs if images else None, img_stride=1, img_offset=0, w_max=w_max, **pan)
    return vol


def _np(vol):
    return {k: (None if t is None else t.cpu().numpy()) for k, t in vol.items()}


def _same_bytes(a, b, keys):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in keys)


# ------------------------------------------------------------------------------------------------ integration, dense
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name,div", CASES)
def test_labels_equal_the_reference_and_the_distance_keeps_its_bytes(cuda, name, div, variant):
    kw = VARIANTS[variant]
    nf = R.SCENES[name][0]
    got = _np(_fuse(cuda, name, div, list(range(nf)), **kw))
    plain = _np(_fuse(cuda, name, div, list(range(nf)), panoptic=False, **kw))
    assert _same_bytes(got, plain, ("tsdf", "wsum", "rgb"))
    assert not plain["label"].any() and not plain["lconf"].any()                             # the plain call knows nothing of them
    ref = _ref(name, div, weight=kw.get("weight", True), w_max=kw.get("w_max", 0.0))
    ok, report = P.labels_match(got["label"], got["lconf"], ref)
    share = ref["flagged"].sum() / ref["touched"].sum()
    print("%s div %d %s: %d touched, %d labelled, flagged %.3f %%, %d voxels switched twice or more; %s" % (
        name, div, variant, ref["touched"].sum(), (got["label"] > 0).sum(), 100 * share, (ref["switches"] >= 2).sum(), report))
    assert share <= 0.01
    assert ok, report
    assert (got["label"] > (1 << 24)).sum() > 100 and set(np.unique(got["label"])) <= {0, P.PLANE_ID, P.SPHERE_ID, P.OTHER_ID}
    if "w_max" in kw:
        assert got["lconf"].max() == np.float32(2.25)


@pytest.mark.parametrize("mutant", P.MUTANTS)
@pytest.mark.parametrize("name,div", CASES)
def test_the_check_rejects_a_wrong_reference(cuda, name, div, mutant):
    nf = R.SCENES[name][0]
    got = _np(_fuse(cuda, name, div, list(range(nf))))
    wrong = _ref(name, div, mutant=mutant)
    wrong = dict(wrong, flagged=_ref(name, div)["flagged"])
    ok, report = P.labels_match(got["label"], got["lconf"], wrong)
    print(name, div, mutant, report)
    assert not ok


def test_split_calls_leave_the_bytes_of_one_call(cuda):
    for div in (1, 8):
        one = _np(_fuse(cuda, "5x24x32", div, [0, 1, 2, 3, 4]))
        two = _np(_fuse(cuda, "5x24x32", div, [3, 4], vol=_fuse(cuda, "5x24x32", div, [0, 1, 2])))
        assert _same_bytes(one, two, ("tsdf", "wsum", "rgb", "label", "lconf"))
        assert (one["label"] > 0).sum() > 1000


def test_a_permuted_ix_matches_the_reference_walking_it(cuda):
    ix = [4, 1, 3, 0, 2]
    got = _np(_fuse(cuda, "5x24x32", 1, ix))
    ok, report = P.labels_match(got["label"], got["lconf"], _ref("5x24x32", 1, ix=ix))
    assert ok, report


# ------------------------------------------------------------------------------------------------ integration, bricks
def _sparse_scene(cuda, name):
    if name not in _sparse_scenes:
        host, ix = SR.scene(name)
        lab = P.label_maps(host[5], 1)
        _sparse_scenes[name] = (host, [_dev(cuda, a) for a in host[:5]], ix, _dev(cuda, lab))
    return _sparse_scenes[name]


def _bricks(cuda, name, ix=None, weight=True, colours=True, w_max=0.0, labels=True):
    """a SparseTSDF of a scene of tsdf_sparse_reference, allocated for all frames and integrated with the frames ix"""
    from pvo_amd.tsdf_sparse import SparseTSDF
    nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES[name]
    host, (poses, disps, intr, imgs, wgt), all_ix, lab_d = _sparse_scene(cuda, name)
    vol = SparseTSDF(origin, gdims, voxel, trunc, colours=colours, device=cuda, cap=2, labels=labels)
    vol.allocate(poses, disps, intr, torch.tensor(all_ix, dtype=torch.long, device=cuda), weight=wgt if weight else None)
    vol.integrate(poses, disps, intr, torch.tensor(all_ix if ix is None else ix, dtype=torch.long, device=cuda), weight=wgt if weight else None,
                  images=imgs, img_stride=1, img_offset=0, w_max=w_max, labels=lab_d if labels else None)
    return vol


def _dense_of(cuda, name, ix=None, weight=True, colours=True, w_max=0.0):
    from pvo_amd import droid_backends as db
    nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES[name]
    host, (poses, disps, intr, imgs, wgt), all_ix, lab_d = _sparse_scene(cuda, name)
    vol = _zeros(cuda, tuple(8 * g for g in gdims), colours)
    db.tsdf_integrate(vol["tsdf"], vol["wsum"], vol["rgb"], poses, disps, intr, torch.tensor(all_ix if ix is None else ix, dtype=torch.long, device=cuda),
                      origin, voxel, trunc, weight=wgt if weight else None, images=imgs if colours else None, img_stride=1, img_offset=0,
                      w_max=w_max, label=vol["label"], lconf=vol["lconf"], labels=lab_d, label_div=1)
    return _np(vol)


def _pool_equals(vol, dense, keys):
    n = vol.bricks
    coord = vol.coord[:n].cpu().numpy()
    for k in keys:
        t = getattr(vol, k)
        if t is None:
            assert dense[k] is None
            continue
        if not np.array_equal(t[:n].cpu().numpy().view(np.uint32), SR.to_bricks(dense[k], coord).view(np.uint32)):
            return False
    return True


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SR.SCENES))
def test_bricks_hold_the_dense_calls_label_bytes(cuda, name, variant):
    kw = {k: v for k, v in VARIANTS[variant].items()}
    if "images" in kw:
        kw["colours"] = kw.pop("images")
    vol = _bricks(cuda, name, **kw)
    dense = _dense_of(cuda, name, **kw)
    assert _pool_equals(vol, dense, ("tsdf", "wsum", "rgb", "label", "lconf"))
    assert int((vol.label[:vol.bricks] > 0).sum()) > 50
    assert not bool(vol.label[vol.bricks:].any()) and not bool(vol.lconf[vol.bricks:].any())  # slots not in use stay empty
    before = (vol.label.clone(), vol.lconf.clone())
    vol._resize(2 * vol.cap)                                                                  # the pools grow by copy, zeroed behind
    for old, new in zip(before, (vol.label, vol.lconf)):
        assert torch.equal(new[:old.shape[0]], old) and not bool(new[old.shape[0]:].any()) and new.shape[0] == 2 * old.shape[0]
    plain = _bricks(cuda, name, labels=False, **kw)                                           # and the plain sparse call's bytes
    plain._resize(vol.cap)
    for k in ("tsdf", "wsum", "rgb"):
        assert (getattr(vol, k) is None and getattr(plain, k) is None) or torch.equal(getattr(vol, k), getattr(plain, k)), k
    d = vol.to_dense()
    assert set(d) == {"tsdf", "wsum", "rgb", "label", "lconf", "allocated"} and set(plain.to_dense()) == {"tsdf", "wsum", "rgb", "allocated"}
    mask = SR.voxel_mask(d["allocated"].cpu().numpy())
    assert np.array_equal(d["label"].cpu().numpy()[mask], dense["label"][mask]) and not d["label"].cpu().numpy()[~mask].any()


def test_bricks_with_more_slots_than_one_cull_chunk(cuda):
    name = "3x12x16"
    long_ix = _sparse_scene(cuda, name)[2] * 90 + [2, 0, 1]
    assert len(long_ix) == 543
    vol = _bricks(cuda, name, ix=long_ix, w_max=40.0)
    dense = _dense_of(cuda, name, ix=long_ix, w_max=40.0)
    assert dense["lconf"].max() == np.float32(40.0)
    assert _pool_equals(vol, dense, ("tsdf", "wsum", "rgb", "label", "lconf"))


def test_bricks_split_calls_leave_the_bytes_of_one_call(cuda):
    name = "5x24x32"
    host, (poses, disps, intr, imgs, wgt), all_ix, lab_d = _sparse_scene(cuda, name)
    one = _bricks(cuda, name, ix=[0, 1, 2, 3, 4])
    two = _bricks(cuda, name, ix=[0, 1, 2])
    two.integrate(poses, disps, intr, torch.tensor([3, 4], dtype=torch.long, device=cuda), weight=wgt, images=imgs, img_stride=1, img_offset=0,
                  labels=lab_d)
    for k in ("tsdf", "wsum", "rgb", "label", "lconf"):
        assert torch.equal(getattr(one, k), getattr(two, k)), k


# ------------------------------------------------------------------------------------------------ mesh
def _mesh_buffers(cuda, vcap, fcap):
    """sentinel-filled output buffers with three rows more than the capacity, viewed at their capacity"""
    fill = lambda n, nbytes, dt: torch.full((n + 3, nbytes), SENTINEL, dtype=torch.uint8, device=cuda).view(dt)
    return {"verts": fill(vcap, 12, torch.float32)[:vcap], "normals": fill(vcap, 12, torch.float32)[:vcap],
            "rgba": fill(vcap, 4, torch.uint8)[:vcap], "faces": fill(fcap, 12, torch.int32)[:fcap],
            "vlabel": fill(vcap, 4, torch.int32)[:vcap], "counts": torch.full((2,), -7, dtype=torch.int32, device=cuda)}


def _tail_untouched(t):
    base = t._base if t._base is not None else t
    return bool((base.view(torch.uint8).reshape(base.shape[0], -1)[t.shape[0]:] == SENTINEL).all())


def _cells(tsdf, wsum, min_weight=1.0):
    """the active cells [V,3] = (cz,cy,cx) in raster order under pvo_tsdf_mesh's rules"""
    nz, ny, nx = tsdf.shape
    corner = lambda a, j: a[(j >> 2):nz - 1 + (j >> 2), ((j >> 1) & 1):ny - 1 + ((j >> 1) & 1), (j & 1):nx - 1 + (j & 1)]
    valid = np.all([corner(wsum >= np.float32(min_weight), j) for j in range(8)], 0)
    n_in = np.sum([corner(tsdf < 0, j) for j in range(8)], 0)
    return np.argwhere(valid & (n_in > 0) & (n_in < 8))


@pytest.mark.parametrize("name,div", CASES)
def test_vertex_labels_of_the_kernels_own_volume(cuda, name, div):
    from pvo_amd import droid_backends as db
    nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
    vol = _fuse(cuda, name, div, list(range(nf)))
    plain = {k: v.cpu().numpy() for k, v in db.tsdf_mesh(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, min_weight=1.0).items()}
    got = {k: v.cpu().numpy() for k, v in db.tsdf_mesh(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, min_weight=1.0,
                                                      label=vol["label"]).items()}
    assert set(got) == set(plain) | {"vlabel"} and "vlabel" not in plain
    for k in plain:
        assert np.array_equal(got[k].view(np.uint8), plain[k].view(np.uint8)), k
    h = _np(vol)
    cells = _cells(h["tsdf"], h["wsum"])
    V, F = plain["counts"].tolist()
    assert len(cells) == V > 20
    want = P.vertex_labels(h["tsdf"], h["label"], cells)
    assert np.array_equal(got["vlabel"], want)
    print("%s div %d: %d vertices, labels %s" % (name, div, V, dict(zip(*np.unique(want, return_counts=True)))))
    assert (want == P.SPHERE_ID).sum() > 5 and (want == P.PLANE_ID).sum() > 5
    # the capacity protocol: one short of the need - full counts, nothing behind the capacity, the front unchanged
    short = _mesh_buffers(cuda, V - 1, F - 1)
    db.tsdf_mesh_into(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, 1.0, short, label=vol["label"])
    assert short["counts"].tolist() == [V, F]
    for k in ("verts", "normals", "rgba", "faces", "vlabel"):
        assert _tail_untouched(short[k]), k
        assert np.array_equal(short[k].cpu().numpy().reshape(short[k].shape[0], -1), got[k][:short[k].shape[0]].reshape(short[k].shape[0], -1)), k
    again = db.tsdf_mesh(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, min_weight=1.0, vcap=5, fcap=7, label=vol["label"])
    for k in got:                                                                             # grows to the need: the same mesh
        assert np.array_equal(again[k].cpu().numpy(), got[k]), k
    # a volume without labels: every vertex 0; a corner's label counts only if it is > 0
    none = db.tsdf_mesh(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, min_weight=1.0, label=torch.full_like(vol["label"], -4))
    assert not bool(none["vlabel"].any()) and none["vlabel"].shape[0] == V


@pytest.mark.parametrize("name", list(SR.SCENES))
def test_sparse_vertex_labels_and_plain_outputs(cuda, name):
    vol = _bricks(cuda, name)
    from pvo_amd import droid_backends as db
    plain = {k: v.cpu().numpy() for k, v in db.tsdf_sparse_mesh(vol.volume(), min_weight=1.0).items()}
    got = {k: v.cpu().numpy() for k, v in vol.mesh(min_weight=1.0).items()}
    assert set(got) == set(plain) | {"vlabel"}
    for k in plain:
        assert np.array_equal(got[k].view(np.uint8), plain[k].view(np.uint8)), k
    d = {k: v.cpu().numpy() for k, v in vol.to_dense().items() if v is not None}
    cells = _cells(d["tsdf"], d["wsum"])
    V, F = plain["counts"].tolist()
    assert len(cells) == V > 20
    grid = vol.grid.cpu().numpy()
    slot = grid[cells[:, 0] >> 3, cells[:, 1] >> 3, cells[:, 2] >> 3].astype(np.int64)
    perm = np.argsort(slot * 512 + (((cells[:, 0] & 7) << 6) | ((cells[:, 1] & 7) << 3) | (cells[:, 2] & 7)), kind="stable")
    want = P.vertex_labels(d["tsdf"], d["label"], cells[perm])                                # sparse order: (slot, raster in the brick)
    assert np.array_equal(got["vlabel"], want) and (want > 0).sum() > 10
    short = _mesh_buffers(cuda, V - 1, F - 1)
    db.tsdf_sparse_mesh_into(vol.volume(), 1.0, short, label=vol.label)
    assert short["counts"].tolist() == [V, F]
    for k in ("verts", "normals", "rgba", "faces", "vlabel"):
        assert _tail_untouched(short[k]), k
        assert np.array_equal(short[k].cpu().numpy().reshape(short[k].shape[0], -1), got[k][:short[k].shape[0]].reshape(short[k].shape[0], -1)), k


# ------------------------------------------------------------------------------------------------ capture
def test_capture_and_replay_give_the_eager_bytes(cuda):
    from pvo_amd import droid_backends as db
    name = "5x24x32"
    nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
    host, (poses, disps, intr, imgs, wgt), lab, lab_d = _scene(cuda, name, 1)
    ix = torch.arange(5, device=cuda)                                                         # (no host-to-device copy inside the capture)

    def run(vol, mesh):
        db.tsdf_integrate(vol["tsdf"], vol["wsum"], vol["rgb"], poses, disps, intr, ix, origin, voxel, trunc, weight=wgt, images=imgs,
                          img_stride=1, img_offset=0, label=vol["label"], lconf=vol["lconf"], labels=lab_d, label_div=1)
        db.tsdf_mesh_into(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, 1.0, mesh, label=vol["label"])

    eager, mesh_eager = _zeros(cuda, dims), _mesh_buffers(cuda, 4096, 8192)
    run(eager, mesh_eager)                                                                    # (also sizes the cached workspaces)
    torch.cuda.synchronize()
    vol, mesh = _zeros(cuda, dims), _mesh_buffers(cuda, 4096, 8192)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            run(vol, mesh)
    torch.cuda.current_stream().wait_stream(side)
    assert not any(bool(t.any()) for t in vol.values())                                       # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert _same_bytes(_np(vol), _np(eager), ("tsdf", "wsum", "rgb", "label", "lconf")) and bool((vol["label"] > 0).any())
    assert mesh["counts"].tolist() == mesh_eager["counts"].tolist() and mesh["counts"][0] > 0
    for k in mesh:
        assert torch.equal(mesh[k], mesh_eager[k]), k


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
        lab = P.label_maps(host[5], 1)
        v.segms_raw[:nf] = _dev(cuda, lab)
        v.ensure_disps_up()[:nf] = disps.repeat_interleave(8, 1).repeat_interleave(8, 2)   # (nearest: enough for the labels)
        v.counter = nf
        _system["droid"], _system["labels"] = droid, lab
    return _system["droid"]


KW = dict(voxel=0.05, trunc=0.15, thresh=0.1, origin=R.SCENES["5x24x32"][4], dims=R.SCENES["5x24x32"][3])


def test_video_tsdf_panoptic_is_the_composed_native_calls(cuda):
    from pvo_amd import droid_backends as db
    droid = _droid(cuda)
    plain = droid.get_mesh(**KW)
    got = droid.get_mesh(panoptic=True, **KW)
    assert set(got) == set(plain) | {"vlabel", "label", "lconf"}
    for k in plain:
        if torch.is_tensor(plain[k]):
            assert torch.equal(plain[k], got[k]), k
    want = db.tsdf_mesh(got["tsdf"], got["wsum"], None, KW["origin"], KW["voxel"], min_weight=1.0, label=got["label"])
    assert torch.equal(want["vlabel"], got["vlabel"]) and got["vlabel"].shape[0] == got["verts"].shape[0] > 500
    v = got["verts"].cpu().numpy().astype(np.float64)
    r = np.abs(np.linalg.norm(v - R.SPHERE_C, axis=1) - R.SPHERE_R)
    lab = got["vlabel"].cpu().numpy()
    on_sphere, far = r < 0.5 * KW["voxel"], np.linalg.norm(v - R.SPHERE_C, axis=1) > R.SPHERE_R + KW["trunc"] + 2 * KW["voxel"]
    print("%d vertices on the sphere: %d carry its id; %d far from it: %d carry the plane's" % (
        on_sphere.sum(), (lab[on_sphere] == P.SPHERE_ID).sum(), far.sum(), (lab[far] == P.PLANE_ID).sum()))
    assert on_sphere.sum() > 50 and (lab[on_sphere] == P.SPHERE_ID).mean() > 0.9 and (lab[far] == P.PLANE_ID).mean() > 0.9
    full = droid.get_mesh(panoptic=True, full_res=True, **KW)                                 # label_div 8 against the 192 x 256 depth
    assert full["vlabel"].shape[0] == full["verts"].shape[0] > 500 and int((full["vlabel"] == P.SPHERE_ID).sum()) > 50
    nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES["5x24x32"]                            # a world of whole bricks
    kw = dict(voxel=voxel, trunc=trunc, thresh=0.1, origin=origin, dims=tuple(8 * g for g in gdims))
    sparse, got = droid.get_mesh(panoptic=True, sparse=True, **kw), droid.get_mesh(panoptic=True, **kw)
    assert sparse["vlabel"].shape[0] == sparse["verts"].shape[0] > 500 and sparse["volume"].labels
    assert set(sparse) == {"verts", "normals", "rgba", "faces", "vlabel", "volume", "origin", "voxel"}
    rows = lambda m: sorted(map(bytes, np.concatenate([m["verts"].cpu().numpy().view(np.uint8).reshape(-1, 12),
                                                       m["vlabel"].cpu().numpy().view(np.uint8).reshape(-1, 4)], 1)))
    assert set(rows(sparse)) <= set(rows(got))                                                # the dense mesh inside allocated space
    from pvo_amd.droid import Droid, default_args
    bare = Droid(default_args(device=str(cuda), image_size=[192, 256], buffer=8, store_images=True))
    assert getattr(bare.video, "segms_raw", None) is None
    bare.video.counter = 2
    with pytest.raises(ValueError):
        bare.video.tsdf(panoptic=True, **KW)


def test_export_tool_writes_labels_and_instances(cuda, tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import export_map
    from pvo_amd.handoff import read_ply_mesh, write_ply_mesh
    droid = _droid(cuda)
    base = ["--datapath", "x", "--map", "a.ply", "--voxel", "0.05", "--filter_thresh_map", "0.1"]
    plain, want = str(tmp_path / "plain.ply"), str(tmp_path / "want.ply")
    args = export_map.parse_args(base + ["--mesh", plain])
    assert args.panoptic is False and args.instances_dir is None
    export_map.write_mesh(droid, args)
    g = droid.get_mesh(voxel=0.05, trunc=None, thresh=0.1, full_res=False, use_sigma=False, max_rel_sigma=None)
    write_ply_mesh(want, g["verts"], g["faces"], g["rgba"], g["normals"])
    assert open(plain, "rb").read() == open(want, "rb").read()                                # without the flag: what it was
    out, inst = str(tmp_path / "pan.ply"), str(tmp_path / "inst")
    args = export_map.parse_args(base + ["--mesh", out, "--panoptic", "--instances_dir", inst])
    assert args.panoptic is True
    line = export_map.write_mesh(droid, args)
    m = read_ply_mesh(out)
    assert "label" in m and m["label"].dtype == np.int32 and len(m["label"]) == len(m["verts"]) == len(g["verts"])
    ids = sorted(int(i) for i in np.unique(m["label"]))
    assert P.SPHERE_ID in ids and P.PLANE_ID in ids and "%d segments" % len(ids) in line
    assert sorted(os.listdir(inst)) == sorted("segment_%d.ply" % i for i in ids)
    assert sum(len(read_ply_mesh(os.path.join(inst, f))["faces"]) for f in os.listdir(inst)) == len(m["faces"])
