"""Surface reconstruction on the device: pvo_tsdf_integrate and pvo_tsdf_mesh (pvo_amd/csrc/tsdf.hip) against tests/tsdf_reference.py -
the weight sums held to EQUALITY and the values to the bound derived there on every voxel whose decisions are not within rounding of
flipping (at most 1 % are, tests/test_tsdf_host.py), four deliberately wrong references that the same check must reject, the case list
of the contract, the mesh of the kernel's own volume (counts and faces EQUAL), and the system path (DepthVideo.tsdf / Droid.get_mesh)."""
import numpy as np
import pytest
import torch

import tsdf_reference as R

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
_scenes, _runs = {}, {}


def _scene(cuda, name):
    if name not in _scenes:
        nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
        host = R.scene(nf, ht, wd)
        dev = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in host[:5]]
        _scenes[name] = (host, dev)
    return _scenes[name]


def _fuse(cuda, name, ix, weight=True, images=True, w_max=0.0, vol=None, disps=None, weights=None):
    """pvo_tsdf_integrate of frames ix of a scene into `vol` (default: a zeroed volume); returns the volume (device tensors)"""
    from pvo_amd import droid_backends as db
    nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
    host, (poses, disps_d, intr, imgs, wgt) = _scene(cuda, name)
    if vol is None:
        vol = (torch.zeros(dims, device=cuda), torch.zeros(dims, device=cuda), torch.zeros(dims + (3,), device=cuda) if images else None)
    db.tsdf_integrate(vol[0], vol[1], vol[2], poses, disps_d if disps is None else disps, intr,
                      torch.tensor(ix, dtype=torch.long, device=cuda), origin, voxel, trunc,
                      weight=(wgt if weights is None else weights) if weight else None,
                      images=imgs if images else None, img_stride=1, img_offset=0, w_max=w_max)
    return vol


def _np(vol):
    return [None if t is None else t.cpu().numpy() for t in vol]


def _ref(name, ix, weight=True, images=True, w_max=0.0, mutant=None, disps=None, weights=None):
    nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
    poses, disps_h, intr, imgs, wgt, hit = R.scene(nf, ht, wd)
    return R.integrate_reference(dims, origin, voxel, trunc, poses, disps_h if disps is None else disps, intr, ix,
                                 weight=(wgt if weights is None else weights) if weight else None, images=imgs if images else None,
                                 img_stride=1, img_offset=0, w_max=w_max, mutant=mutant)


def _full(cuda, name):
    """(kernel volume as numpy, reference) of all frames of a scene with its weights and colours, computed once"""
    if name not in _runs:
        nf = R.SCENES[name][0]
        _runs[name] = (_np(_fuse(cuda, name, list(range(nf)))), _ref(name, range(nf)))
    return _runs[name]


def _bytes_equal(a, b):
    return all((x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ integration
@pytest.mark.parametrize("name", list(R.SCENES))
def test_volume_matches_the_reference(cuda, name):
    got, ref = _full(cuda, name)
    ok, report = R.volume_matches(got[0], got[1], got[2], ref)
    print("%s: %d touched, %d flagged, %d voxel-frame pairs; %s" % (name, ref["touched"].sum(), ref["flagged"].sum(), ref["hits"], report))
    assert ref["flagged"].sum() <= 0.01 * ref["touched"].sum()
    assert ok, report
    # and without weights and colours: the other instantiation
    nf = R.SCENES[name][0]
    plain = _np(_fuse(cuda, name, list(range(nf)), weight=False, images=False))
    ok, report = R.volume_matches(plain[0], plain[1], None, _ref(name, range(nf), weight=False, images=False))
    assert ok, report
    assert np.array_equal(plain[1], np.round(plain[1])) and plain[1].max() <= nf            # unit weights: counts


@pytest.mark.parametrize("name", list(R.SCENES))
@pytest.mark.parametrize("mutant", ["floor_u", "ray_sdf", "unweighted", "no_weight"])
def test_the_check_rejects_a_wrong_reference(cuda, name, mutant):
    """floor(u) in place of rounding, sdf along the ray, an unweighted mean, weight ignored: the kernel's volume must FAIL the check
    of test_volume_matches_the_reference against each, so the bound is not loose enough to hide any of them"""
    got, _ = _full(cuda, name)
    ok, report = R.volume_matches(got[0], got[1], got[2], _ref(name, range(R.SCENES[name][0]), mutant=mutant))
    print(name, mutant, report)
    assert not ok


def test_split_calls_leave_the_bytes_of_one_call(cuda):
    name = "5x24x32"
    one = _np(_fuse(cuda, name, [0, 1, 2, 3, 4]))
    two = _np(_fuse(cuda, name, [3, 4], vol=_fuse(cuda, name, [0, 1, 2])))
    assert _bytes_equal(one, two)
    assert _bytes_equal(one, _full(cuda, name)[0])                                          # a second run: identical bytes


def test_a_permuted_ix_follows_its_order(cuda):
    name, ix = "5x24x32", [3, 0, 4, 2, 1]
    got = _np(_fuse(cuda, name, ix))
    ok, report = R.volume_matches(got[0], got[1], got[2], _ref(name, ix))
    assert ok, report
    assert not _bytes_equal(got, _full(cuda, name)[0])                                      # the order is part of the arithmetic


def test_ids_out_of_range_change_nothing(cuda):
    name = "5x24x32"
    got = _np(_fuse(cuda, name, [-1, 0, 1, 5, 2, 3, -7, 4, 1 << 40]))
    assert _bytes_equal(got, _full(cuda, name)[0])
    only_bad = _np(_fuse(cuda, name, [-1, 5]))
    assert not any(t.view(np.uint32).any() for t in only_bad)


def test_bad_depths_and_zero_weights_are_skipped(cuda):
    name = "3x12x16"
    nf, ht, wd = R.SCENES[name][:3]
    host, dev = _scene(cuda, name)
    disps, wgt = host[1].copy(), host[4].copy()
    disps[0, 5, 7], disps[1, 6, 8], disps[2, 4, 9], disps[1, 3, 3] = 0.0, np.nan, np.inf, -0.5
    wgt[0, 6, 6], wgt[2, 7, 10], wgt[1, 2, 12] = 0.0, -1.0, np.nan
    got = _np(_fuse(cuda, name, [0, 1, 2], disps=torch.from_numpy(disps).to(cuda), weights=torch.from_numpy(wgt).to(cuda)))
    ref = _ref(name, [0, 1, 2], disps=disps, weights=wgt)
    ok, report = R.volume_matches(got[0], got[1], got[2], ref)
    assert ok, report
    assert all(np.isfinite(t).all() for t in got)
    clean = _full(cuda, name)[1]
    assert ref["hits"] < clean["hits"]                                                      # the planted pixels were in use


def test_w_max_caps_the_weight(cuda):
    name, cap = "5x24x32", 2.25
    got = _np(_fuse(cuda, name, [0, 1, 2, 3, 4], w_max=cap))
    ref = _ref(name, range(5), w_max=cap)
    ok, report = R.volume_matches(got[0], got[1], got[2], ref)
    assert ok, report
    assert got[1].max() == np.float32(cap) and (got[1] == np.float32(cap)).sum() > 1000 and _full(cuda, name)[0][1].max() > cap
    assert not np.array_equal(got[0], _full(cuda, name)[0][0])


def test_capture_and_replay_give_the_eager_bytes(cuda):
    from pvo_amd import droid_backends as db
    name = "5x24x32"
    nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
    eager = _fuse(cuda, name, [0, 1, 2, 3, 4])
    mesh_eager = _mesh_buffers(cuda, 4096, 8192)
    db.tsdf_mesh_into(eager[0], eager[1], eager[2], origin, voxel, 1.0, mesh_eager)         # (also sizes the cached workspace)
    torch.cuda.synchronize()
    vol = (torch.zeros(dims, device=cuda), torch.zeros(dims, device=cuda), torch.zeros(dims + (3,), device=cuda))
    mesh = _mesh_buffers(cuda, 4096, 8192)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    host, (poses, disps, intr, imgs, wgt) = _scene(cuda, name)
    ix = torch.arange(5, device=cuda)                                                       # (no host-to-device copy inside the capture)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            db.tsdf_integrate(vol[0], vol[1], vol[2], poses, disps, intr, ix, origin, voxel, trunc, weight=wgt, images=imgs,
                              img_stride=1, img_offset=0)
            db.tsdf_mesh_into(vol[0], vol[1], vol[2], origin, voxel, 1.0, mesh)
    torch.cuda.current_stream().wait_stream(side)
    assert not any(bool(t.any()) for t in vol)                                              # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert _bytes_equal(_np(vol), _np(eager))
    assert mesh["counts"].tolist() == mesh_eager["counts"].tolist() and mesh["counts"][0] > 0
    for k in mesh:
        assert torch.equal(mesh[k], mesh_eager[k]), k


# ------------------------------------------------------------------------------------------------ mesh
def _mesh_buffers(cuda, vcap, fcap, rows=None):
    """sentinel-filled output buffers with `rows` (default: the capacity) + 3 rows, viewed at their capacity"""
    fill = lambda n, nbytes, dt: torch.full((n + 3, nbytes), SENTINEL, dtype=torch.uint8, device=cuda).view(dt)
    return {"verts": fill(vcap, 12, torch.float32)[:vcap], "normals": fill(vcap, 12, torch.float32)[:vcap],
            "rgba": fill(vcap, 4, torch.uint8)[:vcap], "faces": fill(fcap, 12, torch.int32)[:fcap],
            "counts": torch.full((2,), -7, dtype=torch.int32, device=cuda)}


def _tail_untouched(t):
    """the three rows behind a buffer of _mesh_buffers still hold the sentinel"""
    base = t._base if t._base is not None else t
    return bool((base.view(torch.uint8).reshape(base.shape[0], -1)[t.shape[0]:] == SENTINEL).all())


@pytest.mark.parametrize("name", list(R.SCENES))
def test_mesh_of_the_kernels_own_volume(cuda, name):
    from pvo_amd import droid_backends as db
    nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
    got, _ = _full(cuda, name)
    vol = [torch.from_numpy(t).to(cuda) for t in got]
    ref = R.mesh_reference(got[0], got[1], got[2], origin, voxel, 1.0)
    V, F = len(ref["verts"]), len(ref["faces"])
    m = {k: v.cpu().numpy() for k, v in db.tsdf_mesh(vol[0], vol[1], vol[2], origin, voxel, min_weight=1.0).items()}
    print("%s: %d vertices, %d faces" % (name, V, F))
    assert V > 20 and F > 20
    assert m["counts"].tolist() == [V, F] and m["verts"].shape == (V, 3) and m["faces"].shape == (F, 3)
    assert np.array_equal(m["faces"], ref["faces"])
    ev = np.abs(m["verts"].astype(np.float64) - ref["verts"])
    en = np.abs(m["normals"].astype(np.float64) - ref["normals"]).max(1)
    print("   vertices: max error %.3e, max error / bound %.3f; normals: max error %.3e, max error / bound %.3f"
          % (ev.max(), (ev / ref["bound_v"]).max(), en.max(), (en / ref["bound_n"]).max()))
    assert np.all(ev <= ref["bound_v"]) and np.all(en <= ref["bound_n"])
    assert R.colours_match(m["rgba"][:, :3], ref) and np.all(m["rgba"][:, 3] == 255) and m["rgba"][:, :3].max() > 0
    # the default first guess is too small on none of these; an explicit one that is grows to the need and gives the same mesh
    again = db.tsdf_mesh(vol[0], vol[1], vol[2], origin, voxel, min_weight=1.0, vcap=5, fcap=7)
    for k in m:
        assert np.array_equal(again[k].cpu().numpy(), m[k]), k
    # a capacity one short of the need: nothing past it, the full counts, the elements in front unchanged
    short = _mesh_buffers(cuda, V - 1, F - 1)
    db.tsdf_mesh_into(vol[0], vol[1], vol[2], origin, voxel, 1.0, short)
    assert short["counts"].tolist() == [V, F]
    for k in ("verts", "normals", "rgba", "faces"):
        assert _tail_untouched(short[k]), k
        assert np.array_equal(short[k].cpu().numpy(), m[k][:short[k].shape[0]]), k
    # without a colour volume, normals or colours
    bare = _mesh_buffers(cuda, V, F)
    del bare["normals"]
    db.tsdf_mesh_into(vol[0], vol[1], None, origin, voxel, 1.0, bare)
    assert np.array_equal(bare["verts"].cpu().numpy(), m["verts"]) and np.array_equal(bare["faces"].cpu().numpy(), m["faces"])
    assert bare["rgba"][:, :3].max().item() == 0 and bare["rgba"][:, 3].min().item() == 255


def test_mesh_of_volumes_without_a_surface(cuda):
    from pvo_amd import droid_backends as db
    name = "3x12x16"
    nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
    got, _ = _full(cuda, name)
    vol = [torch.from_numpy(t).to(cuda) for t in got]
    for tsdf, wsum, mw in ((torch.zeros(dims, device=cuda), torch.zeros(dims, device=cuda), 1.0),        # all invalid
                           (vol[0], vol[1], float(got[1].max()) + 1.0),                                   # min_weight above every wsum
                           (torch.ones(dims, device=cuda), torch.ones(dims, device=cuda), 1.0),           # all outside
                           (vol[0][:, :1].contiguous(), vol[1][:, :1].contiguous(), 1.0)):                # a dimension without a cell
        out = _mesh_buffers(cuda, 16, 16)
        db.tsdf_mesh_into(tsdf, wsum, None, origin, voxel, mw, out)
        assert out["counts"].tolist() == [0, 0]
        assert bool((out["verts"].view(torch.uint8) == SENTINEL).all()) and bool((out["faces"].view(torch.uint8) == SENTINEL).all())
        m = db.tsdf_mesh(tsdf, wsum, None, origin, voxel, min_weight=mw)
        assert m["verts"].shape == (0, 3) and m["faces"].shape == (0, 3)


# ------------------------------------------------------------------------------------------------ system
_system = {}


def test_mesh_with_more_workgroups_than_scan_threads(cuda):
    """[66,66,66]: 65^3 = 274 625 cells in 1073 workgroups, so every thread of the one-workgroup scan owns MORE than one count (the
    fused scenes stop at 95 workgroups).  The volume is an analytic sphere, not a fusion: counts, the active cells in raster order
    and the faces equal the reference's, vertices and normals lie within its bounds."""
    from pvo_amd import droid_backends as db
    dims, origin, voxel = (66, 66, 66), (-1.0, -0.5, 0.25), 0.05
    tsdf = R.sphere_volume(dims, (32.3, 31.6, 33.7), 18.4, 3.0, cuda)
    wsum = torch.ones_like(tsdf)
    lib_blocks = -(-65 ** 3 // 256)
    assert lib_blocks == 1073 and lib_blocks > 1024
    host = tsdf.cpu().numpy()
    assert not (host == 0).any()                                        # (no corner sits on the surface: inside / outside is unambiguous)
    ref = R.mesh_reference(host, wsum.cpu().numpy(), None, origin, voxel, 1.0)
    V, F = len(ref["verts"]), len(ref["faces"])
    m = {k: v.cpu().numpy() for k, v in db.tsdf_mesh(tsdf, wsum, None, origin, voxel, min_weight=1.0).items()}
    print("sphere in %s: %d vertices, %d faces" % (list(dims), V, F))
    assert V > 20 and F > 20
    assert m["counts"].tolist() == [V, F] and m["verts"].shape == (V, 3) and m["faces"].shape == (F, 3)
    assert np.array_equal(m["faces"], ref["faces"])
    # vertex i within the bound (some 1e-6) of the vertex of the reference's i-th active cell, whose neighbours are a voxel (0.05)
    # away: the set of active cells and their raster order
    ev = np.abs(m["verts"].astype(np.float64) - ref["verts"])
    en = np.abs(m["normals"].astype(np.float64) - ref["normals"]).max(1)
    print("   vertices: max error %.3e, max error / bound %.3f; normals: max error / bound %.3f"
          % (ev.max(), (ev / ref["bound_v"]).max(), (en / ref["bound_n"]).max()))
    assert np.all(ev <= ref["bound_v"]) and np.all(en <= ref["bound_n"])
    # the active cells spread over many workgroups, with empty ones between them
    groups = np.unique(((ref["cells"][:, 0] * 65 + ref["cells"][:, 1]) * 65 + ref["cells"][:, 2]) // 256)
    assert 100 < len(groups) < lib_blocks


def _droid(cuda):
    """a Droid whose video holds the analytic scene at 1/8 of 192 x 256 images: five keyframes, random colours"""
    if "droid" not in _system:
        from pvo_amd.droid import Droid, default_args
        nf, ht, wd, dims, origin, voxel, trunc = R.SCENES["5x24x32"]
        host, (poses, disps, intr, _, _) = _scene(cuda, "5x24x32")
        droid = Droid(default_args(device=str(cuda), image_size=[ht * 8, wd * 8], buffer=8, store_images=True))
        v = droid.video
        v.poses[:nf], v.disps[:nf], v.intrinsics[:nf] = poses, disps, intr
        g = torch.Generator().manual_seed(7)
        v.images[:nf] = torch.randint(0, 256, (nf, 3, ht * 8, wd * 8), generator=g).to(torch.uint8).to(cuda)
        v.counter = nf
        _system["droid"] = droid
    return _system["droid"]


KW = dict(voxel=0.05, trunc=0.15, thresh=0.1, origin=R.SCENES["5x24x32"][4], dims=R.SCENES["5x24x32"][3])


def _sphere_vertices(verts):
    return int((np.abs(np.linalg.norm(verts.cpu().numpy().astype(np.float64) - R.SPHERE_C, axis=1) - R.SPHERE_R) < 0.1).sum())


def test_video_tsdf_is_the_composed_native_calls(cuda):
    from pvo_amd import droid_backends as db
    from pvo_amd.depth_video import DepthVideo
    droid = _droid(cuda)
    v, n = droid.video, droid.video.counter
    out = droid.get_mesh(**KW)
    assert set(out) == {"verts", "normals", "rgba", "faces", "tsdf", "wsum", "origin", "voxel"}
    ix = torch.arange(n, device=cuda)
    m = db.map_points(v.poses, v.disps, v.intrinsics[0].contiguous(), ix, torch.full((n,), KW["thresh"], device=cuda), images=v.images,
                      labels=v.segms)
    assert m["src"].shape[0] > 0.5 * n * 24 * 32                                            # most pixels are confirmed and fused
    keep = torch.zeros(n, 24 * 32, dtype=torch.bool, device=cuda)
    keep[m["src"][:, 0].long(), m["src"][:, 1].long()] = True
    w = DepthVideo.fusion_weights(keep.view(n, 24, 32), v.disps[:n])
    dims = KW["dims"]
    vol, wsum, rgb = torch.zeros(dims, device=cuda), torch.zeros(dims, device=cuda), torch.zeros(dims + (3,), device=cuda)
    db.tsdf_integrate(vol, wsum, rgb, v.poses[:n], v.disps[:n].contiguous(), v.intrinsics[0].contiguous(), ix, KW["origin"], KW["voxel"],
                      KW["trunc"], weight=w, images=v.images, img_stride=8, img_offset=3)
    want = db.tsdf_mesh(vol, wsum, rgb, KW["origin"], KW["voxel"], min_weight=1.0)
    assert torch.equal(out["tsdf"], vol) and torch.equal(out["wsum"], wsum)
    for k in ("verts", "normals", "rgba", "faces"):
        assert torch.equal(out[k], want[k]), k
    assert out["verts"].shape[0] > 500 and out["faces"].shape[0] > 500 and out["voxel"] == 0.05
    same = v.tsdf(**KW)
    assert all(torch.equal(same[k], out[k]) for k in ("verts", "faces", "tsdf", "wsum"))
    # the mesh is the scene's surface, within twice the distance measured on the reference mesh (tests/test_tsdf_host.py)
    dist = R.surface_distance(out["verts"].cpu().numpy())
    print("system mesh: %d vertices, %d faces, max distance %.4f" % (out["verts"].shape[0], out["faces"].shape[0], dist.max()))
    assert dist.max() <= 2.0 * 0.0407 and _sphere_vertices(out["verts"]) > 50
    # default bounds: from the map's points
    auto = v.tsdf(voxel=0.05, thresh=0.1)
    o, d = DepthVideo.tsdf_bounds(m["xyz"], 0.05, 0.15)
    assert auto["origin"] == o and tuple(auto["tsdf"].shape) == d and auto["verts"].shape[0] > 500


def test_reject_removes_the_sphere(cuda):
    droid = _droid(cuda)
    v, n = droid.video, droid.video.counter
    hit = _scene(cuda, "5x24x32")[0][5]
    rej = torch.zeros(v.segms.shape[0], 24, 32, dtype=torch.bool, device=cuda)
    rej[:n] = torch.from_numpy(hit).to(cuda)
    assert _sphere_vertices(droid.get_mesh(**KW)["verts"]) > 50
    out = droid.get_mesh(reject=rej, **KW)
    assert out["verts"].shape[0] > 300 and _sphere_vertices(out["verts"]) == 0


def test_sigma_weights_move_the_surface_toward_the_confident_frames(cuda):
    """frame 2's depths are 1.5 % too large.  With a large sigma on that frame - a relative standard deviation of 0.5 against
    rel0 = 0.05: a weight w <= 1 / 101 - the fused volume moves to the one fused from the OTHER frames alone (same votes, so the same
    pixels): where those gave a weight W >= 1, one more observation moves the mean by w |val - T| / (W + w) <= 2 w / (1 + w) < 0.0197,
    and by at most (k + 1) / (101 k + 1) <= 0.02 of what it moves the unweighted mean of k + 1 frames"""
    droid = _droid(cuda)
    v, n = droid.video, droid.video.counter
    true2 = v.disps[2].clone()
    try:
        v.disps[2] = true2 / 1.015
        vc, vp, _ = v.ensure_uncertainty()
        vc[:n], vp[:n] = (1e-3 * v.disps[:n]) ** 2, 0.0
        vc[2] = (0.5 * v.disps[2]) ** 2
        others = v.tsdf(ix=[0, 1, 3, 4], **KW)
        plain, weighted = v.tsdf(**KW), v.tsdf(use_sigma=True, **KW)
    finally:
        v.disps[2] = true2
        v.disps_var_cond = v.disps_var_pose = v.poses_cov = None
    sel = others["wsum"] >= 1
    d_plain = (plain["tsdf"] - others["tsdf"])[sel].abs()
    d_weighted = (weighted["tsdf"] - others["tsdf"])[sel].abs()
    print("|tsdf - the other frames'| over %d voxels: unweighted mean %.5f max %.3f, sigma-weighted mean %.6f max %.5f"
          % (int(sel.sum()), d_plain.mean(), d_plain.max(), d_weighted.mean(), d_weighted.max()))
    assert int(sel.sum()) > 5000 and d_plain.mean().item() > 1e-3
    assert d_weighted.max().item() < 0.0197 and d_weighted.mean().item() <= 0.02 * d_plain.mean().item()
    assert weighted["wsum"].max() < plain["wsum"].max()
