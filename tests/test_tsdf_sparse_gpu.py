"""The brick volume on the device (pvo_amd/csrc/tsdf_sparse.hip): allocation against the fp64 marking rule's must / may sets
(tests/tsdf_sparse_reference.py), integration against the dense kernel - every voxel of every brick must hold the BYTES
pvo_tsdf_integrate leaves at that voxel of the [8gz,8gy,8gx] volume - and, independently, against tsdf_reference.integrate_reference;
the mesh against pvo_tsdf_mesh of the densified volume (equal counts, vertices equal bytes matched by cell, faces equal after mapping);
capture and replay; DepthVideo.tsdf(sparse=True) and the export tool."""
import numpy as np
import pytest
import torch

import tsdf_reference as R
import tsdf_sparse_reference as SR

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
_scenes, _cache = {}, {}


def _scene(cuda, name):
    """(host arrays, device tensors (poses, disps, intr, images, weight), ix list) of a scene of tsdf_sparse_reference"""
    if name not in _scenes:
        host, ix = SR.scene(name)
        _scenes[name] = (host, [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in host[:5]], ix)
    return _scenes[name]


def _ix(cuda, ix):
    return torch.tensor(ix, dtype=torch.long, device=cuda)


def _volume(cuda, name, colours=True, cap=64):
    from pvo_amd.tsdf_sparse import SparseTSDF
    nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES[name]
    return SparseTSDF(origin, gdims, voxel, trunc, colours=colours, device=cuda, cap=cap)


def _allocate(cuda, name, vol, ix=None, weight=True, z_near=0.0, margin=2.0):
    """one native allocate call (no growth); returns counts[0]"""
    from pvo_amd import droid_backends as db
    host, (poses, disps, intr, imgs, wgt), all_ix = _scene(cuda, name)
    db.tsdf_sparse_allocate(vol.volume(), poses, disps, intr, _ix(cuda, all_ix if ix is None else ix), vol.trunc,
                            weight=wgt if weight else None, z_near=z_near, margin=margin)
    return int(vol.counts[0])


def _fill(vol):
    """every brick of the grid allocated by hand, in raster order: the integration then also meets bricks no frame sees"""
    gz, gy, gx = vol.grid.shape
    n = gz * gy * gx
    if vol.cap < n:
        vol._resize(n)
    vol.grid.copy_(torch.arange(n, dtype=torch.int32, device=vol.device).view(gz, gy, gx))
    vol.coord[:n] = torch.from_numpy(np.argwhere(np.ones((gz, gy, gx), bool)).astype(np.int32)).to(vol.device)
    vol.counts[0] = n
    return vol


def _integrate(cuda, name, vol, ix=None, weight=True, w_max=0.0, z_near=0.0):
    host, (poses, disps, intr, imgs, wgt), all_ix = _scene(cuda, name)
    vol.integrate(poses, disps, intr, _ix(cuda, all_ix if ix is None else ix), weight=wgt if weight else None, images=imgs, img_stride=1,
                  img_offset=0, w_max=w_max, z_near=z_near)
    return vol


def _dense(cuda, name, ix=None, weight=True, colours=True, w_max=0.0, z_near=0.0):
    """pvo_tsdf_integrate into the zeroed [8gz,8gy,8gx] volume: the yardstick; numpy (tsdf, wsum, rgb or None)"""
    from pvo_amd import droid_backends as db
    nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES[name]
    host, (poses, disps, intr, imgs, wgt), all_ix = _scene(cuda, name)
    dims = tuple(8 * g for g in gdims)
    vol = (torch.zeros(dims, device=cuda), torch.zeros(dims, device=cuda), torch.zeros(dims + (3,), device=cuda) if colours else None)
    db.tsdf_integrate(vol[0], vol[1], vol[2], poses, disps, intr, _ix(cuda, all_ix if ix is None else ix), origin, voxel, trunc,
                      weight=wgt if weight else None, images=imgs if colours else None, img_stride=1, img_offset=0, w_max=w_max,
                      z_near=z_near)
    return [None if t is None else t.cpu().numpy() for t in vol]


def _pool(vol):
    """the bricks in use as numpy: (tsdf, wsum, rgb or None), coord"""
    n = vol.bricks
    return [None if t is None else t[:n].cpu().numpy() for t in (vol.tsdf, vol.wsum, vol.rgb)], vol.coord[:n].cpu().numpy()


def _bricks_equal(pool, coord, dense):
    """every voxel of every brick holds the bytes of the dense volume"""
    return all((p is None and d is None) or np.array_equal(p.view(np.uint32), SR.to_bricks(d, coord).view(np.uint32))
               for p, d in zip(pool, dense))


def _marks(name, **kw):
    key = (name,) + tuple(sorted(kw.items()))
    if key not in _cache:
        nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES[name]
        host, ix = SR.scene(name)
        kw.setdefault("weight", host[4])
        _cache[key] = SR.mark_reference(gdims, origin, voxel, trunc, host[0], host[1], host[2], ix, **kw)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ allocation
@pytest.mark.parametrize("name", list(SR.SCENES))
def test_allocation_marks_what_the_rule_says_in_raster_order(cuda, name):
    must, may = _marks(name, margin=2.0)
    vol = _volume(cuda, name)
    want = _allocate(cuda, name, vol)
    grid, coord = vol.grid.cpu().numpy(), vol.coord.cpu().numpy()
    got = grid >= 0
    print("%s: %d bricks allocated of %d; must %d, may %d" % (name, got.sum(), got.size, must.sum(), may.sum()))
    assert not (must & ~got).any() and not (got & ~may).any()
    assert want == got.sum() == vol.bricks and want <= vol.cap
    ref_grid, ref_coord = SR.assign_slots(got)                                                # raster order, grid and coord consistent
    assert np.array_equal(grid, ref_grid) and np.array_equal(coord[:want], ref_coord)
    # a second identical call allocates nothing; a fresh run gives the same bytes
    assert _allocate(cuda, name, vol) == want
    assert np.array_equal(vol.grid.cpu().numpy(), grid) and np.array_equal(vol.coord.cpu().numpy(), coord)
    again = _volume(cuda, name)
    assert _allocate(cuda, name, again) == want
    assert torch.equal(again.grid, vol.grid) and torch.equal(again.coord, vol.coord)
    # the frame that looks away and the ids out of range mark nothing
    nf = SR.SCENES[name][0]
    none = _volume(cuda, name)
    assert _allocate(cuda, name, none, ix=[nf, -1, nf + 1, 1 << 40]) == 0 and bool((none.grid == -1).all())


@pytest.mark.parametrize("kw", [dict(margin=0.0), dict(margin=8.0), dict(z_near=1.1), dict(weight=None)], ids=str)
def test_allocation_follows_margin_z_near_and_weights(cuda, kw):
    name = "5x24x32"
    must, may = _marks(name, **kw)
    vol = _volume(cuda, name)
    run = dict(kw)
    if "weight" in run:
        run["weight"] = False
    _allocate(cuda, name, vol, **run)
    got = (vol.grid >= 0).cpu().numpy()
    print(kw, "%d allocated, must %d, may %d" % (got.sum(), must.sum(), may.sum()))
    assert not (must & ~got).any() and not (got & ~may).any() and must.any()


def test_allocation_skips_invalid_pixels(cuda):
    from pvo_amd import droid_backends as db
    name = "3x12x16"
    nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES[name]
    host, (poses, disps, intr, imgs, wgt), ix = _scene(cuda, name)
    d, w = host[1].copy(), host[4].copy()
    d[0], d[1, :6], w[1, 6:], d[2, :, :8], w[2, :, 8:] = np.nan, np.inf, 0.0, -1.0, np.nan     # nothing valid is left
    vol = _volume(cuda, name)
    db.tsdf_sparse_allocate(vol.volume(), poses, torch.from_numpy(d).to(cuda), intr, _ix(cuda, ix), vol.trunc,
                            weight=torch.from_numpy(w).to(cuda))
    assert int(vol.counts[0]) == 0 and bool((vol.grid == -1).all())


def test_overflow_keeps_the_first_bricks_and_a_second_call_finishes(cuda):
    name = "5x24x32"
    one = _volume(cuda, name)
    want = _allocate(cuda, name, one)
    grid, coord = one.grid.cpu().numpy(), one.coord[:want].cpu().numpy()
    cap = 7
    assert want > 2 * cap
    small = _volume(cuda, name, cap=cap)
    small.tsdf[:] = 3.0
    assert _allocate(cuda, name, small) == want                                               # unclamped
    assert small.bricks == cap
    g = small.grid.cpu().numpy()
    assert np.array_equal(g >= 0, (grid >= 0) & (grid < cap)) and np.array_equal(g[g >= 0], grid[g >= 0])
    assert np.array_equal(small.coord.cpu().numpy(), coord[:cap])
    assert _allocate(cuda, name, small) == want and np.array_equal(small.grid.cpu().numpy(), g)   # again, still too small: the same
    small._resize(want + 3)                                                                   # the old pool copied into a larger one
    assert _allocate(cuda, name, small) == want
    assert np.array_equal(small.grid.cpu().numpy(), grid) and np.array_equal(small.coord[:want].cpu().numpy(), coord)
    assert bool((small.tsdf[:cap] == 3.0).all()) and not bool(small.tsdf[cap:].any())
    # SparseTSDF.allocate does the same on its own: one read, the pool doubled, one more call
    host, (poses, disps, intr, imgs, wgt), ix = _scene(cuda, name)
    auto = _volume(cuda, name, cap=cap)
    assert auto.allocate(poses, disps, intr, _ix(cuda, ix), weight=wgt) == want
    assert auto.cap >= want and auto.cap % cap == 0 and np.array_equal(auto.grid.cpu().numpy(), grid)
    assert np.array_equal(auto.coord[:want].cpu().numpy(), coord)


# ------------------------------------------------------------------------------------------------ integration
VARIANTS = {"colours+weight": dict(), "plain": dict(weight=False, colours=False), "w_max": dict(w_max=2.25),
            "z_near": dict(z_near=None)}          # (None: the scene's Z_NEAR)


@pytest.mark.parametrize("fill", [False, True], ids=["allocated", "every-brick"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SR.SCENES))
def test_bricks_hold_the_dense_kernels_bytes(cuda, name, variant, fill):
    kw = dict(VARIANTS[variant])
    if "z_near" in kw:
        kw["z_near"] = SR.Z_NEAR[name]
    colours = kw.pop("colours", True)
    vol = _volume(cuda, name, colours=colours)
    if fill:
        _fill(vol)
    else:
        _allocate(cuda, name, vol, weight=kw.get("weight", True))
    _integrate(cuda, name, vol, **kw)
    pool, coord = _pool(vol)
    dense = _dense(cuda, name, colours=colours, **kw)
    touched = SR.to_bricks(dense[1], coord) > 0
    print("%s %s: %d bricks, %d of their voxels touched, %d of the dense volume's" % (name, variant, len(coord), touched.sum(), (dense[1] > 0).sum()))
    assert touched.sum() > 100
    assert _bricks_equal(pool, coord, dense)
    if variant == "w_max":
        assert pool[1].max() == np.float32(2.25)
    if fill:                                                                                  # every voxel of the world: the dense volume itself
        assert all(p is None or np.array_equal(SR.to_dense(p, coord, SR.SCENES[name][3]), d) for p, d in zip(pool, dense))


def test_more_slots_than_one_cull_chunk(cuda):
    """N = 6 * 90 + 3 = 543 > 512 slots: the second chunk holds contributing frames, the frame that looks away and ids out of range"""
    name = "3x12x16"
    host, dev, ix = _scene(cuda, name)
    long_ix = ix * 90 + [2, 0, 1]
    assert 512 < len(long_ix) < 1024
    vol = _volume(cuda, name)
    _allocate(cuda, name, vol)
    _integrate(cuda, name, vol, ix=long_ix, w_max=40.0)
    pool, coord = _pool(vol)
    dense = _dense(cuda, name, ix=long_ix, w_max=40.0)
    assert dense[1].max() == np.float32(40.0)                                                 # (the frames of the second chunk counted)
    assert _bricks_equal(pool, coord, dense)


def test_the_cull_removes_pairs_and_keeps_every_contributing_one(cuda):
    """kept[brick] counts the survivors.  A world wider than any frustum (the 5 x 24 x 32 scene's voxel, 3 x 3 x 9 bricks starting 1.2 m
    further left) with EVERY brick allocated by hand and z_near inside the second layer: the first layer of bricks lies behind z_near
    for every frame, the leftmost columns outside every frustum.  The survivors never include the frame that looks away or an id out
    of range, they include every frame that the dense kernel's per-frame volumes show to reach the brick, whole bricks lose every
    frame - and the bricks still hold the dense kernel's bytes."""
    from pvo_amd import droid_backends as db
    from pvo_amd.tsdf_sparse import SparseTSDF
    name = "5x24x32"
    nf, ht, wd, _, _, voxel, trunc = SR.SCENES[name]
    gdims, origin, z_near = (3, 3, 9), (-2.213, -0.617, 0.953), 1.7
    host, (poses, disps, intr, imgs, wgt), ix = _scene(cuda, name)
    vol = _fill(SparseTSDF(origin, gdims, voxel, trunc, colours=True, device=cuda, cap=81))
    n = vol.bricks
    kept = torch.full((vol.cap + 2,), -1, dtype=torch.int32, device=cuda)
    vol.integrate(poses, disps, intr, _ix(cuda, ix), weight=wgt, images=imgs, img_stride=1, img_offset=0, z_near=z_near, kept=kept)
    k = kept.cpu().numpy()
    pool, coord = _pool(vol)
    dims = tuple(8 * g for g in gdims)

    def dense(frames):
        d = (torch.zeros(dims, device=cuda), torch.zeros(dims, device=cuda), torch.zeros(dims + (3,), device=cuda))
        db.tsdf_integrate(d[0], d[1], d[2], poses, disps, intr, _ix(cuda, frames), origin, voxel, trunc, weight=wgt, images=imgs,
                          img_stride=1, img_offset=0, z_near=z_near)
        return [t.cpu().numpy() for t in d]

    assert _bricks_equal(pool, coord, dense(ix))
    reach = np.zeros(n, int)
    for f in range(nf):
        reach += (SR.to_bricks(dense([f])[1], coord).reshape(n, -1) > 0).any(1)
    print("survivors per brick: min %d max %d, %d of %d pairs; contributing pairs %d" % (k[:n].min(), k[:n].max(), k[:n].sum(), n * len(ix), reach.sum()))
    assert (k[n:] == -1).all() and (k[:n] >= reach).all() and k[:n].max() == nf               # (never the frame that looks away)
    assert (k[:n][coord[:, 0] == 0] == 0).all()                                               # behind z_near: zc <= 1.303 + 0.15 (the yaw over 2.5 m) + 6.07 voxels < 1.7
    assert (k[:n][coord[:, 2] == 0] == 0).all()                                               # x <= -1.86: left of every frustum
    assert 0 < reach.sum() and k[:n].sum() < n * nf


def test_split_calls_leave_the_bytes_of_one_call(cuda):
    name = "5x24x32"
    one = _volume(cuda, name)
    _allocate(cuda, name, one)
    _integrate(cuda, name, one, ix=[0, 1, 2, 3, 4])
    two = _volume(cuda, name)
    _allocate(cuda, name, two)
    _integrate(cuda, name, _integrate(cuda, name, two, ix=[0, 1, 2]), ix=[3, 4])
    for a, b in zip(_pool(one)[0], _pool(two)[0]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    again = _volume(cuda, name)                                                               # and a second run: identical bytes
    _allocate(cuda, name, again)
    _integrate(cuda, name, again, ix=[0, 1, 2, 3, 4])
    assert all(torch.equal(a, b) for a, b in ((one.tsdf, again.tsdf), (one.wsum, again.wsum), (one.rgb, again.rgb)))


def test_a_cull_that_drops_a_contributing_frame_fails_the_comparison(cuda):
    """the comparison of test_bricks_hold_the_dense_kernels_bytes against a yardstick in which ONE brick misses ONE frame that
    reaches it - what a cull that wrongly drops the pair would leave"""
    name = "5x24x32"
    vol = _volume(cuda, name)
    _allocate(cuda, name, vol)
    _integrate(cuda, name, vol, ix=[0, 1, 2, 3, 4])
    pool, coord = _pool(vol)
    full, without = _dense(cuda, name, ix=[0, 1, 2, 3, 4]), _dense(cuda, name, ix=[0, 1, 2, 4])
    assert _bricks_equal(pool, coord, full)
    differs = (SR.to_bricks(full[1], coord) != SR.to_bricks(without[1], coord)).reshape(len(coord), -1).sum(1)
    k = int(np.argmin(np.where(differs > 0, differs, 1 << 30)))                               # the brick frame 3 reaches least
    assert differs[k] > 0
    print("brick %d at %s: frame 3 contributes to %d of its voxels" % (k, coord[k], differs[k]))
    bz, by, bx = coord[k]
    mixed = [a.copy() for a in full]
    for m, w in zip(mixed, without):
        m[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = w[8 * bz:8 * bz + 8, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
    assert not _bricks_equal(pool, coord, mixed)


@pytest.mark.parametrize("name", list(SR.SCENES))
def test_bricks_match_the_fp64_reference(cuda, name):
    """independently of the dense kernel: tsdf_reference.volume_matches on the allocated bricks' voxels"""
    nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES[name]
    host, dev, ix = _scene(cuda, name)
    vol = _volume(cuda, name)
    _allocate(cuda, name, vol)
    _integrate(cuda, name, vol)
    pool, coord = _pool(vol)
    ref = R.integrate_reference(tuple(8 * g for g in gdims), origin, voxel, trunc, host[0], host[1], host[2], ix, weight=host[4],
                                images=host[3], img_stride=1, img_offset=0)
    part = {k: (SR.to_bricks(v, coord) if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
    ok, report = R.volume_matches(pool[0], pool[1], pool[2], part)
    print("%s: %d voxels in bricks, %d touched, %d flagged; %s" % (name, part["touched"].size, part["touched"].sum(), part["flagged"].sum(), report))
    assert part["flagged"].sum() <= 0.01 * part["touched"].sum()
    assert ok, report


# ------------------------------------------------------------------------------------------------ mesh
def _mesh_buffers(cuda, vcap, fcap):
    """sentinel-filled output buffers with three rows more than the capacity, viewed at their capacity"""
    fill = lambda n, nbytes, dt: torch.full((n + 3, nbytes), SENTINEL, dtype=torch.uint8, device=cuda).view(dt)
    return {"verts": fill(vcap, 12, torch.float32)[:vcap], "normals": fill(vcap, 12, torch.float32)[:vcap],
            "rgba": fill(vcap, 4, torch.uint8)[:vcap], "faces": fill(fcap, 12, torch.int32)[:fcap],
            "counts": torch.full((2,), -7, dtype=torch.int32, device=cuda)}


def _tail_untouched(t):
    base = t._base if t._base is not None else t
    return bool((base.view(torch.uint8).reshape(base.shape[0], -1)[t.shape[0]:] == SENTINEL).all())


def _cells(tsdf, wsum, min_weight=1.0):
    """(active cells [V,3] = (cz,cy,cx) in raster order, cell_valid bool) of a dense volume under pvo_tsdf_mesh's rules"""
    nz, ny, nx = tsdf.shape
    corner = lambda a, j: a[(j >> 2):nz - 1 + (j >> 2), ((j >> 1) & 1):ny - 1 + ((j >> 1) & 1), (j & 1):nx - 1 + (j & 1)]
    valid = np.all([corner(wsum >= np.float32(min_weight), j) for j in range(8)], 0)
    n_in = np.sum([corner(tsdf < 0, j) for j in range(8)], 0)
    return np.argwhere(valid & (n_in > 0) & (n_in < 8)), valid


def _sparse_order(cells, grid):
    """the permutation that puts dense vertices (raster order of cells) into the sparse order (slot, raster inside the brick)"""
    slot = grid[cells[:, 0] >> 3, cells[:, 1] >> 3, cells[:, 2] >> 3].astype(np.int64)
    assert (slot >= 0).all()
    local = ((cells[:, 0] & 7) << 6) | ((cells[:, 1] & 7) << 3) | (cells[:, 2] & 7)
    return np.argsort(slot * 512 + local, kind="stable")


def _meshed(cuda, name, weight=True):
    key = ("mesh", name, weight)
    if key not in _cache:
        vol = _volume(cuda, name)
        _allocate(cuda, name, vol, weight=weight)
        _integrate(cuda, name, vol, weight=weight)
        _cache[key] = vol
    return _cache[key]


def _assert_the_dense_mesh_in_sparse_order(name, vol, d, dense, sparse):
    """sparse = the dense mesh of the densified volume d under the permutation _sparse_order, byte for byte; returns (V, F)"""
    V, F = dense["counts"].tolist()
    print("%s: %d vertices, %d faces" % (name, V, F))
    assert V > 20 and F > 20 and sparse["counts"].tolist() == [V, F]
    cells, _ = _cells(d["tsdf"].cpu().numpy(), d["wsum"].cpu().numpy())
    assert len(cells) == V
    perm = _sparse_order(cells, vol.grid.cpu().numpy())                                       # sparse vertex i is dense vertex perm[i]
    assert not np.array_equal(perm, np.arange(V))                                             # (the orders do differ)
    for k in ("verts", "normals"):
        assert np.array_equal(sparse[k].view(np.uint32), dense[k][perm].view(np.uint32)), k
    assert np.array_equal(sparse["rgba"], dense["rgba"][perm]) and sparse["rgba"][:, :3].max() > 0
    inv = np.empty(V, np.int64)
    inv[perm] = np.arange(V)
    mapped = inv[dense["faces"]]                                                              # the dense faces in sparse vertex numbers
    assert sorted(map(tuple, mapped)) == sorted(map(tuple, sparse["faces"]))
    # faces: by the owning cell (a face's first vertex) in sparse order, then axis - the dense order is (cell, axis) as well
    assert np.array_equal(sparse["faces"], mapped[np.argsort(mapped[:, 0], kind="stable")])
    return V, F


@pytest.mark.parametrize("name", list(SR.SCENES))
def test_mesh_equals_the_dense_mesh_of_the_densified_volume(cuda, name):
    from pvo_amd import droid_backends as db
    vol = _meshed(cuda, name)
    d = vol.to_dense()
    dense = {k: v.cpu().numpy() for k, v in db.tsdf_mesh(d["tsdf"], d["wsum"], d["rgb"], vol.origin, vol.voxel, min_weight=1.0).items()}
    sparse = {k: v.cpu().numpy() for k, v in vol.mesh(min_weight=1.0).items()}
    V, F = _assert_the_dense_mesh_in_sparse_order(name, vol, d, dense, sparse)
    # the capacity protocol: one short of the need - full counts, nothing behind the capacity, the front unchanged
    short = _mesh_buffers(cuda, V - 1, F - 1)
    db.tsdf_sparse_mesh_into(vol.volume(), 1.0, short)
    assert short["counts"].tolist() == [V, F]
    for k in ("verts", "normals", "rgba", "faces"):
        assert _tail_untouched(short[k]), k
        assert np.array_equal(short[k].cpu().numpy(), sparse[k][:short[k].shape[0]]), k
    again = vol.mesh(min_weight=1.0, vcap=5, fcap=7)                                          # grows to the need: the same mesh
    for k in sparse:
        assert np.array_equal(again[k].cpu().numpy(), sparse[k]), k
    # no surface: min_weight above every wsum; and an empty pool
    none = _mesh_buffers(cuda, 16, 16)
    db.tsdf_sparse_mesh_into(vol.volume(), float(vol.wsum.max()) + 1.0, none)
    assert none["counts"].tolist() == [0, 0] and bool((none["verts"].view(torch.uint8) == SENTINEL).all())
    empty = _volume(cuda, name)
    assert empty.mesh()["counts"].tolist() == [0, 0]


def test_mesh_with_more_bricks_than_scan_threads(cuda):
    """a world of 11 x 10 x 10 bricks, every one allocated: 1100 slots, so every thread of the one-workgroup scan owns MORE than one
    count (the fused scenes hold a few dozen bricks).  The pool holds an analytic sphere (tests/tsdf_reference.sphere_volume) with
    wsum = 1 and a colour ramp; the mesh equals the dense mesh of the densified volume as in the test above."""
    from pvo_amd import droid_backends as db
    from pvo_amd.tsdf_sparse import SparseTSDF
    gdims = (11, 10, 10)
    gz, gy, gx = gdims
    vol = _fill(SparseTSDF((-1.0, -0.5, 0.25), gdims, 0.05, 0.15, colours=True, device=cuda, cap=1100))
    assert vol.bricks == 1100 and vol.cap >= 1100 > 1024
    dims = (8 * gz, 8 * gy, 8 * gx)
    field = R.sphere_volume(dims, (40.3, 39.6, 43.7), 30.4, 3.0, cuda)
    assert not bool((field == 0).any())
    z, y, x = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device=cuda) for n in dims], indexing="ij")
    ramp = torch.stack([(3 * x) % 256, (5 * y) % 256, (7 * z) % 256], -1)
    to_pool = lambda t: t.view((gz, 8, gy, 8, gx, 8) + tuple(t.shape[3:])).permute(*((0, 2, 4, 1, 3, 5) + tuple(range(6, 3 + t.dim())))) \
        .reshape((gz * gy * gx, 8, 8, 8) + tuple(t.shape[3:]))          # (_fill: slot = raster index of the brick)
    vol.tsdf[:1100] = to_pool(field)
    vol.wsum[:1100] = 1.0
    vol.rgb[:1100] = to_pool(ramp)
    d = vol.to_dense()
    assert torch.equal(d["tsdf"], field) and torch.equal(d["rgb"], ramp)
    dense = {k: v.cpu().numpy() for k, v in db.tsdf_mesh(d["tsdf"], d["wsum"], d["rgb"], vol.origin, vol.voxel, min_weight=1.0).items()}
    sparse = {k: v.cpu().numpy() for k, v in vol.mesh(min_weight=1.0).items()}
    _assert_the_dense_mesh_in_sparse_order("sphere in 11x10x10 bricks", vol, d, dense, sparse)


def test_mesh_is_closed_inside_allocated_space_and_lies_on_the_surface(cuda):
    """unit weights, min_weight 1 - how tests/test_tsdf_host.py measured 0.0407 for this voxel size; asserted with its margin of two"""
    name = "5x24x32"
    vol = _meshed(cuda, name, weight=False)
    d = vol.to_dense()
    m = {k: v.cpu().numpy() for k, v in vol.mesh(min_weight=1.0).items()}
    cells, cell_valid = _cells(d["tsdf"].cpu().numpy(), d["wsum"].cpu().numpy())
    perm = _sparse_order(cells, vol.grid.cpu().numpy())
    inner = R.interior_vertices({"cells": cells[perm], "cell_valid": cell_valid})
    shares = R.edge_shares(m["faces"])
    inner_edges = [n for (a, b), n in shares.items() if inner[a] and inner[b]]
    dist = R.surface_distance(m["verts"])
    print("%d vertices, %d edges, %d interior; distance max %.4f" % (len(m["verts"]), len(shares), len(inner_edges), dist.max()))
    assert len(inner_edges) > 100 and max(shares.values()) <= 2 and all(n == 2 for n in inner_edges)
    assert dist.max() <= 2.0 * 0.0407
    assert (np.abs(np.linalg.norm(m["verts"] - R.SPHERE_C, axis=1) - R.SPHERE_R) < 0.1).sum() > 50


# ------------------------------------------------------------------------------------------------ capture
def test_capture_and_replay_give_the_eager_bytes(cuda):
    from pvo_amd import droid_backends as db
    name = "5x24x32"
    host, (poses, disps, intr, imgs, wgt), ix = _scene(cuda, name)
    ixd = _ix(cuda, ix)                                                                       # (no host-to-device copy inside the capture)

    def run(vol, mesh):
        db.tsdf_sparse_allocate(vol.volume(), poses, disps, intr, ixd, vol.trunc, weight=wgt)
        db.tsdf_sparse_integrate(vol.volume(), poses, disps, intr, ixd, vol.trunc, weight=wgt, images=imgs, img_stride=1, img_offset=0)
        db.tsdf_sparse_mesh_into(vol.volume(), 1.0, mesh)

    eager, mesh_eager = _volume(cuda, name), _mesh_buffers(cuda, 4096, 8192)
    run(eager, mesh_eager)                                                                    # (also sizes the cached workspaces)
    torch.cuda.synchronize()
    vol, mesh = _volume(cuda, name), _mesh_buffers(cuda, 4096, 8192)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            run(vol, mesh)
    torch.cuda.current_stream().wait_stream(side)
    assert int(vol.counts[0]) == 0 and not bool(vol.wsum.any())                               # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert int(vol.counts[0]) == int(eager.counts[0]) > 0
    for a, b in ((vol.grid, eager.grid), (vol.coord, eager.coord), (vol.tsdf, eager.tsdf), (vol.wsum, eager.wsum), (vol.rgb, eager.rgb)):
        assert torch.equal(a, b)
    assert mesh["counts"].tolist() == mesh_eager["counts"].tolist() and mesh["counts"][0] > 0
    for k in mesh:
        assert torch.equal(mesh[k], mesh_eager[k]), k


# ------------------------------------------------------------------------------------------------ system
_system = {}


def _droid(cuda):
    """a Droid whose video holds tsdf_reference's analytic scene at 1/8 of 192 x 256 images: five keyframes, random colours"""
    if "droid" not in _system:
        from pvo_amd.droid import Droid, default_args
        nf, ht, wd = 5, 24, 32
        poses, disps, intr = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in R.scene(nf, ht, wd)[:3]]
        droid = Droid(default_args(device=str(cuda), image_size=[ht * 8, wd * 8], buffer=8, store_images=True))
        v = droid.video
        v.poses[:nf], v.disps[:nf], v.intrinsics[:nf] = poses, disps, intr
        g = torch.Generator().manual_seed(7)
        v.images[:nf] = torch.randint(0, 256, (nf, 3, ht * 8, wd * 8), generator=g).to(torch.uint8).to(cuda)
        v.counter = nf
        _system["droid"] = droid
    return _system["droid"]


def test_video_tsdf_sparse_is_the_dense_mesh_inside_allocated_space(cuda):
    from pvo_amd.depth_video import DepthVideo
    droid = _droid(cuda)
    nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES["5x24x32"]
    dims = tuple(8 * g for g in gdims)
    kw = dict(voxel=voxel, trunc=trunc, thresh=0.1, origin=origin)
    sparse = droid.get_mesh(sparse=True, dims=(dims[0] - 3, dims[1] - 7, dims[2] - 1), **kw)  # rounded up to bricks
    assert set(sparse) == {"verts", "normals", "rgba", "faces", "volume", "origin", "voxel"}
    vol = sparse["volume"]
    assert tuple(vol.grid.shape) == gdims and 0 < vol.bricks < vol.grid.numel()
    dense = droid.get_mesh(dims=dims, **kw)
    cells, _ = _cells(dense["tsdf"].cpu().numpy(), dense["wsum"].cpu().numpy())
    assert len(cells) == dense["verts"].shape[0]
    alloc = np.pad((vol.grid >= 0).cpu().numpy(), ((0, 1), (0, 1), (0, 1)))
    inside = np.all([alloc[(cells[:, 0] + (j >> 2)) >> 3, (cells[:, 1] + ((j >> 1) & 1)) >> 3, (cells[:, 2] + (j & 1)) >> 3] for j in range(8)], 0)
    print("dense %d vertices, %d with all corners in allocated bricks; sparse %d" % (len(cells), inside.sum(), sparse["verts"].shape[0]))
    rows = lambda m, sel: sorted(map(bytes, np.concatenate([m["verts"].cpu().numpy().view(np.uint8).reshape(-1, 12),
                                                            m["rgba"].cpu().numpy()], 1)[sel]))
    assert inside.sum() > 500 and rows(sparse, slice(None)) == rows(dense, inside)
    # default world: the full extent of the map's points, in whole bricks; the margin reaches the allocation
    auto = droid.video.tsdf(voxel=voxel, thresh=0.1, sparse=True)
    m = droid.get_map(thresh=0.1)
    o, g = DepthVideo.tsdf_sparse_bounds(m["xyz"], voxel, 3 * voxel)
    assert auto["origin"] == o and tuple(auto["volume"].grid.shape) == g and auto["verts"].shape[0] > 500
    assert droid.video.tsdf(voxel=voxel, thresh=0.1, sparse=True, margin=0)["volume"].bricks < auto["volume"].bricks
    with pytest.raises(ValueError):
        droid.video.tsdf(voxel=1e-7, thresh=0.1, sparse=True)                                 # over the grid limit: a clear error


def test_export_tool_without_sparse_writes_the_bytes_of_the_dense_mesh(cuda, tmp_path):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import export_map
    from pvo_amd.handoff import write_ply_mesh
    droid = _droid(cuda)
    base = ["--datapath", "x", "--map", "a.ply", "--voxel", "0.05", "--filter_thresh_map", "0.1"]
    plain, want = str(tmp_path / "plain.ply"), str(tmp_path / "want.ply")
    args = export_map.parse_args(base + ["--mesh", plain])
    assert args.sparse is False
    line = export_map.write_mesh(droid, args)
    g = droid.get_mesh(voxel=0.05, trunc=None, thresh=0.1, full_res=False, use_sigma=False, max_rel_sigma=None)      # what it called before
    nv, nf = write_ply_mesh(want, g["verts"], g["faces"], g["rgba"], g["normals"])
    assert open(plain, "rb").read() == open(want, "rb").read() and nv > 500
    assert line == "mesh: %d vertices, %d triangles from a %s volume of 0.05-sized voxels written to %s" % (
        nv, nf, "x".join(str(d) for d in g["tsdf"].shape), plain)
    sp = str(tmp_path / "sparse.ply")
    args = export_map.parse_args(base + ["--mesh", sp, "--sparse"])
    assert args.sparse is True and "bricks of 8^3" in export_map.write_mesh(droid, args)
    assert open(sp, "rb").read().startswith(b"ply") and os.path.getsize(sp) > 10000
    with pytest.raises(SystemExit):
        export_map.parse_args(["--datapath", "x", "--map", "a.ply", "--sparse"])
