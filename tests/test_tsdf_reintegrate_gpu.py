"""The live volume on the device: pvo_tsdf_reintegrate and pvo_tsdf_sparse_reintegrate (pvo_amd/csrc/tsdf_reintegrate.hip) against
tests/tsdf_reintegrate_reference.py - the weight sums and the emptied set held to EQUALITY and the values to the bound carried through
the whole remove-then-add history, on every voxel whose decisions are not within rounding of flipping (at most 1 %,
tests/test_tsdf_reintegrate_host.py); the byte identities of the contract (add-only = pvo_tsdf_integrate, one call = two calls, split
slot lists, bricks = dense); its case list; guard bytes around every buffer; capture and replay; and the system path (LiveMap on a
Droid's video, Droid(args.live_map))."""
import numpy as np
import pytest
import torch

import tsdf_reference as R
import tsdf_reintegrate_reference as RR
import tsdf_track_reference as T

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 256
_dev_cases, _refs = {}, {}


def _case(cuda, name, weights):
    """(the host case, its arrays on the device)"""
    key = (name, weights)
    if key not in _dev_cases:
        c = RR.case(name, weights)
        d = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(cuda) for k in ("poses", "disps", "intr", "images", "poses2", "disps2")}
        d["weight"] = None if c["weight"] is None else torch.from_numpy(c["weight"]).to(cuda)
        _dev_cases[key] = (c, d)
    return _dev_cases[key]


def _guarded(cuda, nbytes, fill=0):
    """a buffer of nbytes (a multiple of 4) between two guards; returns (the buffer as uint8, the whole allocation)"""
    base = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=cuda)
    base[GUARD:GUARD + nbytes] = fill
    return base[GUARD:GUARD + nbytes], base


def _guards_ok(base):
    return bool((base[:GUARD] == SENTINEL).all()) and bool((base[-GUARD:] == SENTINEL).all())


class _Vol:
    """a zeroed dense volume whose three buffers sit between guard bytes"""

    def __init__(self, cuda, dims, colours=True):
        n = int(np.prod(dims))
        self.bases = []
        bufs = []
        for k in (1, 1, 3):
            buf, base = _guarded(cuda, 4 * n * k)
            bufs.append(buf.view(torch.float32))
            self.bases.append(base)
        self.tsdf, self.wsum = bufs[0].view(dims), bufs[1].view(dims)
        self.rgb = bufs[2].view(tuple(dims) + (3,)) if colours else None

    def np(self):
        return [None if t is None else t.cpu().numpy() for t in (self.tsdf, self.wsum, self.rgb)]

    def copy_from(self, other):
        self.tsdf.copy_(other.tsdf)
        self.wsum.copy_(other.wsum)
        if self.rgb is not None:
            self.rgb.copy_(other.rgb)
        return self

    def guards_ok(self):
        return all(_guards_ok(b) for b in self.bases)


def _ix(cuda, ix):
    return torch.tensor(list(ix), dtype=torch.long, device=cuda)


def _call(cuda, cd, vol, remove=None, add=None, moved=False, w_floor=RR.W_FLOOR, w_max=0.0):
    """pvo_tsdf_reintegrate on vol: remove / add are keyframe lists; remove reads the case's original frames, add the original ones or
    with moved=True the pushed ones.  The workspace has exactly the bytes the library asks for, between guards."""
    from pvo_amd import _lib, droid_backends as db
    c, d = cd
    rm = None if remove is None else (d["poses"], d["disps"], _ix(cuda, remove), d["weight"])
    ad = None if add is None else ((d["poses2"], d["disps2"]) if moved else (d["poses"], d["disps"])) + (_ix(cuda, add), d["weight"])
    need = _lib.load().pvo_tsdf_reintegrate_workspace_bytes(0 if remove is None else len(remove), 0 if add is None else len(add))
    ws, base = _guarded(cuda, max(int(need), 4), fill=0x5A)
    db.tsdf_reintegrate(vol.tsdf, vol.wsum, vol.rgb, c["origin"], c["voxel"], c["trunc"], d["intr"], remove=rm, add=ad,
                        images=d["images"] if vol.rgb is not None else None, img_stride=1, img_offset=0, w_max=w_max, w_floor=w_floor,
                        workspace=ws)
    torch.cuda.synchronize()
    assert _guards_ok(base) and vol.guards_ok()
    return vol


def _integrated(cuda, cd, ix, colours=True):
    """pvo_tsdf_integrate of keyframes ix into a zeroed volume"""
    from pvo_amd import droid_backends as db
    c, d = cd
    vol = _Vol(cuda, c["dims"], colours)
    db.tsdf_integrate(vol.tsdf, vol.wsum, vol.rgb, d["poses"], d["disps"], d["intr"], _ix(cuda, ix), c["origin"], c["voxel"], c["trunc"],
                      weight=d["weight"], images=d["images"] if colours else None, img_stride=1, img_offset=0)
    return vol


def _ref(name, weights, colours, what):
    """the reference states of a case, computed once: "fused" (all keyframes added), "removed" (all but the middle one removed from
    it), "refreshed" (the middle one removed as it was and added as pushed)"""
    key = (name, weights, colours, what)
    if key not in _refs:
        c = RR.case(name, weights)
        if what == "fused":
            _refs[key] = RR.run(c, RR.empty_state(c["dims"], colours), add=list(range(c["nf"])), colours=colours)
        elif what == "removed":
            _refs[key] = RR.run(c, _ref(name, weights, colours, "fused"), remove=c["rest"], colours=colours)
        else:
            _refs[key] = RR.run(c, _ref(name, weights, colours, "fused"), remove=[c["k"]], add=[c["k"]], moved=True, colours=colours)
    return _refs[key]


def _bytes_equal(a, b):
    return all((x is None and y is None) or np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", list(R.SCENES))
@pytest.mark.parametrize("weights", ["unit", "nondyadic"])
@pytest.mark.parametrize("colours", [True, False])
def test_kernel_matches_the_reference(cuda, name, weights, colours):
    """add-only, remove-only and both (the middle keyframe pushed by RR.PUSH, its depths perturbed) from the kernel's own fused volume:
    wsum and the emptied set EQUAL, tsdf and rgb within the bound the reference carried through the history"""
    cd = _case(cuda, name, weights)
    c = cd[0]
    every = list(range(c["nf"]))
    fused = _call(cuda, cd, _Vol(cuda, c["dims"], colours), add=every)
    for what, vol in (("fused", fused),
                      ("removed", _call(cuda, cd, _Vol(cuda, c["dims"], colours).copy_from(fused), remove=c["rest"])),
                      ("refreshed", _call(cuda, cd, _Vol(cuda, c["dims"], colours).copy_from(fused), remove=[c["k"]], add=[c["k"]], moved=True))):
        ref = _ref(name, weights, colours, what)
        got = vol.np()
        ok, report = RR.state_matches(got[0], got[1], got[2], ref)
        print("%s %s colours %s, %s: %d flagged of %d touched, %d emptied; %s"
              % (name, weights, colours, what, ref["flagged"].sum(), ref["touched"].sum(), ref["emptied"].sum(), report))
        assert ref["flagged"].sum() <= 0.01 * ref["touched"].sum()
        assert ok, report
        assert all(np.isfinite(t).all() for t in got if t is not None)
    if weights == "unit":
        w = fused.np()[1]
        assert np.array_equal(w, np.round(w)) and w.max() <= c["nf"]


@pytest.mark.parametrize("name", list(R.SCENES))
@pytest.mark.parametrize("mutant", RR.MUTANTS)
def test_the_check_rejects_a_wrong_reference(cuda, name, mutant):
    """the kernel's volume must FAIL the check against each deliberately wrong reference: the bound hides none of them"""
    cd = _case(cuda, name, "nondyadic")
    c = cd[0]
    fused = _call(cuda, cd, _Vol(cuda, c["dims"]), add=list(range(c["nf"])))
    kw = dict(remove=[c["k"]], add=[c["k"]], moved=True) if mutant == "new_poses" else dict(remove=c["rest"])
    got = _call(cuda, cd, fused, **kw).np()
    wrong = RR.run(c, _ref(name, "nondyadic", True, "fused"), mutant=mutant, **kw)
    ok, report = RR.state_matches(got[0], got[1], got[2], wrong)
    print(name, mutant, report)
    assert not ok
    right = _ref(name, "nondyadic", True, "refreshed" if mutant == "new_poses" else "removed")
    ok, report = RR.state_matches(got[0], got[1], got[2], right)
    assert ok, report


# ------------------------------------------------------------------------------------------------ the byte identities
@pytest.mark.parametrize("name", list(R.SCENES))
def test_add_only_leaves_the_bytes_of_integrate(cuda, name):
    for weights, colours in (("nondyadic", True), ("unit", False)):
        cd = _case(cuda, name, weights)
        c = cd[0]
        ix = list(range(c["nf"]))[::-1]                                                       # the order is part of the arithmetic
        assert _bytes_equal(_call(cuda, cd, _Vol(cuda, c["dims"], colours), add=ix).np(), _integrated(cuda, cd, ix, colours).np())
    capped = _call(cuda, cd, _Vol(cuda, c["dims"], False), add=ix, w_max=1.5).np()           # the cap reaches the ADD step
    assert capped[1].max() == np.float32(1.5)


@pytest.mark.parametrize("name", list(R.SCENES))
def test_one_call_leaves_the_bytes_of_two_and_of_split_lists(cuda, name):
    cd = _case(cuda, name, "nondyadic")
    c = cd[0]
    every, k = list(range(c["nf"])), c["k"]
    start = _integrated(cuda, cd, every)
    fresh = lambda: _Vol(cuda, c["dims"]).copy_from(start)
    rest = c["rest"]
    one = _call(cuda, cd, fresh(), remove=[k] + rest[:1], add=rest[:1] + [k], moved=True).np()
    two = _call(cuda, cd, _call(cuda, cd, fresh(), remove=[k] + rest[:1]), add=rest[:1] + [k], moved=True).np()
    assert _bytes_equal(one, two)
    split = _call(cuda, cd, fresh(), remove=[k])
    split = _call(cuda, cd, split, remove=rest[:1], add=rest[:1], moved=True)
    split = _call(cuda, cd, split, add=[k], moved=True).np()
    assert _bytes_equal(one, split)
    again = _call(cuda, cd, fresh(), remove=[k] + rest[:1], add=rest[:1] + [k], moved=True).np()
    assert _bytes_equal(one, again)                                                           # the same bytes come out twice
    assert not _bytes_equal(one, start.np())


def test_ids_out_of_range_are_skipped_and_nothing_to_do_writes_nothing(cuda):
    from pvo_amd import droid_backends as db
    name = "5x24x32"
    cd = _case(cuda, name, "nondyadic")
    c, d = cd
    start = _integrated(cuda, cd, range(c["nf"]))
    fresh = lambda: _Vol(cuda, c["dims"]).copy_from(start)
    want = _call(cuda, cd, fresh(), remove=[1, 3], add=[3, 1], moved=True).np()
    got = _call(cuda, cd, fresh(), remove=[-1, 1, c["nf"], 3, 1 << 40], add=[-7, 3, c["nf"] + 2, 1], moved=True).np()
    assert _bytes_equal(got, want)
    only_bad = _call(cuda, cd, fresh(), remove=[-1, c["nf"]], add=[1 << 40, -3], moved=True).np()
    assert _bytes_equal(only_bad, start.np())
    # N_old = N = 0: nothing is written, with and without the tuples
    sent = _Vol(cuda, c["dims"])
    for t in (sent.tsdf, sent.wsum, sent.rgb):
        t.view(torch.uint8).fill_(0x3C)
    before = sent.np()
    _call(cuda, cd, sent, remove=[], add=[])
    db.tsdf_reintegrate(sent.tsdf, sent.wsum, sent.rgb, c["origin"], c["voxel"], c["trunc"], d["intr"], images=d["images"], img_stride=1,
                        img_offset=0)
    torch.cuda.synchronize()
    assert _bytes_equal(sent.np(), before) and sent.guards_ok()
    # a removal from an empty volume leaves it empty, bit for bit
    empty = _call(cuda, cd, _Vol(cuda, c["dims"]), remove=[0, 1]).np()
    assert not any(t.view(np.uint32).any() for t in empty)


# ------------------------------------------------------------------------------------------------ bricks
WORLD = ((4, 5, 6), tuple(np.float32(o) - np.float32(0.4) for o in R.SCENES["5x24x32"][4]))


@pytest.mark.parametrize("weights,colours", [("nondyadic", True), ("unit", False)])
def test_brick_call_leaves_the_bytes_of_the_dense_call(cuda, weights, colours):
    """a world of 4 x 5 x 6 bricks around the scene, one brick wider than the dense volume on its low sides, most of whose bricks do
    not exist: after the same refresh every voxel of every brick holds the bytes the dense call leaves in the [32,40,48] volume"""
    from pvo_amd import _lib, droid_backends as db
    from pvo_amd.tsdf_sparse import SparseTSDF
    c, d = _case(cuda, "5x24x32", weights)
    origin = [float(v) for v in WORLD[1]]
    vol = SparseTSDF(origin, WORLD[0], c["voxel"], c["trunc"], colours=colours, device=cuda, cap=2)
    every, k = _ix(cuda, range(c["nf"])), c["k"]
    vol.allocate(d["poses"], d["disps"], d["intr"], every, weight=d["weight"])
    vol.allocate(d["poses2"], d["disps2"], d["intr"], every, weight=d["weight"])             # the bricks of the pushed keyframe as well
    images = d["images"] if colours else None
    vol.integrate(d["poses"], d["disps"], d["intr"], every, weight=d["weight"], images=images, img_stride=1, img_offset=0)
    dense = vol.to_dense()
    n, total = vol.bricks, int(np.prod(WORLD[0]))
    assert 8 < n < total and not bool(dense["allocated"].all())                              # missing bricks
    remove = (d["poses"], d["disps"], _ix(cuda, [k, 99, 0]), d["weight"])                    # (an id out of range in each set)
    add = (d["poses2"], d["disps2"], _ix(cuda, [0, -1, k]), d["weight"])
    kept_base = torch.full((vol.cap + 2,), -1, dtype=torch.int32, device=cuda)
    need = _lib.load().pvo_tsdf_sparse_reintegrate_workspace_bytes(3, 3)
    ws, ws_base = _guarded(cuda, int(need), fill=0x5A)
    pools = [t.clone() for t in (vol.tsdf, vol.wsum) + ((vol.rgb,) if colours else ())]
    db.tsdf_sparse_reintegrate(vol.volume(), vol.trunc, d["intr"], remove=remove, add=add, images=images, img_stride=1, img_offset=0,
                               kept=kept_base, workspace=ws)
    torch.cuda.synchronize()
    assert _guards_ok(ws_base) and kept_base[vol.cap:].tolist() == [-1, -1]
    kept = kept_base[:n].cpu().numpy()
    print("%d bricks of %d; survivors of 6 slots per brick: min %d, mean %.2f, max %d" % (n, total, kept.min(), kept.mean(), kept.max()))
    assert kept.min() >= 0 and kept.max() <= 4 and bool((kept_base[n:vol.cap] == -1).all())  # the two ids out of range never survive
    for t, was in zip((vol.tsdf, vol.wsum, vol.rgb), pools):                                  # pool slots not in use are not written
        assert torch.equal(t[n:], was[n:])
    db.tsdf_reintegrate(dense["tsdf"], dense["wsum"], dense["rgb"], origin, c["voxel"], c["trunc"], d["intr"], remove=remove, add=add,
                        images=images, img_stride=1, img_offset=0)
    after = vol.to_dense()
    mask = dense["allocated"].repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)
    for key in ("tsdf", "wsum") + (("rgb",) if colours else ()):
        a, b = after[key][mask], dense[key][mask]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), key
    assert not torch.equal(vol.wsum[:n], pools[1][:n])                                        # (something happened)
    # the method allocates for `add` first (growing the pool from 2 bricks), then makes the same call: the bricks that existed BEFORE
    # the refresh hold the dense bytes (a brick allocated for the add holds only what came after it)
    vol2 = SparseTSDF(origin, WORLD[0], c["voxel"], c["trunc"], colours=colours, device=cuda, cap=2)
    vol2.allocate(d["poses"], d["disps"], d["intr"], every, weight=d["weight"])
    vol2.integrate(d["poses"], d["disps"], d["intr"], every, weight=d["weight"], images=images, img_stride=1, img_offset=0)
    n2 = vol2.bricks
    vol2.reintegrate(d["intr"], remove=remove, add=add, images=images, img_stride=1, img_offset=0)
    assert n2 <= vol2.bricks <= n
    old = torch.zeros_like(dense["allocated"])
    cc = vol2.coord[:n2].long()
    old[cc[:, 0], cc[:, 1], cc[:, 2]] = True
    old = old.repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)
    assert torch.equal(vol2.to_dense()["wsum"][old].view(torch.int32), dense["wsum"][old].view(torch.int32))


# ------------------------------------------------------------------------------------------------ capture
def test_capture_and_replay_give_the_eager_bytes(cuda):
    from pvo_amd import droid_backends as db
    cd = _case(cuda, "5x24x32", "nondyadic")
    c, d = cd
    every, k = list(range(c["nf"])), c["k"]
    start = _integrated(cuda, cd, every)
    eager = _call(cuda, cd, _Vol(cuda, c["dims"]).copy_from(start), remove=[k], add=[k], moved=True)
    vol = _Vol(cuda, c["dims"]).copy_from(start)
    ixk = _ix(cuda, [k])                                                                      # (no host-to-device copy inside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            db.tsdf_reintegrate(vol.tsdf, vol.wsum, vol.rgb, c["origin"], c["voxel"], c["trunc"], d["intr"],
                                remove=(d["poses"], d["disps"], ixk, d["weight"]), add=(d["poses2"], d["disps2"], ixk, d["weight"]),
                                images=d["images"], img_stride=1, img_offset=0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _bytes_equal(vol.np(), start.np())                                                 # capture ran nothing
    g.replay()
    torch.cuda.synchronize()
    assert _bytes_equal(vol.np(), eager.np()) and vol.guards_ok()


# ------------------------------------------------------------------------------------------------ system
KW = dict(voxel=T.VOXEL, trunc=T.TRUNC, thresh=0.1, origin=T.ORIGIN, dims=T.DIMS)


def _droid(cuda):
    """a Droid whose video holds tsdf_track_reference's scene at 1/8 of 192 x 256 images: five keyframes, random colours"""
    from pvo_amd.droid import Droid, default_args
    nf, (ht, wd) = T.NFRAMES, T.FUSE_SIZE
    poses, disps, intr, _ = [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in T.scene(*T.FUSE_SIZE)]
    droid = Droid(default_args(device=str(cuda), image_size=[ht * 8, wd * 8], buffer=8, store_images=True))
    v = droid.video
    v.poses[:nf], v.disps[:nf], v.intrinsics[:nf] = poses, disps, intr
    v.tstamp[:nf] = torch.arange(nf, device=cuda, dtype=torch.float32)
    g = torch.Generator().manual_seed(7)
    v.images[:nf] = torch.randint(0, 256, (nf, 3, ht * 8, wd * 8), generator=g).to(torch.uint8).to(cuda)
    v.counter = nf
    return droid


@pytest.mark.parametrize("sparse", [False, True])
def test_live_map_follows_a_keyframe_that_moves_and_comes_back(cuda, sparse):
    """five keyframes fused; keyframe 2 pushed by a voxel: exactly one refresh; restored: one more.  The volume then equals, up to the
    roundings the reference bounds for exactly this history, the one fused from scratch at the final state.
    tol = 0.9 voxels here, not the default quarter voxel: the pushed keyframe's own drift is at least 1 (every pixel kept before and
    after moves by exactly a voxel, one kept in only one of the two counts three), while a keyframe that did NOT move drifts only through
    pixels whose depth-filter votes flip - keyframes 3 and 4 are voted on by keyframe 2 (views ix-1, ix-2, ix-3) - which on this
    scene is 4 % of keyframe 4's pixels, a drift of 0.61 (the depth filter's fp64 reference on the CPU gives the same figure for
    thresholds from 0.05 to 0.4).  With the default tolerance that keyframe is refreshed too, rightly: its weights did change."""
    from pvo_amd.live_map import LiveMap
    droid = _droid(cuda)
    v, n = droid.video, T.NFRAMES
    lm = LiveMap(v, lag=0, tol=0.9, sparse=sparse, **KW)
    assert lm.update() == (n, 0, 0) and sorted(lm.fused) == list(range(n))
    host = lambda t: t.cpu().numpy().copy()
    # (bricks: a brick the pushed keyframe makes necessary later holds only what came after it - compared are the first update's)
    first_bricks = lm.sparse.to_dense()["allocated"] if sparse else None
    state = dict(poses=host(v.poses[:n]), disps=host(v.disps[:n]), weight=host(lm.weight_fused[:n]))
    images = host(v.images[:n, :, 3::8, 3::8])
    assert np.array_equal(state["weight"], np.round(state["weight"])) and state["weight"].mean() > 0.5      # unit weights: kept or not
    run = lambda s, rm, ad: RR.reintegrate_reference(s, T.ORIGIN, T.VOXEL, T.TRUNC, host(v.intrinsics[0]), remove=rm, add=ad, images=images,
                                                     img_stride=1, img_offset=0)
    ref = run(RR.empty_state(T.DIMS), None, (state["poses"], state["disps"], range(n), state["weight"]))
    assert lm.update() == (0, 0, 0)
    true2 = v.poses[2].clone()
    for step in range(2):
        if step == 0:
            v.poses[2, 0] += T.VOXEL
            d = lm.drift(list(range(n)))
            print("drift after the push, in voxels:", [round(x, 4) for x in d.tolist()])
            assert 1.0 - 1e-3 <= d[2].item() < 1.5 and d[[0, 1, 3, 4]].max().item() < 0.9 and d[[0, 1]].max().item() == 0.0
        else:
            v.poses[2] = true2
        assert lm.update() == (0, 1, 0)                                                       # exactly one refresh
        new = dict(poses=host(v.poses[:n]), disps=host(v.disps[:n]), weight=host(lm.weight_fused[:n]))
        ref = run(ref, (state["poses"], state["disps"], [2], state["weight"]), (new["poses"], new["disps"], [2], new["weight"]))
        for key in ("poses", "disps", "weight"):
            state[key][2] = new[key][2]
    assert lm.refreshed_total == 2
    live = lm.sparse.to_dense() if sparse else dict(tsdf=lm.tsdf, wsum=lm.wsum, rgb=lm.rgb)
    dims = T.DIMS
    got = [host(live[k][:dims[0], :dims[1], :dims[2]]) for k in ("tsdf", "wsum", "rgb")]
    if sparse:                                                                                # voxels outside the bricks hold nothing
        inb = host(first_bricks.repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)[:dims[0], :dims[1], :dims[2]])
        assert inb.sum() > 0.2 * inb.size
    assert ref["flagged"].sum() <= 0.01 * ref["touched"].sum()
    if sparse:
        ref["flagged"] = ref["flagged"] | ~inb
    ok, report = RR.state_matches(got[0], got[1], got[2], ref)
    print("live volume (sparse %s) against the reference's history: %s" % (sparse, report))
    assert ok, report
    # against the kernel's own volume fused from scratch at the final state
    scratch = v.tsdf(keep_rgb=True, **KW)
    sref = run(RR.empty_state(T.DIMS), None, (state["poses"], state["disps"], range(n), host(lm.weights(n))))
    un = ~(ref["flagged"] | sref["flagged"])
    sw, st = host(scratch["wsum"]), host(scratch["tsdf"])
    assert np.array_equal((got[1] == 0)[un], (sw == 0)[un])                                   # the emptied set
    assert np.array_equal(got[1][un], sw[un])                                                 # unit weights: exactly
    diff = np.abs(got[0].astype(np.float64) - st.astype(np.float64))
    lim = ref["bound"] + sref["bound"]
    print("   against from-scratch: tsdf max diff %.3e, max share of the two bounds %.3f" % (diff[un].max(), (diff[un] / np.maximum(lim[un], 1e-300)).max()))
    assert np.all(diff[un] <= lim[un])
    mesh = lm.mesh()
    print("   mesh: %d vertices, %d faces; from scratch %d, %d" % (mesh["verts"].shape[0], mesh["faces"].shape[0], scratch["verts"].shape[0],
                                                                  scratch["faces"].shape[0]))
    if not sparse:
        assert (mesh["verts"].shape[0], mesh["faces"].shape[0]) == (scratch["verts"].shape[0], scratch["faces"].shape[0])
    assert mesh["verts"].shape[0] > 500
    # the volume serves the renderer and the tracker unchanged
    vol = lm.as_volume()
    r = v.tsdf_render(vol, ix=[2])
    assert torch.equal(r["depth"], lm.render(ix=[2])["depth"]) and bool((r["depth"] > 0).any())
    if not sparse:                                                                            # the same call on the buffers themselves
        direct = v.tsdf_render(dict(tsdf=lm.tsdf, wsum=lm.wsum, rgb=lm.rgb, origin=list(T.ORIGIN), voxel=T.VOXEL), ix=[2])
        assert all(torch.equal(r[key], direct[key]) for key in r)
    res = v.model_residual(vol, ix=[2])
    assert float(res["share"][0]) > 0 and bool(torch.isfinite(res["median"]).all())
    tr = lm.track(ix=[2])
    assert tr["poses"].shape == (1, 7) and bool(torch.isfinite(tr["poses"]).all())


def _plane_run(cuda, live_map):
    """pvo_amd.synthetic's plane scene through Droid.track and Droid.terminate: the oracle operator takes the network's place in the
    frontend and the backend, the motion filter's place is taken by the scene's feature maps (as synthetic.run_sequence feeds them)"""
    from argparse import Namespace
    from pvo_amd import droid_backends as db
    from pvo_amd.backend import DroidBackend
    from pvo_amd.droid import Droid, default_args
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.geom.se3 import SE3
    from pvo_amd.synthetic import OracleFlowOperator, PlaneScene
    scene = PlaneScene(ht=24, wd=32, n_frames=14, seed=0)
    torch.manual_seed(0)
    droid = Droid(default_args(device=str(cuda), image_size=[scene.ht * 8, scene.wd * 8], buffer=32, store_images=True, live_map=live_map))
    video = droid.video
    op = OracleFlowOperator(scene, video, lambda p, d, k, i, j: db.reproject(p, d, k, i, j)[0])
    droid.frontend = DroidFrontend(op, video, device=cuda, warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20,
                                   frontend_radius=2, frontend_nms=1)
    droid.backend = DroidBackend(Namespace(update=op), video, Namespace(device=str(cuda), backend_radius=2, backend_nms=3, backend_thresh=15.0,
                                                                        beta=0.3, backend_corr="alt"))
    droid.traj_filler = lambda stream: SE3(video.poses[:video.counter].clone())
    g, gi = torch.Generator().manual_seed(1), torch.Generator().manual_seed(3)
    h, w = scene.ht, scene.wd

    def feed(tstamp, image, depth, intrinsics, segments, right=None):
        k = int(tstamp)
        slot = video.counter
        op.bind(slot, k)
        video.append(float(k), None if k else scene.poses[0].to(cuda), None, scene.intr.to(cuda), torch.randn(h, w, 128, generator=g).half().to(cuda),
                     torch.zeros(128, h, w, dtype=torch.half, device=cuda), torch.zeros(128, h, w, dtype=torch.half, device=cuda))
        video.images[slot] = torch.randint(0, 256, (3, 8 * h, 8 * w), generator=gi).to(torch.uint8).to(cuda)
    droid.filterx.track = feed
    updates = []
    if droid.live_map is not None:
        inner = droid.live_map.update
        droid.live_map.update = lambda *a, **kw: updates.append(inner(*a, **kw)) or updates[-1]
    for k in range(scene.n):
        droid.track(float(k), None)
    before = video.poses[:video.counter].clone()
    droid.terminate()
    return droid, before, updates


def test_droid_keeps_a_live_map_and_tracking_is_untouched_by_it(cuda):
    from pvo_amd.depth_video import DepthVideo
    plain, before0, _ = _plane_run(cuda, None)
    assert plain.live_map is None
    with pytest.raises(RuntimeError, match="live_map"):
        plain.get_live_map()
    v0, n = plain.video, plain.video.counter
    voxel = 0.05
    m = plain.get_map(thresh=0.05)
    origin, dims = DepthVideo.tsdf_bounds(m["xyz"], voxel, 3 * voxel)
    droid, before1, updates = _plane_run(cuda, dict(voxel=voxel, origin=origin, dims=dims, thresh=0.05, lag=3))
    v1 = droid.video
    # with the live map on, poses and depths are bit for bit those of the run without it: it only reads the video
    assert v1.counter == n and torch.equal(before1, before0)
    assert torch.equal(v1.poses[:n], v0.poses[:n]) and torch.equal(v1.disps[:n], v0.disps[:n])
    added, refreshed, dropped = [sum(u[k] for u in updates) for k in range(3)]
    print("live map over %d keyframes: %d updates, %d added, %d refreshed, %d dropped; the last (after the global BA) %s"
          % (n, len(updates), added, refreshed, dropped, updates[-1]))
    assert len(updates) == 14 + 1 and added >= n                                             # one per track(), one in terminate()
    assert sorted(droid.live_map.fused) == list(range(n))
    out = droid.get_live_map()
    assert {"tsdf", "wsum", "rgb", "origin", "voxel", "verts", "normals", "rgba", "faces"} <= set(out)
    assert out["verts"].shape[0] > 100 and out["faces"].shape[0] > 100
    # and it is the map of the final state: a second update finds nothing to do
    assert droid.live_map.update(upto=n) == (0, 0, 0)
    scratch = droid.get_mesh(voxel=voxel, thresh=0.05, origin=origin, dims=dims)
    both = (out["wsum"] >= 1) & (scratch["wsum"] >= 1)
    d = (out["tsdf"] - scratch["tsdf"])[both].abs()
    print("   against a volume fused from scratch: %d voxels usable in both, |tsdf difference| mean %.5f max %.4f" % (int(both.sum()), d.mean(), d.max()))
    assert int(both.sum()) > 0.5 * int((scratch["wsum"] >= 1).sum())
