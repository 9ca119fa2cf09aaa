"""The live volume, the parts that need no GPU: the C boundary of pvo_tsdf_reintegrate / pvo_tsdf_sparse_reintegrate (symbols, struct
layouts against the C compiler, every argument check - all of them run before anything touches the device, so NULL and fake pointers
are enough), the conditions on the inputs under which the GPU tests may leave flagged voxels out, the inverse property of the numpy
yardstick (tests/tsdf_reintegrate_reference.py) with the reason w_floor exists, four deliberately wrong references, and the ledger
(pvo_amd.live_map.LiveMap) on CPU tensors with the native call replaced by the reference."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import tsdf_reference as R
import tsdf_reintegrate_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PVO_OK, PVO_EINVAL, PVO_EWORKSPACE = 0, 1, 3
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced: every call below returns before a launch


def _lib():
    from pvo_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.startswith("pvo_tsdf") or name == "pvo_version":
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib, _lib


# ------------------------------------------------------------------------------------------------ the C boundary
def test_symbols_struct_layouts_and_abi_version(tmp_path):
    lib, L = _lib()
    assert lib.pvo_version() == 106 == L.PVO_ABI_VERSION
    D, S = L.TsdfReintegrateArgs, L.TsdfSparseReintegrateArgs
    fields = {"pvo_tsdf_reintegrate_args": [n for n, _ in D._fields_], "pvo_tsdf_sparse_reintegrate_args": [n for n, _ in S._fields_]}
    lines = []
    for struct, names in fields.items():
        lines.append('  printf("%%zu", sizeof(%s));' % struct)
        lines += ['  printf(" %%zu", offsetof(%s, %s));' % (struct, n) for n in names]
        lines.append('  printf("\\n");')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pvo_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [[int(x) for x in line.split()] for line in subprocess.check_output([str(exe)], text=True).strip().split("\n")]
    for row, struct in zip(got, (D, S)):
        assert row == [ctypes.sizeof(struct)] + [getattr(struct, n).offset for n, _ in struct._fields_], struct.__doc__
    assert lib.pvo_tsdf_reintegrate_args_size() == ctypes.sizeof(D) and lib.pvo_tsdf_sparse_reintegrate_args_size() == ctypes.sizeof(S)
    for fn in (lib.pvo_tsdf_reintegrate_workspace_bytes, lib.pvo_tsdf_sparse_reintegrate_workspace_bytes):
        assert fn(0, 0) == 0 and fn(-3, 0) == 0
        assert 64 * 72 <= fn(8, 64) <= 64 * 72 + 512 and fn(8, 0) >= 64 * 8 and fn(0, 8) >= 64 * 8
    # the entry points this pull request leaves alone are still there
    assert lib.pvo_tsdf_integrate_args_size() == ctypes.sizeof(L.TsdfIntegrateArgs)
    assert lib.pvo_tsdf_sparse_integrate_args_size() == ctypes.sizeof(L.TsdfSparseIntegrateArgs)


def _dense_args(L, **kw):
    a = L.TsdfReintegrateArgs()
    a.tsdf = a.wsum = a.intrinsics = FAKE
    a.poses_old = a.disps_old = a.ix_old = a.poses = a.disps = a.ix = FAKE
    a.nz, a.ny, a.nx, a.voxel, a.trunc, a.w_floor = 8, 8, 8, 0.1, 0.3, 2.0 ** -10
    a.N_old, a.N, a.nframes, a.ht, a.wd = 2, 3, 4, 8, 8
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _sparse_args(L, **kw):
    a = L.TsdfSparseReintegrateArgs()
    a.tsdf = a.wsum = a.coord = a.bricks = a.intrinsics = FAKE
    a.poses_old = a.disps_old = a.ix_old = a.poses = a.disps = a.ix = FAKE
    a.gz, a.gy, a.gx, a.cap, a.voxel, a.trunc, a.w_floor = 2, 2, 2, 4, 0.1, 0.3, 2.0 ** -10
    a.N_old, a.N, a.nframes, a.ht, a.wd = 2, 3, 4, 8, 8
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_reintegrate_validates_before_touching_the_device(kind):
    lib, L = _lib()
    fn = lib.pvo_tsdf_reintegrate if kind == "dense" else lib.pvo_tsdf_sparse_reintegrate
    need_fn = lib.pvo_tsdf_reintegrate_workspace_bytes if kind == "dense" else lib.pvo_tsdf_sparse_reintegrate_workspace_bytes
    make = (lambda **kw: _dense_args(L, **kw)) if kind == "dense" else (lambda **kw: _sparse_args(L, **kw))
    call = lambda a, ws=FAKE, n=1 << 20: fn(ctypes.byref(a), ws, n, None)
    assert fn(None, FAKE, 1 << 20, None) == PVO_EINVAL
    for ptr in ("tsdf", "wsum", "intrinsics", "poses_old", "disps_old", "ix_old", "poses", "disps", "ix"):
        assert call(make(**{ptr: None})) == PVO_EINVAL, ptr
    # a set without slots needs no operands
    assert call(make(N_old=0, poses_old=None, disps_old=None, ix_old=None), FAKE, 0) == PVO_EWORKSPACE
    assert call(make(N=0, poses=None, disps=None, ix=None), FAKE, 0) == PVO_EWORKSPACE
    if kind == "dense":
        assert call(make(nz=2048, ny=1024, nx=1024)) == PVO_EINVAL and call(make(nz=-1)) == PVO_EINVAL
    else:
        assert call(make(coord=None)) == PVO_EINVAL and call(make(bricks=None)) == PVO_EINVAL
        assert call(make(gz=-1)) == PVO_EINVAL and call(make(cap=1 << 22)) == PVO_EINVAL and call(make(gx=(1 << 18) + 1)) == PVO_EINVAL
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert call(make(voxel=bad)) == PVO_EINVAL and call(make(trunc=bad)) == PVO_EINVAL
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(make(z_near=bad)) == PVO_EINVAL and call(make(w_max=bad)) == PVO_EINVAL and call(make(w_floor=bad)) == PVO_EINVAL
    assert call(make(N=-1)) == PVO_EINVAL and call(make(N_old=-1)) == PVO_EINVAL and call(make(nframes=-1)) == PVO_EINVAL
    assert call(make(ht=1 << 16, wd=1 << 15)) == PVO_EINVAL
    assert call(make(rgb=FAKE)) == PVO_EINVAL                                                # a colour volume without images
    img = dict(images=FAKE, IH=64, IW=64, img_stride=8, img_offset=3)
    assert call(make(**dict(img, img_stride=9))) == PVO_EINVAL and call(make(**dict(img, img_offset=8))) == PVO_EINVAL
    assert call(make(**dict(img, img_stride=0))) == PVO_EINVAL and call(make(**dict(img, IW=59))) == PVO_EINVAL
    need = need_fn(2, 3)
    assert need > 0
    assert call(make(rgb=FAKE, **img), FAKE, need - 1) == PVO_EWORKSPACE                     # everything else in order
    assert call(make(**img), None, need) == PVO_EWORKSPACE
    assert call(make(), FAKE + 4, need) == PVO_EINVAL                                        # a misaligned workspace
    # nothing to do: no launch
    assert call(make(N=0, N_old=0)) == PVO_OK and call(make(ht=0)) == PVO_OK
    assert call(make(nx=0) if kind == "dense" else make(cap=0)) == PVO_OK


# ------------------------------------------------------------------------------------------------ conditions on the inputs
_states = {}


def _fused(name, weights, colours=True):
    """the reference state after all keyframes of the case were added"""
    key = (name, weights, colours)
    if key not in _states:
        c = RR.case(name, weights)
        _states[key] = RR.run(c, RR.empty_state(c["dims"], colours), add=list(range(c["nf"])), colours=colours)
    return _states[key]


@pytest.mark.parametrize("name", list(R.SCENES))
def test_flagged_voxels_stay_below_one_percent_and_the_bound_says_something(name):
    """the middle keyframe pushed by RR.PUSH with its depths perturbed, removed as it was and added as it is: flags of BOTH sets'
    operands; then all but the middle keyframe removed, where W / Wn is largest.  On the reference alone."""
    for weights in ("scene", "nondyadic", "unit"):
        c = RR.case(name, weights)
        both = RR.run(c, _fused(name, weights), remove=[c["k"]], add=[c["k"]], moved=True)
        rem = RR.run(c, _fused(name, weights), remove=c["rest"])
        for what, s in (("refresh", both), ("remove all but one", rem)):
            touched, flagged = int(s["touched"].sum()), int(s["flagged"].sum())
            un = ~s["flagged"]
            print("%s %s weights, %s: %d touched, %d flagged = %.2f %%, emptied %d, largest W / Wn %.2f, largest bound on an unflagged voxel "
                  "%.3e (rgb %.3e)" % (name, weights, what, touched, flagged, 100.0 * flagged / touched, int(s["emptied"].sum()),
                                       s["max_ratio"], s["bound"][un].max(), s["bound_rgb"][un].max()))
            assert touched > 0.5 * s["touched"].size
            assert flagged <= 0.01 * touched
            # the ratios of successive removals telescope to W_before / W_after <= (1 + 4) / 0.25 = 20 with weights in [0.25, 1] (unit and
            # scene weights: <= 1.5 * 5 / 0.5 = 15); tsdf_reference holds the incoming bound below 1e-4 (rgb 1e-3), a removal's own
            # roundings add K_UN EPS (W + w) / Wn <= 5 * 2^-24 * 2 * 20 = 1.2e-5 each (rgb 255 times that)
            assert s["max_ratio"] <= 20.0
            assert s["bound"][un].max() < 20 * 1e-4 + 4 * 1.2e-5 and s["bound_rgb"][un].max() < 20 * 1e-3 + 4 * 255 * 1.2e-5
        assert int(rem["emptied"].sum()) > 20 and int(both["touched"].sum()) > 0


def test_add_only_is_the_integration_reference():
    """the ADD step restates tsdf_reference.integrate_reference: identical values, weights, bounds and flags from an empty state"""
    for name in R.SCENES:
        c = RR.case(name, "scene")
        s = _fused(name, "scene")
        ref = R.integrate_reference(c["dims"], c["origin"], c["voxel"], c["trunc"], c["poses"], c["disps"], c["intr"], range(c["nf"]),
                                    weight=c["weight"], images=c["images"], img_stride=1, img_offset=0)
        for k in ("tsdf", "wsum", "rgb", "bound", "bound_rgb", "touched", "flagged"):
            assert np.array_equal(s[k], ref[k]), (name, k)
        assert s["hits"] == ref["hits"]


# ------------------------------------------------------------------------------------------------ the inverse property
@pytest.mark.parametrize("name", list(R.SCENES))
@pytest.mark.parametrize("weights", ["unit", "scene", "nondyadic"])
def test_removing_b_from_a_and_b_leaves_a(name, weights):
    c = RR.case(name, weights)
    A, B = [c["k"]], c["rest"]
    full = _fused(name, weights)
    inv = RR.run(c, full, remove=B)
    alone = RR.run(c, RR.empty_state(c["dims"]), add=A)
    un = ~inv["flagged"]
    in_a = alone["touched"] & un
    only_b = full["touched"] & ~alone["touched"] & un
    assert in_a.sum() > 100 and only_b.sum() > 20
    # wsum: every fp32 sum or difference is within EPS of its result, a partial sum of at most max(full wsum): nA + nB additions and nB
    # subtractions on one side, nA additions on the other
    k = (len(A) + 2 * len(B)) + len(A)
    dw = np.abs(inv["wsum"].astype(np.float64) - alone["wsum"].astype(np.float64))
    print("%s %s: |wsum - A's| max %.3e (%d EPS max W = %.3e)" % (name, weights, dw[in_a].max(), k, k * RR.EPS * full["wsum"].max()))
    assert np.all(dw[in_a] <= k * RR.EPS * np.float64(full["wsum"].max()))
    if weights in ("unit", "scene"):                   # integers, or multiples of 1/64 below 2^24 / 64: every sum is exact
        assert np.array_equal(inv["wsum"][un], alone["wsum"][un])
    # values: both sides carry their bound against exact arithmetic, and the fp64 evaluation differs from it by far less
    dt = np.abs(inv["tsdf"] - alone["tsdf"])
    dc = np.abs(inv["rgb"] - alone["rgb"]).max(-1)
    lim_t, lim_c = inv["bound"] + alone["bound"], inv["bound_rgb"] + alone["bound_rgb"]
    print("   tsdf max diff %.3e (share of the bound %.3f), rgb max diff %.3e (share %.3f)"
          % (dt[in_a].max(), (dt[in_a] / lim_t[in_a]).max(), dc[in_a].max(), (dc[in_a] / lim_c[in_a]).max()))
    assert np.all(dt[in_a] <= lim_t[in_a]) and np.all(dc[in_a] <= lim_c[in_a])
    # voxels only B touched: bit-for-bit zero with the floor
    for arr in (inv["tsdf"], inv["wsum"], inv["rgb"]):
        assert not np.any(arr[only_b]) and not np.signbit(arr[only_b]).any()
    assert inv["emptied"][only_b].all() and not inv["emptied"][in_a].any()


def test_without_a_floor_removed_voxels_keep_a_residue():
    """why w_floor exists: with weights whose sums are not exact in fp32, W - sum(w) is a few ulps and not 0"""
    c = RR.case("5x24x32", "nondyadic")
    full = _fused("5x24x32", "nondyadic")
    alone = RR.run(c, RR.empty_state(c["dims"]), add=[c["k"]])
    only_b = full["touched"] & ~alone["touched"]
    bare = RR.run(c, full, remove=c["rest"], w_floor=0.0)
    left = only_b & (bare["wsum"] != 0)
    print("w_floor = 0: %d of %d voxels only the removed frames touched keep wsum in [%.1e, %.1e]"
          % (left.sum(), only_b.sum(), bare["wsum"][left].min(), bare["wsum"][left].max()))
    assert left.sum() > 100 and bare["wsum"][left].max() < 1e-5
    floored = RR.run(c, full, remove=c["rest"], w_floor=RR.W_FLOOR)
    assert not floored["wsum"][only_b].any() and not floored["tsdf"][only_b].any()
    assert (floored["wsum"][alone["touched"]] > 0).all()                                     # none of the live voxels is emptied
    # the scene's own weights are multiples of 1/64: exact sums hide the residue
    cs = RR.case("5x24x32", "scene")
    exact = RR.run(cs, _fused("5x24x32", "scene"), remove=cs["rest"], w_floor=0.0)
    assert not exact["wsum"][only_b].any()


# ------------------------------------------------------------------------------------------------ wrong references
def _as_kernel(s):
    """a reference state rounded to what a kernel would hold: fp32 volumes"""
    return s["tsdf"].astype(np.float32), s["wsum"], None if s["rgb"] is None else s["rgb"].astype(np.float32)


@pytest.mark.parametrize("name", list(R.SCENES))
@pytest.mark.parametrize("mutant", RR.MUTANTS)
def test_the_check_rejects_a_wrong_reference(name, mutant):
    """a removal projected with the NEW poses, w ignored in a removal, an emptied voxel left with its last tsdf and wsum, colours not
    de-integrated: each must FAIL the check that the right reference passes"""
    c = RR.case(name, "nondyadic")
    start = _fused(name, "nondyadic")
    kw = dict(remove=[c["k"]], add=[c["k"]], moved=True) if mutant == "new_poses" else dict(remove=c["rest"])
    right = RR.run(c, start, **kw)
    ok, report = RR.state_matches(*_as_kernel(right), right)
    assert ok, report
    wrong = RR.run(c, start, mutant=mutant, **kw)
    ok, report = RR.state_matches(*_as_kernel(right), wrong)
    print(name, mutant, report)
    assert not ok


# ------------------------------------------------------------------------------------------------ the ledger
class _Video:
    """what LiveMap reads of a DepthVideo, on CPU tensors: the analytic scene in a buffer of 8 slots; every pixel with a positive
    depth is kept"""

    def __init__(self, name="3x12x16", images=True):
        from pvo_amd.depth_video import DepthVideo
        c = RR.case(name, "unit")
        nf, (ht, wd) = c["nf"], c["disps"].shape[1:]
        self.device, self.ht, self.wd, self.counter = torch.device("cpu"), 8 * ht, 8 * wd, nf
        self.poses = torch.zeros(8, 7)
        self.poses[:, 6] = 1.0
        self.disps = torch.ones(8, ht, wd)
        self.poses[:nf], self.disps[:nf] = torch.from_numpy(c["poses"]), torch.from_numpy(c["disps"])
        self.intrinsics = torch.from_numpy(c["intr"])[None].repeat(8, 1)
        self.tstamp = torch.arange(8, dtype=torch.float32) * 3.0
        self.images = None
        if images:
            self.images = torch.zeros(8, 3, 8 * ht, 8 * wd, dtype=torch.uint8)
            self.images[:nf, :, 3::8, 3::8] = torch.from_numpy(c["images"])
        self.fusion_weights = DepthVideo.fusion_weights
        self.map_calls = 0

    def map_points(self, ix, thresh, reject=None):
        self.map_calls += 1
        ok = self.disps[ix] > 0
        f, p = torch.nonzero(ok.flatten(1), as_tuple=True)
        return {"src": torch.stack([ix[f], p], 1)}


def _reference_call(calls):
    """droid_backends.tsdf_reintegrate's signature on CPU tensors, through the numpy reference"""
    def call(tsdf, wsum, rgb, origin, voxel, trunc, intrinsics, remove=None, add=None, images=None, img_stride=8, img_offset=3,
             z_near=0.0, w_max=0.0, w_floor=2.0 ** -10, workspace=None):
        st = RR.empty_state(tuple(tsdf.shape), rgb is not None)
        st.update(tsdf=tsdf.numpy().astype(np.float64), wsum=wsum.numpy().copy())
        if rgb is not None:
            st["rgb"] = rgb.numpy().astype(np.float64)
        sets = [None if s is None else (s[0].numpy(), s[1].numpy(), s[2].numpy(), None if s[3] is None else s[3].numpy()) for s in (remove, add)]
        calls.append(([] if remove is None else remove[2].tolist(), [] if add is None else add[2].tolist()))
        out = RR.reintegrate_reference(st, origin, voxel, trunc, intrinsics.numpy(), remove=sets[0], add=sets[1],
                                       images=None if images is None else images.numpy(), img_stride=img_stride, img_offset=img_offset,
                                       z_near=z_near, w_max=w_max, w_floor=w_floor)
        tsdf.copy_(torch.from_numpy(out["tsdf"].astype(np.float32)))
        wsum.copy_(torch.from_numpy(out["wsum"]))
        if rgb is not None:
            rgb.copy_(torch.from_numpy(out["rgb"].astype(np.float32)))
    return call


def test_live_map_ledger_on_cpu_tensors(monkeypatch):
    from pvo_amd import live_map
    calls = []
    monkeypatch.setattr(live_map.db, "tsdf_reintegrate", _reference_call(calls))
    c = RR.case("3x12x16", "unit")
    v = _Video()
    lm = live_map.LiveMap(v, c["voxel"], c["origin"], c["dims"], trunc=c["trunc"], lag=1)
    assert lm.rgb is not None and tuple(lm.tsdf.shape) == c["dims"] and lm.lag == 1
    # the youngest keyframe (lag 1) waits; the others are new
    assert lm.update() == (2, 0, 0) and calls[-1] == ([], [0, 1]) and lm.fused == {0: 0.0, 1: 3.0}
    assert torch.equal(lm.poses_fused[:2], v.poses[:2]) and torch.equal(lm.disps_fused[:2], v.disps[:2])
    assert torch.equal(lm.weight_fused[:2], torch.ones_like(v.disps[:2])) and not lm.weight_fused[2:].any()
    ref = RR.reintegrate_reference(RR.empty_state(c["dims"]), c["origin"], c["voxel"], c["trunc"], c["intr"],
                                   add=(c["poses"], c["disps"], [0, 1], None), images=c["images"], img_stride=1, img_offset=0)
    assert np.array_equal(lm.wsum.numpy(), ref["wsum"]) and np.allclose(lm.tsdf.numpy(), ref["tsdf"], atol=1e-6)
    assert np.allclose(lm.rgb.numpy(), ref["rgb"], atol=1e-3)                                # colours from [3::8, 3::8]
    # nothing moved: nothing to do, no native call, drift zero
    n_calls = len(calls)
    assert lm.update() == (0, 0, 0) and len(calls) == n_calls
    assert lm.drift([0, 1]).tolist() == [0.0, 0.0]
    assert lm.update(upto=3) == (1, 0, 0) and calls[-1] == ([], [2])
    # keyframe 1 pushed by a voxel along x (camera frame): about one voxel of drift, the others none; exactly one refresh
    before = v.poses[1].clone()
    v.poses[1, 0] += c["voxel"]
    d = lm.drift([0, 1, 2])
    print("drift after a push by one voxel:", d.tolist())
    assert d[0] == 0 and d[2] == 0 and abs(d[1].item() - 1.0) < 1e-3
    assert lm.update(upto=3) == (0, 1, 0) and calls[-1] == ([1], [1])
    assert torch.equal(lm.poses_fused[1], v.poses[1]) and lm.drift([1]).item() == 0.0        # the snapshot follows
    v.poses[1] = before
    assert lm.update(upto=3) == (0, 1, 0) and lm.refreshed_total == 2
    # below the tolerance nothing happens unless forced
    v.poses[1, 0] += 0.1 * c["voxel"]
    assert lm.update(upto=3) == (0, 0, 0) and lm.update(upto=3, force=True) == (0, 3, 0) and calls[-1] == ([0, 1, 2], [0, 1, 2])
    # a pixel kept in only one of the two counts as trunc
    v.disps[2, 0, 0] = 0.0
    lone = lm.drift([2]).item()
    assert abs(lone - np.sqrt(c["trunc"] ** 2 / (12 * 16)) / c["voxel"]) < 1e-4
    v.disps[2, 0, 0] = lm.disps_fused[2, 0, 0]
    # keyframe 1 leaves the window: the slots behind it shift, their time stamps no longer match
    v.poses[1], v.disps[1], v.tstamp[1], v.images[1] = v.poses[2].clone(), v.disps[2].clone(), v.tstamp[2].clone(), v.images[2].clone()
    v.counter = 2
    assert lm.update(upto=2, force=False) == (0, 0, 2) and calls[-1] == ([1, 2], [1])
    assert lm.fused == {0: 0.0, 1: 6.0}
    # the volume is what fusing the remaining two keyframes from scratch gives, up to the removals' roundings
    ref = RR.reintegrate_reference(RR.empty_state(c["dims"]), c["origin"], c["voxel"], c["trunc"], c["intr"],
                                   add=(v.poses.numpy(), v.disps.numpy(), [0, 1], None), images=c["images"][[0, 2, 2]], img_stride=1,
                                   img_offset=0)
    assert np.array_equal(lm.wsum.numpy(), ref["wsum"])                                      # unit weights: exact
    assert np.abs(lm.tsdf.numpy() - ref["tsdf"]).max() < 1e-4
    vol = lm.as_volume()
    assert set(vol) == {"tsdf", "wsum", "rgb", "origin", "voxel"} and vol["tsdf"] is lm.tsdf and vol["voxel"] == c["voxel"]


def test_live_map_refuses_a_floor_at_or_above_min_weight():
    from pvo_amd.live_map import LiveMap
    v = _Video(images=False)
    with pytest.raises(ValueError, match="w_floor"):
        LiveMap(v, 0.1, (0, 0, 0), (4, 4, 4), w_floor=1.0, min_weight=1.0)
    with pytest.raises(ValueError, match="w_floor"):
        LiveMap(v, 0.1, (0, 0, 0), (4, 4, 4), w_floor=0.5, min_weight=0.25)
    lm = LiveMap(v, 0.1, (0, 0, 0), (4, 4, 4), w_floor=0.5, min_weight=1.0)
    assert lm.rgb is None and lm.trunc == pytest.approx(0.3) and lm.lag == 25 and lm.update(upto=0) == (0, 0, 0)


def test_droid_refuses_live_map_with_pipelined_and_brick_labels_are_refused():
    from pvo_amd.droid import Droid, default_args
    assert default_args().live_map is None
    with pytest.raises(ValueError, match="pipelined"):
        Droid(default_args(device="cpu", pipelined=True, live_map=dict(voxel=0.1, origin=(0, 0, 0), dims=(8, 8, 8))))
    from pvo_amd.tsdf_sparse import SparseTSDF
    vol = SparseTSDF((0, 0, 0), (1, 1, 1), 0.1, 0.3, colours=False, device="cpu", cap=1, labels=True)
    with pytest.raises(ValueError, match="cannot be inverted"):
        vol.reintegrate(torch.zeros(4))


def test_export_tool_takes_the_live_map_options_and_is_unchanged_without_them():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_map
    base = ["--datapath", "x", "--map", "a.ply"]
    a = export_map.parse_args(base)
    assert a.live_map is None
    a = export_map.parse_args(base + ["--live_map", "live.ply", "--voxel", "0.05", "--origin", "-1", "-0.5", "0.5", "--dims", "64", "48", "80"])
    assert a.live_map == "live.ply" and a.origin == [-1.0, -0.5, 0.5] and a.dims == [64, 48, 80] and a.sparse is False
    for bad in (["--live_map", "l.ply"], ["--live_map", "l.ply", "--voxel", "0.05"],
                ["--live_map", "l.ply", "--voxel", "0.05", "--origin", "0", "0", "0"]):
        with pytest.raises(SystemExit):
            export_map.parse_args(base + bad)
