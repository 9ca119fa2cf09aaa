"""The brick volume, the parts that need no GPU: the C boundary of pvo_tsdf_sparse_allocate / _integrate / _mesh (symbols, struct
layouts, argument validation - every argument is checked before anything touches the device, so fake pointers are enough), the
properties of the numpy yardstick (tests/tsdf_sparse_reference.py) that the GPU tests rely on, and SparseTSDF's growth logic with the
native calls stubbed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import tsdf_reference as R
import tsdf_sparse_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PVO_OK, PVO_EINVAL, PVO_EWORKSPACE = 0, 1, 3
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced: every call below returns before a launch
CALLS = ("allocate", "integrate", "mesh")


def _lib():
    from pvo_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.startswith("pvo_tsdf") or name == "pvo_version":
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib, _lib


def test_symbols_struct_layouts_and_abi_version(tmp_path):
    lib, L = _lib()
    assert lib.pvo_version() == 106 == L.PVO_ABI_VERSION
    structs = {"allocate": L.TsdfSparseAllocateArgs, "integrate": L.TsdfSparseIntegrateArgs, "mesh": L.TsdfSparseMeshArgs}
    lines = ['  printf("%d\\n", PVO_TSDF_BRICK);']
    want = [L.TSDF_BRICK]
    for call in CALLS:
        S = structs[call]
        lines.append('  printf("%%zu\\n", sizeof(pvo_tsdf_sparse_%s_args));' % call)
        want.append(ctypes.sizeof(S))
        for name, _ in S._fields_:                                   # every field, so also the order
            lines.append('  printf("%%zu\\n", offsetof(pvo_tsdf_sparse_%s_args, %s));' % (call, name))
            want.append(getattr(S, name).offset)
        assert getattr(lib, "pvo_tsdf_sparse_%s_args_size" % call)() == ctypes.sizeof(S)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pvo_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == want
    assert L.TSDF_BRICK == 8 == SR.BRICK
    # workspaces: a byte per brick of the grid (+ twelve per 256, + the slots' constants); five bytes per pool voxel
    G = 40 * 50 * 60
    assert G + 64 * 7 <= lib.pvo_tsdf_sparse_allocate_workspace_bytes(40, 50, 60, 7) <= 1.06 * G + 64 * 7 + 2048
    assert lib.pvo_tsdf_sparse_allocate_workspace_bytes(0, 50, 60, 7) == 0 and lib.pvo_tsdf_sparse_allocate_workspace_bytes(4, 5, 6, 0) == 0
    assert lib.pvo_tsdf_sparse_integrate_workspace_bytes(0) == 0 and 64 * 64 <= lib.pvo_tsdf_sparse_integrate_workspace_bytes(64) <= 64 * 64 + 256
    assert lib.pvo_tsdf_sparse_mesh_workspace_bytes(0) == 0
    assert 5 * 512 * 1000 <= lib.pvo_tsdf_sparse_mesh_workspace_bytes(1000) < 5.1 * 512 * 1000


def _args(L, call, **kw):
    a = {"allocate": L.TsdfSparseAllocateArgs, "integrate": L.TsdfSparseIntegrateArgs, "mesh": L.TsdfSparseMeshArgs}[call]()
    for name, ctype in a._fields_:
        if ctype is ctypes.c_void_p and name not in ("rgb", "weight", "images", "normals", "rgba"):
            setattr(a, name, FAKE)
    a.gz, a.gy, a.gx, a.cap, a.voxel = 2, 3, 4, 16, 0.1
    if call == "mesh":
        a.min_weight, a.vcap, a.fcap = 1.0, 16, 32
    else:
        a.trunc, a.N, a.nframes, a.ht, a.wd = 0.3, 2, 2, 8, 8
    if call == "allocate":
        a.margin = 2.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _call(lib, call, a, ws=FAKE, n=1 << 24):
    return getattr(lib, "pvo_tsdf_sparse_" + call)(ctypes.byref(a) if a is not None else None, ws, n, None)


@pytest.mark.parametrize("call", CALLS)
def test_the_grid_limits_and_scalars_are_validated_before_the_device_is_touched(call):
    lib, L = _lib()
    assert _call(lib, call, None) == PVO_EINVAL
    for bad in (dict(gz=-1), dict(cap=-1), dict(gx=(1 << 18) + 1),                           # 8 gx > 2^21
                dict(gz=1 << 11, gy=1 << 10, gx=1 << 10),                                    # gz*gy*gx = 2^31
                dict(cap=1 << 22),                                                           # cap*512 = 2^31
                dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=float("nan")), dict(voxel=float("inf")),
                dict(origin=(0.0, float("nan"), 0.0)), dict(origin=(float("inf"), 0.0, 0.0))):
        assert _call(lib, call, _args(L, call, **bad)) == PVO_EINVAL, bad
    assert _call(lib, call, _args(L, call, gz=1 << 10, gy=1 << 10, gx=(1 << 11) - 1), None, 0) == PVO_EWORKSPACE    # just below: valid
    for name in ("coord", "bricks"):
        assert _call(lib, call, _args(L, call, **{name: None})) == PVO_EINVAL, name
    need = {"allocate": lib.pvo_tsdf_sparse_allocate_workspace_bytes(2, 3, 4, 2), "integrate": lib.pvo_tsdf_sparse_integrate_workspace_bytes(2),
            "mesh": lib.pvo_tsdf_sparse_mesh_workspace_bytes(16)}[call]
    assert need > 0
    assert _call(lib, call, _args(L, call), FAKE, need - 1) == PVO_EWORKSPACE and _call(lib, call, _args(L, call), None, need) == PVO_EWORKSPACE
    assert _call(lib, call, _args(L, call), FAKE + 4, need + 16) == PVO_EINVAL                # a misaligned workspace


def test_allocate_validates_its_own_arguments():
    lib, L = _lib()
    call = lambda **kw: _call(lib, "allocate", _args(L, "allocate", **kw))
    for name in ("grid", "poses", "disps", "intrinsics", "ix"):
        assert call(**{name: None}) == PVO_EINVAL, name
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert call(trunc=bad) == PVO_EINVAL
    assert call(trunc=500.0) == PVO_EINVAL                                                    # trunc / voxel > 4096
    assert call(z_near=-1.0) == PVO_EINVAL and call(z_near=float("nan")) == PVO_EINVAL
    for bad in (-0.5, 8.5, float("nan")):
        assert call(margin=bad) == PVO_EINVAL
    assert call(N=-1) == PVO_EINVAL and call(ht=1 << 16, wd=1 << 15) == PVO_EINVAL
    assert call(N=0) == PVO_OK and call(gx=0) == PVO_OK and call(ht=0) == PVO_OK              # nothing to mark: no launch
    assert call(cap=0, coord=None, N=0) == PVO_OK


def test_integrate_validates_its_own_arguments():
    lib, L = _lib()
    call = lambda **kw: _call(lib, "integrate", _args(L, "integrate", **kw))
    for name in ("tsdf", "wsum", "poses", "disps", "intrinsics", "ix"):
        assert call(**{name: None}) == PVO_EINVAL, name
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert call(trunc=bad) == PVO_EINVAL
    assert call(z_near=-1.0) == PVO_EINVAL and call(w_max=-1.0) == PVO_EINVAL and call(w_max=float("inf")) == PVO_EINVAL
    assert call(rgb=FAKE) == PVO_EINVAL                                                       # a colour pool without images
    img = dict(images=FAKE, IH=64, IW=64, img_stride=8, img_offset=3)
    assert call(**dict(img, img_stride=9)) == PVO_EINVAL and call(**dict(img, img_offset=8)) == PVO_EINVAL
    assert call(**dict(img, img_stride=0)) == PVO_EINVAL and call(**dict(img, IW=59)) == PVO_EINVAL
    assert _call(lib, "integrate", _args(L, "integrate", **img), FAKE, 8) == PVO_EWORKSPACE   # everything else in order
    assert call(N=0) == PVO_OK and call(cap=0) == PVO_OK and call(wd=0) == PVO_OK             # nothing to fuse: no launch


def test_mesh_validates_its_own_arguments():
    lib, L = _lib()
    call = lambda **kw: _call(lib, "mesh", _args(L, "mesh", **kw))
    for name in ("grid", "tsdf", "wsum", "counts", "verts", "faces"):
        assert call(**{name: None}) == PVO_EINVAL, name
    assert call(min_weight=float("nan")) == PVO_EINVAL and call(vcap=-1) == PVO_EINVAL and call(fcap=-1) == PVO_EINVAL
    assert call(rgba=FAKE + 1) == PVO_EINVAL                                                  # misaligned
    assert _call(lib, "mesh", _args(L, "mesh", vcap=0, fcap=0, verts=None, faces=None), FAKE, 8) == PVO_EWORKSPACE


# ------------------------------------------------------------------------------------------------ the yardstick
_marks = {}


def _marked(name):
    if name not in _marks:
        nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES[name]
        (poses, disps, intr, images, weight, hit), ix = SR.scene(name)
        _marks[name] = SR.mark_reference(gdims, origin, voxel, trunc, poses, disps, intr, ix, weight=weight, margin=2.0)
    return _marks[name]


@pytest.mark.parametrize("name", list(SR.SCENES))
def test_must_covers_the_observed_surface_and_may_is_barely_larger(name):
    """margin = 2: a voxel that some frame projects into its image at a valid pixel whose depth is within trunc of the voxel's, and
    that lies within trunc of the true surface, is at most half a pixel (< 1 voxel on these scenes) beside that pixel's ray and half a
    sample spacing (1 voxel) of depth from a sample, so within 2 voxels of it on every axis: its brick holds a corner's brick index."""
    nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES[name]
    (poses, disps, intr, images, weight, hit), ix = SR.scene(name)
    must, may = _marked(name)
    assert must.any() and not (must & ~may).any()
    extra = int((may & ~must).sum())
    print("%s: %d of %d bricks must, %d may only" % (name, must.sum(), must.size, extra))
    assert extra <= 0.02 * must.sum()
    gz, gy, gx = gdims
    dims = (8 * gz, 8 * gy, 8 * gx)
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in dims], indexing="ij")
    X = np.asarray(origin, np.float32).astype(np.float64) + np.float64(np.float32(voxel)) * np.stack([xx, yy, zz], -1)
    near = R.surface_distance(X.reshape(-1, 3)).reshape(dims) <= trunc
    seen = np.zeros(dims, bool)
    fx, fy, cx, cy = [np.float64(v) for v in intr]
    for f in range(nf):
        Xc = X @ R.rotation(poses[f, 3:]).T + poses[f, :3].astype(np.float64)
        zc = Xc[..., 2]
        with np.errstate(all="ignore"):
            ui, vi = np.floor(fx * Xc[..., 0] / zc + cx + 0.5), np.floor(fy * Xc[..., 1] / zc + cy + 0.5)
        ok = (zc > 0) & (ui >= 0) & (ui < wd) & (vi >= 0) & (vi < ht)
        d = disps[f][np.where(ok, vi, 0).astype(int), np.where(ok, ui, 0).astype(int)].astype(np.float64)
        seen |= ok & (np.abs(1.0 / d - zc) <= trunc)
    want = (near & seen).reshape(gz, 8, gy, 8, gx, 8).any((1, 3, 5))
    print("   %d bricks hold an observed voxel within trunc of the surface" % want.sum())
    assert want.sum() >= 2 and not (want & ~must).any()
    assert not must.all() or name != "5x24x32"                        # the large world is not all surface


def test_marks_follow_margin_z_near_validity_and_ids():
    name = "3x12x16"
    nf, ht, wd, gdims, origin, voxel, trunc = SR.SCENES[name]
    (poses, disps, intr, images, weight, hit), ix = SR.scene(name)
    run = lambda **kw: SR.mark_reference(gdims, origin, voxel, trunc, poses, kw.pop("disps", disps), intr, kw.pop("ix", ix), **kw)[0]
    base = run(margin=2.0)
    assert np.array_equal(base, run(margin=2.0, ix=[0, 1, 2])) and not run(ix=[nf, -1, nf + 1]).any()     # the frame that looks away
    assert not (run(margin=0.0) & ~base).any() and not (base & ~run(margin=8.0)).any()
    dead = disps.copy()
    dead[:nf] = np.nan
    assert not run(disps=dead).any()
    assert not run(z_near=50.0).any()                                 # hi < lo on every ray


def test_slot_assignment_and_layout_round_trip():
    rng = np.random.default_rng(3)
    marked = rng.random((3, 4, 5)) < 0.4
    grid, coord = SR.assign_slots(marked)
    n = int(marked.sum())
    assert coord.shape == (n, 3) and np.array_equal(np.sort(grid[marked]), np.arange(n)) and (grid[~marked] == -1).all()
    assert np.array_equal(coord, np.argwhere(marked)) and all(grid[tuple(c)] == k for k, c in enumerate(coord))
    more = marked | (rng.random(marked.shape) < 0.3)
    grid2, coord2 = SR.assign_slots(more, grid)
    assert np.array_equal(grid2[marked], grid[marked]) and np.array_equal(coord2[:n], coord)
    assert np.array_equal(coord2[n:], np.argwhere(more & ~marked))
    pool = rng.standard_normal((len(coord2), 8, 8, 8, 3)).astype(np.float32)
    dense = SR.to_dense(pool, coord2, marked.shape)
    assert dense.shape == (24, 32, 40, 3) and np.array_equal(SR.to_bricks(dense, coord2), pool)
    bz, by, bx = coord2[5]
    assert np.array_equal(dense[8 * bz + 3, 8 * by + 1, 8 * bx + 6], pool[5, 3, 1, 6])
    assert np.array_equal(SR.voxel_mask(more), np.abs(SR.to_dense(np.ones((len(coord2), 8, 8, 8)), coord2, marked.shape)) > 0)


# ------------------------------------------------------------------------------------------------ SparseTSDF
def test_sparse_tsdf_grows_its_pool_on_overflow(monkeypatch):
    """the native allocate stubbed by the appending rule on CPU tensors: counts is read once, the pool doubled by copy until it fits,
    the call repeated once; the contents and the one-shot grid / coord survive"""
    from pvo_amd import tsdf_sparse as TS
    rng = np.random.default_rng(5)
    marked = rng.random((3, 4, 5)) < 0.5                              # about 30 bricks
    calls = []

    def fake_allocate(vol, poses, disps, intrinsics, ix, trunc, weight=None, z_near=0.0, margin=2.0):
        cap = vol["tsdf"].shape[0]
        calls.append(cap)
        grid, coord = SR.assign_slots(marked, vol["grid"].numpy())
        grid[grid >= cap] = -1
        vol["grid"].copy_(torch.from_numpy(grid))
        k = min(cap, len(coord))
        vol["coord"][:k] = torch.from_numpy(coord[:k])
        vol["counts"][0] = len(coord)

    monkeypatch.setattr(TS.db, "tsdf_sparse_allocate", fake_allocate)
    n = int(marked.sum())
    vol = TS.SparseTSDF((0.0, 0.0, 0.0), (3, 4, 5), 0.1, 0.3, colours=True, device="cpu", cap=4)
    assert vol.cap == 4 and vol.bricks == 0 and (vol.grid == -1).all()
    vol.tsdf[:] = 7.0                                                 # contents that the growth must keep
    assert vol.allocate(None, None, None, None) == n
    assert calls == [4, vol.cap] and vol.cap >= n and vol.cap < 2 * n and vol.cap % 4 == 0 and vol.bricks == n
    want_grid, want_coord = SR.assign_slots(marked)
    assert np.array_equal(vol.grid.numpy(), want_grid) and np.array_equal(vol.coord[:n].numpy(), want_coord)
    assert bool((vol.tsdf[:4] == 7.0).all()) and not vol.tsdf[4:].any() and vol.rgb.shape == (vol.cap, 8, 8, 8, 3)
    assert vol.allocate(None, None, None, None) == n and calls == [4, vol.cap, vol.cap]       # fits: one call
    dense = vol.to_dense()
    assert dense["tsdf"].shape == (24, 32, 40) and dense["rgb"].shape == (24, 32, 40, 3)
    assert np.array_equal(dense["allocated"].numpy(), marked)
    first = want_coord[0]
    assert dense["tsdf"][8 * first[0], 8 * first[1], 8 * first[2]] == 7.0
    assert vol.nbytes() == vol.cap * 512 * 20 + vol.cap * 12 + 60 * 4 + 4
    with pytest.raises(ValueError):
        TS.SparseTSDF((0, 0, 0), (1 << 11, 1 << 10, 1 << 10), 0.1, 0.3, device="cpu")
    with pytest.raises(ValueError):
        TS.SparseTSDF((0, 0, 0), (1, 1, (1 << 18) + 1), 0.1, 0.3, device="cpu")
