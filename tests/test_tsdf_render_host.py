"""Rendering a TSDF volume, the parts that need no GPU: the C boundary of pvo_tsdf_render / pvo_tsdf_sparse_render (symbols, both
structs' layouts against gcc, every PVO_EINVAL case before anything touches the device - fake pointers are enough), and the properties of
the numpy yardstick (tests/tsdf_render_reference.py) that the GPU tests rely on: few flagged pixels, bounds that four wrong variants
fail, the fused analytic scene's render against the closed forms, the label image, and DepthVideo.depth_residual on hand-made tensors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import tsdf_reference as R
import tsdf_sparse_reference as SR
import tsdf_render_reference as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PVO_OK, PVO_EINVAL, PVO_EWORKSPACE = 0, 1, 3
FAKE = 0x1000          # a non-NULL pointer that is never dereferenced: every call below returns before a launch
OPTIONAL = ("rgb", "label", "normal", "rgba", "out_label", "visited")
SPHERE_ID, PLANE_ID = (1 << 25) + 3, (1 << 24) + 5


def _lib():
    from pvo_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.startswith("pvo_tsdf") or name == "pvo_version":
            fn = getattr(lib, name)                                  # AttributeError without the feature
            fn.restype, fn.argtypes = res, args
    return lib, _lib


# ------------------------------------------------------------------------------------------------ the C boundary
def test_symbols_struct_layouts_and_abi_version(tmp_path):
    lib, L = _lib()
    assert lib.pvo_version() == 106 == L.PVO_ABI_VERSION
    for name in ("pvo_tsdf_render_args_size", "pvo_tsdf_render_workspace_bytes", "pvo_tsdf_render", "pvo_tsdf_sparse_render_args_size",
                 "pvo_tsdf_sparse_render_workspace_bytes", "pvo_tsdf_sparse_render"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    lines, want = [], []
    for cname, S in (("pvo_tsdf_render_args", L.TsdfRenderArgs), ("pvo_tsdf_sparse_render_args", L.TsdfSparseRenderArgs)):
        lines.append('  printf("%%zu\\n", sizeof(%s));' % cname)
        want.append(ctypes.sizeof(S))
        for name, _ in S._fields_:                                   # every field, so also the order
            lines.append('  printf("%%zu\\n", offsetof(%s, %s));' % (cname, name))
            want.append(getattr(S, name).offset)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pvo_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == want
    assert lib.pvo_tsdf_render_args_size() == ctypes.sizeof(L.TsdfRenderArgs) == 160
    assert lib.pvo_tsdf_sparse_render_args_size() == ctypes.sizeof(L.TsdfSparseRenderArgs) == 176
    for n in (0, -3):
        assert lib.pvo_tsdf_render_workspace_bytes(n) == 0 == lib.pvo_tsdf_sparse_render_workspace_bytes(n)
    for n in (1, 5, 64, 1000):
        need = lib.pvo_tsdf_render_workspace_bytes(n)
        assert need >= 64 * n and need % 256 == 0 and need == lib.pvo_tsdf_sparse_render_workspace_bytes(n)


def _args(L, sparse, **kw):
    a = (L.TsdfSparseRenderArgs if sparse else L.TsdfRenderArgs)()
    for name, ctype in a._fields_:
        if ctype is ctypes.c_void_p and name not in OPTIONAL:
            setattr(a, name, FAKE)
    if sparse:
        a.gz, a.gy, a.gx, a.cap = 2, 3, 4, 16
    else:
        a.nz, a.ny, a.nx = 5, 6, 7
    a.voxel, a.min_weight, a.N, a.nviews, a.ht, a.wd = 0.1, 1.0, 2, 2, 24, 32
    a.z_near, a.z_far, a.dz = 0.0, 3.0, 0.05
    for k, v in kw.items():
        if k == "origin":
            a.origin[0], a.origin[1], a.origin[2] = v
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
def test_render_validates_before_touching_the_device(sparse):
    lib, L = _lib()
    fn = lib.pvo_tsdf_sparse_render if sparse else lib.pvo_tsdf_render
    need = (lib.pvo_tsdf_sparse_render_workspace_bytes if sparse else lib.pvo_tsdf_render_workspace_bytes)(2)
    call = lambda a, ws=FAKE, n=1 << 24: fn(ctypes.byref(a) if a is not None else None, ws, n, None)
    inf, nan = float("inf"), float("nan")
    assert call(None) == PVO_EINVAL
    bad = [dict(voxel=0.0), dict(voxel=-0.1), dict(voxel=inf), dict(voxel=nan), dict(min_weight=nan), dict(origin=(0.0, inf, 0.0)),
           dict(origin=(nan, 0.0, 0.0)), dict(N=-1), dict(nviews=-1), dict(ht=-1), dict(wd=-2), dict(ht=65536, wd=32768),
           dict(dz=0.0), dict(dz=-0.05), dict(dz=nan), dict(dz=inf), dict(z_near=-0.1), dict(z_near=nan), dict(z_far=0.0), dict(z_far=inf),
           dict(z_near=1.0, z_far=1.0), dict(z_near=2.0, z_far=1.0), dict(z_far=nan),
           dict(z_far=3500.0),                                       # 70000 samples of 0.05: over the 65536 of a pixel's loop
           dict(dz=1.0, z_near=4194300.0, z_far=4194304.0),          # few samples, but z_far / dz = 2^22
           dict(rgba=FAKE + 2), dict(rgba=FAKE + 1), dict(out_label=FAKE),                        # an id image without a label volume
           dict(depth=None), dict(poses=None), dict(intrinsics=None), dict(ix=None), dict(tsdf=None), dict(wsum=None)]
    if sparse:
        bad += [dict(gz=-1), dict(gx=(1 << 18) + 1), dict(gz=2048, gy=2048, gx=2048), dict(cap=-1), dict(cap=1 << 22), dict(grid=None)]
    else:
        bad += [dict(nz=-1), dict(nx=-5), dict(nz=2048, ny=2048, nx=2048), dict(nz=65536, ny=65536, nx=1)]
    for kw in bad:
        assert call(_args(L, sparse, **kw)) == PVO_EINVAL, kw
    # limits that are NOT over: exactly 65536 samples; every optional pointer given
    ok_args = [dict(dz=0.03125, z_near=0.0, z_far=2048.0), dict(rgb=FAKE, label=FAKE, normal=FAKE, rgba=FAKE + 4, out_label=FAKE, visited=FAKE)]
    for kw in ok_args:                                               # ... they get as far as the workspace check
        assert call(_args(L, sparse, **kw), FAKE, need - 1) == PVO_EWORKSPACE, kw
    good = _args(L, sparse)
    assert call(good, FAKE, need - 1) == PVO_EWORKSPACE and call(good, None, need) == PVO_EWORKSPACE
    assert call(good, FAKE + 4, need) == PVO_EINVAL                  # a misaligned workspace
    # no pixel: PVO_OK, whatever the pointers are - but never with a bad scalar
    empty = (L.TsdfSparseRenderArgs if sparse else L.TsdfRenderArgs)()
    for kw in (dict(N=0), dict(ht=0), dict(wd=0)):
        assert call(_args(L, sparse, **kw), None, 0) == PVO_OK, kw
        assert call(_args(L, sparse, depth=None, tsdf=None, poses=None, **kw), None, 0) == PVO_OK, kw
        assert call(_args(L, sparse, dz=0.0, **kw), None, 0) == PVO_EINVAL, kw
    assert call(empty) == PVO_EINVAL                                 # (voxel = 0)
    # an empty volume still needs somewhere to write its misses
    none = dict(cap=0) if sparse else dict(nz=1)
    assert call(_args(L, sparse, depth=None, **none)) == PVO_EINVAL


# ------------------------------------------------------------------------------------------------ the yardstick
_cache = {}


def _volume(name):
    """the reference's fused volume of a scene (fp32, as a kernel would hold it) with analytic labels, and the scene"""
    if name not in _cache:
        nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
        poses, disps, intr, images, weight, hit = R.scene(nf, ht, wd)
        vol = R.integrate_reference(dims, origin, voxel, trunc, poses, disps, intr, range(nf), weight=weight, images=images, img_stride=1,
                                    img_offset=0)
        lab = V.analytic_labels(dims, origin, voxel, SPHERE_ID, PLANE_ID)
        _cache[name] = (vol["tsdf"].astype(np.float32), vol["wsum"], vol["rgb"].astype(np.float32), lab, poses)
    return _cache[name]


def _render(name, which, mutant=None, **kw):
    key = (name, which, mutant) + tuple(sorted(kw.items()))
    if key not in _cache:
        nf, _, _, dims, origin, voxel, trunc = R.SCENES[name]
        tsdf, wsum, rgb, lab, poses = _volume(name)
        if which == "own":
            views, (ht, wd) = poses, V.OWN_SIZE
        else:
            views, (ht, wd) = V.extra_views(poses), V.EXTRA_SIZE
        args = dict(dz=V.DZ_FACTOR * voxel, z_near=0.0, z_far=2.6)
        args.update(kw)
        _cache[key] = V.render_reference(tsdf, wsum, rgb, lab, origin, voxel, views, V.view_intrinsics(ht, wd), range(len(views)), ht, wd,
                                         mutant=mutant, **args)
    return _cache[key]


@pytest.mark.parametrize("name", list(R.SCENES))
def test_few_pixels_are_flagged(name):
    """THE CONDITION of the GPU comparison, on the reference alone: pooled over a scene's views at most 1 % of the pixels are flagged"""
    own, extra = _render(name, "own"), _render(name, "extra")
    flagged = own["flagged"].sum() + extra["flagged"].sum()
    pixels = own["flagged"].size + extra["flagged"].size
    print("%s: %d of %d pixels flagged (%.4f), %d + %d hits" % (name, flagged, pixels, flagged / pixels, own["hit"].sum(), extra["hit"][0].sum()))
    assert flagged <= 0.01 * pixels
    assert own["hit"].mean() > 0.15 and extra["hit"][0].mean() > 0.15                       # there is something to compare
    assert not extra["hit"][1].any() and not extra["hit"][2].any()                          # looking away; starting inside the sphere
    assert not extra["label"][1:].any() and not extra["depth"][1:].any()


@pytest.mark.parametrize("name", list(R.SCENES))
def test_the_reference_matches_itself_and_rejects_wrong_variants(name):
    ref = _render(name, "own")
    ok, report = V.render_matches(V.as_got(ref), ref)
    assert ok, report
    for mutant in V.MUTANTS:
        ok, report = V.render_matches(V.as_got(_render(name, "own", mutant=mutant)), ref)
        print(name, mutant, report)
        assert not ok, mutant


def test_the_lattice_is_global():
    """z_near moves no sample: with z_near inside the range the depths of the pixels hit in both renders are EQUAL, and a ray whose first
    valid sample is already inside becomes a miss"""
    name = "3x12x16"
    a, b = _render(name, "own"), _render(name, "own", z_near=1.31)
    both = a["hit"] & b["hit"]
    assert both.sum() > 100 and np.array_equal(a["depth"][both], b["depth"][both])
    assert (a["hit"] & ~b["hit"]).sum() > 20 and not (b["hit"] & ~a["hit"]).any()           # the sphere (nearer than 1.31) is cut away
    assert V.lattice(1.31, 2.6, 0.072) == (19, 36) and V.lattice(0.0, 2.6, 0.05) == (0, 51)  # (2.6 / 0.05 rounds below 52 in fp32)


def test_render_of_the_fused_analytic_scene_against_the_closed_forms():
    """the reference's render of the reference's fused volume at the scene's own poses: depth against 1/disps' closed form, normals
    against the plane's and the sphere's.  The maxima are what ANALYTIC_DEPTH_ERR / ANALYTIC_NORMAL_ERR record."""
    name = "5x24x32"
    nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]                                   # at the size the keyframes have: the system test's
    tsdf, wsum, rgb, lab, poses = _volume(name)
    ref = V.render_reference(tsdf, wsum, rgb, lab, origin, voxel, poses, V.view_intrinsics(ht, wd), range(nf), ht, wd, 0.5 * voxel, 0.0, 2.6)
    assert ref["flagged"].mean() <= 0.01
    worst_d = worst_n = mean_d = 0.0
    for k in range(len(poses)):
        depth, normal, sphere = V.analytic_view(poses[k], V.view_intrinsics(ht, wd), ht, wd)
        ok = V.interior(sphere) & ref["hit"][k]
        ed = np.abs(ref["depth"][k] - depth)[ok]
        en = np.abs(ref["normal"][k] - normal).max(-1)[ok]
        print("view %d: %d pixels (%d on the sphere), depth error max %.4f mean %.4f, normal error max %.4f mean %.4f"
              % (k, ok.sum(), (ok & sphere).sum(), ed.max(), ed.mean(), en.max(), en.mean()))
        assert ok.sum() > 100 and (ok & sphere).sum() >= 25
        worst_d, worst_n, mean_d = max(worst_d, ed.max()), max(worst_n, en.max()), max(mean_d, ed.mean())
        # the ids: the sphere's on the pixels whose analytic ray hits the sphere, the plane's elsewhere
        lab = ref["label"][k]
        assert np.all(lab[ok & sphere] == SPHERE_ID) and np.all(lab[ok & ~sphere] == PLANE_ID)
        assert not lab[~ref["hit"][k]].any()
    print("maxima: depth %.4f (mean %.4f), normal %.4f" % (worst_d, mean_d, worst_n))
    assert worst_d <= V.ANALYTIC_DEPTH_ERR and worst_n <= V.ANALYTIC_NORMAL_ERR and mean_d <= V.ANALYTIC_DEPTH_MEAN_ERR
    assert worst_d >= 0.5 * V.ANALYTIC_DEPTH_ERR and worst_n >= 0.5 * V.ANALYTIC_NORMAL_ERR   # the recorded numbers are not stale


def test_bricks_that_do_not_exist_are_invalid():
    """the brick rule of the reference: with `allocated` a voxel of another brick is invalid whatever its weight - rays end as misses
    or pass through where the dense volume of the same values gives hits"""
    name = "5x24x32"
    nf, _, _, dims, origin, voxel, trunc = R.SCENES[name]
    tsdf, wsum, rgb, lab, poses = _volume(name)
    pad = [(0, -d % 8) for d in dims]
    t8, w8 = np.pad(tsdf, pad), np.pad(wsum, pad)
    g = [s // 8 for s in t8.shape]
    ht, wd = V.EXTRA_SIZE
    kw = dict(origin=origin, voxel=voxel, poses=poses, intr=V.view_intrinsics(ht, wd), ix=range(nf), ht=ht, wd=wd, dz=0.03, z_near=0.0, z_far=2.6)
    full = V.render_reference(t8, w8, None, None, allocated=np.ones(g, bool), **kw)
    dense = V.render_reference(t8, w8, None, None, **kw)
    assert np.array_equal(full["depth"], dense["depth"]) and full["hit"].sum() > 100
    some = np.ones(g, bool)
    some[:, :, g[2] // 2] = False                                                             # a slab of bricks across the view
    cut = V.render_reference(t8, w8, None, None, allocated=some, **kw)
    assert 0 < cut["hit"].sum() < full["hit"].sum()
    gone = np.where(np.repeat(np.repeat(np.repeat(some, 8, 0), 8, 1), 8, 2), w8, 0)             # the same as weights that are not there
    zeroed = V.render_reference(t8, gone, None, None, **kw)
    assert np.array_equal(cut["hit"], zeroed["hit"]) and np.array_equal(cut["depth"], zeroed["depth"])


# ------------------------------------------------------------------------------------------------ Python
def test_depth_residual_on_hand_made_tensors():
    from pvo_amd.depth_video import DepthVideo
    depth = torch.zeros(3, 4, 5)
    disps = torch.ones(3, 4, 5)
    # frame 0: model depth 2 everywhere; own depths 2 (1 + e) with e = 0, 0.01, .., 0.19
    depth[0] = 2.0
    e = torch.arange(20, dtype=torch.float64) * 0.01
    disps[0] = (1.0 / (2.0 * (1.0 + e))).reshape(4, 5).float()
    # frame 1: half the pixels have no surface, two have no own depth (0, inf), one a NaN
    depth[1] = 4.0
    depth[1, :2] = 0.0
    disps[1] = 0.25
    disps[1, 2, 0], disps[1, 2, 1], disps[1, 2, 2] = 0.0, float("inf"), float("nan")
    disps[1, 3, 4] = 0.2                                                                      # own depth 5 against 4
    # frame 2: nothing rendered
    med, p90, share = DepthVideo.depth_residual(disps, depth)
    assert med.dtype == torch.float64 and med.shape == (3,)
    q = np.quantile(e.numpy(), [0.5, 0.9])
    assert abs(med[0].item() - q[0]) < 1e-6 and abs(p90[0].item() - q[1]) < 1e-6 and share[0].item() == 1.0
    assert share[1].item() == 7 / 20 and med[1].item() == 0.0 and 0.0 < p90[1].item() <= 0.25
    assert share[2].item() == 0.0 and np.isnan(med[2].item()) and np.isnan(p90[2].item())


def test_export_tool_takes_render_dir_only_with_a_mesh(capsys):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_map
    base = ["--datapath", "x", "--map", "a.ply"]
    assert export_map.parse_args(base).render_dir is None
    args = export_map.parse_args(base + ["--mesh", "m.ply", "--voxel", "0.05", "--render_dir", "r", "--panoptic"])
    assert args.render_dir == "r" and args.panoptic is True
    with pytest.raises(SystemExit):
        export_map.parse_args(base + ["--render_dir", "r"])
    assert "--render_dir needs --mesh" in capsys.readouterr().err


def test_the_default_range_and_the_sample_limit():
    """droid_backends' defaults: dz = voxel / 2, z_far = the farthest corner of the box over the views plus one step; a range of more
    than 65536 samples raises and says what to do"""
    from pvo_amd import droid_backends as db
    from pvo_amd._lib import PvoHipError
    poses = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]])
    ix = torch.tensor([0, 1, 7, -1])
    dz, z_near, z_far = db._render_range("t", (11, 21, 31), (-1.0, -2.0, 0.5), 0.1, poses, ix, None, 0.0, None)
    assert dz == 0.05 and z_near == 0.0 and abs(z_far - (0.5 + 1.0 + 1.0 + 0.05)) < 1e-9       # corner z = 1.5, view 1 is one further back
    assert db._render_range("t", (11, 21, 31), (0, 0, 0), 0.1, poses, ix[:1], 0.02, 0.25, 3.0) == (0.02, 0.25, 3.0)
    with pytest.raises(PvoHipError, match="raise dz"):
        db._render_range("t", (11, 21, 31), (0, 0, 0), 0.1, poses, ix, 1e-5, 0.0, 1.0)
    with pytest.raises(PvoHipError, match="raise dz"):
        db._render_range("t", (11, 21, 31), (0, 0, 1e4), 1e-3, poses, ix, None, 0.0, None)
    assert SR.BRICK == 8
