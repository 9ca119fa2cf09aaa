"""Surface reconstruction, the parts that need no GPU: the C boundary of pvo_tsdf_integrate / pvo_tsdf_mesh (symbols, struct layouts,
argument validation - every argument is checked before anything touches the device, so NULL pointers are enough), the properties of
the numpy yardstick (tests/tsdf_reference.py) that the GPU tests rely on, the reference mesh of the analytic scene, the host-side
helpers of DepthVideo and the mesh PLY writer."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import tsdf_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PVO_OK, PVO_EINVAL, PVO_EWORKSPACE = 0, 1, 3


def _lib():
    from pvo_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, (res, args) in _lib.SIGNATURES.items():
        if name.startswith("pvo_tsdf") or name == "pvo_version":
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib, _lib


def test_symbols_struct_sizes_and_abi_version(tmp_path):
    lib, L = _lib()
    assert lib.pvo_version() == 106 == L.PVO_ABI_VERSION
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pvo_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pvo_tsdf_integrate_args), offsetof(pvo_tsdf_integrate_args, origin),\n'
                   '         offsetof(pvo_tsdf_integrate_args, poses), offsetof(pvo_tsdf_integrate_args, images),\n'
                   '         offsetof(pvo_tsdf_integrate_args, img_offset), sizeof(pvo_tsdf_mesh_args), offsetof(pvo_tsdf_mesh_args, vcap),\n'
                   '         offsetof(pvo_tsdf_mesh_args, counts));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    A, M = L.TsdfIntegrateArgs, L.TsdfMeshArgs
    assert got == [ctypes.sizeof(A), A.origin.offset, A.poses.offset, A.images.offset, A.img_offset.offset,
                   ctypes.sizeof(M), M.vcap.offset, M.counts.offset]
    assert lib.pvo_tsdf_integrate_args_size() == ctypes.sizeof(A) and lib.pvo_tsdf_mesh_args_size() == ctypes.sizeof(M)
    assert lib.pvo_tsdf_integrate_workspace_bytes(0) == 0 and 64 * 64 <= lib.pvo_tsdf_integrate_workspace_bytes(64) <= 64 * 64 + 256
    assert lib.pvo_tsdf_mesh_workspace_bytes(1, 9, 9) == 0
    cells = 255 ** 3
    assert 5 * cells <= lib.pvo_tsdf_mesh_workspace_bytes(256, 256, 256) < 5.1 * cells      # a byte and an index per cell


FAKE = 0x1000          # a non-NULL pointer that is never dereferenced: every call below returns before a launch


def _integrate_args(L, **kw):
    a = L.TsdfIntegrateArgs()
    a.tsdf = a.wsum = a.poses = a.disps = a.intrinsics = a.ix = FAKE
    a.nz, a.ny, a.nx, a.voxel, a.trunc = 8, 8, 8, 0.1, 0.3
    a.N, a.nframes, a.ht, a.wd = 2, 2, 8, 8
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_integrate_validates_before_touching_the_device():
    lib, L = _lib()
    call = lambda a, ws=FAKE, n=1 << 20: lib.pvo_tsdf_integrate(ctypes.byref(a), ws, n, None)
    assert lib.pvo_tsdf_integrate(None, FAKE, 1 << 20, None) == PVO_EINVAL
    assert call(_integrate_args(L, tsdf=None)) == PVO_EINVAL
    assert call(_integrate_args(L, wsum=None)) == PVO_EINVAL
    assert call(_integrate_args(L, nz=2048, ny=1024, nx=1024)) == PVO_EINVAL                 # nz*ny*nx = 2^31
    assert call(_integrate_args(L, nz=-1)) == PVO_EINVAL
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert call(_integrate_args(L, voxel=bad)) == PVO_EINVAL
        assert call(_integrate_args(L, trunc=bad)) == PVO_EINVAL
    assert call(_integrate_args(L, z_near=-1.0)) == PVO_EINVAL and call(_integrate_args(L, w_max=-1.0)) == PVO_EINVAL
    assert call(_integrate_args(L, rgb=FAKE)) == PVO_EINVAL                                  # a colour volume without images
    img = dict(images=FAKE, IH=64, IW=64, img_stride=8, img_offset=3)
    assert call(_integrate_args(L, **dict(img, img_stride=9))) == PVO_EINVAL                 # 9 * 7 + 3 = 66 >= 64
    assert call(_integrate_args(L, **dict(img, img_offset=8))) == PVO_EINVAL                 # 8 * 7 + 8 = 64 >= 64
    assert call(_integrate_args(L, **dict(img, img_stride=0))) == PVO_EINVAL
    assert call(_integrate_args(L, **dict(img, IW=59))) == PVO_EINVAL                        # 8 * 7 + 3 = 59 >= 59
    need = lib.pvo_tsdf_integrate_workspace_bytes(2)
    assert need > 0
    assert call(_integrate_args(L, **img), FAKE, need - 1) == PVO_EWORKSPACE                 # everything else in order
    assert call(_integrate_args(L, **img), None, need) == PVO_EWORKSPACE
    assert call(_integrate_args(L, N=0)) == PVO_OK and call(_integrate_args(L, nx=0)) == PVO_OK   # nothing to fuse: no launch


def test_mesh_validates_before_touching_the_device():
    lib, L = _lib()

    def args(**kw):
        a = L.TsdfMeshArgs()
        a.tsdf = a.wsum = a.verts = a.faces = a.counts = FAKE
        a.nz, a.ny, a.nx, a.voxel, a.min_weight, a.vcap, a.fcap = 8, 8, 8, 0.1, 1.0, 16, 32
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a, ws=FAKE, n=1 << 20: lib.pvo_tsdf_mesh(ctypes.byref(a), ws, n, None)
    assert call(args(tsdf=None)) == PVO_EINVAL and call(args(wsum=None)) == PVO_EINVAL and call(args(counts=None)) == PVO_EINVAL
    assert call(args(nz=2048, ny=1024, nx=1024)) == PVO_EINVAL
    assert call(args(voxel=0.0)) == PVO_EINVAL and call(args(voxel=-1.0)) == PVO_EINVAL
    assert call(args(min_weight=float("nan"))) == PVO_EINVAL
    assert call(args(verts=None)) == PVO_EINVAL and call(args(faces=None)) == PVO_EINVAL and call(args(vcap=-1)) == PVO_EINVAL
    assert call(args(rgba=FAKE + 1)) == PVO_EINVAL                                          # misaligned
    need = lib.pvo_tsdf_mesh_workspace_bytes(8, 8, 8)
    assert need >= 5 * 7 ** 3
    assert call(args(), FAKE, need - 1) == PVO_EWORKSPACE and call(args(), None, need) == PVO_EWORKSPACE


_cache = {}


def _reference(name, unit=False):
    """(scene arrays, reference integration) of a scene of tsdf_reference.SCENES, with the scene's weights or with unit weights"""
    key = (name, unit)
    if key not in _cache:
        nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
        sc = R.scene(nf, ht, wd)
        poses, disps, intr, images, weight, hit = sc
        ref = R.integrate_reference(dims, origin, voxel, trunc, poses, disps, intr, range(nf), weight=None if unit else weight,
                                    images=images, img_stride=1, img_offset=0)
        _cache[key] = (sc, ref)
    return _cache[key]


@pytest.mark.parametrize("name", list(R.SCENES))
def test_flagged_voxels_stay_below_one_percent_of_the_touched(name):
    """the condition under which the GPU tests may leave flagged voxels out of the value comparison - on the reference alone"""
    for unit in (False, True):
        sc, ref = _reference(name, unit)
        touched, flagged = int(ref["touched"].sum()), int(ref["flagged"].sum())
        print("%s unit weights %s: %d voxels, %d touched, %d flagged = %.2f %%, max bound %.2e"
              % (name, unit, ref["touched"].size, touched, flagged, 100.0 * flagged / touched, ref["bound"].max()))
        assert touched > 0.5 * ref["touched"].size
        assert flagged <= 0.01 * touched
        assert ref["bound"].max() < 1e-4 and ref["bound_rgb"].max() < 1e-3            # the bounds say something
        assert np.abs(ref["tsdf"]).max() <= 1.0 and (ref["tsdf"] < 0).any() and (ref["tsdf"] > 0).any()


def test_reference_follows_ix_and_skips_ids_out_of_range():
    nf, ht, wd, dims, origin, voxel, trunc = R.SCENES["3x12x16"]
    poses, disps, intr, images, weight, hit = R.scene(nf, ht, wd)
    run = lambda ix: R.integrate_reference(dims, origin, voxel, trunc, poses, disps, intr, ix, weight=weight)
    a, b, c = run([0, 1, 2]), run([2, 0, 1]), run([-1, 0, nf, 1, 2, 7])
    assert np.array_equal(a["tsdf"], c["tsdf"]) and np.array_equal(a["wsum"], c["wsum"])
    assert np.array_equal(a["touched"], b["touched"]) and np.abs(a["tsdf"] - b["tsdf"]).max() < 1e-12
    assert not np.array_equal(a["tsdf"], b["tsdf"])                   # the order is part of the contract's arithmetic
    capped = R.integrate_reference(dims, origin, voxel, trunc, poses, disps, intr, [0, 1, 2], weight=weight, w_max=1.25)
    assert capped["wsum"].max() == np.float32(1.25) and a["wsum"].max() > 1.25
    assert not np.array_equal(capped["tsdf"], a["tsdf"])


# the largest distance of a reference vertex from the true surface, measured on the reference mesh (unit weights, min_weight 1):
# 0.0407, 0.1071 and 0.2263 for voxels of 0.05, 0.12 and 0.17 - 0.8, 0.9 and 1.3 voxels, at the sphere's silhouette where the frames
# disagree.  Asserted with a margin of two.
MEASURED_DISTANCE = {"5x24x32": 0.0407, "3x12x16": 0.1071, "2x9x12": 0.2263}


@pytest.mark.parametrize("name", list(R.SCENES))
def test_reference_mesh_of_the_analytic_scene(name):
    nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
    sc, ref = _reference(name, unit=True)
    m = R.mesh_reference(ref["tsdf"].astype(np.float32), ref["wsum"], ref["rgb"].astype(np.float32), origin, voxel, 1.0)
    V, F = len(m["verts"]), len(m["faces"])
    dist = R.surface_distance(m["verts"])
    print("%s: %d vertices, %d faces, distance from the true surface max %.4f mean %.4f (voxel %g)" % (name, V, F, dist.max(), dist.mean(), voxel))
    assert V > 50 and F > 50 and m["faces"].min() >= 0 and m["faces"].max() < V
    assert dist.max() <= 2.0 * MEASURED_DISTANCE[name]
    # both objects are there: vertices on the sphere and on the plane
    on_sphere = np.abs(np.linalg.norm(m["verts"] - R.SPHERE_C, axis=1) - R.SPHERE_R) < voxel
    assert on_sphere.sum() > 8 and (~on_sphere).sum() > 8
    # every edge belongs to at most two triangles, an interior one to exactly two
    shares = R.edge_shares(m["faces"])
    inner = R.interior_vertices(m)
    inner_edges = [n for (a, b), n in shares.items() if inner[a] and inner[b]]
    print("   %d edges, %d interior" % (len(shares), len(inner_edges)))
    assert max(shares.values()) <= 2 and len(inner_edges) > 0 and all(n == 2 for n in inner_edges)
    # geometric normals point from inside to outside, as the vertex normals (the gradient of the tsdf) do
    v, f = m["verts"], m["faces"]
    gn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert np.all(np.linalg.norm(gn, axis=1) > 0)
    for k in range(3):
        assert np.all((gn * m["normals"][f[:, k]]).sum(1) > 0)
    assert np.allclose(np.linalg.norm(m["normals"], axis=1), 1.0)
    # toward the cameras (at z = 0): outward normals have a negative z on this scene
    assert np.mean(m["normals"][:, 2] < 0) > 0.95


def test_reference_mesh_degenerate_volumes():
    z = np.zeros((4, 5, 6), np.float32)
    assert len(R.mesh_reference(z, z, None, (0, 0, 0), 0.1)["verts"]) == 0                  # nothing valid
    t = np.ones((4, 5, 6), np.float32)
    assert len(R.mesh_reference(t, t, None, (0, 0, 0), 0.1)["verts"]) == 0                  # valid, all outside
    t[:2] = -1.0                                                                             # a flat surface between z = 1 and z = 2
    m = R.mesh_reference(t, np.ones_like(t), None, (0.5, 0, 0), 0.1)
    assert len(m["verts"]) == 4 * 5 and len(m["faces"]) == 2 * 3 * 4
    assert np.allclose(m["verts"][:, 2], 0.15) and np.allclose(m["normals"], [0, 0, 1])
    assert np.allclose(m["verts"][0], [0.55, 0.05, 0.15])
    v, f = m["verts"], m["faces"]
    assert np.all(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])[:, 2] > 0)
    assert len(R.mesh_reference(t, np.ones_like(t), None, (0, 0, 0), 0.1, min_weight=2.0)["verts"]) == 0


def test_fusion_weights_and_bounds_on_cpu_tensors():
    from pvo_amd.depth_video import DepthVideo
    g = torch.Generator().manual_seed(0)
    keep = torch.rand(3, 5, 7, generator=g) > 0.3
    disps = torch.rand(3, 5, 7, generator=g) + 0.2
    sigma = 0.1 * torch.rand(3, 5, 7, generator=g)
    sigma[0, 0, 0], sigma[1, 2, 3], sigma[2, 4, 6] = float("inf"), float("nan"), 0.0
    keep[0, 0, 0] = keep[1, 2, 3] = keep[2, 4, 6] = True
    w = DepthVideo.fusion_weights(keep, disps)
    assert w.dtype == torch.float32 and torch.equal(w, keep.float())
    w = DepthVideo.fusion_weights(keep, disps, sigma, rel0=0.05)
    want = keep.double().numpy() / (1.0 + (sigma.double().numpy() / (0.05 * disps.double().numpy())) ** 2)
    want[0, 0, 0] = want[1, 2, 3] = 0.0
    assert w.dtype == torch.float32 and np.allclose(w.numpy(), want, rtol=1e-5, atol=0) and w[2, 4, 6] == 1.0
    assert w[0, 0, 0] == 0 and w[1, 2, 3] == 0 and bool((w[~keep] == 0).all())
    half = DepthVideo.fusion_weights(torch.ones(1, dtype=torch.bool), torch.tensor([2.0]), torch.tensor([0.2]), rel0=0.1)
    assert abs(half.item() - 0.5) < 1e-6                              # sigma / disp = rel0 counts half

    xyz = torch.randn(5000, 3, generator=g) * torch.tensor([1.0, 0.5, 2.0]) + torch.tensor([0.3, -0.2, 4.0])
    xyz[:10] = 1000.0                                                  # outliers the percentiles leave out
    origin, dims = DepthVideo.tsdf_bounds(xyz, 0.1, 0.3)
    s = np.sort(xyz.numpy().astype(np.float64), axis=0)
    lo, hi = s[int(np.floor(0.01 * 4999))], s[int(np.ceil(0.99 * 4999))]
    assert np.allclose(origin, lo - 0.3) and isinstance(origin[0], float)
    assert dims == tuple(int(np.ceil((hi[e] - lo[e] + 0.6) / 0.1)) + 1 for e in (2, 1, 0))
    assert all(origin[e] + 0.1 * (dims[2 - e] - 1) >= hi[e] + 0.3 - 1e-9 for e in range(3))      # the far side is covered as well
    big = torch.arange(3 * ((1 << 21) + 5), dtype=torch.float32).reshape(-1, 3)                   # more than 2^20 points: a stride of 3
    o2, d2 = DepthVideo.tsdf_bounds(big, 1000.0, 0.0)
    sub = np.sort(big.numpy()[::3].astype(np.float64), axis=0)
    assert len(sub) <= 1 << 20 and np.allclose(o2, sub[int(np.floor(0.01 * (len(sub) - 1)))])


def test_mesh_ply_round_trips_byte_for_byte(tmp_path):
    from pvo_amd.handoff import write_ply_mesh
    rng = np.random.default_rng(1)
    verts = rng.standard_normal((11, 3)).astype(np.float32)
    normals = rng.standard_normal((11, 3)).astype(np.float32)
    rgba = rng.integers(0, 256, (11, 4)).astype(np.uint8)
    faces = rng.integers(0, 11, (7, 3)).astype(np.int32)
    p = str(tmp_path / "sub" / "mesh.ply")
    assert write_ply_mesh(p, torch.from_numpy(verts), torch.from_numpy(faces), rgba, normals) == (11, 7)
    blob = open(p, "rb").read()
    head, body = blob.split(b"end_header\n", 1)
    assert head.decode("ascii").split("\n") == [
        "ply", "format binary_little_endian 1.0", "element vertex 11", "property float x", "property float y", "property float z",
        "property float nx", "property float ny", "property float nz", "property uchar red", "property uchar green",
        "property uchar blue", "element face 7", "property list uchar int vertex_indices", ""]
    want = b"".join(verts[i].tobytes() + normals[i].tobytes() + rgba[i, :3].tobytes() for i in range(11))
    want += b"".join(b"\x03" + faces[i].tobytes() for i in range(7))
    assert body == want
    # positions and faces alone; an empty mesh
    assert write_ply_mesh(p, verts, faces) == (11, 7)
    body = open(p, "rb").read().split(b"end_header\n", 1)[1]
    assert body == verts.tobytes() + b"".join(b"\x03" + faces[i].tobytes() for i in range(7))
    assert write_ply_mesh(p, verts[:0], faces[:0], rgba[:0]) == (0, 0)
    assert open(p, "rb").read().endswith(b"end_header\n")


def test_export_tool_takes_the_mesh_options_and_is_unchanged_without_them():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import export_map
    base = ["--datapath", "x", "--map", "a.ply"]
    a = export_map.parse_args(base)
    assert a.mesh is None and a.voxel is None and a.sigma_weight is False
    a = export_map.parse_args(base + ["--mesh", "m.ply", "--voxel", "0.05", "--trunc", "0.2"])
    assert a.mesh == "m.ply" and a.voxel == 0.05 and a.trunc == 0.2
    for bad in (["--mesh", "m.ply"], ["--mesh", "m.ply", "--voxel", "0"], ["--mesh", "m.ply", "--voxel", "0.1", "--sigma_weight"]):
        with pytest.raises(SystemExit):
            export_map.parse_args(base + bad)
