"""Map export, the parts that need no GPU: the numpy yardstick (tests/map_reference.py) is qualified against the recorded kernel-text
fixtures, the scenes of the GPU tests have the properties those tests rely on, the ctypes mirror of pvo_map_points_args has the
C layout, the PLY writer round-trips, and storing images stays opt-in."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import map_reference as M
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("case", ["a", "b"])
@pytest.mark.parametrize("t", [0.005, 0.05])
def test_map_reference_reproduces_the_recorded_iproj_points_at_the_kept_pixels(case, t):
    """the recorded iproj points are act(G, X) / d for the recorded poses G; the map's point for a world-to-camera pose P is
    act(P^-1, X) / d - so with P = G^-1 (pvo_amd.geom.se3) and the recorded depth_filter votes as the selection, every kept point
    must be the recorded one, to the tolerance tests/test_ba_oracle.py holds that pair to"""
    from pvo_amd.geom.se3 import SE3
    geom = np.load(os.path.join(G, "geom_kernels.npz"))
    poses, disps, intr = geom[case + "_poses"], geom[case + "_disps"], geom[case + "_intr"]
    votes, pts = geom[case + "_depth_filter_t%g" % t], geom[case + "_iproj"]
    inv = SE3(torch.from_numpy(poses).double()).inv().data.float().numpy()
    nf, ht, wd = disps.shape
    r = M.map_reference(inv, disps, intr, np.arange(nf), votes)
    keep = (votes >= 2) & (disps > np.float32(0.5) * disps.astype(np.float64).mean(axis=(1, 2)).astype(np.float32)[:, None, None])
    assert r["total"] == int(keep.sum())
    if t == 0.05:
        assert r["total"] > 0
    f, k = r["src"][:, 0], r["src"][:, 1]
    assert np.array_equal(np.stack([f, k], 1), np.argwhere(keep.reshape(nf, -1)))          # frame order, raster order
    assert np.array_equal(r["frame_start"], np.concatenate([[0], np.cumsum(keep.reshape(nf, -1).sum(1))]))
    assert np.array_equal(r["alpha"], votes.reshape(nf, -1)[f, k].astype(np.uint8))
    assert np.allclose(r["xyz"], pts.reshape(nf, -1, 3)[f, k], rtol=1e-5, atol=1e-5)
    assert np.all(r["bound"] <= 1e-5)                                   # (the derived bound is the tighter of the two here)


def test_scenes_have_the_properties_the_gpu_tests_rely_on():
    """exact fp64 sums in any order; 17-69 % kept; every frame non-empty except frames 0 and 1 of the three-frame scene; votes
    reach 5 on the eight-frame scene (checked with the CPU oracle's depth filter)"""
    for name, (nf, ht, wd, noise) in M.SCENES.items():
        poses, disps, intr = [x.numpy() for x in M.scene(M.SEED, nf, ht, wd, noise)]
        assert np.array_equal(disps * 4096.0, np.round(disps * 4096.0)) and disps.min() > 0
        for f in range(nf):
            a = disps[f].astype(np.float64).reshape(-1)
            assert a.sum() == a[::-1].sum() == np.sort(a).sum()
        for th in M.THRESHOLDS:
            v = O.depth_filter(poses, disps, intr, np.arange(nf), np.full(nf, th, np.float32))
            r = M.map_reference(poses, disps, intr, np.arange(nf), v)
            per = np.diff(r["frame_start"])
            assert 0.15 < r["total"] / float(nf * ht * wd) < 0.75, (name, th)
            if name == "9x12x3":
                assert per[0] == per[1] == 0 and per[2] > 0
            else:
                assert per.min() > 0, (name, th)
            if name == "24x40x8":
                assert v.max() == 5
            assert r["bound"].max() < M.K_POINT * M.EPS * 9.0


def test_reference_skips_frames_out_of_range_and_follows_ix():
    nf, ht, wd, noise = M.SCENES["13x17x7"]
    poses, disps, intr = [x.numpy() for x in M.scene(M.SEED, nf, ht, wd, noise)]
    ix = np.array([6, -1, 0, nf, 3])
    v = np.zeros((len(ix), ht, wd), np.float32)
    ok = [0, 2, 4]
    v[ok] = O.depth_filter(poses, disps, intr, ix[ok], np.full(3, 0.2, np.float32))
    r = M.map_reference(poses, disps, intr, ix, v)
    per = np.diff(r["frame_start"])
    assert per[1] == per[3] == 0 and per[0] > 0 and per[2] > 0 and per[4] > 0
    assert list(dict.fromkeys(r["src"][:, 0].tolist())) == [6, 0, 3]


def test_ctypes_struct_matches_the_c_layout(tmp_path):
    from pvo_amd import _lib
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pvo_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pvo_map_points_args), offsetof(pvo_map_points_args, N),\n'
                   '         offsetof(pvo_map_points_args, images), offsetof(pvo_map_points_args, labels),\n'
                   '         offsetof(pvo_map_points_args, capacity), offsetof(pvo_map_points_args, frame_start));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    A = _lib.MapPointsArgs
    assert got == [ctypes.sizeof(A), A.N.offset, A.images.offset, A.labels.offset, A.capacity.offset, A.frame_start.offset]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.pvo_map_points_args_size.restype = ctypes.c_size_t
    assert lib.pvo_map_points_args_size() == ctypes.sizeof(A)
    lib.pvo_map_points_workspace_bytes.restype = ctypes.c_size_t
    lib.pvo_map_points_workspace_bytes.argtypes = [ctypes.c_int] * 3
    assert lib.pvo_map_points_workspace_bytes(0, 30, 101) == 0
    # one byte per candidate pixel and two ints per workgroup, not the [N,HW] votes + [N,HW,3] points of the composition
    assert 64 * 240 * 808 <= lib.pvo_map_points_workspace_bytes(64, 240, 808) < 1.1 * 64 * 240 * 808


def _read_ply(path):
    with open(path, "rb") as f:
        blob = f.read()
    head, body = blob.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    kinds = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    dt = np.dtype([(l.split()[2], kinds[l.split()[1]]) for l in lines if l.startswith("property")])
    assert len(body) == n * dt.itemsize
    return np.frombuffer(body, dtype=dt), body


def test_ply_writer_round_trips_byte_for_byte(tmp_path):
    from pvo_amd.handoff import write_ply
    rng = np.random.default_rng(0)
    xyz = rng.standard_normal((37, 3)).astype(np.float32)
    rgba = rng.integers(0, 256, (37, 4)).astype(np.uint8)
    lab = rng.integers(-5, 1000, 37).astype(np.int32)
    p = str(tmp_path / "sub" / "cloud.ply")
    assert write_ply(p, torch.from_numpy(xyz), rgba, lab) == 37
    rec, body = _read_ply(p)
    assert rec.dtype.names == ("x", "y", "z", "red", "green", "blue", "label") and rec.dtype.itemsize == 19
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1).view(np.uint32), xyz.view(np.uint32))
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), rgba[:, :3]) and np.array_equal(rec["label"], lab)
    want = b"".join(xyz[i].tobytes() + rgba[i, :3].tobytes() + lab[i].tobytes() for i in range(37))
    assert body == want
    # without colours and labels, and an empty cloud
    assert write_ply(p, xyz) == 37 and _read_ply(p)[0].dtype.names == ("x", "y", "z")
    assert write_ply(p, xyz[:0], rgba[:0]) == 0 and len(_read_ply(p)[0]) == 0


def test_storing_images_is_opt_in():
    from pvo_amd.droid import default_args
    assert default_args().store_images is False
    assert default_args(store_images=True).store_images is True
