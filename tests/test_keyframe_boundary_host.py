"""The keyframe boundary's entry points and bookkeeping, without a device: pvo_update_operator_rows / pvo_graph_update_rows /
pvo_corr_build_tiled_rows / pvo_edge_rows_init are declared, exported and bound, the ABI version and pvo_graph_update_args are
what they were, their argument checks answer before anything touches a device, and DepthVideo's per-frame stamps - what decides
whether a keyframe's static GRU terms are still valid - follow append, __setitem__, rm_keyframe's shift and a foreign write."""
import ctypes
import os
import re

import torch

from pvo_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pvo_update_operator_rows", "pvo_graph_update_rows", "pvo_corr_build_tiled_rows", "pvo_edge_rows_init")
OK, EINVAL = 0, 1

GRAPH_UPDATE_FIELDS = [
    "op", "nframes", "poses", "disps", "intrinsics", "ii", "jj", "target", "delta_dy", "raw_mask", "weight", "full_flow", "segm",
    "max_segments", "vote_thresh", "dy_thresh", "n_in", "target_ba", "weight_ba", "ii_ba", "jj_ba", "t0", "t1", "itrs", "motion_only",
    "lm", "ep", "sys", "ba_ws", "ba_ws_bytes", "clamp_frames", "disp_min", "want_upmask", "context_ahead", "context_ready",
    "want_upsample", "disps_up", "up_frames"]
OPERATOR_FIELDS = [
    "E", "H", "W", "levels", "slots", "num_slots", "coords", "corr", "motion", "net", "net_out", "inp", "P_zr", "P_q", "static_by_slot",
    "seg_ptr", "seg_idx", "K", "heads", "eta_frame", "eta_pos", "R", "damping", "EP", "eta_scale", "eta", "upmask"]


def test_new_entry_points_are_declared_exported_and_bound():
    with open(os.path.join(ROOT, "include", "pvo_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in include/pvo_hip.h"
        assert name in _lib.SIGNATURES, name + " is not bound in _lib.SIGNATURES"
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        # the binding has as many arguments as the declaration
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_abi_version_and_argument_structs_are_unchanged():
    lib = _lib.load()
    assert lib.pvo_version() == 106 and _lib.PVO_ABI_VERSION == 106
    assert [n for n, _ in _lib.GraphUpdateArgs._fields_] == GRAPH_UPDATE_FIELDS
    assert [n for n, _ in _lib.OperatorArgs._fields_] == OPERATOR_FIELDS
    assert lib.pvo_graph_update_args_size() == ctypes.sizeof(_lib.GraphUpdateArgs) == 456
    assert ctypes.sizeof(_lib.OperatorArgs) == 224


def test_argument_checks_answer_without_a_device():
    lib = _lib.load()
    vp = ctypes.c_void_p
    dummy = ctypes.create_string_buffer(64)            # a non-NULL host address no check dereferences
    p = vp(ctypes.addressof(dummy))
    levels = (vp * 4)(p, p, p, p)
    build = lib.pvo_corr_build_tiled_rows
    assert build(p, p, p, p, levels, -1, 128, 8, 8, _lib.PVO_F16, p, None) == EINVAL
    assert build(None, None, None, None, levels, 0, 128, 8, 8, _lib.PVO_F16, None, None) == OK
    assert build(p, p, None, p, levels, 3, 128, 8, 8, _lib.PVO_F16, p, None) == EINVAL
    assert build(p, p, p, None, levels, 3, 128, 8, 8, _lib.PVO_F16, p, None) == EINVAL
    rows = lib.pvo_edge_rows_init
    assert rows(p, p, p, p, p, p, p, p, p, p, p, -1, 8, 16, 0.0, None) == EINVAL
    assert rows(None, None, None, None, None, None, None, None, None, None, None, 0, 8, 16, 0.0, None) == OK
    assert rows(None, p, p, p, p, p, p, p, p, p, p, 2, 8, 16, 0.0, None) == EINVAL
    assert rows(p, p, p, p, None, None, p, p, p, p, p, 2, 8, 16, 0.0, None) == EINVAL
    assert rows(p, p, p, p, p, p, p, p, p, p, p, 2, 8, 16, -1.0, None) == EINVAL
    w = _lib.UpdateWeights()
    w.dtype = _lib.PVO_F16
    a = _lib.OperatorArgs()
    a.E, a.H, a.W = 0, 8, 16
    assert lib.pvo_update_operator_rows(None, ctypes.byref(a), None, None, 0, None) == EINVAL
    assert lib.pvo_update_operator_rows(ctypes.byref(w), ctypes.byref(a), None, None, 0, None) == OK      # no edges: a no-op
    a.E = -1
    assert lib.pvo_update_operator_rows(ctypes.byref(w), ctypes.byref(a), p, None, 0, None) == EINVAL
    u = _lib.GraphUpdateArgs()
    u.op.E, u.op.H, u.op.W = 0, 8, 16
    assert lib.pvo_graph_update_rows(None, ctypes.byref(u), None, 0, 0.0, None, None) == EINVAL
    assert lib.pvo_graph_update_rows(ctypes.byref(w), ctypes.byref(u), None, 0, 0.0, None, None) == OK
    assert lib.pvo_graph_update_rows(ctypes.byref(w), ctypes.byref(u), None, 0, -1.0, p, None) == EINVAL


class _Weights:
    serial, tensors = 7, {}


def _video(n=3):
    from pvo_amd.depth_video import DepthVideo
    v = DepthVideo(image_size=(64, 64), buffer=6, device="cpu")
    g = torch.Generator().manual_seed(1)
    for k in range(n):
        v.append(float(k), None, 1.0, torch.tensor([40.0, 40.0, 32.0, 32.0]), torch.randn(8, 8, 128, generator=g).half(),
                 torch.randn(128, 8, 8, generator=g).half(), torch.randn(128, 8, 8, generator=g).half())
    return v, g


def _pool(v):
    """the video's pool with the convolution replaced by a marker (rows [a, b) <- the frames' first channel): the stamp logic is
    what runs here"""
    pool = v.static_pool(_Weights(), torch.float16)
    calls = []

    def compute(a, b):
        calls.append((a, b))
        pool.P_zr[a:b] = v.inps[a:b, :1].expand(-1, 256, -1, -1)
        pool.P_q[a:b] = v.inps[a:b, :1].expand(-1, 128, -1, -1)
    pool._compute = compute
    return pool, calls


def test_static_rows_follow_the_per_frame_stamps():
    v, g = _video(4)
    pool, calls = _pool(v)
    assert v.static_pool(_Weights(), torch.float16) is pool           # same weights, same dtype: the same pool
    assert not any(pool.valid(f) for f in range(4))
    assert pool.ensure([0, 1, 3, 1]) == 3 and calls == [(0, 2), (3, 4)]      # contiguous runs, one call each
    assert pool.valid(0) and pool.valid(1) and not pool.valid(2) and pool.valid(3)
    assert pool.ensure([0, 1, 3]) == 0 and pool.computed == 3           # nothing to do for rows that are valid
    # append: the new frame's row is not valid, the others stay
    v.append(4.0, None, 1.0, torch.tensor([40.0, 40.0, 32.0, 32.0]), torch.randn(8, 8, 128, generator=g).half(),
             torch.randn(128, 8, 8, generator=g).half(), torch.randn(128, 8, 8, generator=g).half())
    assert not pool.valid(4) and pool.valid(0) and pool.valid(3)
    # video[k] = (...) with an inp: that frame only
    v[1] = (1.0, None, None, None, None, None, v.nets[1].clone(), torch.randn(128, 8, 8, generator=g).half())
    assert not pool.valid(1) and pool.valid(0) and pool.valid(3)
    assert pool.ensure([1]) == 1 and torch.equal(pool.P_q[1, 0], v.inps[1, 0])
    # ... and without one (None = keep up to the item given): nothing moves
    v[0] = (0.5, None, None, None, None)
    assert pool.valid(0)
    # rm_keyframe's shift: row ix + 1 moves to ix with its validity
    v.shift_inps(2)
    assert torch.equal(v.inps[2], v.inps[3]) and pool.valid(2) and torch.equal(pool.P_zr[2], pool.P_zr[3])
    v.shift_inps(3)                                                     # frame 4 was never computed: neither is 3 now
    assert not pool.valid(3) and pool.valid(2)
    n = pool.computed
    assert pool.ensure([2]) == 0 and pool.computed == n
    # a write the video did not make: every frame is invalid
    v.inps[0] = torch.randn(128, 8, 8, generator=g).half()
    assert not any(pool.valid(f) for f in range(5))
    assert pool.ensure([0, 2]) == 2 and pool.valid(0) and pool.valid(2) and not pool.valid(1)
    assert torch.equal(pool.P_q[0, 5], v.inps[0, 0])
    # a foreign write followed by one of the video's own is still noticed
    v.ensure_disps_sens()                                               # (unrelated buffers do not count)
    assert pool.valid(0)
    v.inps[2].mul_(2)
    v.append(5.0, None, 1.0, torch.tensor([40.0, 40.0, 32.0, 32.0]), torch.randn(8, 8, 128, generator=g).half(),
             torch.randn(128, 8, 8, generator=g).half(), torch.randn(128, 8, 8, generator=g).half())
    assert not pool.valid(0) and not pool.valid(2)


def test_other_weights_or_another_dtype_start_a_new_pool():
    v, _ = _video(2)
    pool, _ = _pool(v)
    pool.ensure([0, 1])

    class Other:
        serial, tensors = 8, {}
    p2 = v.static_pool(Other(), torch.float16)
    assert p2 is not pool and not p2.valid(0) and p2.computed == 0
    p3 = v.static_pool(Other(), torch.bfloat16)
    assert p3 is not p2 and p3.P_zr.dtype == torch.bfloat16 and tuple(p3.P_zr.shape) == (6, 256, 8, 8) and tuple(p3.P_q.shape) == (6, 128, 8, 8)
    assert p3.P_zr.permute(0, 2, 3, 1).is_contiguous()                  # channels-last rows
