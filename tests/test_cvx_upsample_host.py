"""Convex 8x upsampling, the parts that need no GPU: the C ABI (header, exported symbols, ctypes binding, the grown
pvo_graph_update_args), FactorGraph(upsample=True) on a host video (DepthVideo.upsample's PyTorch form) and Droid.get_depth(convex=True)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pvo_cvx_upsample", "pvo_cvx_upsample_vjp", "pvo_cvx_upsample_vjp_scratch_bytes")


def test_header_declares_library_exports_and_binding_binds_the_entry_points():
    from pvo_amd import _lib
    header = open(os.path.join(ROOT, "include", "pvo_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b(?:int|size_t)\s+%s\s*\(" % name, header), name + " is not declared in include/pvo_hip.h"
        assert hasattr(lib, name), name + " is not exported by libpvo_hip.so"
        assert name in _lib.SIGNATURES, name + " is not bound by pvo_amd._lib"
    loaded = _lib.load()                                        # (checks the version and the size of the grown argument struct)
    assert loaded.pvo_version() == _lib.PVO_ABI_VERSION
    # argument checks are host code: they answer without a device
    assert loaded.pvo_cvx_upsample(1, 1, 1, None, None, 1, 1, 1, 4, 4, 3, 576, 0, _lib.PVO_F32, _lib.PVO_F16, None) == 1      # D = 3: PVO_EINVAL
    assert loaded.pvo_cvx_upsample(1, 1, 1, None, None, 1, 1, 1, 4, 4, 1, 575, 0, _lib.PVO_F32, _lib.PVO_F16, None) == 1      # 575 channels
    assert loaded.pvo_cvx_upsample(None, 16, 16, None, None, 1, 1, 1, 4, 4, 1, 576, 0, _lib.PVO_F32, _lib.PVO_F16, None) == 1  # null data
    assert loaded.pvo_cvx_upsample(16, 16, 16, None, None, 1, 1, 1, 4, 4, 1, 576, 0, _lib.PVO_F64, _lib.PVO_F16, None) == 4    # fp64 data, fp16 mask
    assert loaded.pvo_cvx_upsample_vjp(16, 16, 16, 16, 16, 1, 4, 4, 1, 576, 0, _lib.PVO_F16, 16, 1 << 20, None) == 4           # no 16-bit backward
    assert loaded.pvo_cvx_upsample_vjp_scratch_bytes(2, 5, 7, 2, _lib.PVO_F32) >= 2 * 5 * 7 * 9 * 2 * 4


def test_graph_update_args_grew_at_the_end():
    from pvo_amd import _lib
    lib = _lib.load()
    assert lib.pvo_graph_update_args_size() == ctypes.sizeof(_lib.GraphUpdateArgs)
    names = [f[0] for f in _lib.GraphUpdateArgs._fields_]
    assert names[-3:] == ["want_upsample", "disps_up", "up_frames"]
    assert names[-6:-3] == ["want_upmask", "context_ahead", "context_ready"]            # what was last before stays where it was
    a = _lib.GraphUpdateArgs
    assert a.context_ready.offset < a.want_upsample.offset < a.disps_up.offset < a.up_frames.offset
    assert a.up_frames.offset + a.up_frames.size == ctypes.sizeof(a)


def _host_graph(upsample, E_pairs=((1, 2), (2, 1), (2, 3), (3, 2), (1, 3)), ht=5, wd=7, buffer=6, seed=0):
    """a FactorGraph on a host DepthVideo with the three native calls stubbed (as tests/test_factor_graph_glue.py does); the stand-in
    operator hands back a random upsampling mask, one row per source frame"""
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.factor_graph import FactorGraph
    g = torch.Generator().manual_seed(seed)
    v = DepthVideo(image_size=(ht * 8, wd * 8), buffer=buffer, device="cpu")
    v.counter = 4
    v.disps[:] = torch.rand(buffer, ht, wd, generator=g) + 0.5
    ii, jj = [p[0] for p in E_pairs], [p[1] for p in E_pairs]
    E, K = len(ii), len(set(ii))
    coords = torch.rand(1, E, ht, wd, 2, generator=g) * 4
    v.reproject = lambda a, b: (coords.clone(), torch.ones(1, E, ht, wd, 1))
    calls = {"ba": 0}

    def ba(target, weight, eta, ii_, jj_, t0, t1, itrs=2, lm=1e-4, ep=0.1, motion_only=False):
        calls["ba"] += 1
        if not motion_only:
            v.disps[1:4] *= 1.25                                                        # the BA moves the depths: the upsampling must read them AFTER it
    v.ba = ba
    mask = torch.randn(1, K, 576, ht, wd, generator=g) * 4

    def update_op(net, inp, corr, motn, ii_, jj_, flag):
        z = lambda c: torch.zeros(1, E, ht, wd, c)
        return torch.zeros(1, E, 128, ht, wd), z(4), z(2), torch.full((1, K, ht, wd), 1e-3), {"disp": mask, "flow": None, "dy_mask": None}, z(2)

    fg = FactorGraph(v, update_op, device="cpu", **({"upsample": True} if upsample else {}))
    fg.ii, fg.jj = torch.tensor(ii), torch.tensor(jj)
    fg._ii_h, fg._jj_h, fg._age_h = list(ii), list(jj), [0] * E
    fg.age = torch.zeros(E, dtype=torch.long)
    fg.net = fg.inp = torch.zeros(1, E, 128, ht, wd)
    fg.segm = torch.zeros(1, E, 1, ht, wd, dtype=torch.int)
    z2 = lambda: torch.zeros(1, E, ht, wd, 2)
    fg.target_cam, fg.weight, fg.raw_mask, fg.delta_dy = coords.clone(), z2(), z2(), z2()
    fg.corr = lambda c: torch.zeros(1, E, 196, ht, wd)
    return v, fg, mask[0], calls


def test_factor_graph_upsample_fills_disps_up_for_exactly_the_source_frames():
    from pvo_amd.droid_net import cvx_upsample
    v, fg, mask, calls = _host_graph(True)
    assert fg.upsample is True and v.disps_up is None                                 # allocated lazily
    fg.update(None, 4, itrs=2)
    assert calls["ba"] == 1 and v.disps_up is not None and v.disps_up.shape == (6, 40, 56)
    src = sorted(set(fg._ii_h))
    assert src == [1, 2, 3]
    want = cvx_upsample(v.disps[src].unsqueeze(-1), mask).squeeze(-1)               # the depths as the BA left them
    assert torch.equal(v.disps_up[src], want)
    rest = [k for k in range(6) if k not in src]
    assert torch.equal(v.disps_up[rest], torch.zeros(len(rest), 40, 56))            # every other frame untouched
    assert float(v.disps_up[src].min()) > 0
    # a motion-only update leaves disps_up alone
    before = v.disps_up.clone()
    v.disps[1:4] *= 0.5
    fg.update(None, 4, itrs=2, motion_only=True)
    assert calls["ba"] == 2 and torch.equal(v.disps_up, before)


def test_factor_graph_without_the_flag_never_touches_disps_up():
    v, fg, _, calls = _host_graph(False)
    assert fg.upsample is False
    fg.update(None, 4, itrs=2)
    assert calls["ba"] == 1 and v.disps_up is None


def test_upsample_is_out_of_scope_on_the_alt_corr_and_sharded_paths():
    v, fg, _, _ = _host_graph(True)
    fg.corr_impl = "alt"
    with pytest.raises(NotImplementedError):
        fg.update_lowmem(steps=1)
    with pytest.raises(NotImplementedError):
        fg._update_fused(None, None, 2, False, 1e-7, False, sharded=object())


def test_get_depth_convex_raises_without_the_flag():
    from pvo_amd.droid import Droid, default_args
    torch.manual_seed(0)
    droid = Droid(default_args(device="cpu", image_size=[32, 48], buffer=4, half_update=False))
    assert droid.frontend.graph.upsample is False
    assert droid.get_depth().shape == (0, 32, 48)                                     # the default form is what it was
    with pytest.raises(RuntimeError, match="upsample"):
        droid.get_depth(convex=True)
    droid2 = Droid(default_args(device="cpu", image_size=[32, 48], buffer=4, half_update=False, upsample=True))
    assert droid2.frontend.graph.upsample is True and droid2.backend.upsample is True
    droid2.video.upsample([0], torch.zeros(1, 576, 4, 6))
    assert droid2.get_depth(convex=True).shape == (0, 32, 48)
