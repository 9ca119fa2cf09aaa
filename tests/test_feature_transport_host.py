"""pvo_feature_transport's contract on the host (no GPU): tests/feature_transport_reference.py, the numpy restatement of the contract
in include/pvo_hip.h, against tests/golden/feature_transport.npz - what the REFERENCE's own methods returned
(tests/golden/gen_transport_golden.py) - in reference mode, held to EQUALITY of src and features; the torch formulation
FeatureFusion falls back on against the restatement; the binding's checks; the ctypes mirror against the C compiler's layout."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import feature_transport_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
golden = R.golden


@pytest.mark.parametrize("case", ("ident_flow", "ident_depth", "negative", "planted", "planted_flow"))
def test_reference_mode_equals_the_reference(case):
    c = golden(case)
    assert c, "the generator dropped %s on the machine that wrote the golden file" % case
    outs, srcs = R.transport([c["ref"]], [c["cur"]], c["flow"], depth=c.get("depth"), order=1, alpha=float(c["alpha"]), mode=R.REFERENCE)
    print(case, "reached", int((c["src"] >= 0).sum()), "of", c["src"].size)
    assert np.array_equal(srcs[0], c["src"])
    assert np.array_equal(outs[0].view(np.uint32), c["out"].view(np.uint32))
    if case == "negative":
        assert (srcs[0] == -1).all()
    if case.startswith("planted"):
        W = c["src"].shape[1]
        assert srcs[0][3, 4] == (1 * W + 1 if case == "planted" else 2 * W + 3) and srcs[0][5, 7] == 1 * W + 6


def test_reference_mode_on_a_resized_flow_equals_the_reference_off_the_marked_cells():
    c = golden("resized")
    ref, cur = [c["ref0"], c["ref1"]], [c["cur0"], c["cur1"]]
    outs, srcs = R.transport(ref, cur, c["flow"], depth=c["depth"], order=1, alpha=float(c["alpha"]), mode=R.REFERENCE)
    for l in range(2):
        skip = c["skip%d" % l]
        differ = srcs[l] != c["src%d" % l]
        print("level", l, "skipped", int(skip.sum()), "of", skip.size, "differing", int(differ.sum()), "outside the mask", int((differ & ~skip).sum()))
        assert skip.mean() <= 0.01
        assert not (differ & ~skip).any()
        assert np.array_equal(outs[l].view(np.uint32)[~skip], c["out%d" % l].view(np.uint32)[~skip])


def test_depth_transport_is_within_fp32_rounding_of_the_reference():
    """depth' = ((r20 X + r21 Y) + r22 Z) + t2 with X = (u - cx) / fx * Z: every operand is rounded to fp32 once (2^-24 relative) and
    each of the at most six operations on a term's path once more; (u - cx) may cancel, so its error is taken against |u| + |cx|.
    Bound: 8 * 2^-24 * (|r20| (|u| + |cx|) / fx Z + |r21| (|v| + |cy|) / fy Z + |r22| Z + |t2|), the reference being its own fp64."""
    c = golden("pose")
    got = R.transport_depth(c["depth"], c["rel_pose"].astype(np.float32), c["intrinsics"].astype(np.float32))
    rel, (fx, fy, cx, cy) = c["rel_pose"], c["intrinsics"]
    Z = c["depth"].astype(np.float64)
    u, v = np.arange(20)[None, :], np.arange(6)[:, None]
    mag = abs(rel[8]) * (u + abs(cx)) / fx * Z + abs(rel[9]) * (v + abs(cy)) / fy * Z + abs(rel[10]) * Z + abs(rel[11])
    err = np.abs(got.astype(np.float64) - c["out"])
    print("worst error / bound", float((err / (8 * 2.0 ** -24 * mag)).max()))
    assert got.dtype == np.float32 and (err <= 8 * 2.0 ** -24 * mag).all()


def _random_case(g, shapes, flow_shape, C, with_depth):
    ref = [g.standard_normal((H, W, C)).astype(np.float32) for H, W in shapes]
    cur = [g.standard_normal((H, W, C)).astype(np.float32) for H, W in shapes]
    flow = g.uniform(-6, 6, flow_shape + (2,)).astype(np.float32)
    depth = g.uniform(-0.5, 4.0, flow_shape).astype(np.float32) if with_depth else None
    return ref, cur, flow, depth


@pytest.mark.parametrize("mode", ("nearest", "reference"))
@pytest.mark.parametrize("order", (1, -1))
def test_the_torch_formulation_equals_the_restatement(mode, order):
    from pvo_amd import vps_fusion
    g = np.random.default_rng(5)
    shapes = [(12, 39), (6, 20), (1, 7), (1, 1)]
    ref, cur, flow, depth = _random_case(g, shapes, (30, 101), 4, True)
    flow[3, 5] = np.nan
    flow[4, 6] = 1e30
    scales = [(W / 101, H / 30) for H, W in shapes]
    cl = lambda a: torch.from_numpy(a)[None].permute(0, 3, 1, 2)
    for dep in (depth, None):
        want = R.transport(ref, cur, flow, scales=scales, depth=dep, order=order, alpha=0.5, mode=R.NEAREST if mode == "nearest" else R.REFERENCE)
        got = vps_fusion.transport_torch([cl(a) for a in ref], [cl(a) for a in cur], torch.from_numpy(flow), scales=scales,
                                         depth=None if dep is None else torch.from_numpy(dep), order=order, alpha=0.5, mode=mode)
        for l in range(len(shapes)):
            assert np.array_equal(got[1][l].numpy(), want[1][l]), (l, dep is None)
            assert np.array_equal(got[0][l][0].permute(1, 2, 0).contiguous().numpy().view(np.uint32), want[0][l].view(np.uint32))
    rel = np.array([1, 0, 0, 0.1, 0, 1, 0, 0.2, 0.05, -0.02, 0.99, 0.3], np.float32)
    intr = np.array([40.0, 38.0, 50.0, 15.0], np.float32)
    if order == 1:
        want = R.transport(ref, None, flow, scales=scales, depth=depth, rel_pose=rel, intrinsics=intr, mode=R.NEAREST if mode == "nearest" else R.REFERENCE)
        got = vps_fusion.transport_torch([cl(a) for a in ref], None, torch.from_numpy(flow), scales=scales, depth=torch.from_numpy(depth),
                                         rel_pose=torch.from_numpy(rel), intrinsics=torch.from_numpy(intr), mode=mode)
        for l in range(len(shapes)):
            assert np.array_equal(got[1][l].numpy(), want[1][l])
            assert np.array_equal(got[0][l][0].permute(1, 2, 0).contiguous().numpy().view(np.uint32), want[0][l].view(np.uint32))


def test_restatement_rounding_edges_and_tie_rule():
    """tx on k + 0.5 rounds up, on -0.5 to cell 0, one ulp below -0.5 leaves; equal keys go to the largest s; the larger disparity wins
    with order = -1"""
    H, W = 1, 7
    flow = np.zeros((H, W, 2), np.float32)
    flow[0, 0, 0] = np.nextafter(np.float32(-0.5), np.float32(-1))         # tx one ulp below -0.5: out
    flow[0, 1, 0] = -1.5                                                   # tx = -0.5 exactly -> cell 0
    flow[0, 2, 0] = 1.5                                                    # tx = 3.5 -> 4
    flow[0, 3, 0] = 1.0                                                    # also 4
    flow[0, 5, 0] = 1e30
    flow[0, 6, 1] = np.inf
    src = R.resolve(flow, H, W)
    assert src.tolist() == [[1, -1, -1, -1, 4, -1, -1]]                    # cell 4 keeps itself: the largest s of 2, 3, 4
    disp = np.array([[1, 1, 5.0, 2.0, 1.0, 1, 1]], np.float32)
    assert R.resolve(flow, H, W, depth=disp, order=-1)[0, 4] == 2 and R.resolve(flow, H, W, depth=disp, order=1)[0, 4] == 4
    disp[0, 2] = np.nan
    disp[0, 3] = -1.0
    disp[0, 4] = 0.0
    assert R.resolve(flow, H, W, depth=disp, order=-1)[0, 4] == -1


def test_fusion_module_on_the_host_and_label_transport():
    from pvo_amd import vps_fusion
    torch.manual_seed(0)
    m = vps_fusion.FeatureFusion(8, alpha=0.5)
    assert set(m.state_dict()) == {"fusion_conv1.weight", "fusion_conv1.bias"} and m.fusion_conv1.weight.shape == (8, 16, 3, 3)
    g = np.random.default_rng(2)
    shapes = {"p2": (6, 20), "p3": (3, 5)}
    ref = {k: torch.from_numpy(g.standard_normal((1, 8) + s).astype(np.float32)) for k, s in shapes.items()}
    cur = {k: torch.from_numpy(g.standard_normal((1, 8) + s).astype(np.float32)) for k, s in shapes.items()}
    flow = torch.from_numpy(g.uniform(-3, 3, (6, 20, 2)).astype(np.float32))
    scales = {k: (s[1] / 20, s[0] / 6) for k, s in shapes.items()}
    out = m(ref, cur, flow, scales=scales)
    assert list(out) == ["p2", "p3"] and all(out[k].shape == ref[k].shape for k in shapes)
    _, srcs = R.transport([ref["p2"][0].permute(1, 2, 0).numpy()], None, flow.numpy(), scales=[scales["p2"]])
    fused = np.concatenate([cur["p2"][0].permute(1, 2, 0).numpy(),
                            R.gather(np.ascontiguousarray(ref["p2"][0].permute(1, 2, 0).numpy()), None, srcs[0], 0.5)], 2)
    want = m.fusion_conv1(torch.from_numpy(fused).permute(2, 0, 1)[None])
    assert torch.allclose(out["p2"], want, rtol=1e-5, atol=1e-5)          # (one convolution, two memory layouts of one input)
    labels = torch.arange(1, 121, dtype=torch.int32).reshape(6, 20)
    src = torch.from_numpy(srcs[0])
    moved = vps_fusion.transport_labels(labels, src)
    assert moved.dtype == torch.int32 and torch.equal(moved, torch.where(src >= 0, src + 1, torch.zeros_like(src)))
    with pytest.raises(ValueError, match="transport_labels"):
        vps_fusion.transport_labels(labels.long(), src)


def test_the_binding_checks_raise_before_the_library_is_touched(monkeypatch):
    from pvo_amd import _lib, droid_backends as db

    def touched():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", touched)
    ref = [torch.zeros(1, 8, 3, 5, dtype=torch.float16).contiguous(memory_format=torch.channels_last)]
    flow = torch.zeros(3, 5, 2)
    for kw in (dict(), dict(mode="bilinear"), dict(order=0), dict(alpha=float("nan")), dict(rel_pose=torch.zeros(12)),
               dict(depth=torch.ones(3, 5), rel_pose=torch.zeros(12), intrinsics=torch.ones(4), order=-1), dict(intrinsics=torch.ones(4))):
        with pytest.raises(ValueError, match="feature_transport"):
            db.feature_transport(ref, None, flow, **kw)
    with pytest.raises(ValueError, match="feature_transport"):
        db.feature_transport(ref * 9, None, flow)
    with pytest.raises(ValueError, match="feature_transport"):
        db.feature_transport(ref, ref + ref, flow)
    with pytest.raises(ValueError, match="feature_transport"):
        db.feature_transport(ref, None, None)


def test_argument_structs_match_the_c_layout(tmp_path):
    from pvo_amd import _lib
    L, A = _lib.TransportLevel, _lib.FeatureTransportArgs
    fields_l = ("ref", "cur", "out", "src", "H", "W", "sx", "sy")
    fields_a = ("flow", "Hf", "Wf", "depth", "Hd", "Wd", "rel_pose", "intrinsics", "C", "dtype", "L", "mode", "order", "alpha", "level")
    src = tmp_path / "layout.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pvo_hip.h"', 'int main(void) {',
             '  printf("%zu %zu %d %d %d\\n", sizeof(pvo_transport_level), sizeof(pvo_feature_transport_args), PVO_TRANSPORT_MAX_LEVELS,',
             '         PVO_TRANSPORT_NEAREST, PVO_TRANSPORT_REFERENCE);']
    lines += ['  printf("%%zu\\n", offsetof(pvo_transport_level, %s));' % f for f in fields_l]
    lines += ['  printf("%%zu\\n", offsetof(pvo_feature_transport_args, %s));' % f for f in fields_a]
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [ctypes.sizeof(L), ctypes.sizeof(A), _lib.TRANSPORT_MAX_LEVELS, _lib.TRANSPORT_NEAREST, _lib.TRANSPORT_REFERENCE]
    want += [getattr(L, f).offset for f in fields_l] + [getattr(A, f).offset for f in fields_a]
    assert got == want
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.pvo_feature_transport_args_size.restype = ctypes.c_size_t
    assert lib.pvo_feature_transport_args_size() == ctypes.sizeof(A)
