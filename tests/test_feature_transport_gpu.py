"""Feature transport on the device: pvo_feature_transport (pvo_amd/csrc/feature_transport.hip) against
tests/feature_transport_reference.py, src and the output BYTES held to equality (the contract is integers and individually rounded fp32
operations): every level shape, flow grid, dtype and level count of the contract's branches, the planted and the rounding cases,
non-finite flow and depth, alpha, byte copies, cur = None, rel_pose, L = 0; guard bytes, repeatability, capture; the fusion module
against an fp64 convolution; and the system path from a tracked factor graph."""
import ctypes

import numpy as np
import pytest
import torch

import feature_transport_reference as R
import operator_bounds_util as B

golden = R.golden

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GUARD = 256
LEVELS = [(24, 78), (12, 39), (6, 20), (3, 5), (1, 7), (1, 1), (3, 5), (1, 1)]
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def _feat(g, H, W, C, dt):
    """numpy features [H,W,C] in the restatement's representation (bfloat16 as uint16 bits)"""
    a = g.standard_normal((H, W, C)).astype(np.float32)
    return a.astype(np.float16) if dt == "f16" else R.f32_to_bf16_bits(a) if dt == "bf16" else a


def _to_dev(cuda, a, dt):
    """[H,W,C] numpy -> channels-last [1,C,H,W] device tensor"""
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if dt == "bf16" else np.ascontiguousarray(a))
    t = t.view(torch.bfloat16) if dt == "bf16" else t
    return t.to(cuda)[None].permute(0, 3, 1, 2)


def _bytes(t):
    """a channels-last [1,C,H,W] (or plain) device tensor -> its bytes in memory order"""
    t = t.permute(0, 2, 3, 1) if t.dim() == 4 else t
    return t.contiguous().view(torch.uint8).cpu().numpy().reshape(-1)


class _Guarded:
    def __init__(self, cuda, nbytes):
        self.n = nbytes
        self.buf = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=cuda)

    @property
    def inner(self):
        return self.buf[GUARD:GUARD + self.n]

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())


def _outputs(cuda, shapes, widths, dtype):
    """guarded, 0xA5-prefilled (outs, srcs) and their allocations"""
    es = torch.empty((), dtype=dtype).element_size()
    gs, outs, srcs = [], [], []
    for (H, W), Cw in zip(shapes, widths):
        go, gsrc = _Guarded(cuda, H * W * Cw * es), _Guarded(cuda, H * W * 4)
        gs += [go, gsrc]
        outs.append(go.inner.view(dtype).view(1, H, W, Cw).permute(0, 3, 1, 2))
        srcs.append(gsrc.inner.view(torch.int32).view(H, W))
    return gs, (outs, srcs)


def _check(cuda, shapes, flow, dt="f16", C=8, depth=None, order=1, mode="nearest", alpha=1.0, with_cur=True, scales=None, rel_pose=None,
           intrinsics=None, seed=0, ref=None, cur=None, what=""):
    """run the native call into guarded buffers, twice, and hold it to the restatement; returns the restatement's (outs, srcs)"""
    from pvo_amd import droid_backends as db
    g = np.random.default_rng(seed)
    ref = [_feat(g, H, W, C, dt) for H, W in shapes] if ref is None else ref
    cur = ([_feat(g, H, W, C, dt) for H, W in shapes] if cur is None else cur) if with_cur else None
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(cuda)
    kw = dict(scales=scales, depth=dev(depth), order=order, rel_pose=dev(rel_pose), intrinsics=dev(intrinsics), alpha=alpha, mode=mode)
    dref = [_to_dev(cuda, a, dt) for a in ref]
    dcur = None if cur is None else [_to_dev(cuda, a, dt) for a in cur]
    widths = [C * (2 if with_cur else 1)] * len(shapes)
    runs = []
    for _ in range(2):
        gs, out = _outputs(cuda, shapes, widths, DTYPES[dt])
        got = db.feature_transport(dref, dcur, dev(flow), out=out, **kw)
        torch.cuda.synchronize()
        assert all(x.intact() for x in gs), what
        runs.append(([_bytes(o) for o in got[0]], [s.cpu().numpy() for s in got[1]]))
    want = R.transport(ref, cur, np.asarray(flow, np.float32), scales=scales, depth=depth, order=order, rel_pose=rel_pose, intrinsics=intrinsics,
                       alpha=alpha, mode=R.NEAREST if mode == "nearest" else R.REFERENCE, bf16=dt == "bf16")
    for l in range(len(shapes)):
        assert np.array_equal(runs[0][1][l], want[1][l]), (what, l, "src", int((runs[0][1][l] != want[1][l]).sum()))
        assert np.array_equal(runs[0][0][l], np.ascontiguousarray(want[0][l]).view(np.uint8).reshape(-1)), (what, l, "out")
        assert np.array_equal(runs[1][1][l], runs[0][1][l]) and np.array_equal(runs[1][0][l], runs[0][0][l]), (what, l, "second call")
    return want


def _field(g, shape, spread, with_depth):
    flow = g.uniform(-spread, spread, shape + (2,)).astype(np.float32)
    depth = g.uniform(-0.3, 4.0, shape).astype(np.float32) if with_depth else None
    return flow, depth


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("L", (1, 3, 8))
def test_every_shape_grid_and_mode_equals_the_restatement(cuda, dt, L):
    g = np.random.default_rng(L)
    shapes = LEVELS[:L]
    reached = 0
    for grid in ((30, 101), (6, 20)):
        scales = [(W / grid[1], H / grid[0]) for H, W in shapes]
        for k, (mode, order, with_depth) in enumerate((("nearest", -1, True), ("nearest", 1, False), ("reference", 1, True), ("nearest", 1, True))):
            flow, depth = _field(g, grid, 9.0 if mode == "nearest" else 3.0, with_depth)
            want = _check(cuda, shapes, flow, dt, 8 if dt != "f32" else 4, depth, order, mode, scales=scales, seed=k, what=(grid, mode, order))
            reached += sum(int((s >= 0).sum()) for s in want[1])
    print(dt, L, "cells reached over all cases", reached)
    assert reached > 100 * L


@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_wide_rows_equal_the_restatement(cuda, dt):
    g = np.random.default_rng(7)
    shapes = [(12, 39), (6, 20), (1, 7)]
    flow, depth = _field(g, (30, 101), 9.0, True)
    scales = [(W / 101, H / 30) for H, W in shapes]
    _check(cuda, shapes, flow, dt, 256, depth, -1, scales=scales, what="C=256")
    _check(cuda, shapes, flow, dt, 256, depth, -1, scales=scales, alpha=0.5, with_cur=False, what="C=256 alpha cur=None")


def test_zero_flow_is_the_identity_and_a_flow_out_of_the_image_leaves_zero_bytes(cuda):
    shapes = LEVELS[:6]
    want = _check(cuda, shapes, np.zeros((6, 20, 2), np.float32), what="zero flow")
    for (H, W), s in zip(shapes, want[1]):
        assert np.array_equal(s, np.arange(H * W, dtype=np.int32).reshape(H, W))
    for mode in ("nearest", "reference"):
        want = _check(cuda, shapes, np.full((6, 20, 2), -200.0, np.float32), mode=mode, what="all out")
        for o, s in zip(want[0], want[1]):
            assert (s == -1).all() and not o[..., 8:].view(np.uint16).any()      # (zero BYTES over the 0xA5 prefill, held by _check)


@pytest.mark.parametrize("mode", ("nearest", "reference"))
@pytest.mark.parametrize("order", (1, -1))
def test_planted_collisions(cuda, mode, order):
    c = golden("planted")
    H, W = c["src"].shape
    flow = np.where(c["flow"] == -2, np.float32(-200), c["flow"])                # (every other cell leaves the image in nearest mode too)
    for dep in (c["depth"], None):
        want = _check(cuda, [(H, W)], flow, "f32", 4, dep, order, mode, ref=[c["ref"]], cur=[c["cur"]], what="planted")
        s = want[1][0]
        first = {(True, 1): 1 * W + 1, (True, -1): 2 * W + 3}.get((dep is not None, order), 2 * W + 3)   # nearest / farthest / last
        assert s[3, 4] == first and s[5, 7] == 1 * W + 6 and (s >= 0).sum() == 2
        if mode == "reference" and order == 1:                                  # the reference's own output
            k = golden("planted" if dep is not None else "planted_flow")
            assert np.array_equal(s, k["src"]) and np.array_equal(want[0][0].view(np.uint32), k["out"].view(np.uint32))


def test_rounding_edges_and_non_finite_operands(cuda):
    H, W = 1, 7
    flow = np.zeros((H, W, 2), np.float32)
    flow[0, 0, 0] = np.nextafter(np.float32(-0.5), np.float32(-1))         # tx one ulp below -0.5: out
    flow[0, 1, 0] = -1.5                                                   # tx = -0.5 exactly -> cell 0
    flow[0, 2, 0] = 1.5                                                    # 3.5 -> 4
    flow[0, 3, 0] = 1.0
    flow[0, 5, 0] = 1e30
    flow[0, 6, 1] = np.inf
    want = _check(cuda, [(H, W)], flow, what="edges")
    assert want[1][0].tolist() == [[1, -1, -1, -1, 4, -1, -1]]
    flow[0, 6] = [np.nan, 0.0]
    flow[0, 5] = [0.0, -np.inf]
    _check(cuda, [(H, W), (1, 1)], flow, mode="reference", what="edges, reference mode")
    disp = np.array([[1, 1, 5.0, 2.0, 1.0, 1, 1]], np.float32)
    assert _check(cuda, [(H, W)], flow, depth=disp, order=-1, what="disparity")[1][0][0, 4] == 2
    disp[0, 2:5] = [np.nan, -1.0, 0.0]
    assert _check(cuda, [(H, W)], flow, depth=disp, order=-1, what="bad depth")[1][0][0, 4] == -1
    g = np.random.default_rng(3)
    flow, depth = _field(g, (30, 101), 9.0, True)
    flow[g.integers(0, 30, 40), g.integers(0, 101, 40), g.integers(0, 2, 40)] = np.tile([np.nan, np.inf, -np.inf, 1e30], 10)
    depth[g.integers(0, 30, 40), g.integers(0, 101, 40)] = np.tile([np.nan, np.inf, 0.0, -2.0], 10)
    shapes = [(24, 78), (6, 20)]
    _check(cuda, shapes, flow, depth=depth, scales=[(W / 101, H / 30) for H, W in shapes], what="non-finite, resized")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_alpha_and_byte_copies(cuda, dt):
    g = np.random.default_rng(11)
    shapes = [(6, 20), (3, 5)]
    flow, depth = _field(g, (6, 20), 3.0, True)
    scales = [(W / 20, H / 6) for H, W in shapes]
    C = 8 if dt != "f32" else 4
    _check(cuda, shapes, flow, dt, C, depth, alpha=0.5, scales=scales, what="alpha 0.5")
    _check(cuda, shapes, flow, dt, C, depth, alpha=-3.0, scales=scales, with_cur=False, what="alpha -3, cur None")
    # alpha = 1: NaN payloads and negative zeros come through as bytes
    ref = [_feat(g, H, W, C, dt) for H, W in shapes]
    cur = [_feat(g, H, W, C, dt) for H, W in shapes]
    odd = {"f16": [0x7E01, 0xFE55, 0x8000, 0x7C01], "bf16": [0x7FC1, 0xFFA5, 0x8000, 0x7F81], "f32": [0x7FC00001, 0xFFA55555, 0x80000000, 0x7F800001]}[dt]
    for a in ref + cur:
        bits = a.view(np.uint32 if dt == "f32" else np.uint16).reshape(-1)
        bits[:: 5] = np.resize(np.array(odd, bits.dtype), bits[:: 5].shape)
    _check(cuda, shapes, np.zeros((6, 20, 2), np.float32), dt, C, ref=ref, cur=cur, what="payloads")


def test_rel_pose_carries_the_depth_first(cuda):
    g = np.random.default_rng(13)
    shapes = [(12, 39), (6, 20)]
    flow, _ = _field(g, (30, 101), 9.0, False)
    depth = g.uniform(0.5, 6.0, (6, 20)).astype(np.float32)
    rel = np.array([0.99, 0.02, -0.1, 0.3, -0.02, 1.0, 0.01, -0.1, 0.4, -0.3, 0.9, -1.5], np.float32)    # some cells end behind the camera
    intr = np.array([12.5, 11.0, 9.5, 2.75], np.float32)
    want = _check(cuda, shapes, flow, depth=depth, rel_pose=rel, intrinsics=intr, scales=[(W / 101, H / 30) for H, W in shapes], what="rel_pose")
    moved = R.transport_depth(depth, rel, intr)
    assert (moved <= 0).any() and (moved > 0).any()
    plain = R.transport([np.zeros((H, W, 8), np.float16) for H, W in shapes], None, flow, depth=depth, scales=[(W / 101, H / 30) for H, W in shapes])
    assert any((a != b).any() for a, b in zip(plain[1], want[1]))              # the transported depth decides otherwise than the plain one


def test_no_levels_and_refused_arguments(cuda):
    from pvo_amd import _lib, droid_backends as db
    flow = torch.zeros(3, 5, 2, device=cuda)
    assert db.feature_transport([], None, flow) == ([], [])
    lib = _lib.load()
    a = _lib.FeatureTransportArgs()
    a.C, a.dtype, a.L, a.mode, a.order, a.alpha = 8, _lib.PVO_F16, 0, 0, 1, 1.0
    assert lib.pvo_feature_transport(ctypes.byref(a), None, 0, None) == 0       # L = 0: PVO_OK, nothing needed
    assert lib.pvo_feature_transport(None, None, 0, None) == 1
    for field, bad in (("L", 9), ("L", -1), ("C", 0), ("C", 4), ("dtype", 3), ("mode", 2), ("order", 0), ("alpha", float("inf")), ("Hf", -1)):
        b = _lib.FeatureTransportArgs.from_buffer_copy(a)
        setattr(b, field, bad)
        assert lib.pvo_feature_transport(ctypes.byref(b), None, 0, None) == 1, field
    ref = torch.zeros(1, 8, 3, 5, dtype=torch.float16, device=cuda).contiguous(memory_format=torch.channels_last)
    for kw in (dict(flow=flow.cpu()), dict(flow=flow.double()), dict(flow=flow[..., :1]), dict(depth=torch.ones(3, 5, 1, device=cuda)),
               dict(scales=[(1.0, 1.0)] * 2), dict(ref_feats=[ref.contiguous()]), dict(ref_feats=[ref[:, :4]]), dict(cur_feats=[ref[:, :, :2]]),
               dict(out=([torch.empty_like(ref)], [torch.empty(3, 5, dtype=torch.int64, device=cuda)])),
               dict(rel_pose=torch.zeros(11, device=cuda), depth=torch.ones(3, 5, device=cuda), intrinsics=torch.ones(4, device=cuda))):
        with pytest.raises(ValueError, match="feature_transport"):
            db.feature_transport(**dict(dict(ref_feats=[ref], cur_feats=None, flow=flow), **kw))


def test_the_workspace_is_sized_by_the_library_and_stays_inside_its_guards(cuda):
    from pvo_amd import _lib
    lib = _lib.load()
    g = np.random.default_rng(17)
    shapes = [(12, 39), (3, 5)]
    flow, _ = _field(g, (30, 101), 9.0, False)
    depth = g.uniform(0.5, 6.0, (6, 20)).astype(np.float32)
    rel = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0.1, -0.1, 0.95, 0.2], np.float32)
    intr = np.array([12.5, 11.0, 9.5, 2.75], np.float32)
    ref = [_feat(g, H, W, 8, "f16") for H, W in shapes]
    keep = [torch.from_numpy(x).to(cuda) for x in (flow, depth, rel, intr)] + [_to_dev(cuda, r, "f16").permute(0, 2, 3, 1).contiguous() for r in ref]
    gs, (outs, srcs) = _outputs(cuda, shapes, [8, 8], torch.float16)
    a = _lib.FeatureTransportArgs()
    a.flow, a.Hf, a.Wf, a.depth, a.Hd, a.Wd = keep[0].data_ptr(), 30, 101, keep[1].data_ptr(), 6, 20
    a.rel_pose, a.intrinsics = keep[2].data_ptr(), keep[3].data_ptr()
    a.C, a.dtype, a.L, a.mode, a.order, a.alpha = 8, _lib.PVO_F16, 2, 0, 1, 1.0
    for l, (H, W) in enumerate(shapes):
        v = a.level[l]
        v.ref, v.out, v.src, v.H, v.W, v.sx, v.sy = keep[4 + l].data_ptr(), outs[l].data_ptr(), srcs[l].data_ptr(), H, W, W / 101, H / 30
    need = lib.pvo_feature_transport_workspace_bytes(ctypes.byref(a))
    assert need == (8 * (12 * 39 + 3 * 5) + 15) // 16 * 16 + 4 * 6 * 20
    ws = _Guarded(cuda, need)
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    assert lib.pvo_feature_transport(ctypes.byref(a), ctypes.c_void_p(ws.inner.data_ptr()), need - 16, stream) == 1      # too small: refused
    assert lib.pvo_feature_transport(ctypes.byref(a), ctypes.c_void_p(ws.inner.data_ptr()), need, stream) == 0
    torch.cuda.synchronize()
    assert ws.intact() and all(x.intact() for x in gs)
    want = R.transport(ref, None, flow, scales=[(W / 101, H / 30) for H, W in shapes], depth=depth, rel_pose=rel, intrinsics=intr)
    for l in range(2):
        assert np.array_equal(srcs[l].cpu().numpy(), want[1][l]) and np.array_equal(_bytes(outs[l]), want[0][l].view(np.uint8).reshape(-1))


def test_capture_and_replay_give_the_direct_bytes(cuda):
    from pvo_amd import droid_backends as db
    g = np.random.default_rng(19)
    shapes = [(12, 39), (6, 20), (1, 1)]
    flow, depth = _field(g, (30, 101), 9.0, True)
    scales = [(W / 101, H / 30) for H, W in shapes]
    ref = [_to_dev(cuda, _feat(g, H, W, 8, "f16"), "f16") for H, W in shapes]
    cur = [_to_dev(cuda, _feat(g, H, W, 8, "f16"), "f16") for H, W in shapes]
    dflow, ddepth = torch.from_numpy(flow).to(cuda), torch.from_numpy(depth).to(cuda)

    def run(out):
        db.feature_transport(ref, cur, dflow, scales=scales, depth=ddepth, order=-1, alpha=0.5, out=out)

    _, direct = _outputs(cuda, shapes, [16] * 3, torch.float16)
    run(direct)                                                                   # (also sizes the cached workspace before the capture)
    torch.cuda.synchronize()
    gs, out = _outputs(cuda, shapes, [16] * 3, torch.float16)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run(out)
    torch.cuda.current_stream().wait_stream(side)
    assert all(bool((x.inner == SENTINEL).all()) for x in gs)                     # the capture ran nothing
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert all(x.intact() for x in gs)
    for l in range(3):
        assert torch.equal(out[1][l], direct[1][l]) and np.array_equal(_bytes(out[0][l]), _bytes(direct[0][l]))


@pytest.mark.parametrize("dtype", (torch.float16, torch.bfloat16))
@pytest.mark.parametrize("C,shapes", ((128, ((6, 20), (3, 5))), (256, ((6, 20),))))
def test_fusion_module_within_the_convolution_bound(cuda, dtype, C, shapes):
    """native transport + native convolution against the fp64 convolution of the same 16-bit operands: K = 9 * 2C + 1 terms"""
    from pvo_amd import vps_fusion
    torch.manual_seed(C)
    dt = "f16" if dtype == torch.float16 else "bf16"
    g = np.random.default_rng(C)
    m = vps_fusion.FeatureFusion(C, alpha=0.5).to(cuda)
    with torch.no_grad():
        m.fusion_conv1.weight.copy_(m.fusion_conv1.weight.to(dtype).float())      # weights the 16-bit type holds exactly
    names = ["p%d" % (l + 2) for l in range(len(shapes))]
    ref = {k: _feat(g, H, W, C, dt) for k, (H, W) in zip(names, shapes)}
    cur = {k: _feat(g, H, W, C, dt) for k, (H, W) in zip(names, shapes)}
    flow, depth = _field(g, (6, 20), 3.0, True)
    scales = {k: (W / 20, H / 6) for k, (H, W) in zip(names, shapes)}
    got = m({k: _to_dev(cuda, v, dt) for k, v in ref.items()}, {k: _to_dev(cuda, v, dt) for k, v in cur.items()}, torch.from_numpy(flow).to(cuda),
            depth=torch.from_numpy(depth).to(cuda), scales=scales, order=-1)
    assert m._packed, "the native path must have packed the weights"
    fused, _ = R.transport([ref[k] for k in names], [cur[k] for k in names], flow, scales=[scales[k] for k in names], depth=depth, order=-1,
                           alpha=0.5, bf16=dt == "bf16")
    w, b = m.fusion_conv1.weight.detach().cpu(), m.fusion_conv1.bias.detach().cpu()
    for k, x in zip(names, fused):
        x = torch.from_numpy(R.bf16_bits_to_f32(x) if dt == "bf16" else x.astype(np.float32)).permute(2, 0, 1)[None]
        r, A = B.conv_ref(x, w, b)
        out, bound = B.linear_bound(r, A, 9 * 2 * C + 1, dtype)
        assert got[k].dtype == dtype and got[k].shape == (1, C) + tuple(x.shape[2:])
        B.assert_within(got[k].cpu(), out, bound, "fusion %s C=%d %s" % (k, C, dt))


def test_from_graph_feeds_the_transport_from_a_tracked_stream(cuda):
    """a short synthetic stream is tracked; one edge's flow and disparity go from the graph to the transport without leaving the device"""
    from pvo_amd import droid_backends as db, vps_fusion
    from pvo_amd.droid import Droid, default_args
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.synthetic import OracleFlowOperator, PlaneScene
    scene = PlaneScene(ht=24, wd=32, n_frames=12, seed=0)
    torch.manual_seed(0)
    droid = Droid(default_args(device=str(cuda), image_size=[scene.ht * 8, scene.wd * 8], buffer=32))
    video = droid.video
    op = OracleFlowOperator(scene, video, lambda p, d, k, i, j: db.reproject(p, d, k, i, j)[0])
    frontend = DroidFrontend(op, video, device=cuda, warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20,
                             frontend_radius=2, frontend_nms=1)
    gen = torch.Generator().manual_seed(1)
    for k in range(scene.n):
        slot = video.counter
        op.bind(slot, k)
        video.append(float(k), None if k else scene.poses[0].to(cuda), None, scene.intr.to(cuda),
                     torch.randn(scene.ht, scene.wd, 128, generator=gen).half().to(cuda),
                     torch.zeros(128, scene.ht, scene.wd, dtype=torch.half, device=cuda), torch.zeros(128, scene.ht, scene.wd, dtype=torch.half, device=cuda))
        frontend()
        if video.counter <= slot:
            op.frame_of.pop(slot, None)
            op.bind(video.counter - 1, k)
    graph = frontend.graph
    graph.update(None, None, use_inactive=True)                                  # (the flow of the edges as they stand now)
    E = graph.ii.shape[0]
    assert E > 0 and tuple(graph.full_flow.shape) == (1, E, scene.ht, scene.wd, 2)
    e = int((graph.jj - graph.ii == 1).nonzero()[0])
    shapes = [(24, 32), (12, 16)]
    kw = vps_fusion.from_graph(graph, e, shapes)
    assert kw["order"] == -1 and kw["scales"] == [(1.0, 1.0), (0.5, 0.5)] and kw["flow"].is_cuda and kw["depth"].is_cuda
    g = np.random.default_rng(23)
    ref = [_feat(g, H, W, 8, "f16") for H, W in shapes]
    cur = [_feat(g, H, W, 8, "f16") for H, W in shapes]
    outs, srcs = db.feature_transport([_to_dev(cuda, a, "f16") for a in ref], [_to_dev(cuda, a, "f16") for a in cur], **kw)
    flow, disp = kw["flow"].cpu().numpy(), kw["depth"].cpu().numpy()
    assert np.array_equal(disp, video.disps[int(graph.ii[e])].cpu().numpy()) and np.abs(flow).max() > 0.5
    want = R.transport(ref, cur, flow, scales=kw["scales"], depth=disp, order=-1)
    for l in range(2):
        assert np.array_equal(srcs[l].cpu().numpy(), want[1][l]) and np.array_equal(_bytes(outs[l]), want[0][l].view(np.uint8).reshape(-1))
    print("edge", e, "reached", [int((s >= 0).sum()) for s in want[1]], "of", [H * W for H, W in shapes])
    assert (want[1][0] >= 0).sum() > 24 * 32 // 2
    labels = torch.arange(1, 24 * 32 + 1, dtype=torch.int32, device=cuda).reshape(24, 32)
    moved = vps_fusion.transport_labels(labels, srcs[0])
    assert torch.equal(moved, torch.where(srcs[0] >= 0, srcs[0] + 1, torch.zeros_like(srcs[0])))
