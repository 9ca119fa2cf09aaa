"""The update operator's trunk per block of edges (pvo_debug_config: edge_blocks with "+trunk"): each block's lookup -> corr_encoder[2]
and 7x7 -> flow_encoder[2] are launched for that block's edges only, in front of its own gates, on the three streams the update
already uses.  The range launches run the whole launches' workgroups on the whole launches' operands, so everything
pvo_update_operator_rows (the precomputed-correlation path: pvo_corr_encode's range) and pvo_graph_update_rows (the tiled-pool
lookup's range) leave behind is bit-identical to the schedule off: for both splits, with and without the other bits of the knob,
with the static terms read through the row table and through the slot pool, in fp16 and bf16, on a one-tile map (16 x 16) and a
ragged one (20 x 40: a second tile row of 4 rows, a last tile column of 8), for E = 2 (below the blocking threshold: today's path),
E = 3 (blocks of 1 + 2 edges) and E = 7 (3 + 4 and 2 + 5).  The range launchers themselves are held to the whole launches row by row."""
import ctypes

import pytest
import torch

CL = torch.channels_last
MAPS = [(16, 16), (20, 40)]
EDGES = [2, 3, 7]
ON = ["half+trunk", "third+trunk", "half+agg+trunk", "third+low+agg+trunk"]
F = 5                                                                             # frames of the static pools / of the window


@pytest.fixture
def knob():
    from pvo_amd import droid_backends as db
    yield lambda v: db.debug_config("edge_blocks", v)
    db.debug_config("edge_blocks", None)


def _rand(cuda, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dt).to(cuda)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32) if t.element_size() == 4 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def test_knob_strings_select_the_trunk_bit(monkeypatch):
    """ "+trunk" is bit 3 of value - 2, every string without it keeps the number it had (no GPU: the call into the library is recorded)"""
    from pvo_amd import _lib, droid_backends as db

    class Lib:
        def pvo_debug_config(self, knob, value):
            seen.append((knob, value))
            return 0
    seen = []
    monkeypatch.setattr(_lib, "load", lambda: Lib())
    want = {None: 0, "off": 1, "half": 2, "third": 3, "half+low": 4, "third+low": 5, "half+agg": 6, "third+low+agg": 9,
            "half+trunk": 10, "third+trunk": 11, "half+agg+trunk": 14, "third+trunk+agg+low": 17, "17": 17}
    for s, v in want.items():
        db.debug_config("edge_blocks", s)
        assert seen[-1] == (_lib.PVO_KNOB_EDGE_BLOCKS, v), s
    with pytest.raises(ValueError):
        db.debug_config("edge_blocks", "trunk")


# ---------------------------------------------------------------------------------------------------------------- the operator
class _Operator:
    """pvo_update_operator_rows on E edges whose source frames are TABLE[:E]; `static` = "table" (frame pools read through the row
    table) or "slots" (static_by_slot: the same pools read through the args' slot table, a NULL row table)"""
    TABLE = [2, 0, 2, 4, 1, 0, 3]

    def __init__(self, cuda, dt, E, H, W, module_seed=5):
        from pvo_amd.modules.update import DynamicUpdateModule
        torch.manual_seed(module_seed)
        self.op = DynamicUpdateModule().to(cuda).eval().to(dt)
        self.weights = self.op.packed_weights(dt)
        self.cuda, self.dt, self.E, self.H, self.W = cuda, dt, E, H, W
        r = _rand(cuda, dt, 17)
        self.pools = self.op.static_terms(torch.relu(r(F, 128, H, W)).contiguous(memory_format=CL), dt)
        frames = self.TABLE[:E]
        self.rows = torch.tensor(frames, dtype=torch.int32, device=cuda)
        # GraphAgg: the edges grouped by source frame
        src = sorted(set(frames))
        order = [e for f in src for e in range(E) if frames[e] == f]
        ptr = [0]
        for f in src:
            ptr.append(ptr[-1] + frames.count(f))
        self.agg = (torch.tensor(ptr, dtype=torch.int32, device=cuda), torch.tensor(order, dtype=torch.int32, device=cuda), len(src))
        from pvo_amd import _lib
        n = _lib.load().pvo_operator_workspace_bytes(E, len(src), H, W) + 256
        self.ws = torch.zeros(n, dtype=torch.uint8, device=cuda)

    def inputs(self, seed):
        r = _rand(self.cuda, self.dt, seed)
        E, H, W = self.E, self.H, self.W
        return dict(net=torch.tanh(r(E, 128, H, W)).contiguous(memory_format=CL), motion=r(E, 8, H, W).contiguous(memory_format=CL),
                    corr=r(E, 196, H, W).contiguous(memory_format=CL))

    def enqueue(self, t, static):
        """one call on the current stream, not waited for; returns its outputs"""
        from pvo_amd import _lib, droid_backends as db
        E, H, W, K = self.E, self.H, self.W, self.agg[2]
        assert self.weights.struct.flags & _lib.PVO_OP_ENC_SIDE_STREAM and not self.weights.struct.flags & _lib.PVO_OP_SINGLE_STREAM
        new = lambda c, n: torch.zeros(n, H, W, c, dtype=self.dt, device=self.cuda).permute(0, 3, 1, 2)
        o = dict(net_out=new(128, E), heads=new(8, E), eta=torch.zeros(K, H, W, device=self.cuda), upmask=new(576, K))
        a = _lib.OperatorArgs()
        db._fill_operator_args(a, E, H, W, None, self.rows if static == "slots" else None, F if static == "slots" else 0, None, t["corr"],
                               t["motion"], t["net"], o["net_out"], None, self.pools[0], self.pools[1], self.agg, o["heads"], None,
                               o["eta"], o["upmask"])
        a.static_by_slot = 1 if static == "slots" else 0
        st = ctypes.c_void_p(torch.cuda.current_stream(self.cuda).cuda_stream)
        rc = _lib.load().pvo_update_operator_rows(ctypes.byref(self.weights.struct), ctypes.byref(a),
                                                  ctypes.c_void_p(self.rows.data_ptr()) if static == "table" else None,
                                                  ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(), st)
        _lib.check(rc, "update operator")
        return o


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("hw", MAPS, ids=["16x16", "20x40"])
@pytest.mark.parametrize("E", EDGES)
def test_operator_rows_trunk_blocked_equals_unblocked(cuda, knob, dt, hw, E):
    case = _Operator(cuda, dt, E, *hw)
    t = case.inputs(23)
    for static in ("table", "slots"):
        knob("off")
        case.ws.fill_(0x5A)                  # (every run starts from this: rows of c1 / f1 / CF that a block skipped would keep it)
        ref = case.enqueue(t, static)
        torch.cuda.synchronize()
        ws_ref = case.ws.clone()
        for k in ref:
            assert torch.isfinite(ref[k].float()).all(), k
        assert ref["net_out"].float().abs().max() > 0 and ref["heads"].float().abs().max() > 0
        for on in ON:
            knob(on)
            case.ws.fill_(0x5A)
            got = case.enqueue(t, static)
            torch.cuda.synchronize()
            for k in ("net_out", "heads", "eta", "upmask"):
                assert _same(got[k], ref[k]), (static, on, k)
            assert torch.equal(case.ws, ws_ref), (static, on, "workspace")      # every intermediate too: c1, f1, CF, Z, r * net, ...


@pytest.mark.gpu
def test_back_to_back_calls_keep_their_own_inputs(cuda, knob):
    """three calls on one stream with inputs A, B, A and no wait in between: each result is the unblocked result for its own inputs
    (a block that read the neighbouring call's c1 / f1 / CF rows from the shared workspace would not be)"""
    case = _Operator(cuda, torch.float16, 7, 20, 40)
    A, B = case.inputs(31), case.inputs(32)
    knob("off")
    ref = {}
    for name, t in (("A", A), ("B", B)):
        ref[name] = case.enqueue(t, "table")
        torch.cuda.synchronize()
    assert not _same(ref["A"]["net_out"], ref["B"]["net_out"])
    for on in ON:
        knob(on)
        outs = [case.enqueue(t, "table") for t in (A, B, A)]
        torch.cuda.synchronize()
        for name, got in zip("ABA", outs):
            for k in ("net_out", "heads", "eta", "upmask"):
                assert _same(got[k], ref[name][k]), (on, name, k)


# ---------------------------------------------------------------------------------------------------------------- the graph update
GRAPH_EDGES = ([0, 1, 1, 2, 2, 3, 0], [1, 0, 2, 1, 3, 2, 2])


def _window(cuda, dt, H, W, E):
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.factor_graph import FactorGraph
    from pvo_amd.geom.se3 import SE3
    from pvo_amd.modules.update import DynamicUpdateModule
    g = torch.Generator().manual_seed(4)
    video = DepthVideo(image_size=(H * 8, W * 8), buffer=F + 1, device=cuda)
    if dt != torch.float16:              # (the video keeps its maps in the operator's 16-bit type)
        video.fmaps, video.nets, video.inps = video.fmaps.to(dt), video.nets.to(dt), video.inps.to(dt)
    xi = torch.tensor([0.04, 0.01, 0.02, 0.0, 0.01, 0.005])
    for k in range(F):
        video.append(float(k), SE3.exp(k * xi).data.to(cuda), (0.5 + torch.rand(H, W, generator=g)).to(cuda),
                     torch.tensor([20.0, 21.0, W / 2 + 0.1 * k, H / 2.0]).to(cuda), torch.randn(H, W, 128, generator=g).to(dt).to(cuda),
                     torch.tanh(torch.randn(128, H, W, generator=g)).to(dt).to(cuda),
                     torch.relu(torch.randn(128, H, W, generator=g)).to(dt).to(cuda))
    torch.manual_seed(4)
    graph = FactorGraph(video, DynamicUpdateModule().to(cuda).eval().to(dt), device=cuda, max_factors=16)
    graph.want_upmask = True
    graph.add_factors(GRAPH_EDGES[0][:E], GRAPH_EDGES[1][:E])
    graph.target_cam = graph.target_cam + 0.3 * torch.randn(graph.target_cam.shape, generator=g).to(cuda)
    return video, graph


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("hw", MAPS, ids=["16x16", "20x40"])
@pytest.mark.parametrize("E", EDGES)
def test_graph_update_rows_trunk_blocked_equals_unblocked(cuda, knob, monkeypatch, dt, hw, E):
    """two pvo_graph_update_rows from a fixed state (the first computes its gate context itself, whole, in front of both blocks' gates;
    the second takes the one the first computed ahead): the hidden state, targets, weights, masks, delta_dy, damping, poses, depths,
    the full flow and the WHOLE workspace (the heads' outputs, eta, the upsampling mask and every intermediate live there) equal the
    schedule off.  "slots": the same call with a NULL row table and the static terms laid out by correlation-volume slot."""
    from pvo_amd import _lib, droid_backends as db
    H, W = hw
    video, graph = _window(cuda, dt, H, W, E)
    assert graph._fused_ok() and graph.P_zr is not None
    names = ("net", "target_cam", "weight", "raw_mask", "delta_dy")
    state = {n: getattr(graph, n).clone() for n in names}
    p0, d0, dm0 = video.poses.clone(), video.disps.clone(), graph.damping.clone()
    mode = {"static": "table", "calls": 0, "ws": None, "keep": None}
    real = db.graph_update

    def graph_update(weights, a, ws, stereo_baseline=0.0, static_rows=None):
        mode["calls"] += 1
        mode["ws"] = ws
        assert static_rows is not None and stereo_baseline == 0.0
        assert weights.struct.flags & _lib.PVO_OP_ENC_SIDE_STREAM and not weights.struct.flags & _lib.PVO_OP_SINGLE_STREAM
        if mode["static"] == "table":
            return real(weights, a, ws, static_rows=static_rows)
        slots = torch.tensor(list(graph.corr.slots), dtype=torch.long, device=cuda)
        src = torch.tensor(graph._ii_h, dtype=torch.long, device=cuda)
        pz = torch.zeros(graph.corr.capacity, H, W, 256, dtype=dt, device=cuda).permute(0, 3, 1, 2)
        pq = torch.zeros(graph.corr.capacity, H, W, 128, dtype=dt, device=cuda).permute(0, 3, 1, 2)
        pz[slots], pq[slots] = graph.P_zr[src], graph.P_q[src]
        mode["keep"] = (pz, pq)
        a.op.P_zr, a.op.P_q, a.op.static_by_slot = pz.data_ptr(), pq.data_ptr(), 1
        with torch.cuda.device(cuda):
            _lib.check(_lib.load().pvo_graph_update_rows(ctypes.byref(weights.struct), ctypes.byref(a), ctypes.c_void_p(ws.data_ptr()),
                                                         ws.numel(), 0.0, None, ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)),
                       "graph_update (slot pool)")

    monkeypatch.setattr(db, "graph_update", graph_update)

    def run(value):
        knob(value)
        for n in names:
            getattr(graph, n).copy_(state[n])
        video.poses.copy_(p0); video.disps.copy_(d0); graph.damping.copy_(dm0)
        for _ in range(2):
            graph.update(None, None, use_inactive=True)
        torch.cuda.synchronize()
        out = {n: getattr(graph, n).clone() for n in names}
        out.update(damping=graph.damping.clone(), poses=video.poses.clone(), disps=video.disps.clone(), full_flow=graph.full_flow.clone(),
                   workspace=mode["ws"].clone())
        return out

    for static in ("table", "slots"):
        mode["static"] = static
        run("off")                       # (the first run leaves the workspace's never-written padding as every later run finds it)
        ref = run("off")
        assert mode["calls"] >= 4
        for k in ("net", "target_cam", "weight", "poses", "disps"):
            assert torch.isfinite(ref[k].float()).all(), k
        assert not _same(ref["net"], state["net"]) and not _same(ref["poses"], p0)
        for on in ON:
            got = run(on)
            for k in ref:
                assert _same(got[k], ref[k]), (static, on, k)


# ---------------------------------------------------------------------------------------------------------------- the range launchers
RE, RE0, RE1, RH, RW = 3, 1, 3, 20, 40
SENTINEL = 0x7B7B


def _range_case(cuda, dt, which):
    """-> (call(y, e0, e1), a fresh sentinel-filled output): one of the trunk's launches on E = 3 edges of a 20 x 40 map"""
    from pvo_amd import _lib, droid_backends as db
    r = _rand(cuda, dt, 41 + len(which))
    code = {torch.float16: _lib.PVO_F16, torch.bfloat16: _lib.PVO_BF16}[dt]
    E, H, W = RE, RH, RW
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    keep = []

    def launcher(idx, levels, x, w, bias, Cout=0, relu=0, ystride=0, yoff=0, slots=None, num_slots=0):
        keep.extend([levels, x, w, bias, slots])

        def call(y, e0, e1, alive=keep):      # (the closure keeps every operand alive: `levels` holds addresses only)
            st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
            with torch.cuda.device(cuda):
                _lib.check(_lib.load().pvo_debug_trunk_range(idx, levels, vp(x), vp(w), vp(bias), vp(y), E, e0, e1, H, W, Cout, relu,
                                                             ystride, yoff, vp(slots), num_slots, code, st), which)
        return call

    def out(channels):
        return torch.full((E, H, W, channels), SENTINEL, dtype=torch.int16, device=cuda)

    bias = lambda n: torch.randn(n, generator=torch.Generator().manual_seed(3)).to(cuda)
    if which.startswith("lookup"):
        NV = 5 if which == "lookup_slots" else E
        pyr = [r(NV, H, W, *db.tiled_level_shape(H, W, l)) for l in range(4)]
        keep.append(pyr)
        levels = (ctypes.c_void_p * 4)(*[lv.data_ptr() for lv in pyr])
        g = torch.Generator().manual_seed(9)
        coords = (torch.rand(E, H, W, 2, generator=g) * torch.tensor([W + 6.0, H + 6.0]) - 3.0).to(cuda).contiguous()      # some taps off the map
        wenc = db.corr_encoder_weights(r(128, 196, 1, 1, sc=0.1), dt)
        slots = torch.tensor([4, 0, 2], dtype=torch.int32, device=cuda) if which == "lookup_slots" else None
        return launcher(0, levels, coords, wenc, bias(128), slots=slots, num_slots=NV if slots is not None else 0), out(128)
    if which == "corr_encode":
        return launcher(1, None, r(E, H, W, 196), db.corr_encoder_weights(r(128, 196, 1, 1, sc=0.1), dt), bias(128)), out(128)
    if which == "conv7x7_c8":
        return launcher(2, None, r(E, H, W, 8), db.conv7x7_c8_weights(r(128, 8, 7, 7, sc=0.1), dt), bias(128)), out(128)
    if which == "conv3x3_c128_64":       # flow_encoder[2]: 64 channels into columns [128, 192) of CF
        return launcher(3, None, r(E, H, W, 128), db.conv3x3_c128_weights(r(64, 128, 3, 3, sc=0.05), dt), bias(64), 64, 1, 192, 128), out(192)
    if which == "conv3x3_c128_128":      # corr_encoder[2]: 128 channels into columns [0, 128) of CF
        return launcher(3, None, r(E, H, W, 128), db.conv3x3_c128_weights(r(128, 128, 3, 3, sc=0.05), dt), bias(128), 128, 1, 192, 0), out(192)
    raise KeyError(which)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("which", ["lookup_slots", "lookup_own_volumes", "corr_encode", "conv7x7_c8", "conv3x3_c128_64", "conv3x3_c128_128"])
def test_range_launch_writes_its_edges_like_the_whole_launch_and_nothing_else(cuda, dt, which):
    """edges [1, 3) of 3 on 20 x 40 into a sentinel-filled output: their rows carry the whole launch's bits, edge 0's rows (and the
    columns of a strided output the launch does not own) keep the sentinel; [0, 1) then completes the whole launch's output"""
    call, whole = _range_case(cuda, dt, which)
    part = whole.clone()
    call(whole, 0, RE)
    call(part, RE0, RE1)
    torch.cuda.synchronize()
    assert (whole != SENTINEL).any(dim=-1).all()                        # every row of the whole launch was written ...
    assert torch.isfinite(whole.view(dt).float()[whole != SENTINEL]).all()
    assert torch.equal(part[RE0:RE1], whole[RE0:RE1])
    assert (part[:RE0] == SENTINEL).all()
    assert len(torch.unique(whole[RE0:RE1].view(RE1 - RE0, -1), dim=0)) == RE1 - RE0      # ... and the edges differ: an edge offset of 0 would show
    call(part, 0, RE0)
    torch.cuda.synchronize()
    assert torch.equal(part, whole)
