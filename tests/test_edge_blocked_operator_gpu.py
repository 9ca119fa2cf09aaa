"""The edge-blocked schedule of the update operator (pvo_debug_config: edge_blocks): gates -> candidate -> heads launched per block
of edges on two streams run the same workgroups on the same operands as the whole launches, so everything pvo_update_operator_rows
and pvo_graph_update_rows leave behind is bit-identical to the schedule off - for every split / priority / GraphAgg.conv1 choice of
the knob, with the static terms read through the row table and through the slot pool, in fp16 and bf16, on a one-tile map (16 x 16)
and a ragged one (20 x 40: a second tile row of 4 rows, a last tile column of 8 that takes the half-width main loop), for
E = 1, 2 (below the blocking threshold: today's path), E = 3 (blocks of 1 + 2 edges) and E = 7 (3 + 4 and 2 + 5)."""
import ctypes

import pytest
import torch

CL = torch.channels_last
MAPS = [(16, 16), (20, 40)]
EDGES = [1, 2, 3, 7]
ON = ["half", "third", "half+low", "third+low", "half+agg", "third+low+agg"]      # every bit of the knob, both splits
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
def test_operator_rows_blocked_equals_unblocked(cuda, knob, dt, hw, E):
    case = _Operator(cuda, dt, E, *hw)
    t = case.inputs(23)
    for static in ("table", "slots"):
        knob("off")
        ref = case.enqueue(t, static)
        torch.cuda.synchronize()
        ws_ref = case.ws.clone()
        for k in ref:
            assert torch.isfinite(ref[k].float()).all(), k
        assert ref["net_out"].float().abs().max() > 0 and ref["heads"].float().abs().max() > 0
        for on in ON:
            knob(on)
            got = case.enqueue(t, static)
            torch.cuda.synchronize()
            for k in ("net_out", "heads", "eta", "upmask"):
                assert _same(got[k], ref[k]), (static, on, k)
            assert torch.equal(case.ws, ws_ref), (static, on, "workspace")      # every intermediate too: Z, r * net, z of the heads, ...


@pytest.mark.gpu
def test_back_to_back_calls_keep_their_own_inputs(cuda, knob):
    """three calls on one stream with inputs A, B, A and no wait in between: each result is the unblocked result for its own inputs
    (a block that read the neighbouring call's r * net / z / hidden state from the shared workspace would not be)"""
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
def test_graph_update_rows_blocked_equals_unblocked(cuda, knob, monkeypatch, dt, hw, E):
    """two pvo_graph_update_rows from a fixed state (the second takes the gate context the first computed ahead): the hidden state,
    targets, weights, masks, damping, poses, depths and the WHOLE workspace (the heads' outputs, eta, the upsampling mask and every
    intermediate live there) equal the schedule off.  "slots": the same call with a NULL row table and the static terms laid out
    by correlation-volume slot (static_by_slot)."""
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
