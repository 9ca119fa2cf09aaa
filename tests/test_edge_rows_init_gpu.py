"""pvo_edge_rows_init through FactorGraph.add_factors: the state rows of new edges written by ONE launch equal, bit for bit, what
the per-tensor formulation gives - index_select of the source frames' hidden state, DepthVideo's reprojection, zero fills - and
the rows of the edges that were already there are not touched.  Once on a stereo video with an edge (i, i)."""
import pytest
import torch

H, W, F = 8, 16, 5
LIVE = ([0, 1], [1, 0])
NEW = ([3, 1, 4], [2, 4, 3])


def _window(cuda, stereo):
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.factor_graph import FactorGraph
    from pvo_amd.geom.se3 import SE3
    from pvo_amd.modules.update import DynamicUpdateModule
    g = torch.Generator().manual_seed(4)
    video = DepthVideo(image_size=(H * 8, W * 8), buffer=F + 1, device=cuda)
    xi = torch.tensor([0.04, 0.01, 0.02, 0.0, 0.01, 0.005])
    for k in range(F):
        video.append(float(k), SE3.exp(k * xi).data.to(cuda), (0.5 + torch.rand(H, W, generator=g)).to(cuda),
                     torch.tensor([20.0, 21.0, 8.0 + 0.1 * k, 4.0]).to(cuda), torch.randn(H, W, 128, generator=g).half().to(cuda),
                     torch.tanh(torch.randn(128, H, W, generator=g)).half().to(cuda),
                     torch.relu(torch.randn(128, H, W, generator=g)).half().to(cuda),
                     **(dict(right_fmap=torch.randn(H, W, 128, generator=g).half().to(cuda)) if stereo else {}))
    torch.manual_seed(4)
    graph = FactorGraph(video, DynamicUpdateModule().to(cuda).eval().half(), device=cuda, max_factors=16)
    return video, graph, g


@pytest.mark.gpu
@pytest.mark.parametrize("stereo", [False, True])
def test_new_edges_state_rows_equal_the_per_tensor_formulation(cuda, stereo, monkeypatch):
    from pvo_amd import droid_backends as db
    video, graph, g = _window(cuda, stereo)
    calls = []
    real = db.edge_rows_init
    monkeypatch.setattr(db, "edge_rows_init", lambda *a, **k: (calls.append(k.get("baseline")), real(*a, **k))[1])
    graph.add_factors(*LIVE)
    # the live rows carry state the next add must not touch
    names = ("target_cam", "weight", "raw_mask", "delta_dy")
    for n in names:
        getattr(graph, n).copy_(torch.randn(getattr(graph, n).shape, generator=g).to(cuda))
    graph.net.copy_(torch.randn(graph.net.shape, generator=g).half().to(cuda))
    before = {n: getattr(graph, n).clone() for n in names + ("net",)}
    ii_new, jj_new = (NEW[0] + [2], NEW[1] + [2]) if stereo else NEW              # (a stereo edge (i, i) among the new ones)
    graph.add_factors(list(ii_new), list(jj_new))
    torch.cuda.synchronize()
    n = len(ii_new)
    assert len(calls) == 2 and calls[1] == (video.stereo_baseline if stereo else 0.0)
    assert graph._ii_h == LIVE[0] + list(ii_new) and graph.net.shape[1] == 2 + n
    # the per-tensor formulation, computed here
    ii, jj = torch.tensor(ii_new, device=cuda), torch.tensor(jj_new, device=cuda)
    want_net = torch.index_select(video.nets, 0, ii)
    want_target = torch.empty(n, H, W, 2, device=cuda)
    db.reproject(video.poses, video.disps, video.intrinsics, ii, jj, out=want_target, baseline=video.rig_baseline())
    assert torch.equal(graph.net[0, 2:], want_net) and graph.net.dtype == video.nets.dtype
    assert torch.equal(graph.target_cam[0, 2:], want_target) and torch.isfinite(want_target).all()
    for name in ("weight", "raw_mask", "delta_dy"):
        t = getattr(graph, name)
        assert tuple(t.shape) == (1, 2 + n, H, W, 2) and not t[0, 2:].any(), name
    if stereo:       # the (i, i) edge is the rig's transform, not the identity
        grid = torch.stack(torch.meshgrid(torch.arange(W, device=cuda).float(), torch.arange(H, device=cuda).float(), indexing="xy"), -1)
        assert (graph.target_cam[0, -1] - grid).abs().max() > 0.5
    for name in before:
        assert torch.equal(getattr(graph, name)[:, :2], before[name]), name + ": live rows"
    # the graph's tensors are still the rows of its own buffers (nothing was re-allocated or copied out)
    assert graph._edge_rows("weight").owns(graph.weight[0]) and graph._edge_rows("net").owns(graph._net_rows())


@pytest.mark.gpu
def test_edge_rows_init_wrapper_rejects_other_layouts(cuda):
    from pvo_amd import droid_backends as db
    video, graph, _ = _window(cuda, False)
    ii, jj = torch.tensor([0, 1], device=cuda), torch.tensor([1, 0], device=cuda)
    f = lambda: torch.empty(2, H, W, 2, device=cuda)
    net = torch.empty(2, H, W, 128, dtype=torch.half, device=cuda)
    nets = video.nets.permute(0, 2, 3, 1)
    with pytest.raises(db.PvoHipError):
        db.edge_rows_init(nets, video.poses, video.disps, video.intrinsics, ii, jj, net.float(), f(), f(), f(), f())
    with pytest.raises(db.PvoHipError):
        db.edge_rows_init(nets, video.poses, video.disps, video.intrinsics, ii, jj, net, f(), f().double(), f(), f())
    with pytest.raises(db.PvoHipError):
        db.edge_rows_init(nets, video.poses, video.disps, video.intrinsics, ii.int(), jj, net, f(), f(), f(), f())
