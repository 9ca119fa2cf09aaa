"""The static GRU terms live per keyframe on the video: over a scripted life of a small window - edges built, an update, edges
dropped and re-added, a keyframe removed, a keyframe appended, a frame's context features overwritten behind the video's back -
the pool row of every frame with a live edge equals, bit for bit, update_op.static_terms of that frame's context features, and
nothing is convolved that does not have to be."""
import pytest
import torch

H = W = 16
NKF, RAD = 5, 2


def _check(graph, video, what):
    op = graph.update_op
    for f in sorted(set(graph._ii_h)):
        pz, pq = op.static_terms(video.inps[f:f + 1], torch.float16)
        assert torch.equal(graph.P_zr[f], pz[0]) and torch.equal(graph.P_q[f], pq[0]), "%s: frame %d" % (what, f)


def _frame(g, cuda):
    return (torch.randn(H, W, 128, generator=g).half().to(cuda), torch.tanh(torch.randn(128, H, W, generator=g)).half().to(cuda),
            torch.relu(torch.randn(128, H, W, generator=g)).half().to(cuda))


@pytest.mark.gpu
def test_static_terms_follow_the_keyframes_through_a_windows_life(cuda):
    import bench
    from pvo_amd.factor_graph import FactorGraph
    video, graph = bench.make_window(cuda, seed=2, H8=H, W8=W, NKF=NKF, buffer=8, add_edges=False, max_factors=32,
                                     intr=(12.0, 12.0, 8.0, 8.0))
    g = torch.Generator().manual_seed(9)
    # build the edges
    graph.add_neighborhood_factors(0, NKF, r=RAD)
    pool = video.static_pool(graph.update_op.packed_weights(torch.float16), torch.float16)
    assert graph.P_zr is pool.P_zr and graph.P_q is pool.P_q and pool.computed == NKF
    assert tuple(pool.P_zr.shape) == (8, 256, H, W) and tuple(pool.P_q.shape) == (8, 128, H, W) and pool.P_zr.dtype == torch.float16
    _check(graph, video, "built")
    # update
    graph.weight = torch.rand(graph.weight.shape, generator=g).to(cuda)
    p0 = video.poses.clone()
    graph.update(None, None, use_inactive=True)
    torch.cuda.synchronize()
    assert torch.isfinite(video.poses).all() and torch.isfinite(graph.net.float()).all() and not torch.equal(video.poses, p0)
    _check(graph, video, "updated")
    # the newest frame's edges dropped and re-added: no static convolution runs
    newest = NKF - 1
    pairs = [(i, j) for i, j in zip(graph._ii_h, graph._jj_h) if newest in (i, j)]
    graph.rm_factors([newest in (i, j) for i, j in zip(graph._ii_h, graph._jj_h)])
    graph.add_factors([p[0] for p in pairs], [p[1] for p in pairs])
    assert pool.computed == NKF
    _check(graph, video, "re-added")
    graph.update(None, None, use_inactive=True)
    # a second graph on the same video shares the pools, and computes nothing either
    other = FactorGraph(video, graph.update_op, device=cuda, max_factors=8)
    other.add_factors([0, 1], [1, 0])
    assert other.P_zr is graph.P_zr and other.P_q is graph.P_q and pool.computed == NKF
    other.update(None, None)
    _check(other, video, "second graph")
    # rm_keyframe: frame 3 takes frame 4's place, rows included
    inp4 = video.inps[4].clone()
    graph.rm_keyframe(3)
    video.counter -= 1
    assert torch.equal(video.inps[3], inp4) and pool.valid(3) and pool.computed == NKF
    assert 3 in graph._ii_h and max(graph._ii_h) == 3
    _check(graph, video, "keyframe removed")
    # a new keyframe and its edges: one frame is convolved
    fmap, net, inp = _frame(g, cuda)
    video.append(4.0, video.poses[3].clone(), torch.ones(H, W, device=cuda), video.intrinsics[0].clone(), fmap, net, inp)
    assert not pool.valid(4)
    graph.add_factors([4, 3, 4, 2], [3, 4, 2, 4])
    assert pool.computed == NKF + 1
    _check(graph, video, "keyframe appended")
    graph.update(None, None, use_inactive=True)
    torch.cuda.synchronize()
    assert torch.isfinite(graph.net.float()).all()
    # a frame's context features written directly, while no edge of it is live: its row is computed again when an edge needs it
    fmap, net, inp = _frame(g, cuda)
    video.append(5.0, video.poses[4].clone(), torch.ones(H, W, device=cuda), video.intrinsics[0].clone(), fmap, net, inp)
    graph.add_factors([5], [4])
    assert pool.computed == NKF + 2
    stale = graph.P_q[5].clone()
    graph.rm_factors([i == 5 for i in graph._ii_h])
    assert 5 not in graph._ii_h
    video.inps[5] = torch.relu(torch.randn(128, H, W, generator=g)).half().to(cuda)
    graph.add_factors([5], [4])
    assert pool.computed == NKF + 3 and not torch.equal(graph.P_q[5], stale)
    _check(graph, video, "foreign write")
