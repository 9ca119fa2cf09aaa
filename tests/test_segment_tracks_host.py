"""Segment association on the host: tests/segment_assoc_reference.py against its planted counts and its mutants, dense_labels, and the
SegmentTracks ledger's rules with the native call replaced by the reference (pvo_amd/segment_tracks.py is plain torch)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import segment_assoc_reference as R
from pvo_amd.segment_tracks import SegmentTracks, dense_labels, graph_segment_associate


@pytest.mark.parametrize("name", sorted(R.PLANTED))
def test_the_reference_gives_the_planted_counts(name):
    c, want = R.PLANTED[name]()
    got = R.run(c)
    for k, v in want.items():
        assert np.array_equal(got[k], v), (name, k, got[k])
    assert (got["match"][:, 0] == -1).all() and np.array_equal(got["area_i"], got["overlap"].sum(2))
    assert np.array_equal(got["match"] >= 0, got["match_d"] > 0) and np.array_equal(got["match"] >= 0, got["match_n"] > 0)


def test_the_rounding_case_hinges_on_fp32():
    """0.49999997f + 0.5f is 1.0f in fp32 and below 1 in fp64: the planted pixel tells the two apart"""
    t = np.float32(0.49999997)
    assert np.floor(t + np.float32(0.5)) == 1.0 and np.floor(np.float64(t) + 0.5) == 0.0
    assert np.floor(np.float32(-0.50000006) + np.float32(0.5)) == -1.0
    assert float(np.float32(R.MIN_IOU)) * 10 > 3 and np.float32(3) / np.float32(10) >= np.float32(R.MIN_IOU)      # the sliver's 3 / 10


@pytest.mark.parametrize("size", R.SIZES)
def test_the_scene_is_what_its_docstring_says(size):
    sc = R.scene(*size)
    got = R.run(sc, valid=None, cls=None)
    p0, p1, p2 = sc["perm"][0], sc["perm"][1], sc["perm"][2]
    ov = got["overlap"]
    assert (ov[0, p0[4], p1[4]], got["area_i"][0, p0[4]], got["area_j"][0, p1[4]]) == (3, 6, 7) and got["match"][0, p0[4]] == -1
    assert ov[0, p0[5], p1[5]] == ov[0, p0[5], p1[6]] == 4 and got["match"][0, p0[5]] == min(p1[5], p1[6])       # best_j ties: the lowest b
    a = min(p1[5], p1[6])
    assert got["match"][1, a] == p2[5] and got["match"][1, max(p1[5], p1[6])] == -1                                # best_i ties: the lowest a
    assert got["area_i"][0, 0] == 0 and got["area_j"][0, 0] == 2 * size[0]                                         # the strip leaves the frame
    assert np.array_equal(got["match"][4, 1:], np.where(got["area_j"][4, 1:] > 0, np.arange(1, R.S), -1))         # the self edge
    for e, (i, j) in enumerate(R.EDGES[:4]):                                  # the rectangle and the disc follow their motion
        for t in (2, 3):
            assert got["match"][e, sc["perm"][i][t]] == sc["perm"][j][t], (e, t)


@pytest.mark.parametrize("size", R.SIZES)
@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_changes_the_scene(size, mutant):
    sc = R.scene(*size)
    assert not R.same(R.run(sc, valid=None, cls=None, mutant=mutant), R.run(sc, valid=None, cls=None)), (size, mutant)


def test_riders_and_spread_labels():
    sc = R.scene(9, 12)
    plain, masked, vetoed = R.run(sc, valid=None, cls=None), R.run(sc, cls=None), R.run(sc, valid=None)
    assert masked["overlap"].sum() < plain["overlap"].sum() and np.array_equal(masked["area_j"], plain["area_j"])
    p0, p1 = sc["perm"][0], sc["perm"][1]
    assert vetoed["match"][0, p0[5]] == p1[5] and np.array_equal(vetoed["overlap"], plain["overlap"])              # half 6 is another class
    for S in (48, 128, 160):
        wide = R.spread(sc, S)
        assert wide["labels"].max() > S // 2 and len(np.unique(wide["labels"])) == len(np.unique(sc["labels"]))
        for kw in (dict(valid=None, cls=None), dict()):
            a, b = R.run(wide, S=S, **kw), R.run(sc, **kw)
            assert np.array_equal(a["match_n"].sum(1), b["match_n"].sum(1)) and np.array_equal(np.sort(a["area_j"], 1)[:, -R.S:], np.sort(b["area_j"], 1))


def test_dense_labels_against_numpy():
    rng = np.random.RandomState(0)
    raw = rng.choice([-7, 0, 3, 26001, 26002, 41000, 2 ** 31 - 1], size=(4, 6, 5)).astype(np.int32)
    raw[2] = 0                                                                # a frame with no segments
    raw[3] = np.where(raw[3] > 0, 3, raw[3])                                  # and one with a single segment
    dense, ids, count = dense_labels(torch.from_numpy(raw))
    assert dense.dtype == torch.int32 and ids.dtype == torch.int32 and count.dtype == torch.int64
    S = ids.shape[1]
    assert S == 1 + max(len(np.unique(f[f > 0])) for f in raw)
    for f in range(4):
        u = np.unique(raw[f][raw[f] > 0])
        assert int(count[f]) == len(u) and ids[f, 1:1 + len(u)].tolist() == u.tolist() and not ids[f, 1 + len(u):].any() and ids[f, 0] == 0
        want = np.where(raw[f] > 0, 1 + np.searchsorted(u, raw[f]), 0)
        assert np.array_equal(dense[f].numpy(), want)
    d0, i0, c0 = dense_labels(torch.zeros(2, 3, 3, dtype=torch.int32))
    assert not d0.any() and i0.shape == (2, 1) and c0.tolist() == [0, 0]
    assert dense_labels(torch.zeros(0, 3, 3, dtype=torch.int32))[1].shape == (0, 1)


# ------------------------------------------------------------------------------------------------------------------ the ledger
def _graph(edges, ids, tstamp=None):
    """a graph as the ledger reads it: host edge lists and the video's stamps; `ids` [n][S] are the raw ids behind the dense labels"""
    n = len(ids)
    video = SimpleNamespace(tstamp=torch.tensor(tstamp if tstamp is not None else [10.0 * k for k in range(n)]), counter=n)
    return SimpleNamespace(_ii_h=[e[0] for e in edges], _jj_h=[e[1] for e in edges], video=video)


def _tables(edges, ids, matches):
    """solve= for SegmentTracks: matches[(i, j)] = {a: (b, n, d)}"""
    S = len(ids[0])
    calls = []

    def solve(graph, edges=None, min_iou=0.25, cls_div=None):
        calls.append(list(edges))
        E = len(edges)
        m, n, d = -torch.ones(E, S, dtype=torch.int32), torch.zeros(E, S, dtype=torch.int32), torch.zeros(E, S, dtype=torch.int32)
        for k, e in enumerate(edges):
            for a, (b, nn, dd) in matches.get((graph._ii_h[e], graph._jj_h[e]), {}).items():
                m[k, a], n[k, a], d[k, a] = b, nn, dd
        return dict(match=m, match_n=n, match_d=d, ids=torch.tensor(ids, dtype=torch.int32),
                    ii=torch.tensor([graph._ii_h[e] for e in edges]), jj=torch.tensor([graph._jj_h[e] for e in edges]))
    return solve, calls


def test_inheritance_and_fresh_ids():
    ids = [[0, 10, 20, 0], [0, 7, 9, 11]]
    edges = [(1, 0), (0, 1)]                                                  # (the backward edge is not walked)
    solve, calls = _tables(edges, ids, {(0, 1): {1: (2, 5, 8), 2: (1, 3, 9)}, (1, 0): {1: (1, 9, 9)}})
    st = SegmentTracks(solve=solve)
    st.observe(_graph(edges, ids))
    assert calls == [[1]]
    # frame 0 has nothing to lean on: fresh ids in ascending raw id; frame 1 inherits through the matches, raw 11 is unmatched
    assert st.entries == {(0.0, 10): 1, (0.0, 20): 2, (10.0, 9): 1, (10.0, 7): 2, (10.0, 11): 3}
    assert st.table() == [(0.0, 10, 1), (0.0, 20, 2), (10.0, 7, 2), (10.0, 9, 1), (10.0, 11, 3)]
    assert st.tracks() == {1: [(0.0, 10), (10.0, 9)], 2: [(0.0, 20), (10.0, 7)], 3: [(10.0, 11)]}
    assert SegmentTracks(solve=solve).observe(_graph([(1, 0)], ids)) == 0 and len(calls) == 1      # no forward edge: nothing is solved


def test_two_claimants_of_one_track_and_the_order_of_candidates():
    ids = [[0, 10, 0], [0, 30, 0], [0, 5, 6]]
    edges = [(0, 2), (1, 2), (0, 1)]
    # frame 1's segment inherits track 1 from frame 0; frame 2's b = 1 claims track 1 over (0, 2) with 1 / 2, b = 2 over (1, 2) with 3 / 4
    solve, _ = _tables(edges, ids, {(0, 1): {1: (1, 4, 5)}, (0, 2): {1: (1, 1, 2)}, (1, 2): {1: (2, 3, 4)}})
    st = SegmentTracks(solve=solve)
    st.observe(_graph(edges, ids))
    assert st.entries == {(0.0, 10): 1, (10.0, 30): 1, (20.0, 6): 1, (20.0, 5): 2}           # the larger IoU keeps it, the loser is fresh
    # one segment, two candidates of EQUAL IoU (1 / 2 and 2 / 4) with different tracks: the larger i wins
    ids = [[0, 10], [0, 30], [0, 5]]
    solve, _ = _tables(edges[:2], ids, {(0, 2): {1: (1, 1, 2)}, (1, 2): {1: (1, 2, 4)}})
    st = SegmentTracks(solve=solve)
    st.observe(_graph(edges[:2], ids))
    assert st.entries == {(0.0, 10): 1, (10.0, 30): 2, (20.0, 5): 2}
    solve, _ = _tables(edges[:2], ids, {(0, 2): {1: (1, 2, 3)}, (1, 2): {1: (1, 2, 4)}})      # 2 / 3 > 2 / 4: the IoU comes first
    st = SegmentTracks(solve=solve)
    st.observe(_graph(edges[:2], ids))
    assert st.entries[(20.0, 5)] == 1
    # the same i, equal IoU: the lower a
    ids = [[0, 10, 20], [0, 5, 0]]
    solve, _ = _tables([(0, 1)], ids, {(0, 1): {2: (1, 1, 2), 1: (1, 2, 4)}})
    st = SegmentTracks(solve=solve)
    st.observe(_graph([(0, 1)], ids))
    assert st.entries[(10.0, 5)] == 1


def test_the_first_assignment_sticks_and_remove():
    ids = [[0, 10, 20], [0, 7, 9]]
    edges = [(0, 1)]
    solve, _ = _tables(edges, ids, {(0, 1): {1: (2, 5, 8), 2: (1, 3, 9)}})
    st = SegmentTracks(solve=solve)
    st.observe(_graph(edges, ids))
    first = dict(st.entries)
    swapped, _ = _tables(edges, ids, {(0, 1): {1: (1, 5, 8), 2: (2, 3, 9)}})                   # a later update sees it the other way round
    st._solve = swapped
    st.observe(_graph(edges, ids))
    assert st.entries == first and st.observations == 2
    st.remove(10.0)                                                           # the keyframe goes; the next one in its slot is matched anew
    assert st.entries == {(0.0, 10): 1, (0.0, 20): 2}
    st.observe(_graph(edges, ids, tstamp=[0.0, 15.0]))
    assert st.entries == {(0.0, 10): 1, (0.0, 20): 2, (15.0, 7): 1, (15.0, 9): 2} and st.next_id == 3
    # a track already held by a segment of the keyframe is not given to a second one
    ids3 = [[0, 10, 20], [0, 7, 9, 8]]
    late, _ = _tables(edges, [r + [0] * (4 - len(r)) for r in ids3], {(0, 1): {1: (3, 7, 8)}})
    st._solve = late
    st.observe(_graph(edges, ids3, tstamp=[0.0, 15.0]))
    assert st.entries[(15.0, 8)] == 3 and st.entries[(15.0, 7)] == 1


def test_track_map_is_a_table_gather():
    raw = torch.tensor([[[10, 10, 20], [0, -4, 20]], [[9, 7, 7], [7, 11, 0]]], dtype=torch.int32)
    video = SimpleNamespace(segms_raw=raw, tstamp=torch.tensor([0.0, 10.0, 99.0]), counter=2)
    st = SegmentTracks(video)
    st.entries = {(0.0, 10): 1, (0.0, 20): 2, (10.0, 9): 1, (10.0, 7): 5}                        # raw 11 has no track
    tm = st.track_map()
    assert tm.dtype == torch.int32 and tm.tolist() == [[[1, 1, 2], [0, 0, 2]], [[1, 5, 5], [5, 0, 0]]]
    video.counter = 0                                                         # before the first keyframe: an empty map, not an error
    none = st.track_map()
    assert none.shape == (0, 2, 3) and none.dtype == torch.int32


def _sequence(size, nframes=6):
    """the plain scene as a video and a graph, and solve= through the reference: raw ids 26000 + 10 * the frame's permuted label"""
    edges = tuple((k, k + 1) for k in range(nframes - 1)) + tuple((k, k + 2) for k in range(nframes - 2)) + ((3, 1),)
    sc = R.scene(*size, nframes=nframes, edges=edges, plain=True)
    raw = torch.from_numpy(np.where(sc["labels"] > 0, 26000 + 10 * sc["labels"], 0).astype(np.int32))
    video = SimpleNamespace(segms_raw=raw, tstamp=torch.arange(nframes).float() * 2.5, counter=nframes)

    def native(ops, min_iou):
        assert ops["labels"].dtype == torch.int32 and ops["valid"] is None and ops["cls"] is None
        got = R.associate(ops["labels"].numpy(), ops["ii"].numpy(), ops["jj"].numpy(), ops["target"].numpy(), ops["S"], min_iou=min_iou)
        return {k: torch.from_numpy(v) for k, v in got.items()}

    def graph(upto):
        keep = [e for e, (i, j) in enumerate(edges) if i < upto and j < upto]
        ii, jj = torch.tensor([edges[e][0] for e in keep]), torch.tensor([edges[e][1] for e in keep])
        t = torch.from_numpy(sc["target"][keep])
        ys, xs = torch.meshgrid(torch.arange(size[0]).float(), torch.arange(size[1]).float(), indexing="ij")
        coords0 = torch.stack([xs, ys], -1)[None].expand_as(t)
        z = torch.zeros(nframes, *size)
        return SimpleNamespace(video=SimpleNamespace(segms_raw=raw, segms=None, poses=z, disps=z, intrinsics=torch.ones(1, 4), tstamp=video.tstamp, counter=upto),
                               ii=ii, jj=jj, _ii_h=ii.tolist(), _jj_h=jj.tolist(), ht=size[0], wd=size[1], coords0=coords0, full_flow=t - coords0)

    solve = lambda g, **kw: graph_segment_associate(g, native=native, **kw)
    return sc, video, graph, solve


@pytest.mark.parametrize("size", ((9, 12), (24, 32)))
def test_a_sequence_with_permuted_ids_gets_the_true_ids_up_to_one_bijection(size):
    sc, video, graph, solve = _sequence(size)
    st = SegmentTracks(video, solve=solve)
    for upto in (3, 4, 6):                                                    # the window grows, as the frontend's does
        st.observe(graph(upto))
    tm = st.track_map().numpy()
    truth = sc["truth"]
    pairs = set(zip(truth.ravel().tolist(), tm.ravel().tolist()))
    assert len(pairs) == len({p[0] for p in pairs}) == len({p[1] for p in pairs}) == 4 and (0, 0) in pairs, pairs
    assert not np.array_equal(sc["labels"], truth)                            # (the ids as given are NOT consistent)
    out = st.last
    assert out["ids"].shape[0] == 6 and set(R.OUTPUTS) <= set(out)


def test_object_tracks_by_track():
    """Droid.get_object_tracks(by_track=True): the entries re-keyed by the track of (tstamp_i, label); one without a track is left out"""
    from pvo_amd.droid import Droid
    entry = lambda ti, tj, label: dict(tstamp_i=ti, tstamp_j=tj, label=label, count=100, status=0)
    by_label = {7: [entry(0.0, 1.0, 7)], 9: [entry(1.0, 2.0, 9), entry(2.0, 3.0, 9)], 4: [entry(0.0, 1.0, 4)]}
    ledger = SimpleNamespace(entries={(0.0, 7): 1, (1.0, 9): 1, (2.0, 9): 2})
    fake = SimpleNamespace(frontend=SimpleNamespace(object_tracks=SimpleNamespace(tracks=lambda: by_label)), segment_tracks=ledger, flush=lambda: None)
    assert Droid.get_object_tracks(fake) is by_label
    got = Droid.get_object_tracks(fake, by_track=True)
    assert {k: [(e["tstamp_i"], e["label"], e["track"]) for e in v] for k, v in got.items()} == {1: [(0.0, 7, 1), (1.0, 9, 1)], 2: [(2.0, 9, 2)]}
    fake.segment_tracks = None
    with pytest.raises(RuntimeError, match="segment_tracks"):
        Droid.get_object_tracks(fake, by_track=True)


def test_segment_tracks_need_the_raw_ids():
    from pvo_amd.droid import Droid, default_args
    with pytest.raises(ValueError, match="store_segment_ids"):
        Droid(default_args(device="cpu", segment_tracks=True))
    assert default_args().segment_tracks is None
    g = SimpleNamespace(video=SimpleNamespace(segms_raw=None))
    with pytest.raises(ValueError, match="store_segment_ids"):
        graph_segment_associate(g)


def test_export_tool_takes_track_ids_only_with_panoptic():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import export_map
    base = ["--datapath", "x", "--map", "a.ply", "--mesh", "m.ply", "--voxel", "0.05"]
    assert export_map.parse_args(base).track_ids is False
    assert export_map.parse_args(base + ["--panoptic", "--track_ids"]).track_ids is True
    with pytest.raises(SystemExit):
        export_map.parse_args(base + ["--track_ids"])
