"""Object motion, the yardstick held to itself and the host layer (CPU, seconds): tests/object_motion_reference.py recovers the sphere's
true motion and the plane's identity, the conditions the GPU tests rely on (member counts, cond(H), at most 1 % of the pixels flagged on
every case they run), every deliberately wrong reference at least 10 bounds away in some output, the Jacobian against finite differences,
the struct mirror against the header; pvo_amd.object_motion's edge_jobs against a brute-force loop, ObjectTracks' bookkeeping with a stub
in place of the native call, and FactorGraph.object_motion's operand assembly on CPU tensors."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import object_motion_reference as M

_cache = {}
SPHERE, PLANE = (0, 3, 6), (1, 4, 7)            # M.jobs' indices of the two segments on the edges (1,2), (3,1), (0,4)


def _scene(size, exact=False):
    if ("scene", size, exact) not in _cache:
        _cache[("scene", size, exact)] = M.scene(*size, exact=exact)
    return _cache[("scene", size, exact)]


def _run(size, case="plain", start=None, mutant=None, exact=False, **kw):
    key = (size, case, start, mutant, exact, tuple(sorted(kw.items())))
    if key not in _cache:
        sc = _scene(size, exact)
        je, jl = M.jobs(sc)
        args = dict(M.PARAMS, **M.CASES[case])
        args.update(kw)
        s = M.perturbed_start(sc, je) if start == "perturbed" else None
        _cache[key] = M.motion_reference(sc, je, jl, start=s, mutant=mutant, store32=not exact, **args)
    return _cache[key]


@pytest.mark.parametrize("size", M.SIZES)
def test_the_reference_recovers_the_motion_and_the_identity(size):
    sc, Tw = _scene(size), M.true_motion()
    exact, ref = _run(size, exact=True), _run(size)
    je, _ = M.jobs(sc)
    for n in SPHERE:
        # fp64 throughout, exact targets: eight steps from the NULL start reach the true A
        # (the motion goes through the cameras' quaternions as stored in fp32, each within 2 EPS of unit length: 16 EPS covers the four uses)
        assert M.pose_difference(exact["rel"][n], sc["truth"][je[n]]) < 1e-10 and M.pose_difference(exact["motion"][n], Tw) < 16 * M.EPS
        d = M.pose_difference(ref["motion"][n], Tw)
        print(size, "job", n, "motion to truth %.3e, truth_bound %.3e, pose_bound %.3e" % (d, ref["truth_bound"][n], ref["pose_bound"][n]))
        assert d <= ref["truth_bound"][n] < 5e-3
    for n in PLANE:
        assert exact["info"][n, 0, 0] < 1e-20 and M.pose_difference(exact["motion"][n], M.IDENTITY) < 16 * M.EPS
        assert ref["info"][n, 0, 0] < 1e-6 and M.pose_difference(ref["motion"][n], M.IDENTITY) <= ref["truth_bound"][n]
    n = 9                                                                   # edge (2,2): frame 2 is the identity camera
    assert np.array_equal(ref["motion"][n], ref["rel"][n]) and M.pose_difference(ref["motion"][n], Tw) <= ref["truth_bound"][n]


@pytest.mark.parametrize("size", M.SIZES)
def test_the_scene_gives_what_the_gpu_tests_rely_on(size):
    ref = _run(size)
    print(size, "cond(H) at the start: sphere", np.round(ref["cond"][list(SPHERE)]), "plane", np.round(ref["cond"][list(PLANE)]))
    assert np.all(np.isfinite(ref["cond"][list(SPHERE)]))
    # 163 / 23 / 54 contributing pixels on edge (1,2); frames 3 and 0 see the sphere a little smaller at 24 x 32 (159 and 162)
    counts = [int(ref["info"][n, 0, 1]) for n in SPHERE]
    print(size, "sphere pixels on the three edges", counts)
    assert counts[0] >= M.MIN_MEMBERS[size] and min(counts) >= M.MIN_MEMBERS[size] - 4
    assert M.MIN_MEMBERS[size] >= M.PARAMS["min_count"]
    status = ref["info"][:, -1, 3]
    assert np.array_equal(status, [0, 0, 1] * 4 + [1, 0, 4])
    assert np.all(ref["info"][[2, 5, 8, 11], :, 1] == 4) and np.all(ref["info"][12, :, 1] == 0) and not ref["centroid"][12].any()
    assert np.all(ref["info"][14] == (0, 0, 0, 4)) and np.array_equal(ref["motion"][14], M.IDENTITY)


@pytest.mark.parametrize("size", M.SIZES)
@pytest.mark.parametrize("case", sorted(M.CASES))
def test_few_pixels_sit_on_a_decision(size, case):
    """the flagged share of the reference alone, on every case the GPU test runs.  The z_min variants: 1.15 cuts through the sphere, 1.5
    leaves it out"""
    for start, iters in ((None, 0), ("perturbed", 0), ("perturbed", 1), (None, 8), ("perturbed", 8)):
        ref = _run(size, case, start, iters=iters)
        share = ref["flagged"].mean()
        print(size, case, start, iters, "flagged %.4f" % share)
        assert share <= 0.01
    if case == "huber":                                                     # the variant does what it is there for
        ref = _run(size, case, "perturbed", iters=0)
        a = np.sqrt((ref["residual"] ** 2).sum(-1))[ref["votes"]]            # (over all jobs: both branches of k are taken)
        assert (a > 0.5).mean() > 0.1 and (a <= 0.5).mean() > 0.1
    if case == "zcut":
        assert 0 < _run(size, case, None, iters=0)["info"][0, 0, 1] < _run(size, "plain", None, iters=0)["info"][0, 0, 1]
    if case == "zfar":
        z = _run(size, case, None, iters=0)["info"]
        assert z[0, 0, 1] == 0 and z[0, 0, 3] == 1 and z[1, 0, 1] == _run(size, "plain", None, iters=0)["info"][1, 0, 1]


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_every_mutant_is_far_from_the_reference(mutant):
    """the bound is not vacuous: each deliberately wrong variant is at least 10 bounds away in some output of some case"""
    worst = 0.0
    for size in M.SIZES:
        for case, start, iters in (("plain", "perturbed", 1), ("plain", None, 8), ("huber", "perturbed", 0), ("huber", "perturbed", 8)):
            g = M.gap(_run(size, case, start, mutant=mutant, iters=iters), _run(size, case, start, iters=iters))
            print(mutant, size, case, start, iters, "gap %.3g bounds" % g)
            worst = max(worst, g)
    assert worst >= 10.0


def test_the_reference_passes_its_own_check_and_a_mutant_does_not():
    ref = _run((13, 19), "plain", "perturbed", iters=1)
    ok, report = M.motion_matches(M.as_got(ref), ref)
    assert ok, report
    ok, report = M.motion_matches(M.as_got(_run((13, 19), "plain", "perturbed", mutant="right_retraction", iters=1)), ref)
    assert not ok, report


def test_the_jacobian_is_the_derivative_of_the_residual():
    size = (13, 19)
    sc = _scene(size)
    A = M.perturbed_start(sc, np.array([0]))[0]
    ev = M.evaluate(sc, 0, 2, A)
    h = 1e-6
    for k in range(6):
        xi = np.zeros(6); xi[k] = h
        d = np.concatenate(M.T.se3_exp(xi))
        up = M.evaluate(sc, 0, 2, M.pose_mul(d, A))
        d[:3], d[3:6] = -d[:3], -d[3:6]
        dn = M.evaluate(sc, 0, 2, M.pose_mul(d, A))
        v = ev["votes"]
        num = (up["r"][v] - dn["r"][v]) / (2 * h)
        assert np.allclose(num, ev["J"][v][..., k], rtol=1e-5, atol=1e-5), k


def test_the_struct_mirror_follows_the_header():
    from pvo_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvo_hip.h")).read()
    name, mirror = "pvo_object_motion_args", _lib.ObjectMotionArgs
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    fields = []
    for line in body.split(";"):
        line = line.strip()
        if not line:
            continue
        names = line.split(",")
        names[0] = names[0].split()[-1]
        fields += [re.sub(r"[\*\s]|\[\d+\]", "", v) for v in names]
    assert fields == [f[0] for f in mirror._fields_] and mirror.__doc__ == name
    lib = _lib.load()
    assert lib.pvo_object_motion_args_size() == ctypes.sizeof(mirror)
    assert _lib.OBJECT_MOTION_MAX_ITERS == int(re.search(r"#define PVO_OBJECT_MOTION_MAX_ITERS (\d+)", header).group(1))
    assert lib.pvo_version() == 106 == _lib.PVO_ABI_VERSION and "still 106, object motion" in header
    assert lib.pvo_object_motion_workspace_bytes(0, 24, 32) == 0 and lib.pvo_object_motion_workspace_bytes(3, 24, 32) >= 3 * (64 + 3 * 128)
    from pvo_amd import build
    assert "object_motion.hip" in build.HIP_SOURCES


# ------------------------------------------------------------------------------------------------------------ the host layer
def _brute_jobs(labels, ii, min_pixels, member=None, skip=(0,)):
    out = []
    for e, i in enumerate(ii.tolist()):
        lab = labels[i]
        for l in sorted(set(lab.reshape(-1).tolist())):
            if l in skip:
                continue
            m = lab == l
            if member is not None:
                m = m & member[e]
            if int(m.sum()) >= min_pixels and int(m.sum()) > 0:
                out.append((e, l, int(m.sum())))
    return out


def test_edge_jobs_against_a_brute_force_loop():
    from pvo_amd.object_motion import edge_jobs
    g = torch.Generator().manual_seed(0)
    labels = torch.randint(-2, 6, (4, 7, 9), generator=g).int()
    labels[labels == 4] = 1000                                              # (any integers)
    ii, jj = torch.tensor([2, 0, 3, 3, 1]), torch.tensor([1, 1, 2, 0, 0])
    member = torch.rand(5, 7, 9, generator=g) < 0.6
    for kw in (dict(min_pixels=1), dict(min_pixels=9), dict(min_pixels=5, member=member), dict(min_pixels=1, skip=(0, 1000, -1)),
               dict(min_pixels=1, skip=())):
        je, jl, px = edge_jobs(labels, ii, jj, **kw)
        want = _brute_jobs(labels, ii, **kw)
        assert je.dtype == torch.int64 and jl.dtype == torch.int32 and px.dtype == torch.int64
        assert list(zip(je.tolist(), jl.tolist(), px.tolist())) == want and want == sorted(want), kw
    assert len(_brute_jobs(labels, ii, 1)) > len(_brute_jobs(labels, ii, 9)) > 0
    for je, jl, px in (edge_jobs(labels, ii, jj, 64), edge_jobs(labels, ii[:0], jj[:0], 1), edge_jobs(torch.zeros(4, 7, 9).int(), ii, jj, 1)):
        assert je.shape == jl.shape == px.shape == (0,) and je.dtype == torch.int64 and jl.dtype == torch.int32      # an empty result


def _fake_graph(raw_ids):
    g = torch.Generator().manual_seed(1)
    ht, wd, E, F = 6, 8, 3, 4
    segms = torch.zeros(F, 1, ht, wd, dtype=torch.int32)
    segms[:, 0, :, 4:] = 1
    segms[:, 0, :2, :2] = 2
    raw = None
    if raw_ids:
        raw = torch.full((F, ht, wd), 40, dtype=torch.int32)
        raw[:, 3:] = 50
    video = SimpleNamespace(poses=torch.randn(F, 7, generator=g), disps=torch.rand(F, ht, wd, generator=g) + 0.5,
                            intrinsics=torch.tensor([[6.0, 6.0, 3.5, 2.5]]).repeat(F, 1), segms=segms, segms_raw=raw)
    y, x = torch.meshgrid(torch.arange(ht).float(), torch.arange(wd).float(), indexing="ij")
    raw_mask = torch.full((1, E, ht, wd, 2), 3.0)
    raw_mask[0, 1, :, 4:, 0] = -3.0                                          # edge 1: the right half is dynamic
    return SimpleNamespace(video=video, ht=ht, wd=wd, coords0=torch.stack([x, y], -1), full_flow=torch.randn(1, E, ht, wd, 2, generator=g),
                           ii=torch.tensor([0, 1, 2]), jj=torch.tensor([1, 2, 3]), raw_mask=raw_mask, dy_thresh=0.5)


def test_factor_graph_object_motion_assembles_its_operands():
    from pvo_amd.factor_graph import FactorGraph
    seen = {}

    def native(ops, job_edge, job_label, **kw):
        seen.update(ops=ops, job_edge=job_edge, job_label=job_label, kw=kw)
        return dict(rel=torch.zeros(len(job_edge), 7))

    graph = _fake_graph(False)
    out = FactorGraph.object_motion(graph, min_pixels=4, native=native, iters=3)
    ops = seen["ops"]
    assert torch.equal(ops["target"], (graph.coords0 + graph.full_flow)[0]) and ops["target"].shape == (3, 6, 8, 2) and ops["target"].is_contiguous()
    assert torch.equal(ops["labels"], graph.video.segms[:, 0]) and ops["labels"].dtype == torch.int32      # no raw ids stored: the dense ones
    assert ops["poses"] is graph.video.poses and ops["disps"] is graph.video.disps and torch.equal(ops["intrinsics"], graph.video.intrinsics[0])
    assert seen["kw"] == dict(iters=3)
    assert list(zip(seen["job_edge"].tolist(), seen["job_label"].tolist())) == [(e, l) for e in range(3) for l in (1, 2)]      # 0: no segment
    assert set(out) == {"rel", "job_edge", "job_label", "ii", "jj"} and torch.equal(out["ii"], graph.ii)
    out = FactorGraph.object_motion(graph, min_pixels=5, native=native)
    assert out["job_label"].tolist() == [1, 1, 1]                                                            # the 2 x 2 patch is too small
    out = FactorGraph.object_motion(graph, edges=[2, 1], min_pixels=4, native=native)
    assert out["ii"].tolist() == [2, 1] and torch.equal(seen["ops"]["target"], (graph.coords0 + graph.full_flow)[0, [2, 1]])
    out = FactorGraph.object_motion(graph, min_pixels=4, dynamic_share=0.9, native=native)
    assert list(zip(out["job_edge"].tolist(), out["job_label"].tolist())) == [(1, 1)]                       # only edge 1's right half moves
    assert FactorGraph.object_motion(graph, min_pixels=4, dynamic_share=1.01, native=native)["job_edge"].numel() == 0
    graph = _fake_graph(True)                                                                                # raw ids stored: they are the labels
    out = FactorGraph.object_motion(graph, min_pixels=4, native=native)
    assert torch.equal(seen["ops"]["labels"], graph.video.segms_raw) and sorted(set(out["job_label"].tolist())) == [40, 50]


def test_object_tracks_bookkeeping():
    from pvo_amd.object_motion import ObjectTracks
    calls = []

    def solve(graph, edges, min_pixels, dynamic_share, **kw):
        calls.append((list(edges), min_pixels, dynamic_share, kw))
        n = len(edges)
        je = torch.arange(n).repeat_interleave(2)
        info = torch.zeros(2 * n, 1, 4)
        info[:, 0, 0], info[:, 0, 1] = float(len(calls)), 70.0
        info[1::2, 0, 3] = 1.0
        motion = torch.zeros(2 * n, 7)
        motion[:, 0] = float(len(calls))
        return dict(motion=motion, centroid=torch.ones(2 * n, 3), info=info, job_edge=je, job_label=torch.tensor([5, 3] * n, dtype=torch.int32),
                    ii=torch.tensor([graph._ii_h[e] for e in edges]), jj=torch.tensor([graph._jj_h[e] for e in edges]))

    video = SimpleNamespace(tstamp=torch.tensor([0.0, 2.0, 3.0, 7.0, 9.0]))
    graph = SimpleNamespace(video=video, _ii_h=[0, 1, 0, 1, 2, 1], _jj_h=[1, 0, 2, 2, 3, 2])
    assert ObjectTracks.consecutive(graph._ii_h, graph._jj_h) == [0, 3, 4]
    led = ObjectTracks(video, min_pixels=32, dynamic_share=0.5, solve=solve, iters=4)
    assert led.observe(SimpleNamespace(video=video, _ii_h=[1, 2], _jj_h=[0, 0])) == 0 and not calls      # no edge (k, k + 1): no call
    assert led.observe(graph) == 6
    assert calls == [([0, 3, 4], 32, 0.5, dict(centroid=True, iters=4))]
    assert sorted(led.entries) == [(0.0, 2.0, 3), (0.0, 2.0, 5), (2.0, 3.0, 3), (2.0, 3.0, 5), (3.0, 7.0, 3), (3.0, 7.0, 5)]
    e = led.entries[(2.0, 3.0, 3)]
    assert (e["count"], e["status"], e["E"], e["label"], e["tstamp_i"], e["tstamp_j"]) == (70, 1, 1.0, 3, 2.0, 3.0) and e["motion"][0] == 1.0
    graph._ii_h, graph._jj_h = [2, 3], [3, 4]                                 # a later observation replaces (3, 7) and adds (7, 9)
    assert led.observe(graph) == 4
    assert led.entries[(3.0, 7.0, 5)]["motion"][0] == 2.0 and led.entries[(2.0, 3.0, 5)]["motion"][0] == 1.0 and len(led.entries) == 8
    tracks = led.tracks()                                                     # per label, in time order
    assert sorted(tracks) == [3, 5] and [(t["tstamp_i"], t["tstamp_j"]) for t in tracks[5]] == [(0.0, 2.0), (2.0, 3.0), (3.0, 7.0), (7.0, 9.0)]
    led.remove(3.0)                                                           # the keyframe stamped 3 is removed: both its pairs go
    assert sorted(k[:2] for k in led.entries if k[2] == 5) == [(0.0, 2.0), (7.0, 9.0)] and len(led.entries) == 4


def test_the_switch_is_off_by_default_and_the_binding_refuses_cpu_tensors():
    from pvo_amd import droid_backends as db
    from pvo_amd.droid import default_args
    from pvo_amd.frontend import DroidFrontend
    assert default_args().object_motion is None and DroidFrontend.object_tracks is None
    sc = _scene((9, 12))
    t = {k: torch.from_numpy(np.ascontiguousarray(sc[k])) for k in ("poses", "disps", "intr", "labels", "ii", "jj", "target")}
    with pytest.raises(ValueError, match="device tensor"):
        db.object_motion(t["poses"], t["disps"], t["intr"], t["labels"], t["ii"], t["jj"], t["target"], torch.zeros(1).long(), torch.zeros(1).int())
