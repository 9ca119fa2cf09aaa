"""The reprojection-family kernels (pvo_amd/csrc/geom.hip, depth_vote.h) against the fp64 yardstick of tests/geom_reference.py, which
tests/test_geom_fp64_host.py qualifies without a GPU: every value within its derived bound, every settled decision equal, every mutant
reference rejected; the bit identities between the entry points over the whole case list; guard rows around every output; refusals by
return code."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import geom_reference as R

pytestmark = pytest.mark.gpu

PVO_EINVAL = 1


@functools.lru_cache(maxsize=None)
def _graph(ht, wd):
    return R.graph_case(ht, wd)


@functools.lru_cache(maxsize=None)
def _ref(kind, ht, wd, extra=None, mutant=None):
    """the references are computed once per (kind, case, mutant) and shared; nobody writes to them"""
    poses, disps, intr, ii, jj = _graph(ht, wd)
    if kind == "projmap":
        return R.projmap(poses, disps, intr[0], ii, jj, mutant=mutant)
    if kind == "iproj":
        return R.iproj(poses, disps, intr[0], mutant=mutant)
    if kind == "reproject":
        return R.reproject(poses, disps, intr, ii, jj, baseline=extra or 0.0, mutant=mutant)
    return R.frame_distance(poses, disps, intr[0], ii, jj, extra, mutant=mutant)


def _dev(cuda, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


def _np(*ts):
    return [t.detach().cpu().numpy() for t in ts]


def _hold(kind, got, ht, wd, extra=None, skip=()):
    ok, rep = R.check(kind, got, _ref(kind, ht, wd, extra))
    print("%dx%d %-14s %-6s worst err/bound %.3f unsettled %.4f" % (ht, wd, kind, "" if extra is None else extra, rep["worst"], rep["unsettled"]))
    assert ok, (kind, extra, rep)
    for m in R.MUTANTS[kind]:
        if m in skip:
            continue
        assert R.check(kind, got, _ref(kind, ht, wd, extra, m))[1]["mismatches"] > 0, (kind, extra, m)
    return rep


@pytest.mark.parametrize("ht,wd", R.GRAPH_MAPS + R.LINE_MAPS)
def test_projmap_iproj_and_reproject_stay_within_their_bounds(cuda, ht, wd):
    from pvo_amd import droid_backends as db
    poses, disps, intr, ii, jj = _dev(cuda, *_graph(ht, wd))
    _hold("projmap", _np(*db.projmap(poses, disps, intr[0].contiguous(), ii, jj)), ht, wd)
    _hold("iproj", _np(db.iproj(poses, disps, intr[0].contiguous()))[0], ht, wd)
    c, v = db.reproject(poses, disps, intr, ii, jj)
    _hold("reproject", _np(c, v), ht, wd)
    out = torch.full((ii.numel(), ht, wd, 2), float("nan"), device=cuda)
    c2, v2 = db.reproject(poses, disps, intr, ii, jj, out=out)
    assert c2 is out and torch.equal(c2, c) and torch.equal(v2, v)
    cb, vb = db.reproject(poses, disps, intr, ii, jj, baseline=R.BASELINE)
    _hold("reproject", _np(cb, vb), ht, wd, extra=R.BASELINE)
    rig = ii == jj
    assert torch.equal(cb[~rig], c[~rig]) and not torch.equal(cb[rig], c[rig])
    out.fill_(float("nan"))
    c3, v3 = db.reproject(poses, disps, intr, ii, jj, out=out, baseline=R.BASELINE)
    assert c3 is out and torch.equal(c3, cb) and torch.equal(v3, vb)


@pytest.mark.parametrize("ht,wd", R.GRAPH_MAPS)
def test_frame_distance_stays_within_its_summation_bound(cuda, ht, wd):
    from pvo_amd import droid_backends as db
    poses, disps, intr, ii, jj = _dev(cuda, *_graph(ht, wd))
    for beta in R.BETAS:
        got = _np(db.frame_distance(poses, disps, intr[0].contiguous(), ii, jj, beta))[0]
        # ratio_fp32 differs from the contract only AT 0.75 (the exact edges below); beta = 1 has no translation-only term to drop
        _hold("frame_distance", got, ht, wd, extra=beta, skip=("ratio_fp32",) + (("no_beta",) if beta == 1.0 else ()))
        assert (got == 1000.0).any() and (got < 100.0).any()


@pytest.mark.parametrize("name", [c[0] for c in R.DEPTH_CASES])
def test_depth_filter_votes_equal_the_reference_where_settled(cuda, name):
    from pvo_amd import droid_backends as db
    case = R.depth_case(name)
    poses, disps, intr, ix, thresh = _dev(cuda, *case)
    got = _np(db.depth_filter(poses, disps, intr, ix, thresh))[0]
    ok, rep = R.check("depth_filter", got, R.depth_filter(*case))
    print("%-10s unsettled %.4f mismatches %d votes up to %d" % (name, rep["unsettled"], rep["mismatches"], got.max()))
    assert ok, rep
    for m in R.MUTANTS["depth_filter"]:
        rep = R.check("depth_filter", got, R.depth_filter(*case, mutant=m))[1]
        assert rep["mismatches"] > 0 or got.max() == 0, (name, m)        # (one frame, or a map no tap fits into: all votes 0)
    if name in ("1x3x5", "4x1x70", "4x70x1"):
        assert got.max() == 0
    else:
        assert got.max() >= 2


def test_exact_arithmetic_edges_with_nothing_exempt(cuda):
    """Z exactly on and one lattice step either side of the thresholds, and the 0.75 rule at 12 of 16: the kernels' arithmetic is exact
    on these inputs, so validity, the clamp and the 1000 are held to the reference on every element"""
    from pvo_amd import droid_backends as db
    case = R.exact_threshold_case()
    poses, disps, intr, ii, jj = _dev(cuda, *case[:5])
    ok, rep = R.check("projmap", _np(*db.projmap(poses, disps, intr[0].contiguous(), ii, jj)), R.projmap(case[0], case[1], case[2][0], case[3], case[4]), exact=True)
    assert ok, rep
    ok, rep = R.check("reproject", _np(*db.reproject(poses, disps, intr, ii, jj)), R.reproject(*case[:5]), exact=True)
    assert ok, rep
    for nvalid in (12, 13, 0):
        case = R.exact_ratio_case(nvalid)
        got = _np(db.frame_distance(*_dev(cuda, *case), 1.0))[0]
        ok, rep = R.check("frame_distance", got, R.frame_distance(*case, 1.0), exact=True)
        assert ok, (nvalid, got, rep)
        assert (got[0] == 1000.0) == (nvalid != 13)
        if nvalid == 12:
            assert R.check("frame_distance", got, R.frame_distance(*case, 1.0, mutant="ratio_fp32"), exact=True)[1]["mismatches"] > 0


@pytest.mark.parametrize("ht,wd", R.GRAPH_MAPS)
def test_entry_points_agree_bit_for_bit_over_the_case_list(cuda, ht, wd):
    """frame_distance_bidirectional = 0.5 * (d(ii, jj) + d(jj, ii)); reproject_motion = reproject's coordinates and validity and
    graph_motion's features in both 16-bit types, with and without a baseline; baseline = 0 is the plain entry point"""
    from pvo_amd import droid_backends as db
    from pvo_amd import _lib
    poses, disps, intr, ii, jj = _dev(cuda, *_graph(ht, wd))
    k0 = intr[0].contiguous()
    for beta in R.BETAS:
        both = db.frame_distance_bidirectional(poses, disps, k0, ii, jj, beta)
        assert torch.equal(both, 0.5 * (db.frame_distance(poses, disps, k0, ii, jj, beta) + db.frame_distance(poses, disps, k0, jj, ii, beta)))
    E = ii.numel()
    g = torch.Generator().manual_seed(11)
    target = (60.0 * torch.randn(1, E, ht, wd, 2, generator=g)).to(cuda)
    ddy = (3.0 * torch.randn(1, E, ht, wd, 2, generator=g)).to(cuda)
    raw = (40.0 * torch.randn(1, E, ht, wd, 2, generator=g)).to(cuda)
    for baseline in (0.0, R.BASELINE):
        c0, v0 = db.reproject(poses, disps, intr, ii, jj, baseline=baseline)
        for dtype in (torch.float16, torch.bfloat16):
            m0 = db.graph_motion(target, c0[None].contiguous(), ddy, raw, dtype)
            c1, v1, m1 = db.reproject_motion(poses, disps, intr, ii, jj, target, ddy, raw, dtype, baseline=baseline)
            assert torch.equal(c0, c1) and torch.equal(v0, v1)
            assert torch.equal(m0.contiguous().view(torch.int16), m1.contiguous().view(torch.int16))
            assert (m1.float() == 64).any() and (m1.float() == -64).any()      # both clamps are reached
    # pvo_reproject_rig with baseline 0 through the C ABI = pvo_reproject
    c0, v0 = db.reproject(poses, disps, intr, ii, jj)
    c2, v2 = torch.empty_like(c0), torch.empty_like(v0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    assert _lib.load().pvo_reproject_rig(p(poses), p(disps), p(intr), p(ii), p(jj), p(c2), p(v2), E, ht, wd, 0.0, st) == 0
    assert torch.equal(c0, c2) and torch.equal(v0, v2)


SENTINEL = -12288.0                                                       # exact in fp32, fp16 and bf16


@pytest.mark.parametrize("ht,wd", [(9, 29), (3, 5)])
def test_outputs_are_written_completely_and_guard_rows_stay_untouched(cuda, ht, wd):
    """through the C ABI: each output sits between two guard rows inside a larger buffer, the output itself pre-filled with NaN, the
    guards with a sentinel; afterwards no NaN is left (no output of these cases is NaN) and both guards still hold the sentinel"""
    from pvo_amd import _lib
    lib = _lib.load()
    poses, disps, intr, ii, jj = _dev(cuda, *_graph(ht, wd))
    k0 = intr[0].contiguous()
    E, nf, HW = ii.numel(), disps.shape[0], ht * wd
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    G = 64                                                               # guard elements either side

    def guarded(n, dtype=torch.float32):
        buf = torch.full((n + 2 * G,), SENTINEL, dtype=dtype, device=cuda)
        buf[G:G + n] = float("nan")
        return buf, buf[G:G + n]

    def intact(name, buf, n):
        assert not torch.isnan(buf[G:G + n].float()).any(), name + ": an element was not written"
        assert (buf[:G] == SENTINEL).all() and (buf[G + n:] == SENTINEL).all(), name + ": a guard row was written"
    cb, c = guarded(E * HW * 3); vb, v = guarded(E * HW)
    assert lib.pvo_projmap(p(poses), p(disps), p(k0), p(ii), p(jj), p(c), p(v), E, ht, wd, st) == 0
    intact("projmap coords", cb, E * HW * 3); intact("projmap valid", vb, E * HW)
    pb, pts = guarded(nf * HW * 3)
    assert lib.pvo_iproj(p(poses), p(disps), p(k0), p(pts), nf, ht, wd, st) == 0
    intact("iproj", pb, nf * HW * 3)
    for baseline in (None, R.BASELINE):
        cb, c = guarded(E * HW * 2); vb, v = guarded(E * HW)
        if baseline is None:
            assert lib.pvo_reproject(p(poses), p(disps), p(intr), p(ii), p(jj), p(c), p(v), E, ht, wd, st) == 0
        else:
            assert lib.pvo_reproject_rig(p(poses), p(disps), p(intr), p(ii), p(jj), p(c), p(v), E, ht, wd, baseline, st) == 0
        intact("reproject coords", cb, E * HW * 2); intact("reproject valid", vb, E * HW)
    db_, d = guarded(E)
    assert lib.pvo_frame_distance(p(poses), p(disps), p(k0), p(ii), p(jj), p(d), E, ht, wd, 0.3, st) == 0
    intact("frame_distance", db_, E)
    db_, d = guarded(E)
    assert lib.pvo_frame_distance_bidirectional(p(poses), p(disps), p(k0), p(ii), p(jj), p(d), E, ht, wd, 0.3, st) == 0
    intact("frame_distance_bidirectional", db_, E)
    ix = torch.arange(nf, device=cuda)
    th = torch.full((nf,), 0.05, device=cuda)
    kb, k = guarded(nf * HW)
    assert lib.pvo_depth_filter(p(poses), p(disps), p(k0), p(ix), p(th), p(k), nf, nf, ht, wd, st) == 0
    intact("depth_filter", kb, nf * HW)
    g = torch.Generator().manual_seed(2)
    tg, dd, rm = [torch.randn(E, ht, wd, 2, generator=g).to(cuda) for _ in range(3)]
    for code, dtype in ((_lib.PVO_F16, torch.float16), (_lib.PVO_BF16, torch.bfloat16)):
        cb, c = guarded(E * HW * 2); vb, v = guarded(E * HW); mb, m = guarded(E * HW * 8, dtype)
        assert lib.pvo_reproject_motion(p(poses), p(disps), p(intr), p(ii), p(jj), p(c), p(v), p(tg), p(dd), p(rm), p(m), E, ht, wd, code, st) == 0
        intact("reproject_motion coords", cb, E * HW * 2); intact("reproject_motion valid", vb, E * HW); intact("reproject_motion motion", mb, E * HW * 8)
        mb, m = guarded(E * HW * 8, dtype)
        assert lib.pvo_graph_motion(p(tg), p(c), p(dd), p(rm), p(m), E, ht, wd, code, st) == 0
        intact("graph_motion", mb, E * HW * 8)
    torch.cuda.synchronize()


def test_refusals_come_back_as_return_codes_and_empty_graphs_as_empty_outputs(cuda):
    """E = 65536 exceeds the grid's y extent: PVO_EINVAL from pvo_projmap, pvo_reproject and pvo_iproj before any launch (the output
    buffers here are far too small for such a launch and stay untouched); a negative baseline likewise.  E = 0: empty outputs."""
    from pvo_amd import _lib
    from pvo_amd import droid_backends as db
    lib = _lib.load()
    poses, disps, intr, ii, jj = _dev(cuda, *_graph(3, 5))
    k0 = intr[0].contiguous()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    c, v = torch.full((64,), SENTINEL, device=cuda), torch.full((64,), SENTINEL, device=cuda)
    assert lib.pvo_projmap(p(poses), p(disps), p(k0), p(ii), p(jj), p(c), p(v), 65536, 3, 5, st) == PVO_EINVAL
    assert lib.pvo_reproject(p(poses), p(disps), p(intr), p(ii), p(jj), p(c), p(v), 65536, 3, 5, st) == PVO_EINVAL
    assert lib.pvo_iproj(p(poses), p(disps), p(k0), p(c), 65536, 3, 5, st) == PVO_EINVAL
    E = ii.numel()
    assert lib.pvo_reproject_rig(p(poses), p(disps), p(intr), p(ii), p(jj), p(c), p(v), 1, 3, 5, -0.1, st) == PVO_EINVAL
    tg = torch.zeros(E, 3, 5, 2, device=cuda)
    m = torch.zeros(E, 3, 5, 8, dtype=torch.float16, device=cuda)
    assert lib.pvo_reproject_motion_rig(p(poses), p(disps), p(intr), p(ii), p(jj), p(c), p(v), p(tg), p(tg), p(tg), p(m), 1, 3, 5, _lib.PVO_F16, -0.1, st) == PVO_EINVAL
    torch.cuda.synchronize()
    assert (c == SENTINEL).all() and (v == SENTINEL).all()
    with pytest.raises(_lib.PvoHipError):
        db.reproject(poses, disps, intr, ii, jj, baseline=-0.1)
    none = torch.zeros(0, dtype=torch.long, device=cuda)
    assert db.projmap(poses, disps, k0, none, none)[0].shape == (0, 3, 5, 3)
    c0, v0 = db.reproject(poses, disps, intr, none, none)
    assert c0.shape == (0, 3, 5, 2) and v0.shape == (0, 3, 5, 1)
    assert db.frame_distance(poses, disps, k0, none, none, 0.3).shape == (0,)
    assert db.frame_distance_bidirectional(poses, disps, k0, none, none, 0.3).shape == (0,)
    assert db.depth_filter(poses, disps, k0, none, torch.zeros(0, device=cuda)).shape == (0, 3, 5)


def test_wrappers_refuse_inputs_that_are_not_float32_before_any_launch(cuda):
    """poses, disps and intrinsics of another type were read as fp32 - an fp16 `disps` past its end.  Every reprojection wrapper now
    raises PvoHipError first."""
    from pvo_amd import _lib
    from pvo_amd import droid_backends as db
    poses, disps, intr, ii, jj = _dev(cuda, *_graph(3, 5))
    k0 = intr[0].contiguous()
    E = ii.numel()
    ix, th = torch.arange(2, device=cuda), torch.full((2,), 0.05, device=cuda)
    tg = torch.zeros(1, E, 3, 5, 2, device=cuda)
    calls = {
        "projmap": lambda a, b, c: db.projmap(a, b, c[0].contiguous(), ii, jj),
        "iproj": lambda a, b, c: db.iproj(a, b, c[0].contiguous()),
        "depth_filter": lambda a, b, c: db.depth_filter(a, b, c[0].contiguous(), ix, th),
        "reproject": lambda a, b, c: db.reproject(a, b, c, ii, jj),
        "reproject_motion": lambda a, b, c: db.reproject_motion(a, b, c, ii, jj, tg, tg, tg, torch.float16),
    }
    for name, call in calls.items():
        call(poses, disps, intr)                                         # the call itself is fine ...
        for k in range(3):                                               # ... and refused with any one input in another type
            for other in (torch.float16, torch.float64):
                args = [poses, disps, intr]
                args[k] = args[k].to(other)
                with pytest.raises(_lib.PvoHipError, match="float32"):
                    call(*args)
    torch.cuda.synchronize()
