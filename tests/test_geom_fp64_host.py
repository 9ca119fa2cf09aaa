"""The reprojection family's fp64 yardstick (tests/geom_reference.py), qualified without a GPU: the C oracle - the uncontracted kernel
text in fp32 - stands in for the kernels.  check() accepts its output on every case and rejects it against every mutant reference, it
accepts the recorded kernel-text fixtures, the unsettled share stays under 1 % on the reference's own account, every branch of the
contracts is exercised among the settled elements, and the exact-arithmetic edges hold with nothing exempt."""
import os

import numpy as np
import pytest

import geom_reference as R
from oracle import oracle as O

G = os.path.join(os.path.dirname(__file__), "golden")

# mutants a case cannot tell from the contract, with the reason
BLIND = {
    ("depth_filter", "1x3x5"): ("symmetric", "inverse_depth"),        # one frame: no neighbour view, every vote is 0
    ("depth_filter", "4x1x70"): ("symmetric", "inverse_depth"),       # no tap fits into a map one pixel high or wide: every vote is 0
    ("depth_filter", "4x70x1"): ("symmetric", "inverse_depth"),
}


def _graph_runs(ht, wd, kinds=("projmap", "iproj", "reproject", "frame_distance")):
    """(label, kind, oracle output, reference function of a mutant) for one map size"""
    poses, disps, intr, ii, jj = R.graph_case(ht, wd)
    runs = []
    if "projmap" in kinds:
        runs.append(("projmap", "projmap", O.projmap(poses, disps, intr[0], ii, jj), lambda m: R.projmap(poses, disps, intr[0], ii, jj, mutant=m)))
    if "iproj" in kinds:
        runs.append(("iproj", "iproj", O.iproj(poses, disps, intr[0]), lambda m: R.iproj(poses, disps, intr[0], mutant=m)))
    if "reproject" in kinds:
        runs.append(("reproject", "reproject", O.reproject(poses, disps, intr, ii, jj), lambda m: R.reproject(poses, disps, intr, ii, jj, mutant=m)))
    if "frame_distance" in kinds:
        for beta in R.BETAS:
            runs.append(("frame_distance beta=%g" % beta, "frame_distance", O.frame_distance(poses, disps, intr[0], ii, jj, beta),
                         lambda m, beta=beta: R.frame_distance(poses, disps, intr[0], ii, jj, beta, mutant=m)))
    return runs


@pytest.mark.parametrize("ht,wd", R.GRAPH_MAPS + R.LINE_MAPS)
def test_check_accepts_the_oracle_and_rejects_every_mutant_on_the_graph_cases(ht, wd):
    line = (ht, wd) in R.LINE_MAPS
    kinds = ("projmap", "iproj", "reproject") if line else ("projmap", "iproj", "reproject", "frame_distance")
    for label, kind, got, ref in _graph_runs(ht, wd, kinds):
        ok, rep = R.check(kind, got, ref(None))
        print("%dx%d %-24s worst err/bound %.3f unsettled %.4f" % (ht, wd, label, rep["worst"], rep["unsettled"]))
        assert ok, (label, rep)
        for m in R.MUTANTS[kind]:
            if m == "ratio_fp32":                                     # differs from the contract only AT 0.75: the exact edges below
                continue
            if m == "no_beta" and label.endswith("beta=1"):           # beta = 1 has no translation-only term to drop
                continue
            ok, rep = R.check(kind, got, ref(m))
            assert rep["mismatches"] > 0, (label, m, rep)


def test_stereo_edges_follow_the_rig_transform():
    """baseline > 0: the edges (2, 2) and (5, 5) are u - fx b d exactly as the rig transform states it (tests/stereo_reference.py holds
    the kernels to that form); the oracle has no baseline, so the reference is qualified against the closed form here"""
    poses, disps, intr, ii, jj = R.graph_case(9, 29)
    ref = R.reproject(poses, disps, intr, ii, jj, baseline=R.BASELINE)
    plain = R.reproject(poses, disps, intr, ii, jj)
    u = np.arange(29, dtype=np.float64)[None, :]
    for e in np.nonzero(ii == jj)[0]:
        f = ii[e]
        want = u - np.float64(intr[f, 0]) * np.float64(np.float32(R.BASELINE)) * disps[f].astype(np.float64)
        assert np.allclose(ref["value"][e, ..., 0], want, rtol=0, atol=1e-5)
        assert ref["decision"][e].all() and ref["decision_settled"][e].all()
    other = ii != jj
    assert np.array_equal(ref["value"][other], plain["value"][other]) and np.array_equal(ref["bound"][other], plain["bound"][other])
    ok, rep = R.check("reproject", O.reproject(poses, disps, intr, ii, jj), ref)
    assert rep["mismatches"] > 0                                       # ... and a reprojection without the rig is told apart


@pytest.mark.parametrize("name", [c[0] for c in R.DEPTH_CASES])
def test_check_accepts_the_oracle_and_rejects_every_mutant_on_the_depth_filter_cases(name):
    poses, disps, intr, ix, thresh = R.depth_case(name)
    got = O.depth_filter(poses, disps, intr, ix, thresh)
    ref = R.depth_filter(poses, disps, intr, ix, thresh)
    ok, rep = R.check("depth_filter", got, ref)
    print("%-10s unsettled %.4f votes up to %d" % (name, rep["unsettled"], got.max()))
    assert ok, rep
    for m in R.MUTANTS["depth_filter"]:
        _, rep = R.check("depth_filter", got, R.depth_filter(poses, disps, intr, ix, thresh, mutant=m))
        if m in BLIND.get(("depth_filter", name), ()):
            assert got.max() == 0
        else:
            assert rep["mismatches"] > 0, (name, m, rep)


def test_special_disparities_follow_ieee_rules_and_leave_the_other_pixels_alone():
    """the case with disparities 0, negative, inf and NaN: those pixels get no vote (a negative one may), and a pixel none of whose taps
    in any view is one of them keeps the votes it has in the scene without them"""
    poses, disps, intr, ix, thresh = R.depth_case("10x9x29s")
    import map_reference as M
    clean = M.scene(M.SEED, 10, 9, 29, 0.02)[1].numpy()
    special = ~np.isfinite(disps) | (disps <= 0)
    assert special.sum() >= 6 and np.isnan(disps).any() and np.isinf(disps).any() and (disps == 0).any() and (disps < 0).any()
    ref, ref_clean = R.depth_filter(poses, disps, intr, ix, thresh), R.depth_filter(poses, clean, intr, ix, thresh)
    got = O.depth_filter(poses, disps, intr, ix, thresh)
    dead = ~np.isfinite(disps) | (disps == 0)
    for b, f in enumerate(ix):
        assert np.all(ref["value"][b][dead[f]] == 0) and np.all(got[b][dead[f]] == 0)
    changed = ref["value"] != ref_clean["value"]
    assert changed.any() and changed.mean() < 0.1                       # only pixels at or next to a special one move
    frames = np.array([3, 5])
    assert not changed[np.isin(ix, np.concatenate([frames + o for o in (-5, -4, -3, 0, 1, 2, 3)]), invert=True)].any()


def test_a_tie_by_construction_is_flagged_unsettled():
    """with cy ON a pixel row the scene's motion (translation in x and z, rotation about y) leaves v_j = cy exactly on that row in every
    view: its tap cell hangs on the last bit, the reference must say so, and the case list avoids it (depth_case moves cy off the lattice)"""
    poses, disps, intr, ix, thresh = R.depth_case("4x18x16")
    tie = intr.copy()
    tie[3] = 9.0
    flagged = ~R.depth_filter(poses, disps, tie, ix, thresh)["value_settled"]
    assert flagged[:, 9].mean() > 0.5 and flagged[:, :9].mean() < 0.01 and flagged[:, 10:].mean() < 0.01
    assert not (~R.depth_filter(poses, disps, intr, ix, thresh)["value_settled"])[:, 9].any()


def test_unsettled_share_and_branch_coverage_of_the_case_lists():
    """the reference alone: every case stays under the 1 % cap, and among the SETTLED elements of the lists both sides of every Z
    threshold, Z below zero, votes 0 to 6, a tap refused at each border, and frame_distance both finite and 1000 occur"""
    cover = {}

    def take(kind, ref):
        flags = [f for f in (ref["value_settled"], ref.get("decision_settled")) if f is not None and f.size]
        share = max([1.0 - np.mean(f) for f in flags] + [0.0])
        assert share <= R.UNSETTLED_CAP, (kind, share)
        for k, v in ref["cover"].items():
            cover[kind, k] = cover.get((kind, k), False) or v
    for ht, wd in R.GRAPH_MAPS + R.LINE_MAPS:
        poses, disps, intr, ii, jj = R.graph_case(ht, wd)
        take("projmap", R.projmap(poses, disps, intr[0], ii, jj))
        take("reproject", R.reproject(poses, disps, intr, ii, jj))
        take("reproject", R.reproject(poses, disps, intr, ii, jj, baseline=R.BASELINE))
        take("iproj", R.iproj(poses, disps, intr[0]))
        if (ht, wd) in R.GRAPH_MAPS:
            for beta in R.BETAS:
                take("frame_distance", R.frame_distance(poses, disps, intr[0], ii, jj, beta))
    for case in R.DEPTH_CASES:
        poses, disps, intr, ix, thresh = R.depth_case(case[0])
        take("depth_filter", R.depth_filter(poses, disps, intr, ix, thresh))
    want = [("projmap", k) for k in ("Z>0.25", "Z<=0.25", "Z>0.01", "Z<=0.01", "Z<0")]
    want += [("reproject", k) for k in ("Z>0.2", "Z<=0.2", "Z<0.1", "Z>=0.1", "Z<0")]
    want += [("frame_distance", "finite"), ("frame_distance", "1000"), ("frame_distance", "finite with 0.2<Z<=0.25")]
    want += [("depth_filter", "votes%d" % n) for n in range(7)] + [("depth_filter", k) for k in ("left", "top", "right", "bottom")]
    missing = [w for w in want if not cover.get(w)]
    assert not missing, missing


def test_bounds_are_first_order_in_the_roundings_and_carry_the_depth():
    """sanity of the derivation itself: on the 24 x 43 case the projection bound grows like 1 / Z^2 toward small Z (the median of
    bound * Z^2 / EPS over the projected pixels stays within a decade across Z), and the frame_distance bound is a small multiple of
    EPS times the value - far below the 2 HW EPS an any-order bound would grant"""
    poses, disps, intr, ii, jj = R.graph_case(24, 43)
    ref = R.frame_distance(poses, disps, intr[0], ii, jj, 0.3)
    fin = (ref["bound"] > 0) & (ref["value"] > 0.1)
    rel = ref["bound"][fin] / (R.EPS * ref["value"][fin])
    assert fin.any() and rel.max() < 400 and rel.max() < 0.2 * 2 * 24 * 43
    e = 4                                                              # the edge 3 -> 5: Z from below zero to ~0.9
    with np.errstate(all="ignore"):
        Y = R._act(R._edge_pose(poses, ii[e:e + 1], jj[e:e + 1], None), R._rays(R._intr(intr[0]), 24, 43), R._inputs(poses, disps, ii[e:e + 1])[5])
    Z = Y[2].v[0]
    b = R.projmap(poses, disps, intr[0], ii, jj)["bound"][e].reshape(-1, 3)[:, 0]
    near, far = (Z > 0.01) & (Z < 0.05), Z > 0.5
    assert near.sum() >= 3 and far.sum() >= 3
    assert np.median(b[near]) > 30 * np.median(b[far])


@pytest.mark.parametrize("case", ["a", "b"])
def test_check_accepts_the_recorded_kernel_text_fixtures(case):
    z = np.load(os.path.join(G, "geom_kernels.npz"))
    poses, disps, intr, ii, jj = [z[case + "_" + k] for k in ("poses", "disps", "intr", "ii", "jj")]
    ok, rep = R.check("projmap", (z[case + "_projmap_coords"], z[case + "_projmap_valid"]), R.projmap(poses, disps, intr, ii, jj))
    assert ok, rep
    ok, rep = R.check("iproj", z[case + "_iproj"], R.iproj(poses, disps, intr))
    assert ok, rep
    for beta in ("0.3", "1", "0"):
        ok, rep = R.check("frame_distance", z[case + "_frame_distance_beta" + beta], R.frame_distance(poses, disps, intr, ii, jj, float(beta)))
        assert ok, (beta, rep)
    nf = disps.shape[0]
    for t in ("0.005", "0.05"):
        ok, rep = R.check("depth_filter", z[case + "_depth_filter_t" + t],
                          R.depth_filter(poses, disps, intr, np.arange(nf), np.full(nf, float(t), np.float32)))
        assert ok, (t, rep)


def test_exact_threshold_edges_with_nothing_exempt():
    """Z exactly at 0.25 and one lattice step either side of 0.25, fp32 0.2, fp32 0.1 and fp32 0.01: validity and the clamp must be the
    reference's, settled or not"""
    poses, disps, intr, ii, jj, zs = R.exact_threshold_case()
    pm, rp = R.projmap(poses, disps, intr[0], ii, jj), R.reproject(poses, disps, intr, ii, jj)
    Zref = R._act(R._edge_pose(poses, ii, jj, None), R._rays(R._intr(intr[0]), 3, 5), R._inputs(poses, disps, ii)[5])[2].v[0]
    assert np.array_equal(Zref, zs)                                    # the reference sees the same exact Z
    assert np.array_equal(pm["decision"].reshape(-1), zs > np.float64(R.MIN_DEPTH_NATIVE)) and not pm["decision"].reshape(-1)[0]
    assert np.array_equal(rp["decision"].reshape(-1), zs > np.float64(R.MIN_DEPTH_PY))
    # the settled rule itself: every pixel placed within a lattice step of a threshold is flagged, the padding at Z = 0.5 is not
    assert not pm["decision_settled"].reshape(-1)[:3].any() and pm["decision_settled"].reshape(-1)[9:].all()
    assert not rp["decision_settled"].reshape(-1)[3:5].any() and not rp["value_settled"].reshape(-1, 2)[5:7].any()
    for thr in (R.MIN_DEPTH_NATIVE, R.MIN_DEPTH_PY, R.CLAMP_DEPTH, R.PROJ_DEPTH):      # both sides of each, one step away at most
        assert (zs > np.float64(thr)).any() and (zs <= np.float64(thr)).any()
        assert np.abs(zs - np.float64(thr)).min() <= 2.0 ** -24
    ok, rep = R.check("projmap", O.projmap(poses, disps, intr[0], ii, jj), pm, exact=True)
    assert ok, rep
    ok, rep = R.check("reproject", O.reproject(poses, disps, intr, ii, jj), rp, exact=True)
    assert ok, rep
    for kind, got, mutant in (("projmap", O.projmap(poses, disps, intr[0], ii, jj), R.projmap(poses, disps, intr[0], ii, jj, mutant="valid_0.2")),
                              ("reproject", O.reproject(poses, disps, intr, ii, jj), R.reproject(poses, disps, intr, ii, jj, mutant="no_clamp"))):
        assert R.check(kind, got, mutant, exact=True)[1]["mismatches"] > 0


@pytest.mark.parametrize("nvalid,want", [(12, 1000.0), (13, None), (0, 1000.0)])
def test_exact_ratio_edges_with_nothing_exempt(nvalid, want):
    """4 x 4, beta = 1: 12 valid of 16 is exactly 1000.0 because the rule runs in double; an fp32 evaluation says 0.75 < 0.75 is false"""
    poses, disps, intr, ii, jj = R.exact_ratio_case(nvalid)
    ref = R.frame_distance(poses, disps, intr, ii, jj, 1.0)
    got = O.frame_distance(poses, disps, intr, ii, jj, 1.0)
    if want is not None:
        assert ref["value"][0] == want and ref["bound"][0] == 0
    else:
        assert 0 < ref["value"][0] < 100 and ref["bound"][0] > 0
    ok, rep = R.check("frame_distance", got, ref, exact=True)
    assert ok, rep
    if nvalid == 12:
        wrong = R.frame_distance(poses, disps, intr, ii, jj, 1.0, mutant="ratio_fp32")
        assert wrong["value"][0] != 1000.0 and R.check("frame_distance", got, wrong, exact=True)[1]["mismatches"] > 0


def test_empty_graph_gives_empty_references():
    poses, disps, intr, ii, jj = R.graph_case(3, 5)
    none = np.zeros(0, np.int64)
    assert R.projmap(poses, disps, intr[0], none, none)["value"].shape == (0, 3, 5, 3)
    assert R.reproject(poses, disps, intr, none, none)["value"].shape == (0, 3, 5, 2)
    assert R.frame_distance(poses, disps, intr[0], none, none, 0.3)["value"].shape == (0,)
    ok, rep = R.check("reproject", (np.zeros((0, 3, 5, 2), np.float32), np.zeros((0, 3, 5, 1), np.float32)), R.reproject(poses, disps, intr, none, none))
    assert ok and rep["worst"] == 0 and rep["unsettled"] == 0
