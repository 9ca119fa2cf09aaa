"""tests/altcorr_reference.py checked on the CPU: the fp64 reference against the oracle's lookup of the explicit volume and against its
own adjoint identity, the shared inputs against the conditions they are there for, the derived bounds against two correct fp32
implementations with different summation orders (the plain stand-in and the C oracle), and every named mutation rejected."""
import numpy as np
import pytest
import torch

import altcorr_reference as R
from oracle import oracle as O

IDS = [R.case_id(c) for c in R.CASES]


@pytest.mark.parametrize("cfg", R.CASES, ids=IDS)
def test_inputs_reach_the_borders_without_hiding_behind_zeros(cfg):
    """a cap, not a measurement: at most 0.60 of the forward outputs (0.85 on the 2 x 3 target) have all four taps outside, and every
    special coordinate is in every (b, s) plane of at least 32 pixels, each plane meeting the list at a different rotation"""
    B, S, H1, W1, H2, W2, C, r = cfg
    c = R.reference(cfg)
    share = R.zero_share(c["magnitude"])
    print("%s: zero-magnitude share %.3f" % (R.case_id(cfg), share))
    assert share <= (R.ZERO_SHARE_CAP_2X3 if (H2, W2) == (2, 3) else R.ZERO_SHARE_CAP)
    assert share > 0.0                                                        # (the border is reached at all)
    pix = R.special_pixels(H1, W1)
    assert len(pix) == min(16, H1 * W1 // 2) and len(set(pix.tolist())) == len(pix)
    planes = c["coords"].reshape(B * S, H1 * W1, 2)
    for p in range(B * S):
        if H1 * W1 >= 32:
            assert R.specials_present(planes[p], H2, W2), p
        if p > 0:
            assert not np.array_equal(planes[p][pix], planes[0][pix])
    assert np.isfinite(c["coords"]).all()


@pytest.mark.parametrize("cfg", R.CASES, ids=IDS)
def test_reference_is_the_oracle_lookup_of_the_explicit_volume(cfg):
    """the fp64 volume handed to the oracle's corr_index_forward (scatter form, [B,rd(x),rd(y),H1,W1]) gives the reference up to the
    oracle's weights, which it forms in fp32: three roundings per weight, and the rounding of dx itself for coordinates in (-1, 0), which
    1 - dx amplifies (33 U at the worst coordinate of these inputs, -0.0013).  64 U magnitude: any slip in the window, the channel order
    or the border handling is of order one"""
    B, S, H1, W1, H2, W2, C, r = cfg
    c = R.reference(cfg)
    rd = 2 * r + 1
    vol = np.einsum("bhwc,byxc->bhwyx", c["f1"].astype(np.float64), c["f2"].astype(np.float64))
    for s in range(S):
        want = O.corr_index_forward(vol, np.ascontiguousarray(c["coords"][:, s].transpose(0, 3, 1, 2)), r)
        R.assert_within(want.reshape(B, rd * rd, H1, W1), c["value"][:, s], 64 * R.U * c["magnitude"][:, s], "%s sample %d" % (R.case_id(cfg), s))


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("cfg", R.CASES, ids=IDS)
def test_reference_backward_is_the_adjoint(cfg, exact):
    """<grad, forward(f1, f2)> = <g1, f1> = <g2, f2> (the form is linear in each map) to 1e-12 of sum |grad| magnitude"""
    c = R.reference(cfg, exact)
    d = lambda a: torch.from_numpy(a).double()
    lhs = float((d(c["grad"]) * c["value"]).sum())
    scale = float((d(c["grad"]).abs() * c["magnitude"]).sum())
    assert scale > 0
    assert abs(lhs - float((c["bwd"]["g1"] * d(c["f1"])).sum())) <= 1e-12 * scale
    assert abs(lhs - float((c["bwd"]["g2"] * d(c["f2"])).sum())) <= 1e-12 * scale
    assert abs(scale - float((c["bwd"]["g1_mag"] * d(c["f1"]).abs()).sum())) <= 1e-12 * scale
    assert abs(scale - float((c["bwd"]["g2_mag"] * d(c["f2"]).abs()).sum())) <= 1e-12 * scale
    # K: every (pixel, sample) window lands on a target pixel at most once; all of them together (2r+2)^2 times the inside share
    assert float(c["bwd"]["K"].max()) <= cfg[1] * cfg[2] * cfg[3] and float(c["bwd"]["K"].sum()) > 0


def _check_forward(fn, cfg, label):
    """(worst ratio of the bound check, then the exact check) of a forward implementation fn(f1, f2, coords, r) -> float32 numpy"""
    c, e = R.reference(cfg), R.reference(cfg, True)
    worst = R.assert_within(fn(c["f1"], c["f2"], c["coords"], cfg[7]), c["value"], R.forward_bound(c["magnitude"], cfg[6]), label + " forward")
    R.assert_equal(torch.from_numpy(fn(e["f1"], e["f2"], e["coords"], cfg[7])), R.exact_want(e["value"], e["magnitude"], label), label + " forward, exact")
    return worst


def _check_backward(fn, cfg, label, exact_too=True):
    c, e = R.reference(cfg), R.reference(cfg, True)
    g1, g2 = fn(c["f1"], c["f2"], c["coords"], c["grad"], cfg[7])
    w1 = R.assert_within(g1, c["bwd"]["g1"], R.g1_bound(c["bwd"]), label + " g1")
    w2 = R.assert_within(g2, c["bwd"]["g2"], R.g2_bound(c["bwd"]), label + " g2")
    if exact_too:
        g1, g2 = fn(e["f1"], e["f2"], e["coords"], e["grad"], cfg[7])
        R.assert_equal(torch.from_numpy(g1), R.exact_want(e["bwd"]["g1"], e["bwd"]["g1_mag"], label), label + " g1, exact")
        R.assert_equal(torch.from_numpy(g2), R.exact_want(e["bwd"]["g2"], e["bwd"]["g2_mag"], label), label + " g2, exact")
    return w1, w2


@pytest.mark.parametrize("cfg", R.CASES, ids=IDS)
def test_clean_standin_is_within_the_bounds_and_exact_on_dyadic_operands(cfg):
    """forward (C + 8) U magnitude, g1 (T + 8) U magnitude, g2 (K + 8) U magnitude (derivations at R.forward_bound, R.g1_bound,
    R.g2_bound): a correct fp32 implementation in the kernels' order has ample room, and returns the reference's bits where every
    product and sum is exact"""
    assert _check_forward(R.standin, cfg, R.case_id(cfg) + " stand-in") < 1
    assert max(_check_backward(R.standin_backward, cfg, R.case_id(cfg) + " stand-in")) < 1


@pytest.mark.parametrize("cfg", R.CASES, ids=IDS)
def test_c_oracle_is_within_the_bounds(cfg):
    """the oracle is fp32 with another summation order (32-channel slabs scattered with fma; its backward sums in fp64): the bounds
    hold for it too, and on dyadic operands (four of the cases) it returns the reference's bits"""
    exact = cfg in R.EXACT_HOST_CASES
    c, e = R.reference(cfg), R.reference(cfg, True)
    label = R.case_id(cfg) + " oracle"
    assert R.assert_within(O.altcorr_forward(c["f1"], c["f2"], c["coords"], cfg[7]), c["value"], R.forward_bound(c["magnitude"], cfg[6]), label + " forward") < 1
    if exact:
        R.assert_equal(torch.from_numpy(O.altcorr_forward(e["f1"], e["f2"], e["coords"], cfg[7])), R.exact_want(e["value"], e["magnitude"], label), label + " forward, exact")
    assert max(_check_backward(O.altcorr_backward, cfg, label, exact_too=exact)) < 1


def _rejected(check, needle):
    try:
        check()
    except AssertionError as e:
        assert needle in str(e), str(e)
        return True
    return False


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_is_rejected(mutation):
    """each way of going wrong is over the bound in EVERY case where it can change a value (batch: B > 1, sample0: S > 1, chan and
    trunc: r > 0, tail: C % 64 != 0; the others everywhere), through the forward where the mutation touches it and through the backward;
    and on dyadic operands elements differ in at least one case"""
    over, differ = [], []
    for cfg in R.CASES:
        if not R.applicable(mutation, cfg):
            continue
        c, e, r, C = R.reference(cfg), R.reference(cfg, True), cfg[7], cfg[6]
        hits, xhits = [], []
        if mutation in R.FORWARD_MUTATIONS:
            hits.append(_rejected(lambda: R.assert_within(R.standin(c["f1"], c["f2"], c["coords"], r, mutation), c["value"],
                                                          R.forward_bound(c["magnitude"], C), "forward"), "over the bound"))
            xhits.append(_rejected(lambda: R.assert_equal(torch.from_numpy(R.standin(e["f1"], e["f2"], e["coords"], r, mutation)),
                                                          R.exact_want(e["value"], e["magnitude"], "forward"), "forward"), "elements differ"))
            assert hits[0], (mutation, cfg, "forward")
        g1, g2 = R.standin_backward(c["f1"], c["f2"], c["coords"], c["grad"], r, mutation)
        hits.append(_rejected(lambda: R.assert_within(g1, c["bwd"]["g1"], R.g1_bound(c["bwd"]), "g1"), "over the bound"))
        hits.append(_rejected(lambda: R.assert_within(g2, c["bwd"]["g2"], R.g2_bound(c["bwd"]), "g2"), "over the bound"))
        x1, x2 = R.standin_backward(e["f1"], e["f2"], e["coords"], e["grad"], r, mutation)
        xhits.append(_rejected(lambda: R.assert_equal(torch.from_numpy(x1), R.exact_want(e["bwd"]["g1"], e["bwd"]["g1_mag"], "g1"), "g1"), "elements differ"))
        xhits.append(_rejected(lambda: R.assert_equal(torch.from_numpy(x2), R.exact_want(e["bwd"]["g2"], e["bwd"]["g2_mag"], "g2"), "g2"), "elements differ"))
        assert any(hits[-2:]), (mutation, cfg, "backward")
        over.append(cfg)
        differ.append(any(xhits))
    assert over and any(differ), mutation


def test_assert_within_demands_exact_zeros_and_refuses_nan():
    z = torch.zeros(3, dtype=torch.float64)
    assert R.assert_within(np.array([0.0, -0.0, 0.0], np.float32), z, z, "zeros") == 0.0
    assert _rejected(lambda: R.assert_within(np.array([0.0, 1e-45, 0.0], np.float32), z, z, "denormal"), "over the bound")
    assert _rejected(lambda: R.assert_within(np.array([0.0, np.nan, 0.0], np.float32), z, z + 1, "nan"), "over the bound")
