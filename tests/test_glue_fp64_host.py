"""The graph glue's yardstick (tests/glue_reference.py), qualified without a GPU: it reproduces what the reference's own
FactorGraph.update recorded (tests/golden/factor_graph_glue_{plain,segm}.npz) from the same fp32 head outputs, its check rejects every
mutant against those recordings, the cases of the GPU test are settled where they claim to be, and the vote behaves at equality."""
import os

import numpy as np
import pytest

import glue_reference as Q

G = os.path.join(os.path.dirname(__file__), "golden")


def _fixture(name):
    d = dict(np.load(os.path.join(G, "factor_graph_glue_%s.npz" % name)))
    heads = np.concatenate([d["delta"][0], d["weight_out"][0], d["delta_m"][0]], -1).astype(np.float32)      # fp32: nothing is rounded
    got = dict(raw_mask=d["out_raw_mask"][0], target=d["out_target_cam"][0], delta_dy=d["out_delta_dy"][0], weight=d["out_weight"][0],
               full_flow=d["out_full_flow"][0], target_ba=d["ba_target"], weight_ba=d["ba_weight"])
    return d, heads, got


def _vote(d, heads, seg0=False):
    segm = d["segm"][0, :, 0]
    tot, dyn, settled = Q.segment_hist(segm, d["raw_mask"][0], heads, 16, 0.5)
    assert settled.all()
    return (segm, tot, dyn, 0.5)


@pytest.mark.parametrize("name", ["plain", "segm"])
def test_reference_reproduces_the_recorded_update_and_rejects_the_mutants(name):
    """the recorded sigmoid is PyTorch's, which the bound (derived for the kernel's 1 / (1 + expf(-x))) does not describe: the weights
    are held to 4 EPS relative here, everything else to equality through check_post"""
    d, heads, got = _fixture(name)
    vote = _vote(d, heads) if name == "segm" else None
    ref = Q.post(d["coords1"][0], heads, d["raw_mask"][0], 0.5, vote=vote)
    assert ref["settled"].all()
    for k in ("weight", "weight_ba"):
        assert np.allclose(got[k], ref[k], rtol=4 * Q.EPS, atol=0), k
    same = dict(got, weight=ref["weight"], weight_ba=ref["weight_ba"])
    ok, rep = Q.check_post(same, ref)
    assert ok, rep
    bits = Q.motion(d["target_cam"][0], d["coords1"][0], d["delta_dy"][0], d["raw_mask"][0], bf16=False)
    want = np.moveaxis(d["motn"][0], 1, -1)                                  # [E,H,W,8] fp32, clamped
    assert np.array_equal(Q.from_bits(bits, False), want.astype(np.float16).astype(np.float32))
    for m in Q.MUTANTS:
        if m == "vote_seg0" and name == "plain":
            continue
        wrong = Q.post(d["coords1"][0], heads, d["raw_mask"][0], 0.5, vote=vote, mutant=m)
        assert Q.check_post(got, wrong)[1]["mismatches"] > 0, m
    if name == "segm":                                                       # the vote changed something, and segment 0 matters to the mutant
        plain = Q.post(d["coords1"][0], heads, d["raw_mask"][0], 0.5)
        assert (plain["static"] != ref["static"]).any()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", Q.SHAPES)
def test_cases_are_settled_and_reach_what_they_claim(shape, bf16):
    E, H, W = shape
    for S in Q.SEGMENTS:
        c = Q.case(E, H, W, bf16, S=S)
        assert np.array_equal(Q.from_bits(Q.to_bits(c["heads"], bf16), bf16), c["heads"])      # the heads are 16-bit values
        for th in Q.DY_THRESH:
            tot, dyn, settled = Q.segment_hist(c["segm"], c["raw_mask"], c["heads"], S, th)
            assert settled.all(), (S, th)                                    # the counts are exact on these inputs
            assert tot.sum() == E * H * W and (dyn <= tot).all() and 0 < dyn.sum() < tot.sum()
            ref = Q.post(c["coords1"], c["heads"], c["raw_mask"], th, vote=(c["segm"], tot, dyn, 0.5))
            assert ref["settled"].all()
            assert ref["static"].any() and (~ref["static"]).any()
        assert c["segm"].min() < 0 and c["segm"].max() >= S                  # both clamps of the id
        if S == 70:
            assert len(set(c["segm"].reshape(-1)[:64].tolist())) >= 60       # a wave with (nearly) one id per lane
    rm = (c["raw_mask"] + c["heads"][..., 6:8]).astype(np.float32)
    assert (rm == 0).sum() >= 3                                              # sigmoid exactly 0.5
    st, se = Q.decide(rm, 0.5)
    assert st[rm == 0].all() and se[rm == 0].all()                           # ... is static at dy_thresh 0.5, and settled
    f = Q.from_bits(Q.motion(c["target"], c["coords1"], c["delta_dy"], c["raw_motion"], bf16), bf16)
    assert (f == 64).any() and (f == -64).any()
    half = Q.from_bits(Q.motion(c["target"], c["coords1"], c["delta_dy"], c["raw_motion"], bf16, clamp=32.0), bf16)
    assert not np.array_equal(f, half)                                       # the mutant clamp is visible on this case


def test_vote_at_equality_is_not_forced_and_segment_zero_never_is():
    segm = np.array([[[0, 1, 2, 3, -4, 9]]], np.int32)                       # -4 counts as 0, 9 as S - 1 = 4
    tot = np.array([[10, 4, 4, 0, 4]], np.int32)
    dyn = np.array([[10, 2, 3, 0, 4]], np.int32)
    f = Q.forced(segm, tot, dyn, 0.5, 5)
    assert f.tolist() == [[[False, False, True, False, False, True]]]        # 10/10 in segment 0: no; 2/4 == 0.5: no; 3/4: yes; 0/1: no
    assert Q.forced(segm, tot, dyn, 0.5, 5, seg0=True).tolist() == [[[True, False, True, False, True, True]]]


def test_sigmoid_bound_is_a_few_roundings():
    x = np.linspace(-30, 30, 601).astype(np.float32)
    s, e = Q.sigmoid(x)
    assert np.all(e <= 4.0 * Q.EPS * s + Q.TINY) and np.all(e >= 2.0 * Q.EPS * s)
    s32 = (np.float32(1.0) / (np.float32(1.0) + np.exp(-x).astype(np.float32))).astype(np.float32)   # numpy's own fp32 chain fits it
    assert np.all(np.abs(s32 - s) <= e)
