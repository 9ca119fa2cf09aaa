"""The graph-glue kernels (pvo_graph_motion, pvo_graph_post, pvo_segment_hist) against tests/glue_reference.py in fp16 and bf16: the
motion features bit for bit, the counts and everything whose arithmetic is exact or rounds once to equality, the two sigmoids within
their derived bound, decisions where settled; every mutant rejected; the vote at equality; the wrappers' refusals."""
import numpy as np
import pytest
import torch

import glue_reference as Q

pytestmark = pytest.mark.gpu

DTYPES = [(torch.float16, False), (torch.bfloat16, True)]


def _t(a, cuda, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return t if dtype is None else t.to(dtype)


def _heads(c, cuda, dtype):
    """[E,8,H,W] channels-last 16-bit tensor of the case's (already 16-bit) head values"""
    h = _t(c["heads"], cuda, dtype)
    assert torch.equal(h.float().cpu(), torch.from_numpy(c["heads"]))
    return h.permute(0, 3, 1, 2)


def _post(db, c, heads, cuda, thresh, vote=None):
    E, H, W, _ = c["coords1"].shape
    raw = _t(c["raw_mask"], cuda)[None].contiguous()
    tb, wb = torch.full((E, 2, H, W), float("nan"), device=cuda), torch.full((E, 2, H, W), float("nan"), device=cuda)
    target, ddy, weight, flow = db.graph_post(_t(c["coords1"], cuda)[None].contiguous(), heads, raw, tb, wb, thresh, vote=vote)
    return {k: v.cpu().numpy() for k, v in dict(raw_mask=raw[0], target=target[0], delta_dy=ddy[0], weight=weight[0], full_flow=flow[0],
                                                target_ba=tb, weight_ba=wb).items()}


@pytest.mark.parametrize("dtype,bf16", DTYPES)
@pytest.mark.parametrize("shape", Q.SHAPES)
def test_motion_features_equal_the_fp32_restatement_bit_for_bit(cuda, shape, dtype, bf16):
    from pvo_amd import droid_backends as db
    E, H, W = shape
    c = Q.case(E, H, W, bf16)
    want = Q.motion(c["target"], c["coords1"], c["delta_dy"], c["raw_motion"], bf16)
    args = [_t(c[k], cuda)[None].contiguous() for k in ("target", "coords1", "delta_dy", "raw_motion")]
    got = db.graph_motion(*args, dtype)
    assert got.shape == (1, E, 8, H, W)
    bits = got[0].permute(0, 2, 3, 1).contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(bits, want)
    f = Q.from_bits(bits, bf16)
    assert (f == 64).any() and (f == -64).any()
    assert not np.array_equal(bits, Q.motion(c["target"], c["coords1"], c["delta_dy"], c["raw_motion"], bf16, clamp=32.0))


@pytest.mark.parametrize("dtype,bf16", DTYPES)
@pytest.mark.parametrize("shape", Q.SHAPES)
def test_segment_hist_and_graph_post_match_the_reference(cuda, shape, dtype, bf16):
    from pvo_amd import droid_backends as db
    E, H, W = shape
    worst = 0.0
    for S in Q.SEGMENTS:
        c = Q.case(E, H, W, bf16, S=S)
        heads = _heads(c, cuda, dtype)
        segm = _t(c["segm"], cuda)
        for th in Q.DY_THRESH:
            tot_r, dyn_r, settled = Q.segment_hist(c["segm"], c["raw_mask"], c["heads"], S, th)
            assert settled.all()
            tot, dyn = db.segment_hist(segm, _t(c["raw_mask"], cuda)[None].contiguous(), heads, S, th)
            assert np.array_equal(tot.cpu().numpy(), tot_r) and np.array_equal(dyn.cpu().numpy(), dyn_r), (S, th)
            if S not in (16, 70) and th != 0.5:
                continue
            for vote_r, vote in ((None, None), ((c["segm"], tot_r, dyn_r, 0.5), (segm, tot, dyn, 0.5))):
                got = _post(db, c, heads, cuda, th, vote)
                ref = Q.post(c["coords1"], c["heads"], c["raw_mask"], th, vote=vote_r)
                ok, rep = Q.check_post(got, ref)
                assert ok, (S, th, vote is not None, rep)
                worst = max(worst, rep["worst"])
                for m in Q.MUTANTS:
                    if m == "vote_seg0" and (vote is None or S == 1):
                        continue
                    wrong = Q.post(c["coords1"], c["heads"], c["raw_mask"], th, vote=vote_r, mutant=m)
                    if m == "vote_seg0" and np.array_equal(wrong["static"], ref["static"]):
                        continue                                              # segment 0 is not over the threshold on this edge set
                    assert Q.check_post(got, wrong)[1]["mismatches"] > 0, (S, th, m)
    print("%s %s graph_post weight: worst err/bound %.3f" % (shape, dtype, worst))


@pytest.mark.parametrize("dtype,bf16", DTYPES)
def test_vote_at_equality_is_not_forced_one_more_is_and_segment_zero_never(cuda, dtype, bf16):
    """tables handed to graph_post directly: segment 0 all dynamic (never forced), segment 1 at 2 of 4 with thresh 0.5 (equality: not
    forced), segment 2 at 3 of 4 (forced), segment 3 empty (0 / max(0, 1)), ids -4 and 9 clamped to 0 and 4 (4 of 4: forced)"""
    from pvo_amd import droid_backends as db
    c = Q.case(1, 5, 7, bf16)
    c["raw_mask"] = np.abs(c["raw_mask"]) + 3.0                               # every pixel static on its own
    c["heads"][..., 6:8] = 0.0
    c["segm"] = (np.arange(35).reshape(1, 5, 7) % 6).astype(np.int32)
    c["segm"][c["segm"] == 4] = -4
    c["segm"][c["segm"] == 5] = 9
    tot = np.array([[10, 4, 4, 0, 4]], np.int32)
    dyn = np.array([[10, 2, 3, 0, 4]], np.int32)
    heads = _heads(c, cuda, dtype)
    got = _post(db, c, heads, cuda, 0.5, (_t(c["segm"], cuda), _t(tot, cuda), _t(dyn, cuda), 0.5))
    ref = Q.post(c["coords1"], c["heads"], c["raw_mask"], 0.5, vote=(c["segm"], tot, dyn, 0.5))
    ok, rep = Q.check_post(got, ref)
    assert ok, rep
    dynamic = ~ref["static"][0, ..., 0]
    ids = np.arange(35).reshape(5, 7) % 6
    assert np.array_equal(dynamic, (ids == 2) | (ids == 5))
    moved = got["delta_dy"][0, ..., 0] != 0
    assert np.array_equal(moved, dynamic & (c["heads"][0, ..., 2] != 0))
    assert Q.check_post(got, Q.post(c["coords1"], c["heads"], c["raw_mask"], 0.5, vote=(c["segm"], tot, dyn, 0.5), mutant="vote_seg0"))[1]["mismatches"] > 0


def test_glue_wrappers_refuse_wrong_types_and_shapes_before_any_launch(cuda):
    from pvo_amd import _lib
    from pvo_amd import droid_backends as db
    E, H, W = 2, 5, 7
    c = Q.case(E, H, W, False)
    heads = _heads(c, cuda, torch.float16)
    coords1 = _t(c["coords1"], cuda)[None].contiguous()
    raw = _t(c["raw_mask"], cuda)[None].contiguous()
    tb, wb = torch.zeros(E, 2, H, W, device=cuda), torch.zeros(E, 2, H, W, device=cuda)
    segm = _t(c["segm"], cuda)
    db.graph_post(coords1, heads, raw.clone(), tb, wb, 0.5)
    db.segment_hist(segm, raw, heads, 16, 0.5)
    for other in (torch.float16, torch.float64):
        for k in range(4):
            args = [coords1, raw.clone(), tb, wb]
            args[k] = args[k].to(other)
            with pytest.raises(_lib.PvoHipError, match="float32"):
                db.graph_post(args[0], heads, args[1], args[2], args[3], 0.5)
        with pytest.raises(_lib.PvoHipError, match="float32"):
            db.segment_hist(segm, raw.to(other), heads, 16, 0.5)
    for bad_tb, bad_wb in ((torch.zeros(E, H, W, 2, device=cuda), wb), (tb, torch.zeros(E, 2, H, W - 1, device=cuda)),
                           (torch.zeros(E - 1, 2, H, W, device=cuda), wb)):
        with pytest.raises(_lib.PvoHipError, match=r"\[E,2,H,W\]"):
            db.graph_post(coords1, heads, raw.clone(), bad_tb, bad_wb, 0.5)
    with pytest.raises(_lib.PvoHipError):
        db.graph_post(coords1, heads, raw[:, :1].contiguous(), tb, wb, 0.5)
    with pytest.raises(_lib.PvoHipError):
        db.segment_hist(segm[:1].contiguous(), raw, heads, 16, 0.5)
    torch.cuda.synchronize()
