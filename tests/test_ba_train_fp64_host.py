"""The cases of tests/ba_train_reference.py on the host: every case is admitted (each mask fires, spares, and no sample lies in a
band where fp32 could take the other branch), the written-out step equals pvo_amd.geom.ba.BA bit for bit, and the acceptance rule
of tests/test_ba_train_fp64_gpu.py has the power to reject a wrong implementation: every mutant of the reference, evaluated in fp32
on the CPU, fails it on some output of some case.  No GPU."""
import pytest
import torch

import ba_train_reference as R


@pytest.mark.parametrize("shape", R.CASES, ids=R.CASE_IDS)
def test_case_is_admitted(shape):
    c = R.case(*shape)
    a = c.admission
    print("%s: seed %d, %d samples nudged off the bands; band of Z %.3g, of d1 %.3g" % (shape, c.seed, c.nudged, a["band_Z"], a["band_d1"]))
    for k, cnt in enumerate(a["counts"]):
        print("  step %d: " % k + ", ".join("%s on %d of %d" % (n, f, tot) for n, (f, tot) in cnt.items()))
    assert a["offenders"] is None and a["ok"] and len(a["counts"]) == c.steps
    for cnt in a["counts"]:
        assert all(f >= R.MIN_FIRE for f, _ in cnt.values())
    B, P, fixedp, ht, wd, _ = shape
    assert torch.unique(c.ii).numel() == P - 1 and bool((c.ii == c.jj).any())
    assert all(torch.isfinite(v).all() for v in c.ref.values())
    # the step written out for the cut is the specification, bit for bit
    assert torch.equal(c.ref["_cut_poses"], c.ref["poses"]) and torch.equal(c.ref["_cut_disps"], c.ref["disps"])
    # inputs are exact in fp32
    assert all(torch.equal(v, v.float().double()) for v in c.s.values())
    # with the bands clear PyTorch's fp32 evaluation takes every branch as fp64 does, and passes the rule it defines
    ratios, bad = R.accept(c.pt32, c.ref, c.e_pt)
    assert not bad, bad
    print("  e_pt: " + ", ".join("%s %.2g" % kv for kv in c.e_pt.items()))


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_the_rule_rejects_the_mutant(mutant):
    caught = []
    for shape, cid in zip(R.CASES, R.CASE_IDS):
        c = R.case(*shape)
        got = R.evaluate_mutant(c.s, c.ii, c.jj, c.fixedp, c.steps, mutant)
        ratios, bad = R.accept(got, c.ref, c.e_pt)
        worst = max(ratios, key=lambda k: ratios[k])
        print("%s on %s: largest error %.3g x e_pt (%s); fails %d checks" % (mutant, cid, ratios[worst], worst, len(bad)))
        if bad:
            caught.append(cid)
    assert caught, "no case rejects " + mutant
