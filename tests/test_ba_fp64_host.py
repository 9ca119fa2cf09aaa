"""The plain bundle adjustment against fp64, host side: tests/ba_reference.py is qualified - its reduced system is the first half of the
step it stands beside, its fixed-point decoding inverts the device's encoding - and every case tests/test_ba_fp64_gpu.py runs is held
to the ADMISSION rule stated there.  Per admitted case this prints s_case, the fp32 restatement's share of each bound and every
mutation's excess (profiles/r15_ba_fp64.txt records them).  The second half does the same for the sensor-depth prior and stereo edges
(tests/ba_rider_reference.py; what tests/test_ba_riders_fp64_gpu.py runs; profiles/r26_ba_riders_fp64.txt).  No GPU is needed."""
import numpy as np
import pytest

import ba_reference as B
import ba_rider_reference as RR
import calib_reference as C

_id = lambda t: "-".join(t)


def test_control_is_window_general_and_the_regimes_change_what_they_name():
    s, g = B.regime_window("control", **B.GRAPHS["tiny"]), C.window_general(7, 6, 9, 12, radius=2, t0=1)
    assert all(np.array_equal(np.asarray(s[k]), np.asarray(g[k])) for k in g)
    b = B.regime_window("behind", **B.GRAPHS["tiny"])
    frac = B.masked_fraction(b)
    print("behind: %.3f of the pixels have Z < MIN_DEPTH" % frac)
    assert 0.05 < frac < 0.3 and B.near_count(b) == 0 and B.masked_fraction(s) == 0.0
    w = B.regime_window("sparse_weights", **B.GRAPHS["tiny"])["weight"]
    assert abs(float((w == 0).float().mean()) - 0.5) < 0.03 and abs(float(((w > 0) & (w < 0.01)).float().mean()) - 0.25) < 0.03
    eta = B.regime_window("eta_wide", **B.GRAPHS["tiny"])["eta"]
    assert float(eta.min()) < 1e-5 and float(eta.max()) > 0.3
    h = B.regime_window("heavy", **B.GRAPHS["tiny"])
    assert np.array_equal(h["weight"].numpy(), s["weight"].numpy() * 2.0 ** 26) and np.array_equal(h["eta"].numpy(), s["eta"].numpy() * 2.0 ** 26)


def test_reduced_system_is_the_first_half_of_the_step_and_decoding_inverts_the_fixed_point():
    c = B.case("tiny", "behind", "local")
    s, f, base = c["s"], c["f"], c["base"]
    S, rhs = B.reduced_system(f, s)
    assert np.array_equal(np.diag(S), base["S_diag"]) and np.abs(S - S.T).max() <= 1e-12 * np.abs(S).max()
    A = S.copy()
    A[np.diag_indices_from(A)] += c["ep"] + c["lm"] * np.diag(S)
    L = np.linalg.cholesky(A)
    dx = np.linalg.solve(L.T, np.linalg.solve(L, rhs)).reshape(-1, 6)
    assert np.array_equal(dx, base["dx"])
    TS, Tr = B.reduced_abs(f, s)
    assert np.all(TS >= np.abs(S) * (1 - 1e-12)) and np.all(Tr >= np.abs(rhs) * (1 - 1e-12))
    # the device's layout: the lower block triangle only, in units of 2^-28; what lies above it is never read
    P = s["t1"] - s["t0"]
    low = B.lower_blocks(P)
    words = np.concatenate([np.where(low, np.rint(S * 2.0 ** 28), 12345.0).reshape(-1), np.rint(rhs * 2.0 ** 28)]).astype(np.int64)
    S2, r2 = B.decode_sys(words, P)
    assert np.abs(S2 - S).max() <= 2.0 ** -29 * 1.0000001 and np.abs(r2 - rhs).max() <= 2.0 ** -29 and np.array_equal(S2, S2.T)
    # the structural support holds every non-zero of the fp64 system and leaves blocks out
    sup = np.kron(B.block_support(s), np.ones((6, 6))) > 0
    assert not np.any(S[low & ~sup]) and np.all(np.abs(S[low & sup]).reshape(-1) >= 0)
    big, _ = B.window_of("twin39", "control")
    assert 0 < B.block_support(big).sum() < 39 * 40 // 2
    nS, nr = B.fix_addends(s)
    assert np.all((nS > 0) == B.block_support(s)) and nr.min() > 0


@pytest.mark.parametrize("key", B.ADMITTED, ids=_id)
def test_admission_and_mutations(key):
    """the admission rule (ba_reference's docstring) for one case, then the check that the bound can catch what 1e-4 cannot: four wrong
    variants of the step must each leave the bound in dx or in dz, and in `behind` so must the step without MIN_DEPTH"""
    c = B.case(*key)
    s, sc, base = c["s"], c["sc"], c["base"]
    name = _id(key)
    assert not base["rejected"]
    print("%s: s_case dx %.2e dz %.2e" % (name, sc["dx"], sc["dz"]))
    assert 4 * sc["dx"] <= B.CAP and 4 * sc["dz"] <= B.CAP                     # a case this sensitive is replaced, not loosened
    assert B.near_count(s) == 0
    if key[1] == "behind":
        assert B.masked_fraction(s) > 0.05
    f32, st = B.restatement(c)
    ok_x, sh_x = B.share("dx", st["dx"], c, 0.5)
    ok_z, sh_z = B.share("dz", st["dz"], c, 0.5)
    S, rhs = B.reduced_system(c["f"], s)
    bS, br = B.sys_bound(s, B.reduced_abs(c["f"], s))
    S32, r32 = B.reduced_system(f32, s)
    low = B.lower_blocks(s["t1"] - s["t0"])
    sh_S = float((np.abs(S32 - S)[low] / np.maximum(bS[low], 1e-300)).max())
    sh_r = float((np.abs(r32 - rhs) / np.maximum(br, 1e-300)).max())
    print("%s: fp32 restatement's share of the bound dx %.3f dz %.3f S %.3f rhs %.3f" % (name, sh_x, sh_z, sh_S, sh_r))
    assert ok_x and ok_z and sh_x <= 0.5 and sh_z <= 0.5
    assert sh_S <= 1.0 and sh_r <= 1.0
    muts = B.mutations(c)
    if key[1] == "behind":
        muts["no_min_depth"] = B.unmasked_step(c)
    for m, r in muts.items():
        _, ex = B.share("dx", r["dx"], c)
        _, ez = B.share("dz", r["dz"], c)
        print("%s: mutation %-12s exceeds the bound %.1f x in dx, %.1f x in dz" % (name, m, ex, ez))
        assert max(ex, ez) > 1.0, m


def test_the_reduced_bound_separates_a_1e_3_error_of_the_reduced_system():
    c = B.case("tiny", "control", "local")
    s, f = c["s"], c["f"]
    S, rhs = B.reduced_system(f, s)
    bS, br = B.sys_bound(s, B.reduced_abs(f, s))
    low = B.lower_blocks(s["t1"] - s["t0"])
    Hs = f["Hs"].copy()
    Hs[1] *= 1.001
    Hs[2] = np.swapaxes(Hs[1], 1, 2)
    for name, g in (("Eij x 1.001", dict(f, Eij=f["Eij"] * 1.001)), ("Hs ij x 1.001", dict(f, Hs=Hs))):
        S2, _ = B.reduced_system(g, s)
        ex = float((np.abs(S2 - S)[low] / bS[low]).max())
        print("reduced system, %s: %.0f x the bound" % (name, ex))
        assert ex > 50.0


@pytest.mark.parametrize("key", B.TWO_STEPS, ids=_id)
def test_two_chained_steps_meet_the_cap_with_the_chains_sensitivity(key):
    c = B.chain(*key)
    print("%s x2: s_case dx %.2e dz %.2e" % (_id(key), c["sc"]["dx"], c["sc"]["dz"]))
    assert 4 * c["sc"]["dx"] <= B.CAP and 4 * c["sc"]["dz"] <= B.CAP and not c["base"]["rejected"]
    assert c["near_mid"] == 0                                                  # the second step's masks coincide too
    a = C.scene_args(c["s"])
    one = C.ba_calib(*a, 1, c["lm"], c["ep"], 0.1, 0, assembly="fp64")
    assert np.array_equal(one["dx"], B.case(*key)["base"]["dx"])                # assembly="fp64": one step of the chain IS the case's step
    assert not np.array_equal(C.ba_calib(*a, 1, c["lm"], c["ep"], 0.1, 0)["dx"], one["dx"])      # ... and the default is still the oracle's


def test_light_is_left_out_for_the_reason_the_docstring_gives():
    c = B.case("tiny", "light", "local")
    _, st = B.restatement(c)
    _, sh = B.share("dz", st["dz"], c)
    print("light: s_case dz %.1e, fp32 restatement's share %.2f" % (c["sc"]["dz"], sh))
    assert sh > 0.5


def test_the_overflow_zone_is_what_it_says():
    s, k, d, largest = B.overflow_window()
    print("overflow zone: x 2^%d, largest diagonal entry %.3e (2^35 = %.3e), largest addend %.3e" % (k, d, 2.0 ** 35, largest))
    assert 2.0 ** 35 <= d < 2.0 ** 36 and largest < B.FIX_LIMIT


# ------------------------------------------------------------------------------------------------ the riders: sensor-depth prior, stereo edges
_rid = lambda t: "-".join(x for x in t if x)


def test_without_a_map_and_without_a_stereo_edge_the_extended_reference_is_the_parents():
    """calib_reference.step / ba_reference._reduce with sens=None run the parent commit's statements and nothing else: against its
    recorded arrays (tests/golden/ba_tiny_control_local_step.npz, written by the parent's files - identical bits on the host that
    wrote them, printed here; held to 2^-40 because numpy's matrix products are the host BLAS's, whose order of additions is the
    CPU's), and bit for bit in this process against an all-zero map, a rider window without a part, and the unextended calls"""
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "ba_tiny_control_local_step.npz"))
    c = B.case("tiny", "control", "local")
    s, f, base = c["s"], c["f"], c["base"]
    S, rhs = B.reduced_system(f, s)
    TS, Tr = B.reduced_abs(f, s)
    got = dict(dx=base["dx"], dz=base["dz"], poses=base["poses"], disps=base["disps"], S=S, rhs=rhs, TS=TS, Tr=Tr)
    print("bit-identical to the recorded arrays: %s" % {k: bool(np.array_equal(got[k], g[k])) for k in got})
    for k in got:
        assert got[k].shape == g[k].shape and np.abs(got[k] - g[k]).max() <= 2.0 ** -40 * np.abs(g[k]).max(), k
    a = C.scene_args(s)
    zero = np.zeros_like(a[1])
    z = C.step(f, a[0], a[1], a[2], a[5], a[6], a[7], a[8], a[9], c["lm"], c["ep"], 0.1, 0, sens=zero)
    assert all(np.array_equal(z[k], base[k]) for k in ("dx", "dz", "poses", "disps", "S_diag"))
    S0, r0 = B.reduced_system(f, s, sens=zero)
    T0 = B.reduced_abs(f, s, sens=zero)
    assert np.array_equal(S0, S) and np.array_equal(r0, rhs) and np.array_equal(T0[0], TS) and np.array_equal(T0[1], Tr)
    n = RR.case("tiny", "control", "local", "none")
    assert n["s"]["sens"] is None and n["s"]["n_stereo"] == 0 and all(np.array_equal(n["f"][k], f[k]) for k in C.FIELDS)
    assert all(np.array_equal(n["base"][k], base[k]) for k in ("dx", "dz", "poses", "disps"))
    (Sn, rn), (bSn, brn) = RR.reduced(n["s"], n["f"])
    bS, br = B.sys_bound(s, (TS, Tr))
    assert np.array_equal(Sn, S) and np.array_equal(rn, rhs) and np.array_equal(bSn, bS) and np.array_equal(brn, br)
    assert B.frame_rows(n["s"]) == B.frame_rows(s) and B.n_add(5) == B.n_add(5, prior=False) == B.n_add(5, prior=True) - 2


def test_the_rider_windows_are_what_they_say():
    c = RR.case("tiny", "control", "local", "both")
    s, s0 = c["s"], B.window_of("tiny", "control")[0]
    F, ht, wd = s["disps"].shape
    meas = s["sens"] > 0
    rel = ((s["sens"] - s["disps"]).abs() / s["disps"])[meas]
    assert 0.6 < float(meas.float().mean()) < 0.8 and 0.05 < float(rel.max()) <= 0.1001
    ns = s["n_stereo"]
    assert ns == F and s["ii"][:ns].tolist() == list(range(F)) == s["jj"][:ns].tolist() and s["st"][:ns].all() and not s["st"][ns:].any()
    assert all(np.array_equal(s[k][ns:].numpy(), s0[k].numpy()) for k in ("ii", "jj", "target", "weight")) and np.array_equal(s["eta"].numpy(), s0["eta"].numpy())
    assert 0.5 <= float(s["weight"][:ns].min()) and float(s["weight"][:ns].max()) <= 1.5
    f = c["f"]
    for k in ("Hs", "vs", "Eii", "Eij", "Hci", "Hcj", "Hcc", "vc", "gc"):           # exact zeros: no identity edge leaks in
        ax = 1 if k in ("Hs", "vs") else 0
        assert not np.moveaxis(f[k], ax, 0)[:ns].any() and np.moveaxis(f[k], ax, 0)[ns:].any()
    assert (f["Cii"][:ns] > 0).all()
    # a stereo edge's terms are the assembly's own formula with G = (I, (-b, 0, 0)): pixel_jacobians under that transform agrees
    J = RR._rig_jacobians(s, np.arange(ns))
    Cr, br = np.einsum("ecx,ecx,ecx->ex", J["w"], J["Jz"], J["Jz"]), np.einsum("ecx,ecx,ecx->ex", J["w"], J["r"], J["Jz"])
    assert np.abs(Cr - f["Cii"][:ns]).max() <= 1e-6 * f["Cii"][:ns].max() and np.abs(br - f["bz"][:ns]).max() <= 1e-6 * np.abs(f["bz"][:ns]).max()
    assert not J["Jz"][:, 1].any() and np.all(J["Jz"][:, 0] < 0)
    f32 = RR.rider_fields(s, "oracle")
    assert np.abs(f32["Cii"][:ns] - f["Cii"][:ns]).max() <= 1e-5 * f["Cii"][:ns].max()
    # the targets are the true right view: the residual at the TRUE depth is the 0.1 px of noise
    import stereo_reference as SR
    import torch
    low = torch.rand(1, 1, 6, 8, generator=torch.Generator().manual_seed(7)) * 0.8 + 0.2       # (the recipe's first draw)
    d_gt = torch.nn.functional.interpolate(low, size=(ht, wd), mode="bilinear", align_corners=True)[0, 0].numpy().astype(np.float64)
    v, u = np.meshgrid(np.arange(ht, dtype=np.float64), np.arange(wd, dtype=np.float64), indexing="ij")
    pu, pv = SR.stereo_project(u, v, d_gt, s["intr"].numpy(), s["baseline"])
    res = np.stack([s["target"][:ns, 0].numpy() - pu, s["target"][:ns, 1].numpy() - pv])
    assert abs(float(res.mean())) < 0.02 and 0.08 < float(res.std()) < 0.12 and float(np.abs(u - pu).min()) > 0.1
    # the row table: every window frame of `tiny` gets six more rows from its stereo edge; twice merges, 65 + does not
    r0, r1 = B.frame_rows(s0), B.frame_rows(s)
    assert all(r1[fr] == r0[fr] + 6 for fr in range(s["t0"], s["t1"])) and r1[0] == r0[0]
    tw = RR.rider_window("tiny", "control", "stereo", **RR.options("tiny", "stereo", "twice"))
    assert tw["n_stereo"] == F + 1 and B.frame_rows(tw) == r1
    dg = RR.rider_window("tiny", "control", "stereo", **RR.options("tiny", "stereo", "deg65"))
    assert B.max_out_degree(dg) == 69 and B.frame_rows(dg)[2] == 6 + 6 * (17 * 3 + 1) + 1 and B.frame_paths(dg)[2][0] == "stream"
    nS, nr = B.fix_addends(s)
    n0S, n0r = B.fix_addends(s0)
    assert np.array_equal(nS, n0S) and np.array_equal(nr, n0r)                  # a stereo edge is no fixed-point addend (fix_addends)
    assert B.launch_form(s) == "fused256"


@pytest.mark.parametrize("key", RR.ADMITTED, ids=_rid)
def test_rider_admission_and_mutations(key):
    """ba_reference's admission rule, unchanged, for one case with the prior and / or stereo edges - then THE TERM MUST BE VISIBLE:
    every wrong variant of the term (ba_rider_reference.MUTATIONS) leaves the bound in dx or in dz"""
    c = RR.case(*key)
    s, sc, base = c["s"], c["sc"], c["base"]
    name = _rid(key)
    assert not base["rejected"]
    print("%s [%s]: 4 s_case dx %.2e dz %.2e" % (name, B.launch_form(s), 4 * sc["dx"], 4 * sc["dz"]))
    assert 4 * sc["dx"] <= B.CAP and 4 * sc["dz"] <= B.CAP
    assert B.near_count(dict(s, ii=s["ii"][~s["st"]], jj=s["jj"][~s["st"]])) == 0      # ordinary edges; a stereo edge has Z = 1
    f32, st = RR.restatement(c)
    ok_x, sh_x = B.share("dx", st["dx"], c, 0.5)
    ok_z, sh_z = B.share("dz", st["dz"], c, 0.5)
    (S, rhs), (bS, br) = RR.reduced(s, c["f"])
    S32, r32 = B.reduced_system(f32, s, sens=RR.sens_of(s), alpha=s["alpha"])
    low = B.lower_blocks(s["t1"] - s["t0"])
    sh_S = float((np.abs(S32 - S)[low] / np.maximum(bS[low], 1e-300)).max())
    sh_r = float((np.abs(r32 - rhs) / np.maximum(br, 1e-300)).max())
    print("%s: fp32 restatement's share of the bound dx %.3f dz %.3f S %.3f rhs %.3f" % (name, sh_x, sh_z, sh_S, sh_r))
    assert ok_x and ok_z and sh_x <= 0.5 and sh_z <= 0.5 and sh_S <= 1.0 and sh_r <= 1.0
    for m, r in RR.mutations(c).items():
        _, ex = B.share("dx", r["dx"], c)
        _, ez = B.share("dz", r["dz"], c)
        print("%s: mutation %-20s exceeds the bound %.1f x in dx, %.1f x in dz" % (name, m, ex, ez))
        if m == "prior_without_edges" and RR.frame_without_edges(s) is None:
            # every window frame has an out-edge: the condition has nothing to decide and the variant IS the true step.  Where it
            # decides - RR.NO_EDGES, at `tiny` and S-B size - it must be seen like any other
            assert np.array_equal(r["dx"], base["dx"]) and np.array_equal(r["dz"], base["dz"])
            continue
        assert max(ex, ez) > 1.0, m


def test_every_mutation_is_asserted_somewhere_at_tiny_and_at_sb_size():
    for g in ("tiny", "sb"):
        seen = set()
        for k in RR.ADMITTED:
            if k[0] == g:
                seen |= set(RR.MUTATIONS[k[3]]) - ({"prior_without_edges"} if k[4] != "no_edges" else set())
        assert seen == set(RR.MUTATIONS["both"]), g


@pytest.mark.parametrize("key", sorted(RR.LEFT_OUT), ids=_rid)
def test_what_is_left_out_still_misses_what_the_list_says(key):
    what, figure = RR.LEFT_OUT[key]
    c = RR.case(*key)
    if what.startswith("cap"):
        got = 4 * c["sc"][what[4:]]
        print("%s: 4 s_case(%s) = %.2e (listed %.2e), cap %.0e" % (_rid(key), what[4:], got, figure, B.CAP))
        assert got > B.CAP
    else:
        _, st = RR.restatement(c)
        _, got = B.share("dz", st["dz"], c)
        print("%s: s_case(dz) %.1e, the fp32 restatement's share of the bound on dz %.2f (listed %.2f)" % (_rid(key), c["sc"]["dz"], got, figure))
        assert got > 0.5
    assert abs(got - figure) <= 0.1 * figure                                   # (the list says what is measured)


def test_two_chained_steps_with_both_riders_and_the_prior_read_from_the_end_of_the_step():
    key = RR.TWO_STEPS
    c = RR.chain(*key[:4])
    print("%s x2: 4 s_case dx %.2e dz %.2e" % (_rid(key), 4 * c["sc"]["dx"], 4 * c["sc"]["dz"]))
    assert 4 * c["sc"]["dx"] <= B.CAP and 4 * c["sc"]["dz"] <= B.CAP and not c["base"]["rejected"]
    one = RR.chained(c["s"], 1, c["lm"], c["ep"])
    assert np.array_equal(one["dx"], RR.case(*key)["base"]["dx"])                 # one step of the chain IS the case's step
    wrong = RR.chained(c["s"], 2, c["lm"], c["ep"], prior_from_end=True)
    _, ex = B.share("dx", wrong["dx"], c)
    _, ez = B.share("dz", wrong["dz"], c)
    print("%s x2: the prior read from the end-of-step depth exceeds the bound %.1f x in dx, %.1f x in dz" % (_rid(key), ex, ez))
    assert max(ex, ez) > 1.0


def test_the_reduced_bound_separates_a_stereo_edges_cii_on_the_wrong_depth_frame():
    """the analogue of test_the_reduced_bound_separates_a_1e_3_error_of_the_reduced_system: the stereo edge of frame 3 adds its Cii
    (and bz) to frame 2's depth terms instead"""
    c = RR.case("tiny", "control", "local", "stereo")
    s, f = c["s"], c["f"]
    (S, rhs), (bS, br) = RR.reduced(s, f)
    low = B.lower_blocks(s["t1"] - s["t0"])
    g = dict(f, Cii=f["Cii"].copy(), bz=f["bz"].copy())
    assert s["ii"][2] == 2 and s["ii"][3] == 3 and s["st"][2] and s["st"][3]
    g["Cii"][2] += f["Cii"][3]; g["bz"][2] += f["bz"][3]
    g["Cii"][3] = 0.0; g["bz"][3] = 0.0
    S2, r2 = B.reduced_system(g, s)
    ex = max(float((np.abs(S2 - S)[low] / bS[low]).max()), float((np.abs(r2 - rhs) / br).max()))
    print("reduced system, a stereo edge's Cii on the wrong depth frame: %.0f x the bound" % ex)
    assert ex > 50.0
