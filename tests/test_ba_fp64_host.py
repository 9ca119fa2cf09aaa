"""The plain bundle adjustment against fp64, host side: tests/ba_reference.py is qualified - its reduced system is the first half of the
step it stands beside, its fixed-point decoding inverts the device's encoding - and every case tests/test_ba_fp64_gpu.py runs is held
to the ADMISSION rule stated there.  Per admitted case this prints s_case, the fp32 restatement's share of each bound and every
mutation's excess (profiles/r15_ba_fp64.txt records them).  No GPU is needed."""
import numpy as np
import pytest

import ba_reference as B
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
