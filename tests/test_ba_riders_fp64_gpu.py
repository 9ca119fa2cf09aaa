"""The sensor-depth prior (pvo_ba_depth_prior / pvo_ba_prior) and stereo edges (pvo_ba_stereo / pvo_ba_rig) of the dense bundle
adjustment on the GPU against fp64, in every form of pvo_ba_local's launch rule - tests/ba_rider_reference.py on top of
tests/ba_reference.py, every case admitted on the CPU by tests/test_ba_fp64_host.py first.  The cuts are test_ba_fp64_gpu.py's:

  A  the reduced system   ba_plan -> ba_depth_prior and / or ba_stereo -> ba_local: `sys` entry by entry within ba_reference.sys_bound
                          (with the prior's roundings and the stereo edge's row block counted), exact zeros outside the support; a
                          motion-only system has the bits it has without the stereo edges;
  C  the whole step       db.ba(..., disps_sens=, stereo_baseline=): dx per pose and dz per depth frame within 4 s_case + floors of the
                          fp64 step - the tiny regimes under both dampings, S-B size, one window per launch form, two chained steps,
                          and the row table's edges with a stereo edge in it (twice, at the back, 65 + out-edges, a source in front of
                          the window with no other out-edge, one eta row);
  the prior's edges       a measured frame without out-edges keeps dz = 0; sens == disps has the bits of the eta' form in the staged
                          and the 512-pixel forms too; NaN, negative and -inf are no measurement, +inf is a status and a zero pose update.

Every test asserts the launch form (and where it matters the frames' paths) of the window WITH its stereo edges before anything runs
on the device, and prints its form and the device's share of the bound (profiles/r26_ba_riders_fp64.txt)."""
import numpy as np
import pytest
import torch

import ba_reference as B
import ba_rider_reference as RR

pytestmark = pytest.mark.gpu

_id = lambda t: "-".join(x for x in t if x)
n64 = lambda t: t.detach().cpu().numpy().astype(np.float64)


def _operands(s, cuda, sens="own"):
    d = lambda t: t.to(cuda).contiguous().clone()
    o = {k: d(s[k]) for k in ("poses", "disps", "intr", "target", "weight", "eta", "ii", "jj")}
    sens = s["sens"] if isinstance(sens, str) else sens
    o["sens"] = None if sens is None else d(sens)
    return o


def _ba(o, s, iters, lm, ep, eta=None):
    """db.ba with the window's riders on the operands `o` (poses and disps are updated in place) -> (dx, dz, status)"""
    from pvo_amd import droid_backends as db
    st = torch.full((4,), -1, dtype=torch.int32, device=o["disps"].device)
    dx, dz = db.ba(o["poses"], o["disps"], o["intr"], o["target"], o["weight"], o["eta"] if eta is None else eta, o["ii"], o["jj"], s["t0"], s["t1"],
                   iters, lm, ep, False, status=st, disps_sens=o["sens"], alpha=s["alpha"], stereo_baseline=s["baseline"])
    return dx, dz, st


def _local(o, s, cuda, motion_only=False):
    """ba_plan -> the riders -> ba_local on a workspace and a zeroed `sys` of its own -> the int64 words"""
    from pvo_amd import droid_backends as db
    F, ht, wd = s["disps"].shape
    P, HW, E = s["t1"] - s["t0"], ht * wd, s["ii"].shape[0]
    ws = db.ba_workspace(E, P, F, HW, cuda)
    sysw = torch.zeros((6 * P) ** 2 + 6 * P, dtype=torch.int64, device=cuda)
    db.ba_plan(o["ii"], o["jj"], F, HW, -1 if motion_only else o["eta"].shape[0], s["t0"], s["t1"], ws)
    if o["sens"] is not None:
        db.ba_depth_prior(ws, E, P, F, HW, o["sens"], s["alpha"])
    if s["baseline"] > 0:
        db.ba_stereo(ws, E, P, F, HW, s["baseline"])
    db.ba_local(o["poses"], o["disps"], o["intr"], o["target"], o["weight"], None if motion_only else o["eta"], o["ii"], o["jj"], s["t0"], s["t1"],
                motion_only, sysw, ws)
    return sysw.cpu().numpy()


def _assert_form(key, s):
    form = B.launch_form(s)
    assert form == B.LAUNCH_FORMS[key[0]]
    want = RR.PATHS.get((key[0], key[3], key[4]))
    kinds = sorted({p for p, _, _ in B.frame_paths(s).values()})
    if want is not None:
        assert kinds == sorted(want), kinds
    return "%s; %s" % (form, " ".join(kinds))


# ------------------------------------------------------------------------------------------------ A: the reduced system
def _assert_system(key, c, cuda):
    s, f = c["s"], c["f"]
    form = _assert_form(key, s)
    P = s["t1"] - s["t0"]
    n6 = 6 * P
    (S, rhs), (bS, br) = RR.reduced(s, f)
    words = _local(_operands(s, cuda), s, cuda)
    raw = words[:n6 * n6].reshape(n6, n6)
    low = B.lower_blocks(P)
    sup = np.kron(B.block_support(s), np.ones((6, 6))) > 0
    assert not raw[~low].any() and not raw[low & ~sup].any()
    Sd, rd = B.decode_sys(words, P)
    eS, er = np.abs(Sd - S), np.abs(rd - rhs)
    sel = low & sup
    sh_S, sh_r = float((eS[sel] / bS[sel]).max()), float((er / br).max())
    print("%s [%s]: reduced system, device's share of the bound S %.3f rhs %.3f (largest entry %.2e)" % (_id(key), form, sh_S, sh_r, np.abs(S).max()))
    assert np.all(eS[sel] <= bS[sel]) and np.all(er <= br)
    assert raw[sel].any() and np.abs(Sd).max() > 0.5 * np.abs(S).max()


@pytest.mark.parametrize("key", RR.CUT_A, ids=_id)
def test_reduced_system_with_the_riders_matches_fp64_within_the_summation_bound(cuda, key):
    _assert_system(key, RR.case(*key), cuda)


@pytest.mark.parametrize("graph", ["tiny", "win29_odd", "c512_odd"])
def test_a_motion_only_system_has_the_bits_it_has_without_the_stereo_edges(cuda, graph):
    """include/pvo_hip.h, pvo_ba_stereo: a motion-only step gets nothing from a stereo edge - in front of the graph's edges or behind"""
    front = RR.rider_window(graph, "control", "stereo", **RR.options(graph, "stereo"))
    back = RR.rider_window(graph, "control", "stereo", **dict(RR.options(graph, "stereo"), back=True))
    plain = RR.rider_window(graph, "control", "none")
    assert front["n_stereo"] > 0 and plain["n_stereo"] == 0 and plain["ii"].shape[0] == front["ii"].shape[0] - front["n_stereo"]
    words = [_local(_operands(s, cuda), s, cuda, motion_only=True) for s in (plain, front, back)]
    print("%s [%s]: motion-only system, %d non-zero words" % (graph, B.launch_form(front), int((words[0] != 0).sum())))
    assert words[0].any() and np.array_equal(words[0], words[1]) and np.array_equal(words[0], words[2])


# ------------------------------------------------------------------------------------------------ C: the whole step
def _assert_step(name, c, dx, dz, st, form):
    base = c["base"]
    assert st.tolist() == [0, len(base["kx"]), 0, 0]
    ok_x, sh_x = B.share("dx", n64(dx), c)
    ok_z, sh_z = B.share("dz", n64(dz), c)
    print("%s [%s]: s_case dx %.2e dz %.2e; device's share of the bound dx %.3f dz %.3f" % (name, form, c["sc"]["dx"], c["sc"]["dz"], sh_x, sh_z))
    assert 4 * max(c["sc"]["dx"], c["sc"]["dz"]) <= B.CAP
    assert ok_x and ok_z


@pytest.mark.parametrize("key", RR.TINY + RR.SB + RR.LAUNCHES, ids=_id)
def test_one_step_with_the_riders_matches_the_fp64_step_within_its_own_sensitivity(cuda, key):
    c = RR.case(*key)
    s = c["s"]
    form = _assert_form(key, s)
    o = _operands(s, cuda)
    dx, dz, st = _ba(o, s, 1, c["lm"], c["ep"])
    _assert_step(_id(key), c, dx, dz, st, form)
    F = s["disps"].shape[0]
    kx = torch.from_numpy(c["base"]["kx"]).to(cuda)
    d0, d1 = s["disps"].to(cuda).reshape(F, -1)[kx], o["disps"].reshape(F, -1)[kx]
    # (the retraction: test_ba_fp64_gpu.py's bound for d0 + dz as one fused multiply-add or two roundings)
    assert bool(((d1 - (d0 + dz)).abs() <= 2.0 ** -22 * torch.maximum(torch.maximum(d0.abs(), dz.abs()), d1.abs())).all())


def test_two_iterations_with_both_riders_match_two_chained_fp64_steps(cuda):
    """disps[f] is the value at the START of each step for the prior (include/pvo_hip.h): tests/test_ba_fp64_host.py shows that a chain
    whose prior reads the depth the step ends with leaves this bound"""
    key = RR.TWO_STEPS
    c = RR.chain(*key[:4])
    s = c["s"]
    form = _assert_form(key, s)
    dx, dz, st = _ba(_operands(s, cuda), s, 2, c["lm"], c["ep"])
    _assert_step(_id(key) + " x2", c, dx, dz, st, form)


@pytest.mark.parametrize("key", RR.ROW_TABLE, ids=_id)
def test_the_row_tables_edges_with_a_stereo_edge(cuda, key):
    """cut A and cut C where a stereo edge meets the row table's other branches (ba_rider_reference.VARIANTS)"""
    c = RR.case(*key)
    s = c["s"]
    form = _assert_form(key, s)
    deg = B.max_out_degree(s)
    assert (deg > B.BALLOT_EDGES) == (key[4] == "deg65")
    _assert_system(key, c, cuda)
    dx, dz, st = _ba(_operands(s, cuda), s, 1, c["lm"], c["ep"])
    _assert_step(_id(key), c, dx, dz, st, form)


# ------------------------------------------------------------------------------------------------ the prior's edges
@pytest.mark.parametrize("key", RR.NO_EDGES, ids=_id)
def test_a_measured_frame_without_out_edges_keeps_its_depths(cuda, key):
    c = RR.case(*key)
    s = c["s"]
    form = _assert_form(key, s)
    fr = RR.frame_without_edges(s)
    assert s["t0"] <= fr < s["t1"] and not bool((s["ii"] == fr).any()) and bool((s["sens"][fr] > 0).any())
    _assert_system(key, c, cuda)
    o = _operands(s, cuda)
    dx, dz, st = _ba(o, s, 1, c["lm"], c["ep"])
    _assert_step(_id(key), c, dx, dz, st, form)
    k = int(np.nonzero(c["base"]["kx"] == fr)[0][0])
    assert not bool(dz[k].any()) and torch.equal(o["disps"][fr].cpu(), s["disps"][fr]) and not c["base"]["dz"][k].any()


@pytest.mark.parametrize("graph", ["win29", "c512"])
def test_a_map_equal_to_the_depths_takes_the_step_of_the_swapped_eta_bit_for_bit(cuda, graph):
    """include/pvo_hip.h, pvo_ba_depth_prior: residual exactly 0 gives, for ONE step, the bits of pvo_ba with
    eta' = where(disps_sens > 0, alpha, eta) - where ba_depth_kernel runs in front (tests/test_rgbd_gpu.py holds the fused form)"""
    s = RR.rider_window(graph, "control", "prior")
    form = B.launch_form(s)
    assert form == B.LAUNCH_FORMS[graph] and form != "fused256"
    kx = torch.from_numpy(np.unique(np.concatenate([np.arange(s["t0"], s["t1"]), s["ii"].numpy()])))
    meas = s["sens"] > 0
    zero_res = torch.where(meas, s["disps"], torch.zeros_like(s["disps"]))
    eta2 = torch.where(meas[kx], torch.full_like(s["eta"], s["alpha"]), s["eta"])
    lm, ep = B.DAMPINGS["local"]
    a, b, plain = _operands(s, cuda, sens=zero_res), _operands(s, cuda, sens=None), _operands(s, cuda, sens=None)
    ra = _ba(a, s, 1, lm, ep)
    rb = _ba(b, s, 1, lm, ep, eta=eta2.to(cuda).contiguous())
    _ba(plain, s, 1, lm, ep)
    print("%s [%s]: sens == disps against the swapped eta, one step" % (graph, form))
    assert ra[2].tolist()[0] == 0 and torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    assert torch.equal(a["poses"], b["poses"]) and torch.equal(a["disps"], b["disps"]) and not torch.equal(a["disps"], plain["disps"])


def test_what_is_no_measurement_and_what_is_a_poisoned_one(cuda):
    """include/pvo_hip.h, pvo_ba_depth_prior: NaN, a negative value and -inf are no measurement - the bits of 0 there; +inf is a
    poisoned operand: a status and a zero pose update, never a wrong step.  Arithmetic on non-finite VALUES only: every index is the
    clean window's."""
    key = ("tiny", "control", "local", "prior", "")
    c = RR.case(*key)
    s = c["s"]
    form = _assert_form(key, s)
    F, ht, wd = s["disps"].shape
    fr = 3
    pix = torch.nonzero(s["sens"][fr].view(-1) > 0).view(-1)[[0, 11, 12, 30, 60]].tolist()      # measured pixels, two of them neighbours
    assert s["t0"] <= fr < s["t1"] and len(set(pix)) == 5 and all(float(s["sens"][fr].view(-1)[p]) > 0 for p in pix)
    none, zero = s["sens"].clone(), s["sens"].clone()
    for p, v in zip(pix, (float("nan"), -1.0, float("-inf"), -0.0, float("nan"))):
        none[fr].view(-1)[p] = v
        zero[fr].view(-1)[p] = 0.0
    oa, ob = _operands(s, cuda, sens=none), _operands(s, cuda, sens=zero)
    ra, rb = _ba(oa, s, 1, c["lm"], c["ep"]), _ba(ob, s, 1, c["lm"], c["ep"])
    assert ra[2].tolist() == [0, len(c["base"]["kx"]), 0, 0]
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]) and torch.equal(oa["disps"], ob["disps"]) and bool(torch.isfinite(oa["disps"]).all())
    inf = s["sens"].clone()
    inf[fr].view(-1)[pix[0]] = float("inf")
    oi = _operands(s, cuda, sens=inf)
    dx, dz, st = _ba(oi, s, 1, c["lm"], c["ep"])
    print("tiny-prior [%s]: NaN, -1, -inf, -0 are the bits of 0; +inf: status %s, max |dx| %.1e" % (form, st.tolist(), float(dx.abs().max())))
    assert st.tolist() == [1, len(c["base"]["kx"]), 0, 0]
    assert not bool(dx.any()) and torch.equal(oi["poses"], s["poses"].to(cuda))
    k = int(np.nonzero(c["base"]["kx"] == fr)[0][0])
    finite = torch.isfinite(dz)
    finite[k, pix[0]] = True
    assert bool(finite.all())                                                  # the depth-only step is non-finite at that pixel alone
    # the call after it computes what a fresh one computes (the flag and the system are cleared by the solve that consumed them)
    oc = _operands(s, cuda)
    dx2, dz2, st2 = _ba(oc, s, 1, c["lm"], c["ep"])
    _assert_step("tiny-prior after +inf", c, dx2, dz2, st2, form)
