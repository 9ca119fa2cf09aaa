"""SE(3) exp / log / retraction and their gradients at every rotation angle, against tests/se3_reference.py (the matrix exponential of the
twist in fp64 and its autograd; for log's gradient the inverse-function identity).  Each case runs on the torch formulation (CPU) and on
the native kernels (GPU), in fp32 and fp64, over the sweep [A, 64, 6]: the 19 angles of se3_reference.ANGLES from 0 to pi - 1e-3 plus
both sides of every cutoff of pvo_amd.geom.se3, translations of N(0, I) and 10 N(0, I).  The bounds are multiples of the type's eps
(the unit roundoff) and do not depend on the angle: a closed form that cancels, or a series cut short, shows as a multiple of 1 / theta.
Each case prints its per-angle maxima."""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import se3_reference as R
from pvo_amd.geom import se3 as S
from pvo_amd.geom.se3 import SE3

# the formulation's cutoffs: on theta for the coefficients, and on |v| = sin(theta / 2) for log's quaternion coefficient, as angles
CUTS = tuple(sorted(set(S.CUTOFF.values()) | set(2.0 * math.asin(c) for c in S.Q_CUTOFF.values())))
TH = torch.tensor(R.angles(CUTS), dtype=torch.float64)
XI = R.sweep(64, 0, CUTS)                                                     # [A, 64, 6], never written to
A, N = XI.shape[:2]
UPTO3 = TH <= 3.0

IMPLS = ["torch", pytest.param("native", marks=pytest.mark.gpu)]
DTYPES = [torch.float32, torch.float64]
both = lambda f: pytest.mark.parametrize("impl", IMPLS)(pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])(f))


def _device(request, impl):
    return request.getfixturevalue("cuda") if impl == "native" else torch.device("cpu")


def _eps(dtype):
    """eps_T: the unit roundoff of the type, 2^-24 / 2^-53 (half of torch.finfo's eps, the spacing at 1): 64 eps = 3.8e-6 in fp32"""
    return 0.5 * torch.finfo(dtype).eps


def _grad_bound(dtype):
    """64 eps (3.8e-6) in fp32; in fp64 1e-12: four decades under what the 1e-6 switch gave at 1.5e-6, three above reference = code at theta >= 1"""
    return 64 * _eps(dtype) if dtype == torch.float32 else 1e-12


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _tau_scale(xi):
    return xi[..., :3].norm(dim=-1).clamp(min=1.0)


def _report(name, impl, dtype, fig, bound, rows=None):
    """fig [A]: one figure per angle; prints them all, then asserts that they are finite and within the bound"""
    th = TH if rows is None else TH[rows]
    fig = fig.detach().double().cpu()
    print("\n%s, %s %s, bound %.3g" % (name, impl, str(dtype).replace("torch.", ""), bound))
    print("  " + "  ".join("%.4g:%.2e" % (t, f) for t, f in zip(th.tolist(), fig.tolist())))
    bad = [(t, f) for t, f in zip(th.tolist(), fig.tolist()) if not f <= bound]          # (NaN is bad)
    assert not bad, "%s: (theta, figure) over %.3g: %s" % (name, bound, bad)


def _rel_per_angle(got, ref):
    """[A, n, k] -> [A]: the largest error of an angle over the largest reference entry of that angle; NaN where anything is not finite"""
    got, ref = got.detach().double().cpu().flatten(1), ref.detach().double().cpu().flatten(1)
    rel = (got - ref).abs().max(1).values / ref.abs().max(1).values
    return torch.where(torch.isfinite(got).all(1), rel, torch.full_like(rel, float("nan")))


@functools.lru_cache(None)
def _inputs(dtype):
    """the sweep rounded to dtype, and the reference on exactly those inputs: matrices, and the VJPs for the fixed cotangents"""
    x = XI.to(dtype)
    xr = x.double().clone().requires_grad_(True)
    M, t = R.exp_ref(xr)
    ct, cR = _randn((A, N, 3), 1), _randn((A, N, 3, 3), 2)
    gt, = torch.autograd.grad((t * ct).sum(), xr, retain_graph=True)
    gR, = torch.autograd.grad((M[..., :3, :3] * cR).sum(), xr)
    return x, M.detach(), ct, cR, gt, gR


@functools.lru_cache(None)
def _poses(dtype):
    """one random pose per row (fp64 exp of 0.5 N(0, I), rounded to dtype) and its matrix"""
    X = SE3.exp(0.5 * _randn((A, N, 6), 3)).data.to(dtype)
    return X, R.pose_matrix(X)


def _check_values(name, impl, dtype, g, M, xi):
    """translation, rotation and unit norm of the group elements g [A, n, 7] against the matrices M, as the issue's case (a)"""
    g = g.detach().double().cpu()
    eps, th = _eps(dtype), TH[:, None]
    et = (g[..., :3] - M[..., :3, 3]).norm(dim=-1) / ((1 + th + th * th) * _tau_scale(xi))
    _report(name + " translation / ((1 + th + th^2) max(1, |tau|))", impl, dtype, et.max(1).values, 16 * eps)
    eR = (R.quat_matrix(g[..., 3:]) - M[..., :3, :3]).abs().flatten(2).max(2).values
    _report(name + " rotation matrix", impl, dtype, eR.max(1).values, 16 * eps)
    _report(name + " | |q| - 1 |", impl, dtype, (g[..., 3:].norm(dim=-1) - 1).abs().max(1).values, 8 * eps)


def _check_grads(name, impl, dtype, x, g, ct, cR, gt, gR):
    """VJPs of g(x) [A, n, 7] with respect to x for a cotangent on the translation and one on the rotation matrix of the quaternion"""
    dev = x.device
    got_t, = torch.autograd.grad((g[..., :3].double() * ct.to(dev)).sum(), x, retain_graph=True)
    got_R, = torch.autograd.grad((R.quat_matrix(g[..., 3:]) * cR.to(dev)).sum(), x)
    assert got_t.dtype == dtype and got_R.dtype == dtype
    _report(name + " VJP of the translation", impl, dtype, _rel_per_angle(got_t, gt), _grad_bound(dtype))
    _report(name + " VJP of the rotation", impl, dtype, _rel_per_angle(got_R, gR), _grad_bound(dtype))


@both
def test_exp_values(request, impl, dtype):
    x, M = _inputs(dtype)[:2]
    X = SE3.exp(x.to(_device(request, impl)))
    assert X.data.dtype == dtype
    _check_values("exp", impl, dtype, X.data, M, x.double())


@both
def test_exp_gradients(request, impl, dtype):
    x, _, ct, cR, gt, gR = _inputs(dtype)
    x = x.to(_device(request, impl)).clone().requires_grad_(True)
    _check_grads("exp", impl, dtype, x, SE3.exp(x).data, ct, cR, gt, gR)


def _near_pi_rows(dtype):
    """two group elements with |w| < 1e-6, one of either sign: log's w -> 0 branch"""
    v = torch.tensor([[0.6, -0.48, 0.64], [-0.28, 0.96, 0.0]], dtype=torch.float64)
    q = torch.cat([v, torch.tensor([[5e-7], [-3e-7]], dtype=torch.float64)], -1)
    q = q / q.norm(dim=-1, keepdim=True)
    t = torch.tensor([[0.3, -1.2, 2.0], [-4.0, 0.5, 7.0]], dtype=torch.float64)
    return torch.cat([t, q], -1).to(dtype)


@both
def test_log_values(request, impl, dtype):
    dev, eps = _device(request, impl), _eps(dtype)
    X = SE3.exp(XI).data.to(dtype)                                             # fp64 group elements, rounded to dtype
    xi = SE3(X.to(dev)).log().double().cpu()
    assert torch.isfinite(xi).all()
    err = (xi - XI).abs().max(-1).values / _tau_scale(XI)
    _report("log |log(X) - xi| / max(1, |tau|)", impl, dtype, err.max(1).values[UPTO3], 32 * eps, UPTO3)

    def round_trip(name, g, rows=None):
        y = SE3(g.to(dev)).log().double().cpu()
        assert torch.isfinite(y).all(), name
        e = (R.exp_ref(y)[0] - R.pose_matrix(g)).abs().flatten(-2).max(-1).values / g[..., :3].double().norm(dim=-1).clamp(min=1.0)
        if e.dim() == 1:
            print("\n%s, %s %s: %s, bound %.3g" % (name, impl, dtype, e.tolist(), 64 * eps))
            assert (e <= 64 * eps).all(), (name, e.tolist())
        else:
            _report(name, impl, dtype, e.max(1).values if rows is None else e.max(1).values[rows], 64 * eps, rows)
    round_trip("log round trip at pi - 1e-3", X, ~UPTO3)
    round_trip("log round trip of -q", torch.cat([X[..., :3], -X[..., 3:]], -1))
    rows = _near_pi_rows(dtype)
    assert (rows[:, 6].abs() < 1e-6).all() and rows[0, 6] > 0 > rows[1, 6]
    round_trip("log round trip at |w| < 1e-6", rows)


@both
def test_log_gradients(request, impl, dtype):
    """the inverse-function identity: the VJP of log(exp(xi)) with respect to xi is the cotangent"""
    x = XI.to(dtype).to(_device(request, impl)).clone().requires_grad_(True)
    c = _randn((A, N, 6), 4).to(dtype)
    got, = torch.autograd.grad((SE3.exp(x).log() * c.to(x.device)).sum(), x)
    _report("log VJP of log(exp(xi)) against the cotangent", impl, dtype, _rel_per_angle(got, c)[UPTO3], 64 * _eps(dtype), UPTO3)


@both
def test_retraction(request, impl, dtype):
    """X.retr(a) = Exp(a) X, the path of geom/ba.py: values and the gradients with respect to a"""
    dev = _device(request, impl)
    a = _inputs(dtype)[0]
    X, MX = _poses(dtype)
    ar = a.double().clone().requires_grad_(True)
    M = R.exp_ref(ar)[0] @ MX
    ct, cR = _randn((A, N, 3), 5), _randn((A, N, 3, 3), 6)
    gt, = torch.autograd.grad((M[..., :3, 3] * ct).sum(), ar, retain_graph=True)
    gR, = torch.autograd.grad((M[..., :3, :3] * cR).sum(), ar)
    x = a.to(dev).clone().requires_grad_(True)
    Y = SE3(X.to(dev)).retr(x)
    assert Y.data.dtype == dtype
    _check_values("retr", impl, dtype, Y.data, M.detach(), a.double())
    _check_grads("retr", impl, dtype, x, Y.data, ct, cR, gt, gR)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,atol,rtol", [(torch.float64, 1e-12, 1e-10), (torch.float32, 2e-6, 2e-4)], ids=["fp64", "fp32"])
def test_kernels_equal_the_torch_formulation_on_the_sweep(cuda, dtype, atol, rtol):
    """the tolerances of test_se3.py's parity tests (whose inputs are O(1): the absolute one scales with max(1, |tau|) here), at the
    angles they never enter; the gradients per angle"""
    from test_se3 import torch_formulation
    X0 = _poses(dtype)[0].to(cuda)
    cot = [_randn((A, N, k), 7 + i).to(cuda, dtype) for i, k in enumerate((7, 6, 7))]

    def run():
        x = XI.to(cuda, dtype).requires_grad_(True)
        E = SE3.exp(x)
        outs = [E.data, E.log(), SE3(X0).retr(x).data]
        grads = [torch.autograd.grad((o * c).sum(), x, retain_graph=True)[0] for o, c in zip(outs, cot)]
        return [o.detach() for o in outs], grads
    on, gn = run()
    with torch_formulation():
        ot, gt = run()
    scale = _tau_scale(XI).to(cuda)[..., None]
    for name, n_, t_ in zip(("exp", "log", "retr"), on, ot):
        _report("parity " + name + " values / max(1, |tau|)", "native", dtype, ((n_ - t_).abs() / scale).flatten(1).max(1).values, atol)
    for name, n_, t_ in zip(("exp", "log", "retr"), gn, gt):
        _report("parity " + name + " gradients", "native", dtype, _rel_per_angle(n_, t_), rtol)


# ---- the native training BA: its own retraction, differentiated through se3_exp on dual numbers -----------------------------------------

@functools.lru_cache(None)
def _ba_scene():
    """test_ba_native._scene at B = 1, P = 4, 6 x 7, made so that one step's dx has a rotation of some 1e-4 and a translation of 0.3.
    Perturbing the initial poses does not do that here: one damped Gauss-Newton step on 42 pixels answers any pose offset, lateral or
    forward, exact depths or not, with a rotation of about half its translation (measured: 1e-2 to 1.5e-1 at a translation of 0.3).
    So the target is placed where the step's own linearisation puts the offset delta (rotation 3e-4, translation 0.3 per free pose):
    target = coords(poses, disps) + Ji delta_i + Jj delta_j + flow noise of 1e-3 px, whose least-squares step is delta itself; the
    weights are 1000 x the scene's so that the damping (0.1 on the diagonal) does not bend it.  -> scene, ii, jj, the fp64 torch BA's
    poses after one step and its gradients"""
    from test_ba_native import _run, _scene
    from pvo_amd.geom import projective_ops as pops
    from pvo_amd.geom.ba import BA as torch_BA
    s, ii, jj = _scene(1, 4, 6, 7, seed=2)
    g = torch.Generator().manual_seed(102)
    d = torch.randn(1, 4, 6, generator=g, dtype=torch.float64)
    d[..., :3] *= 0.3 / d[..., :3].norm(dim=-1, keepdim=True)
    d[..., 3:] *= 3e-4 / d[..., 3:].norm(dim=-1, keepdim=True)
    d[:, 0] = 0                                                               # the fixed pose
    c, _, (Ji, Jj, _) = pops.projective_transform(SE3(s["poses"]), s["disps"], s["intr"], ii, jj, jacobian=True)
    s["target"] = (c + (Ji @ d[:, ii, None, None, :, None])[..., 0] + (Jj @ d[:, jj, None, None, :, None])[..., 0] +
                   1e-3 * torch.randn(c.shape, generator=g, dtype=torch.float64))
    s["weight"] = 1000.0 * s["weight"]
    G, _, grads = _run(torch_BA, s, ii, jj, 1, steps=1, dev="cpu")
    return s, ii, jj, G, grads


def test_ba_scene_steps_into_the_small_rotation_band():
    """the condition the native-BA test relies on, on the fp64 torch BA's step log(p1 p0^-1): at least half of the free poses have a
    rotation in [1e-5, 1e-3] and a translation of at least 0.1"""
    s, _, _, G, _ = _ba_scene()
    dx = (SE3(G) * SE3(s["poses"]).inv()).log()[0, 1:]
    rot, tr = dx[:, 3:].norm(dim=-1), dx[:, :3].norm(dim=-1)
    print("\nBA step: rotation %s, translation %s" % (rot.tolist(), tr.tolist()))
    inside = (rot >= 1e-5) & (rot <= 1e-3) & (tr >= 0.1)
    assert 2 * int(inside.sum()) >= inside.numel(), (rot.tolist(), tr.tolist())


@pytest.mark.gpu
def test_native_ba_gradients_with_a_step_in_the_small_rotation_band(cuda):
    """pvo_ba_train_vjp in fp32 against the fp64 torch BA, gradients with respect to target and weight, to the tolerance of
    test_ba_native.test_fp32_matches_reference_fixtures (1e-3 of the largest entry + 1e-7)"""
    from test_ba_native import _close_grads, _run
    from pvo_amd.geom import ba_native
    s, ii, jj, _, ref = _ba_scene()
    _, _, got = _run(ba_native.BA, {k: v.float() for k, v in s.items()}, ii, jj, 1, steps=1, dev=str(cuda))
    got = {k: got[k].double().cpu() for k in ("target", "weight")}
    for k in got:
        print("\nnative BA grad_%s: max error %.3g of max |ref| %.3g" % (k, (got[k] - ref[k]).abs().max().item(), ref[k].abs().max().item()))
    _close_grads(got, {k: ref[k] for k in got}, 1e-3, 1e-7)


# ---- the yardstick and the two copies of the constants --------------------------------------------------------------------------------

def test_reference_against_multiprecision():
    """exp_ref qualifies before anything is held to it: against mpmath's expm at 40 digits, its translation is within 8 eps max(1, |tau|)
    (half of the value tests' bound: the reference may use no more of it), at small, middle and large angles and |tau| up to 30"""
    import mpmath as mp
    worst = 0.0
    with mp.workdps(40):
        for a in (8, 12, 15, 17):                                             # theta = 1e-4, 1e-2, 0.5, 3
            for r in (3, 40, 50, 63):
                xi = XI[a, r]
                E = mp.expm(mp.matrix([[mp.mpf(v) for v in row] for row in R.twist(xi).tolist()]))
                t = R.exp_ref(xi)[1].tolist()
                err = max(abs(float(E[i, 3] - mp.mpf(t[i]))) for i in range(3)) / max(1.0, float(xi[:3].norm()))
                worst = max(worst, err)
    print("\nexp_ref against 40 digits: %.3g, bound %.3g" % (worst, 8 * _eps(torch.float64)))
    assert worst <= 8 * _eps(torch.float64)


def test_header_and_formulation_carry_the_same_constants():
    """csrc/se3_dual.h (Cut<float>, Cut<double>, the SE3_SERIES tables) against CUTOFF, TERMS, Q_CUTOFF and the S_ tables of geom/se3.py:
    the sweep takes its cutoff sides from the Python module, so the header must not drift from it"""
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(S.__file__)), "..", "csrc", "se3_dual.h")).read()
    for ctype, dtype in (("float", torch.float32), ("double", torch.float64)):
        m = re.search(r"struct Cut<%s> \{ static constexpr double theta = ([0-9.e-]+), n = ([0-9.e-]+); static constexpr int terms = (\d+); \};" % ctype, text)
        assert m, ctype
        assert (float(m.group(1)), float(m.group(2)), int(m.group(3))) == (S.CUTOFF[dtype], S.Q_CUTOFF[dtype], S.TERMS[dtype])
    tables = {name: body for name, body in re.findall(r"^SE3_SERIES\((\w+),([^)]*)\)", text, re.M)}
    pairs = dict(kImag=S.S_IMAG, kReal=S.S_REAL, kC1=S.S_C1, kC2=S.S_C2, kLogC2=S.S_LOG_C2, kAtan=S.S_ATAN + (0.0, 0.0, 0.0))
    assert set(tables) == set(pairs)
    for name, want in pairs.items():
        got = tuple(float(a) / float(b) if b else float(a) for a, b in re.findall(r"(-?[0-9.]+)(?: / ([0-9.]+))?", tables[name]))
        assert got == tuple(want), name
