"""The training path's native bundle adjustment (pvo_amd/csrc/ba_train.hip; proj_fwd_kernel / proj_vjp_kernel of se3_ops.hip) against
the fp64 HOST reference of tests/ba_train_reference.py, on cases in which every mask fires, a frame has no out-edges, an edge has
i == j, an edge is listed twice and keyframes' edges are not contiguous (admitted on the host: tests/test_ba_train_fp64_host.py).

  fp32   the error of every output (poses, disps, dx, the five gradients), relative to the largest fp64 magnitude, is at most
         FACTOR = 4 times e_pt, the same error of PyTorch's own fp32 evaluation - the larger of the CPU's and of the PyTorch
         formulation on the device, which sums in another order.  Zero patterns of disps and rejected systems are exact.
  fp64   poses, disps and dx within 1e-9, gradients within 1e-8 of the largest plus 1e-12 (test_fp64_two_steps_match_torch_ba's).
  reject a system the reference rejects gives dx = 0 exactly, in both types, and leaves the other batch element's bits alone.
  cut    proj_transform / proj_transform_vjp alone by the same rules; validity bit-equal.
  state  the C entry points on buffers of the test's own: NaN or zeros in workspace and scratch change no bit, nothing is written
         beyond the declared byte counts or beside an output, a second backward repeats g_target / g_weight / g_eta bit for bit.
         (g_poses / g_disps are summed with floating-point atomics by proj_vjp_kernel: they are compared to the rounding of a
         reordered sum, not bit for bit.)
  codes  every refusal is answered before any launch: poisoned outputs stay as they were.
No test passes a frame index outside [0, P).

Every figure is printed on a line that starts with `ba_train`; profiles/r22_ba_train_fp64.txt is those lines of one run."""
import ctypes

import pytest
import torch

import ba_train_reference as R
from test_se3 import torch_formulation

ONE_STEP = [(c, i) for c, i in zip(R.CASES, R.CASE_IDS) if c[5] == 1]
GUARD = 4096


def _case(shape):
    c = R.case(*shape)
    assert c.admission["ok"] and c.admission["offenders"] is None               # (tests/test_ba_train_fp64_host.py prints the counts)
    return c


def _native_step(*a):
    from pvo_amd.geom import ba_native
    G, d, dx = ba_native.step(*a[:8], fixedp=a[8])
    return G, d, dx, None


# ---- fp32 and fp64, forward and backward -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.CASES, ids=R.CASE_IDS)
def test_fp32_error_is_within_four_times_pytorchs_own(cuda, shape):
    """Measured on an MI355X (profiles/r22_ba_train_fp64.txt): the largest ratio of the 82 figures is 2.08 (g_eta of B2-P5-fix1-6x7-steps1),
    the median 0.7; the projection cut's largest is 1.91"""
    c = _case(shape)
    cid = R.CASE_IDS[R.CASES.index(shape)]
    with torch_formulation():
        dev32, _ = R.evaluate_torch(c.s, c.ii, c.jj, c.fixedp, c.steps, torch.float32, cuda)
    e_dev = R.errors(dev32, c.ref)
    e_pt = R.larger(c.e_pt, e_dev)
    got, _ = R.run_chain(_native_step, c.s, c.ii, c.jj, c.fixedp, c.steps, torch.float32, cuda)
    ratios, bad = R.accept(got, c.ref, e_pt)
    err = R.errors(got, c.ref)
    for k in ratios:
        print("ba_train fp32 %s %-8s error %.3g of the largest %.3g; e_pt %.3g (cpu %.3g, device %.3g); ratio %.2f"
              % (cid, k, err[k], R.scale_of(c.ref, k), e_pt[k], c.e_pt[k], e_dev[k], ratios[k]))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("shape", R.CASES, ids=R.CASE_IDS)
def test_fp64_matches_the_host_reference(cuda, shape):
    c = _case(shape)
    cid = R.CASE_IDS[R.CASES.index(shape)]
    got, _ = R.run_chain(_native_step, c.s, c.ii, c.jj, c.fixedp, c.steps, torch.float64, cuda)
    bad = []
    for k in R.outputs_of(c.ref):
        if not c.ref[k].numel():
            continue
        err, scale = float((got[k] - c.ref[k]).abs().max()), R.scale_of(c.ref, k)
        tol = 1e-8 * scale + 1e-12 if k.startswith("g_") else 1e-9
        print("ba_train fp64 %s %-8s error %.3g, largest %.3g; share of the tolerance %.3g" % (cid, k, err, scale, err / tol))
        if not err <= tol:
            bad.append((k, err, tol))
    assert torch.equal(got["disps"] == 0, c.ref["disps"] == 0)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_a_rejected_system_gives_exactly_zero_dx_and_leaves_the_other_element_alone(cuda, dtype):
    """batch element 1 with negated weights is not positive definite: the reference rejects it (dx = 0), and so must the kernel,
    exactly, in either type; element 0 keeps every bit of the run in which element 1 is sound"""
    from pvo_amd.geom import ba_native
    from pvo_amd.geom.se3 import SE3
    c = _case((2, 5, 1, 6, 7, 1))
    s = dict(c.s)
    s["weight"] = c.s["weight"].clone()
    s["weight"][1] = -s["weight"][1]
    with torch.no_grad():
        _, _, cut = R.ba_step(*[s[k] if k != "poses" else SE3(s[k]) for k in ("target", "weight", "eta", "poses", "disps", "intr")], c.ii, c.jj, c.fixedp)
    assert bool((cut["dx"][1] == 0).all()) and float(cut["dx"][0].abs().max()) > 0

    def run(sc):
        a = [sc[k].to(cuda, dtype) for k in ("target", "weight", "eta")]
        G, d, dx = ba_native.step(*a, SE3(sc["poses"].to(cuda, dtype)), sc["disps"].to(cuda, dtype), sc["intr"].to(cuda, dtype), c.ii, c.jj, fixedp=c.fixedp)
        return G.data, d, dx
    sound, broken = run(c.s), run(s)
    assert torch.equal(broken[2][1], torch.zeros_like(broken[2][1]))
    assert torch.equal(broken[0][1], c.s["poses"][1].to(cuda, dtype))           # Exp(0) G == G, bit for bit
    assert torch.isfinite(broken[1]).all()
    for a, b in zip(sound, broken):
        assert torch.equal(a[0], b[0])


# ---- the projection cut ----------------------------------------------------------------------------------------------------------------

def _native_projection(c, dtype, dev):
    from pvo_amd import droid_backends as db
    poses, disps, intr = (c.s[k].to(dev, dtype).contiguous() for k in ("poses", "disps", "intr"))
    ii, jj = c.ii.to(dev), c.jj.to(dev)
    x1, valid, (Ji, Jj, Jz) = db.proj_transform(poses, disps, intr, ii, jj, jacobian=True)
    cot = {k: v.to(dev, dtype) for k, v in R.projection_cotangents(x1.shape[:4]).items()}
    gp, gd = db.proj_transform_vjp(poses, disps, intr, ii, jj, cot["x1"], cot["Ji"], cot["Jj"], cot["Jz"])
    out = dict(x1=x1, Ji=Ji, Jj=Jj, Jz=Jz, g_poses=gp, g_disps=gd)
    return {k: v.double().cpu() for k, v in out.items()}, valid.float().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("shape,cid", ONE_STEP, ids=[i for _, i in ONE_STEP])
def test_projection_cut(cuda, shape, cid, dtype):
    c = _case(shape)
    ref, valid_ref = R.projection_cut(c.s, c.ii, c.jj)
    Z = c.cuts[0]["Z"]
    near = Z < 0.1
    assert int(near.sum()) >= R.MIN_FIRE and torch.equal(valid_ref[..., 0] > 0, Z > 0.2)
    got, valid = _native_projection(c, dtype, cuda)
    assert valid.shape == valid_ref.shape and torch.equal(valid, valid_ref)             # bit-equal: 0.0 / 1.0, no sample left out
    err = R.errors(got, ref)
    # the rows behind the guard alone (1 / Z replaced by 1, derivative 0), relative to the same largest values
    err_near = {k: float((got[k] - ref[k])[near].abs().max()) / R.scale_of(ref, k) for k in ("x1", "Ji", "Jj", "Jz")}
    bad = []
    if dtype == torch.float32:
        cpu32, v_cpu = R.projection_cut(c.s, c.ii, c.jj, torch.float32)
        with torch_formulation():
            dev32, v_dev = R.projection_cut(c.s, c.ii, c.jj, torch.float32, cuda)
        assert torch.equal(v_cpu, valid_ref) and torch.equal(v_dev, valid_ref)
        e_pt = R.larger(R.errors(cpu32, ref), R.errors(dev32, ref))
        for k in err:
            ratio = err[k] / e_pt[k] if e_pt[k] > 0 else (0.0 if err[k] == 0 else float("inf"))
            print("ba_train cut fp32 %s %-8s error %.3g of the largest %.3g (Z < 0.1 rows: %.3g); e_pt %.3g; ratio %.2f"
                  % (cid, k, err[k], R.scale_of(ref, k), err_near.get(k, float("nan")), e_pt[k], ratio))
            if not err[k] <= R.FACTOR * e_pt[k]:
                bad.append((k, err[k], e_pt[k]))
    else:
        for k in err:
            scale = R.scale_of(ref, k)
            tol = 1e-9 if k == "x1" else 1e-8 * scale + 1e-12                       # coordinates as values, Jacobians and VJPs as gradients
            e = err[k] * scale
            print("ba_train cut fp64 %s %-8s error %.3g, largest %.3g (Z < 0.1 rows: %.3g); share of the tolerance %.3g"
                  % (cid, k, e, scale, err_near.get(k, float("nan")) * scale, e / tol))
            if not e <= tol:
                bad.append((k, e, tol))
    assert not bad, bad


# ---- the C entry points on buffers of the test's own ----------------------------------------------------------------------------------

class _Guarded:
    """`nbytes` bytes with GUARD bytes of 0xFF (NaN in either type) before and after; the payload starts as `fill` bytes"""

    def __init__(self, nbytes, dev, fill=0xFF):
        self.n = int(nbytes)
        self.buf = torch.full((2 * GUARD + self.n,), 0xFF, dtype=torch.uint8, device=dev)
        self.payload = self.buf[GUARD:GUARD + self.n]
        self.payload.fill_(fill)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + GUARD) if self.n else None

    def guards_intact(self):
        return bool((self.buf[:GUARD] == 0xFF).all()) and bool((self.buf[GUARD + self.n:] == 0xFF).all())

    def untouched(self):
        return bool((self.buf == 0xFF).all())

    def tensor(self, dtype, shape):
        return self.payload.clone().view(dtype).view(shape)


def _operands(c, dtype, dev, P=None):
    from pvo_amd.geom import ba_native
    o = {k: c.s[k].to(dev, dtype).contiguous() for k in R.LEAVES + ("intr",)}
    o["ii"], o["jj"] = c.ii.to(dev).contiguous(), c.jj.to(dev).contiguous()
    o["plan"] = ba_native.make_plan(o["ii"])
    cp, cd = R.cotangents(*c.s["disps"].shape)
    o["g_poses_out"], o["g_disps_out"] = cp.to(dev, dtype).contiguous(), cd.to(dev, dtype).contiguous()
    return o


def _sizes(c, dtype):
    B, P, fixedp, ht, wd, _ = c.shape
    N, M, isz = c.ii.shape[0], P - 1, torch.empty(0, dtype=dtype).element_size()
    return dict(B=B, P=P, N=N, M=M, ht=ht, wd=wd, fixedp=fixedp, isz=isz,
                poses=B * P * 7 * isz, disps=B * P * ht * wd * isz, dx=B * 6 * (P - fixedp) * isz, edge=B * N * ht * wd * 2 * isz,
                eta=B * M * ht * wd * isz)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _forward(lib, o, z, out, ws, ws_bytes, dt, stream, **over):
    a = dict(poses=_p(o["poses"]), P=z["P"], M=z["M"], fixedp=z["fixedp"])
    a.update(over)
    kx, kk, kptr, kedge = o["plan"]
    return lib.pvo_ba_train(a["poses"], _p(o["disps"]), _p(o["intr"]), _p(o["target"]), _p(o["weight"]), _p(o["eta"]), _p(o["ii"]), _p(o["jj"]),
                            _p(kx), _p(kk), _p(kptr), _p(kedge), z["B"], a["P"], z["N"], a["M"], z["ht"], z["wd"], a["fixedp"],
                            out["poses"].ptr, out["disps"].ptr, out["dx"].ptr, ws.ptr, ws_bytes, dt, stream)


def _backward(lib, o, z, out, ws, ws_bytes, scratch, scratch_bytes, dt, stream, **over):
    a = dict(poses=_p(o["poses"]), P=z["P"], M=z["M"], fixedp=z["fixedp"])
    a.update(over)
    kx, kk, kptr, kedge = o["plan"]
    return lib.pvo_ba_train_vjp(a["poses"], _p(o["disps"]), _p(o["intr"]), _p(o["target"]), _p(o["weight"]), _p(o["ii"]), _p(o["jj"]),
                                _p(kx), _p(kk), _p(kptr), _p(kedge), z["B"], a["P"], z["N"], a["M"], z["ht"], z["wd"], a["fixedp"],
                                _p(o["g_poses_out"]), _p(o["g_disps_out"]), out["g_target"].ptr, out["g_weight"].ptr, out["g_eta"].ptr,
                                out["g_poses"].ptr, out["g_disps"].ptr, ws.ptr, ws_bytes, scratch.ptr, scratch_bytes, dt, stream)


def _outputs(z, dev):
    fwd = {k: _Guarded(z[k], dev) for k in ("poses", "disps", "dx")}
    bwd = {"g_target": _Guarded(z["edge"], dev), "g_weight": _Guarded(z["edge"], dev), "g_eta": _Guarded(z["eta"], dev),
           "g_poses": _Guarded(z["poses"], dev), "g_disps": _Guarded(z["disps"], dev)}
    return fwd, bwd


def _run_c(c, dtype, dev, fill, backwards=1):
    """pvo_ba_train and `backwards` x pvo_ba_train_vjp with workspace and scratch pre-filled with `fill` bytes -> the outputs (of
    every backward) as tensors; asserts the status and every guard"""
    from pvo_amd import _lib, droid_backends as db
    lib, dt, z, o = _lib.load(), db._DT[dtype], _sizes(c, dtype), _operands(c, dtype, dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    nws = lib.pvo_ba_train_workspace_bytes(z["B"], z["P"], z["N"], z["M"], z["ht"] * z["wd"], dt)
    nsc = lib.pvo_ba_train_vjp_scratch_bytes(z["B"], z["P"], z["N"], z["M"], z["ht"] * z["wd"], dt)
    assert nws > 0 and nsc > 0
    ws, scratch = _Guarded(nws, dev, fill), _Guarded(nsc, dev, fill)
    fwd, bwd = _outputs(z, dev)
    with torch.cuda.device(dev):
        assert _forward(lib, o, z, fwd, ws, nws, dt, stream) == 0
        res = {k: g.tensor(dtype, -1) for k, g in fwd.items()}
        state = ws.payload.clone()
        for r in range(backwards):
            if r:
                scratch.payload.fill_(fill)
                for g in bwd.values():
                    g.payload.fill_(0xFF)
            assert _backward(lib, o, z, bwd, ws, nws, scratch, nsc, dt, stream) == 0
            res.update({k + "#%d" % r: g.tensor(dtype, -1) for k, g in bwd.items()})
        torch.cuda.synchronize(dev)
    for name, g in list(fwd.items()) + list(bwd.items()) + [("workspace", ws), ("scratch", scratch)]:
        assert g.guards_intact(), name + ": written beside the buffer"
    assert torch.equal(state, ws.payload), "the backward wrote into the forward's state"
    return res


WS_CASES = [s for s in ONE_STEP if s[0] in ((2, 5, 1, 6, 7, 1), (1, 4, 1, 9, 29, 1), (1, 4, 4, 6, 7, 1), (2, 17, 1, 6, 7, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("shape,cid", WS_CASES, ids=[i for _, i in WS_CASES])
def test_workspace_and_scratch_are_written_before_read_and_nothing_beside_them(cuda, shape, cid, dtype):
    c = _case(shape)
    nan = _run_c(c, dtype, cuda, 0xFF, backwards=2)
    zero = _run_c(c, dtype, cuda, 0x00)
    eps = torch.finfo(dtype).eps
    for k, v in nan.items():
        assert torch.isfinite(v).all(), k + ": read before written (or not written at all)"
    for k in ("poses", "disps", "dx", "g_target#0", "g_weight#0", "g_eta#0"):
        assert torch.equal(nan[k], zero[k]), k
    for k in ("g_target", "g_weight", "g_eta"):                                 # a second backward on the same state
        assert torch.equal(nan[k + "#0"], nan[k + "#1"]), k
    for k in ("g_poses", "g_disps"):                                            # atomics: at most N x chunks <= 128 addends reordered
        scale = float(zero[k + "#0"].abs().max())
        for other in (nan[k + "#0"], nan[k + "#1"]):
            assert float((other - zero[k + "#0"]).abs().max()) <= 128 * eps * scale, k
    # the entry points compute what the wrappers do: the host reference, at the type's accuracy
    tol = 1e-9 if dtype == torch.float64 else 1e-3
    assert float((zero["poses"].double().cpu().view(c.ref["poses"].shape) - c.ref["poses"]).abs().max()) <= tol
    assert float((zero["disps"].double().cpu().view(c.ref["disps"].shape) - c.ref["disps"]).abs().max()) <= tol * 10


REFUSALS = [  # name, expected status, case, what changes
    ("workspace_one_byte_short", 3, (2, 5, 1, 6, 7, 1), {}),
    ("seventeen_free_poses", 4, (2, 17, 1, 6, 7, 1), dict(fixedp=0)),
    ("sixteen_bit_dtype", 4, (2, 5, 1, 6, 7, 1), {}),
    ("null_pointer", 1, (2, 5, 1, 6, 7, 1), dict(poses=None)),
    ("fixedp_above_P", 1, (2, 5, 1, 6, 7, 1), dict(fixedp=6)),
    ("M_above_P", 1, (2, 5, 1, 6, 7, 1), dict(M=6)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,status,shape,over", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_are_answered_before_any_launch(cuda, name, status, shape, over):
    """PVO_EINVAL = 1, PVO_EWORKSPACE = 3, PVO_EUNSUPPORTED = 4 (include/pvo_hip.h), from both entry points, with every output
    still holding its poison afterwards"""
    from pvo_amd import _lib, droid_backends as db
    c = _case(shape)
    dtype = torch.float32
    lib, z, o = _lib.load(), _sizes(c, dtype), _operands(c, dtype, cuda)
    dt = _lib.PVO_F16 if name == "sixteen_bit_dtype" else db._DT[dtype]
    stream = ctypes.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    nws = lib.pvo_ba_train_workspace_bytes(z["B"], z["P"], z["N"], z["M"], z["ht"] * z["wd"], db._DT[dtype])
    nsc = lib.pvo_ba_train_vjp_scratch_bytes(z["B"], z["P"], z["N"], z["M"], z["ht"] * z["wd"], db._DT[dtype])
    ws, scratch = _Guarded(nws, cuda), _Guarded(nsc, cuda)
    fwd, bwd = _outputs(z, cuda)
    short = 1 if name == "workspace_one_byte_short" else 0
    with torch.cuda.device(cuda):
        assert _forward(lib, o, z, fwd, ws, nws - short, dt, stream, **over) == status
        assert _backward(lib, o, z, bwd, ws, nws - short, scratch, nsc, dt, stream, **over) == status
        if short:
            assert _backward(lib, o, z, bwd, ws, nws, scratch, nsc - 1, dt, stream) == status
        torch.cuda.synchronize(cuda)
    for k, g in list(fwd.items()) + list(bwd.items()) + [("workspace", ws), ("scratch", scratch)]:
        assert g.untouched(), k
    if name == "seventeen_free_poses":                                          # 16 are taken: the limit is where the header puts it
        assert _forward(lib, o, z, fwd, ws, nws, dt, stream) == 0
        torch.cuda.synchronize(cuda)
        assert not fwd["poses"].untouched()
