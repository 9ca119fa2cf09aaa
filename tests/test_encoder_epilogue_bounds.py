"""The kernels between the per-frame encoders' convolutions (pvo_amd/csrc/encoder_ops.hip: pvo_bias_norm_act, its sliced form
pvo_bias_norm_act_split, pvo_conv1x1_planes, pvo_frame_normalise) against fp64 / exact references of their own operands, in fp16 and
bf16, on the switching points of their forms, with every buffer between NaN guards.  No element is exempt and no bound is tuned.

THE INSTANCE NORM.  The kernel computes, per plane of HW values,
    t = round16(x + bias[c]);  m = sum(t) / HW;  q = sum((t - m)^2);  r = 1 / sqrtf(q / HW + eps);  out = round16((t - m) r)
in fp32 (EPS = 2^-24 per operation), then ReLU / round16(residual + .) / ReLU.  t is reproduced bit for bit on the CPU (fp32 torch, then
the cast: the same two IEEE roundings), mean mu, biased variance var and y = (t - mu) / sqrt(var + eps) are taken in fp64.  The
normalised value before its rounding may differ from y by delta, derived to first order and doubled for the second-order terms, as
accum() of operator_bounds_util.py doubles:
  m      any summation tree of depth D errs by at most D EPS sum|t|; the division by HW adds EPS |m| <= EPS mean|t|:
         |m - mu| <= (D + 1) EPS mean|t|.  In y this is divided by sqrt(var + eps):                 (D + 1) EPS mean|t| / sqrt(var + eps)
  t - m  one rounding:                                                                              1 EPS |y|
  q / HW each term (t - m)^2 carries the subtraction's rounding twice and the product's once (3), the tree D, the division 1 - the
         D + 4 of the formula -, and the shift of m moves q by HW (m - mu)^2 only, second order.  The square root halves a relative
         error:                                                                                      (D + 4) / 2 EPS |y|
  + eps  one rounding of q / HW + eps, halved:                                                       0.5 EPS |y|
  r      sqrtf and the reciprocal, taken at 2 EPS each (both are correctly rounded in this build; 2 is the issue's allowance):  4 EPS |y|
  (.) r  the final product:                                                                          1 EPS |y|
                                          delta = 2 [ (D + 1) EPS mean|t| / sqrt(var + eps) + |y| ((D + 4) / 2 + 7) EPS ]     (6.5 <= 7)
(On planes smaller than D the tree term is what it can be at most, min(D, HW - 1) roundings, and at HW = 1 the division is exact: there
delta = 0, as t - t / 1 is 0 in fp32 - the plain formula would leave every element of a one-pixel plane two-valued, against the cap below.)
D is a declared contract, D = ceil(HW / threads) + 22 with threads = 1024 / 512 / 256 for HW >= 16384 / >= 2048 / below.  The
one-workgroup kernel: a thread's chain of n = ceil(HW / threads) terms is n - 1 roundings (even planes: the pair's sum and the add, n / 2
times), the wave tree 4 + 2, the up to 16 waves' partial sums in order 15: n + 20 <= D.  The split form, S = 4 (16) slices of L =
ceil(HW / S) values on 256 threads: a slice's chain ceil(L / 256) - 1, its tree 6, its four waves 3, and one addition to the running
statistic per combination step, S: ceil(HW / 1024) + 8 + 4 for S = 4 (threads = 512: D = ceil(HW / 512) + 22, more) and ceil(HW / 4096) +
8 + 16 for S = 16 (D = ceil(HW / 1024) + 22, more): the additions stay under the same D.
A FINDING OF THAT ARITHMETIC: Chan's step also rounds mk - mean, nk / tot and their product (3 EPS |mk - mean| nk / tot), and in the
worst case - the whole mass of |t| in the first slice - these add 3 (1 + H_15) = 13 EPS mean|t| at S = 16: the strict first-order count of
the split form's mean is then ceil(HW / 4096) + 38 against D + 1 = ceil(HW / 1024) + 23, more than the undoubled allowance for 16384 <= HW <
22100 (42 against 39 at HW = 16384; the |y| term likewise 33 against 28), and it is the doubling that covers it there.  The second-order
terms the doubling is for are of the order D^2 EPS^2 = 1e-11, so nothing is lost; the measured error is a few percent of delta.

THE CHECK.  lo = round16(y - delta), hi = round16(y + delta); rounding, ReLU and round16(residual + .) are monotone non-decreasing, so
f(lo) <= out <= f(hi) element by element, f = the rest of the chain in fp32 torch on the CPU; where f(lo) == f(hi) that is bit for bit;
NaN fails.  So that the interval cannot hide a failure, on the standard operands (x = 2 randn + 0.3, bias = randn) at least 85 % of the
elements must have lo == hi (the share is printed; a CPU emulation gave at most 9.4 % two-valued in fp16, 1.6 % in bf16).  With mean / std
= 20 the share of two-valued elements rises (71 % in fp16 at HW = 48480), so that case is interval-only.

WHAT THE SUITE CANNOT DISTINGUISH.  A one-pass variance E[t^2] - E[t]^2 in fp32 passes the interval at mean / std = 20 at two of the CPU
tests' three sizes in fp16 (its cancellation error, about mean^2 / var = 400 roundings, is of the order of the allowance there; the count is
printed): the standard, near-constant and mean / std = 20 operands do not reliably tell it from the two-pass kernel.  At mean / std of about 900 (fp16 integers 1000 .. 1003) the bound does reject it, and
test_interval_rejects_a_one_pass_variance_far_from_zero holds that; the GPU tests run the same operands on the kernel.
Not run: the wrapper's fall-back to the one-workgroup kernel for more than 65535 planes of HW >= 8192 (gigabytes).

The GPU tests carry the gpu mark one by one: the module also holds the CPU tests which prove that the interval check fails on a faithful
fp32 stand-in of the kernel once its variance is divided by HW - 1, an odd plane's last element or a short slice's tail is left out of the
statistics, the bias comes from the next channel, eps is omitted or the outer ReLU is applied before the residual add."""
import ctypes

import pytest
import torch

import encoder_bounds_util as E
import operator_bounds_util as B

gpu = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
_CODE = {torch.float16: 1, torch.bfloat16: 2}
# HW around every switch: 1 / 2 (degenerate, scalar / paired), 63 .. 65 (one wave), 2047 / 2048 (256 -> 512 threads), 8190 .. 8193 (the split
# form starts: 4 slices, 8193 with a shorter last one), 16383 .. 16385 (512 -> 1024 threads, 4 -> 16 slices); odd and even everywhere
SWITCH_HW = [1, 2, 63, 64, 65, 2047, 2048, 8190, 8192, 8193, 16383, 16384, 16385]
PRODUCT = [(2, 32, 120, 404), (1, 64, 60, 202), (3, 128, 30, 101), (2, 16, 7, 9)]
SHAPES = [(2, 3, 1, hw) for hw in SWITCH_HW] + PRODUCT
# (norm, residual, relu_inner, relu_outer, bias): a block's first layer / the stem, its shortcut, its second layer, in the instance-norm and the
# norm-free encoder (extractor.py forward_inference), and the shortcut's norm behind pvo_conv1x1_planes, which has no bias left
COMBOS = [(True, False, True, False, True), (True, False, False, False, True), (True, True, True, True, True), (True, False, False, False, False),
          (False, False, True, False, True), (False, False, False, False, True), (False, True, True, True, True)]
CPU_HW = [63, 2047, 8193]


def _id(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return None


def _seed(*v):
    s = 29
    for x in v:
        s = (s * 1000003 + int(x)) % (2 ** 31)
    return torch.Generator().manual_seed(s)


def _operands(shape, dtype, kind="standard"):
    """(x, bias, residual) on the CPU.  standard: x = 2 randn + 0.3, bias = randn; far: mean / std near 20; constant: two adjacent 16-bit
    values (8 and 8 + 2^-7 in fp16, 1 and 1 + 2^-7 in bf16: variance 2^-16 = 1.5e-5, of the order of eps = 1e-5) and no bias;
    integers: 1000 .. 1003 (fp16 only), mean / std near 900, no bias"""
    g = _seed(*shape, _CODE[dtype], len(kind))
    N, C, H, W = shape
    r = torch.randn(shape, generator=g).to(dtype)
    if kind == "standard":
        return (torch.randn(shape, generator=g) * 2.0 + 0.3).to(dtype), torch.randn(C, generator=g).to(dtype), r
    if kind == "far":
        return (torch.randn(shape, generator=g) * 2.0 + 40.0).to(dtype), torch.randn(C, generator=g).to(dtype), r
    if kind == "constant":
        base = 8.0 if dtype == torch.float16 else 1.0
        x = (base + torch.randint(0, 2, shape, generator=g).double() * 2.0 ** -7).to(dtype)
        assert bool((x.double() - base).abs().max() == 2.0 ** -7)
        return x, None, r
    assert kind == "integers" and dtype == torch.float16
    return (1000.0 + torch.randint(0, 4, shape, generator=g)).to(dtype), None, r


# ------------------------------------------------------------------------------------------------ CPU: the check can fail
def _standin_forms(HW):
    return [False, True] if E.slices_of(HW) else [False]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("HW", CPU_HW)
def test_standin_is_inside_the_interval(HW, dtype):
    """the fp32 stand-in in the kernels' order of operations, both forms: inside the interval on the standard operands, the near-constant
    plane and mean / std = 20, its error before the rounding under delta, and the standard operands under the two-valued cap"""
    shape = (2, 3, 1, HW)
    for kind in ("standard", "constant", "far"):
        x, b, r = _operands(shape, dtype, kind)
        stats = E.norm_interval(E.biased(x, b))
        for split in _standin_forms(HW):
            what = "stand-in %s HW=%d split=%s %s" % (kind, HW, split, _id(dtype))
            ratio = float(((E.standin_bias_norm_act(x, b, split=split, return_normalised=True).double() - stats[2]).abs() / stats[3]).max())
            print("%s: max err / delta before the rounding = %.3g" % (what, ratio))
            assert ratio < 1.0
            for norm, res, ri, ro, _ in COMBOS[:3]:
                flo, fhi, share = E.epilogue_interval(x, b, r if res else None, True, ri, ro, stats=stats)
                E.assert_inside(E.standin_bias_norm_act(x, b, r if res else None, relu_inner=ri, relu_outer=ro, split=split), flo, fhi, what)
        if kind == "standard":
            print("stand-in HW=%d %s: two-valued share %.4f" % (HW, _id(dtype), share))
            assert share <= 0.15


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("mutation", E.MUTATIONS)
def test_interval_rejects_every_mutation(mutation, dtype):
    """each mutant of the stand-in raises at one or more of HW = 63, 2047, 8193 (the sizes that reject it are printed)"""
    kind = "constant" if mutation == "eps_omitted" else "standard"
    rejected = []
    for HW in CPU_HW:
        x, b, r = _operands((2, 3, 1, HW), dtype, kind)
        for split in ([True] if mutation == "short_slice_tail_skipped" else _standin_forms(HW)):
            if split and not E.slices_of(HW):
                continue
            flo, fhi, _ = E.epilogue_interval(x, b, r, True, True, True)
            E.assert_inside(E.standin_bias_norm_act(x, b, r, relu_inner=True, relu_outer=True, split=split), flo, fhi, "clean")
            try:
                E.assert_inside(E.standin_bias_norm_act(x, b, r, relu_inner=True, relu_outer=True, split=split, mutation=mutation), flo, fhi, mutation)
            except AssertionError as e:
                assert "outside the interval" in str(e)
                rejected.append((HW, split))
    print("%s %s: rejected at (HW, split) = %s" % (mutation, _id(dtype), rejected))
    assert rejected, "the interval accepts %s at every size" % mutation


def test_interval_rejects_a_one_pass_variance_far_from_zero():
    """E[t^2] - E[t]^2 in fp32: accepted at mean / std = 20 (the known gap: module docstring), rejected on fp16 integers 1000 .. 1003, where
    the squares (1e6) leave fp32's exact integers after sixteen of them; the two-pass stand-in passes on the same operands"""
    dtype = torch.float16
    accepted_at_20 = 0
    for HW in CPU_HW:
        x, b, _ = _operands((2, 3, 1, HW), dtype, "far")
        flo, fhi, _ = E.epilogue_interval(x, b, None, True, False, False)
        try:
            E.assert_inside(E.standin_bias_norm_act(x, b, one_pass=True), flo, fhi, "one pass, mean / std = 20, HW=%d" % HW)
            accepted_at_20 += 1
        except AssertionError:
            pass
    print("one-pass variance at mean / std = 20: accepted at %d of %d sizes" % (accepted_at_20, len(CPU_HW)))
    rejected = 0
    for HW in CPU_HW:
        x, b, _ = _operands((2, 3, 1, HW), dtype, "integers")
        flo, fhi, _ = E.epilogue_interval(x, b, None, True, False, False)
        E.assert_inside(E.standin_bias_norm_act(x, b), flo, fhi, "two pass, integers, HW=%d" % HW)
        try:
            E.assert_inside(E.standin_bias_norm_act(x, b, one_pass=True), flo, fhi, "one pass, integers, HW=%d" % HW)
        except AssertionError:
            rejected += 1
    assert rejected >= 1


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_conv1x1_bound_rejects_a_dropped_product_and_exact_check_a_swapped_channel(dtype):
    """the two checks of pvo_conv1x1_planes on an fp32 CPU convolution rounded twice: clean passes; one product missing from every output of
    the last pixel is over the bound; two input channels exchanged differ in bits on integers"""
    g = _seed(7, _CODE[dtype])
    x, w, b = torch.randn(1, 128, 7, 9, generator=g).to(dtype), (torch.randn(64, 128, generator=g) * 0.1).to(dtype), torch.randn(64, generator=g).to(dtype)

    def standin(x, w, b, drop=False):
        acc = torch.einsum("oc,nchw->nohw", w.float(), x.float())
        if drop:
            acc[:, :, -1, -1] -= w.float()[None, :, 5] * x.float()[:, None, 5, -1, -1]
        return (acc.to(dtype).float() + b.float().view(1, -1, 1, 1)).to(dtype)
    ref, bound = E.conv1x1_bound(*E.conv1x1_ref(x, w, b, 1), 128, dtype)
    assert B.assert_within(standin(x, w, b), ref, bound, "clean %s" % _id(dtype)) < 1.0
    with pytest.raises(AssertionError, match="over the bound"):
        B.assert_within(standin(x, w, b, drop=True), ref, bound, "dropped product %s" % _id(dtype))
    x, w, b = B.int_tensor(g, (1, 128, 7, 9), -3, 3, dtype), B.int_tensor(g, (64, 128), -2, 2, dtype), B.int_tensor(g, (64,), -4, 4, dtype)
    want = _conv1x1_exact(x, w, b, 1, dtype)
    B.assert_bits(standin(x, w, b), want, "clean integers")
    xs = x.clone()
    xs[:, 3], xs[:, 4] = x[:, 4], x[:, 3]
    with pytest.raises(AssertionError, match="elements differ"):
        B.assert_bits(standin(xs, w, b), want, "swapped channels")


# ------------------------------------------------------------------------------------------------ GPU plumbing
def call(name, *args):
    """the C entry point `name` on the current stream with tensors passed as their pointers"""
    from pvo_amd import _lib
    conv = [ctypes.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args]
    rc = getattr(_lib.load(), name)(*conv, None)
    assert rc == 0, (name, rc)


def _guarded_out(shape, dtype, dev):
    return B.Guarded(int(torch.Size(shape).numel()), dtype, dev, 4096)


def _check_out(g, what):
    torch.cuda.synchronize()
    assert g.guards_untouched(), "%s: written outside the output" % what
    assert not bool(torch.isnan(g.inner).any()), "%s: unwritten or NaN outputs" % what


def run_bna(dev, x, bias, residual, norm, ri, ro, form, what, in_place=False):
    """bias_norm_act on guarded device copies of the CPU operands -> the output on the CPU.  form: None = the wrapper's choice (the
    split form from HW = 8192 on), False = the one-workgroup kernel, "direct" = pvo_bias_norm_act_split itself with `ws` between guards."""
    from pvo_amd import droid_backends as db
    N, C, H, W = x.shape
    gx = B.guarded_copy(x.to(dev), 4096)
    gr = None if residual is None else B.guarded_copy(residual.to(dev), 4096)
    gb = None if bias is None else B.guarded_copy(bias.to(dev), 4096)
    go = None if in_place else _guarded_out(x.shape, x.dtype, dev)
    out = gx if in_place else go.view(*x.shape)
    if form == "direct":
        S = E.slices_of(H * W)
        ws = B.Guarded(2 * N * C * S, torch.float32, dev, 4096)
        call("pvo_bias_norm_act_split", gx, gb, gr, out, N * C, C, H * W, 1 if norm else 0, E.EPS_NORM, 1 if ri else 0, 1 if ro else 0, _CODE[x.dtype],
             ws.inner if norm else None, ws.numel if norm else 0)
        torch.cuda.synchronize()
        assert ws.guards_untouched(), "%s: written outside the workspace" % what
        assert not norm or not bool(torch.isnan(ws.inner).any()), "%s: a slice left no statistics" % what
    else:
        y = db.bias_norm_act(gx, gb, gr, norm=norm, relu_inner=ri, relu_outer=ro, out=out, split=form)
        assert y.data_ptr() == out.data_ptr()
    if go is not None:
        _check_out(go, what)
        assert bool(torch.equal(gx.cpu(), x)), "%s: x changed" % what
    torch.cuda.synchronize()
    if gr is not None:
        assert bool(torch.equal(gr.cpu(), residual)), "%s: the residual changed" % what
    return out.cpu()


def _forms(HW):
    return [None, False, "direct"] if E.slices_of(HW) else [None]


def check_bna_case(dev, shape, dtype, kind, combos, cap):
    """every combination and form of one operand set against the interval; prints the two-valued share and the least error / delta"""
    x, b, r = _operands(shape, dtype, kind)
    HW = shape[2] * shape[3]
    stats = {True: E.norm_interval(E.biased(x, b)), False: E.norm_interval(E.biased(x, None))}
    for norm, res, ri, ro, with_bias in combos:
        bias = b if with_bias else None
        st = stats[bias is not None]
        flo, fhi, share = E.epilogue_interval(x, bias, r if res else None, norm, ri, ro, stats=st)
        for form in _forms(HW):
            what = "bias_norm_act %s %s %s norm=%d res=%d relu=%d%d bias=%d form=%s" % (kind, _id(shape), _id(dtype), norm, res, ri, ro, bias is not None, form)
            got = run_bna(dev, x, bias, r if res else None, norm, ri, ro, form, what)
            E.assert_inside(got, flo, fhi, what)
            if norm and not (res or ri or ro):
                print("%s: two-valued share %.4f, least err / delta %.3g" % (what, share, E.least_error(got, st[2], st[3])))
        if norm and cap:
            assert share <= 0.15, "%s: %.1f %% of the elements have lo != hi" % (_id(shape), 100 * share)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_bias_norm_act_interval_every_shape_and_form(cuda, shape, dtype):
    """standard operands, every combination the encoders use plus the norm without bias, every form the size has (HW >= 8192: the wrapper's
    split form, the one-workgroup kernel, and pvo_bias_norm_act_split called directly with its workspace between guards): each inside the
    interval, at least 85 % of the elements bit for bit; x, residual, out between NaN guards"""
    check_bna_case(cuda, shape, dtype, "standard", COMBOS, cap=True)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("HW", [2, 63, 2048, 8193, 16384, 48480])
@pytest.mark.parametrize("kind", ["constant", "far"])
def test_bias_norm_act_interval_near_constant_and_far_planes(cuda, kind, HW, dtype):
    """constant: two adjacent 16-bit values, variance 1.5e-5 against eps = 1e-5 - a kernel without eps is 29 % off; far: mean / std = 20
    (interval only, no cap on the two-valued share: module docstring)"""
    check_bna_case(cuda, (2, 3, 1, HW), dtype, kind, COMBOS[1:3], cap=False)


@gpu
def test_bias_norm_act_interval_integers_far_from_zero(cuda):
    """fp16 integers 1000 .. 1003 (mean / std = 900): the operands on which the interval rejects a one-pass variance"""
    for HW in CPU_HW + [16384]:
        check_bna_case(cuda, (2, 3, 1, HW), torch.float16, "integers", COMBOS[3:4], cap=False)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("HW", [63, 64, 2048, 8193, 16384])
def test_bias_norm_act_in_place_equals_out_of_place(cuda, HW, dtype):
    """out = x: the same bits as out of place, in every form (the statistics are finished before the first element is overwritten)"""
    x, b, r = _operands((2, 3, 1, HW), dtype, "standard")
    for norm, res, ri, ro, _ in COMBOS[2:3] + COMBOS[5:6]:
        for form in _forms(HW):
            what = "in place HW=%d %s norm=%d form=%s" % (HW, _id(dtype), norm, form)
            want = run_bna(cuda, x, b, r if res else None, norm, ri, ro, form, what)
            B.assert_bits(run_bna(cuda, x, b, r if res else None, norm, ri, ro, form, what, in_place=True), want, what)


# ------------------------------------------------------------------------------------------------ pvo_conv1x1_planes
def _conv1x1_exact(x, w, b, stride, dtype):
    """the bits on integer operands: the sum is exact in fp32 and rounded to storage, the bias added exactly and the sum rounded again -
    exact_want once per rounding of the kernel (bf16 keeps integers up to 256 only, so the first rounding does act)"""
    ref0, A0, bd = E.conv1x1_ref(x, w, b, stride)
    v = B.exact_want(ref0, A0, dtype)
    return B.exact_want(v.double() + bd, A0 + bd.abs(), dtype)


def run_conv1x1(dev, x, w, b, stride, what):
    """pvo_conv1x1_planes with x, w, bias and the output between NaN guards -> the output on the CPU; the wrapper gives the same bits"""
    from pvo_amd import droid_backends as db
    N, Cin, H, W = x.shape
    Cout = w.shape[0]
    gx, gw = B.guarded_copy(x.to(dev), 4096), B.guarded_copy(w.to(dev), 4096)
    gb = None if b is None else B.guarded_copy(b.to(dev), 4096)
    shape = (N, Cout, (H - 1) // stride + 1, (W - 1) // stride + 1)
    go = _guarded_out(shape, x.dtype, dev)
    call("pvo_conv1x1_planes", gx, gw, gb, go.inner, N, Cin, Cout, H, W, stride, _CODE[x.dtype])
    _check_out(go, what)
    y = db.conv1x1_planes(gx, gw, gb, stride=stride)
    assert tuple(y.shape) == shape, (what, tuple(y.shape), shape)
    B.assert_bits(y, go.view(*shape), what + ": wrapper against the entry point")
    return y.cpu()


# N x (H, W) x stride: HW = 1, 63, 64, 65 around the 64-pixel tile, the smallest and the 1/8-resolution product map; stride 2 on odd and even
# heights and widths ((H - 1) // 2 + 1 rows / columns) and on one pixel
CONV_MAPS = [(1, (1, 1), 1), (3, (7, 9), 1), (1, (8, 8), 1), (3, (5, 13), 1), (1, (30, 101), 1),
             (3, (7, 9), 2), (1, (8, 9), 2), (1, (7, 10), 2), (3, (1, 1), 2)]


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("Cout", [64, 128, 256])
@pytest.mark.parametrize("Cin", [32, 64, 128])
def test_conv1x1_planes_bound_and_exact(cuda, Cin, Cout, dtype):
    """y = round16(round16(acc) + bias), K = Cin products added in fp32: the two roundings bounded as encoder_bounds_util.conv1x1_bound
    derives (linear_bound for the first, stored() for the 16-bit add and the second); on integers (x in [-3, 3], w in [-2, 2], bias in
    [-4, 4]: A <= 6 x 128 + 4) the exact bits; bias = None equals a zero bias; every map of CONV_MAPS"""
    for N, (H, W), stride in CONV_MAPS:
        g = _seed(N, H, W, stride, Cin, Cout, _CODE[dtype])
        what = "conv1x1_planes %d->%d N=%d %dx%d stride %d %s" % (Cin, Cout, N, H, W, stride, _id(dtype))
        x, w, b = torch.randn(N, Cin, H, W, generator=g).to(dtype), (torch.randn(Cout, Cin, generator=g) * 0.1).to(dtype), torch.randn(Cout, generator=g).to(dtype)
        ref, bound = E.conv1x1_bound(*E.conv1x1_ref(x, w, b, stride), Cin, dtype)
        B.assert_within(run_conv1x1(cuda, x, w, b, stride, what), ref, bound, what)
        none = run_conv1x1(cuda, x, w, None, stride, what + " no bias")
        ref, bound = E.conv1x1_bound(*E.conv1x1_ref(x, w, None, stride), Cin, dtype)
        B.assert_within(none, ref, bound, what + " no bias")
        B.assert_bits(run_conv1x1(cuda, x, w, torch.zeros_like(b), stride, what + " zero bias"), none, what + " zero bias against none")
        x, w, b = B.int_tensor(g, (N, Cin, H, W), -3, 3, dtype), B.int_tensor(g, (Cout, Cin), -2, 2, dtype), B.int_tensor(g, (Cout,), -4, 4, dtype)
        B.assert_bits(run_conv1x1(cuda, x, w, b, stride, what + " exact"), _conv1x1_exact(x, w, b, stride, dtype), what + " exact")


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("Cin,Cout", [(32, 64), (64, 128), (128, 256), (128, 64)])
def test_conv1x1_planes_permutation_filter_selects_planes(cuda, Cin, Cout, dtype):
    """w = a 0 / 1 matrix with one 1 per output channel: the output is the selected input plane (every s-th row and column of it) bit for
    bit - channel order, the tile's pixel order and the stride's gather, element by element"""
    for N, (H, W), stride in CONV_MAPS:
        g = _seed(N, H, W, stride, Cin, Cout, 5)
        sel = torch.cat([torch.randperm(Cin, generator=g) for _ in range(-(-Cout // Cin))])[:Cout]
        w = torch.zeros(Cout, Cin, dtype=dtype)
        w[torch.arange(Cout), sel] = 1.0
        x = torch.randn(N, Cin, H, W, generator=g).to(dtype)
        what = "permutation %d->%d N=%d %dx%d stride %d %s" % (Cin, Cout, N, H, W, stride, _id(dtype))
        B.assert_bits(run_conv1x1(cuda, x, w, None, stride, what), x[:, sel, ::stride, ::stride].contiguous(), what)


# ------------------------------------------------------------------------------------------------ pvo_frame_normalise
_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
_KIND = {torch.int32: 0, torch.uint8: 1, torch.float32: 2}


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("in_dtype", [torch.int32, torch.uint8, torch.float32], ids=_id)
@pytest.mark.parametrize("size", [(1, 1), (1, 255), (1, 256), (1, 257), (37, 53)], ids=_id)
def test_frame_normalise_bits(cuda, size, in_dtype, dtype):
    """bit for bit the fp32 element-wise sequence on the CPU - flip BGR -> RGB, / 255, - mean, / std, cast - (every step one IEEE
    operation on both sides), around the 256-thread block, with the values 0 and 255 in every channel or (one pixel) spread over
    the channels, fractional values for float32 frames; the output between NaN guards"""
    from pvo_amd import droid_backends as db
    H, W = size
    g = _seed(H, W, _KIND[in_dtype], _CODE[dtype])
    if in_dtype == torch.float32:
        img = torch.rand(3, H, W, generator=g) * 255.0
    else:
        img = torch.randint(0, 256, (3, H, W), generator=g).to(in_dtype)
    flat = img.view(3, -1)
    if H * W == 1:
        flat[0, 0], flat[1, 0] = 0, 255
    else:
        flat[:, 0], flat[:, -1] = 0, 255
    assert float(img.min()) == 0 and float(img.max()) == 255
    mean, std = torch.tensor(_MEAN)[:, None, None], torch.tensor(_STD)[:, None, None]
    want = (((img.flip(0)[None].float() / 255.0) - mean) / std).to(dtype)
    what = "frame_normalise %s %s -> %s" % (_id(size), _id(in_dtype), _id(dtype))
    dimg = img.to(cuda)
    go = _guarded_out((1, 3, H, W), dtype, cuda)
    m, s = (ctypes.c_float * 3)(*_MEAN), (ctypes.c_float * 3)(*_STD)
    call("pvo_frame_normalise", dimg, go.inner, H, W, m, s, _KIND[in_dtype], _CODE[dtype])
    _check_out(go, what)
    B.assert_bits(go.view(1, 3, H, W).cpu(), want, what)
    B.assert_bits(db.frame_normalise(dimg, _MEAN, _STD, dtype).cpu(), want, what + " (wrapper)")
