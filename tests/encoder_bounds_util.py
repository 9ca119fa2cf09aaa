"""Helpers of tests/test_encoder_epilogue_bounds.py: the fp64 reference of the encoder epilogue (bias, instance norm, ReLU, residual
add), the interval a correct kernel's output must lie in, the double-rounding bound of the 1 x 1 convolution, and an fp32 CPU stand-in
of the epilogue kernel with the mutations that prove the interval check can fail.

Vocabulary beyond operator_bounds_util.py (all tensors on the CPU):
  t        round16(fp32(x) + fp32(bias[c])): what the kernel normalises, bit-identical to it by IEEE arithmetic
  y        (t - mean) / sqrt(var + eps) in fp64, mean and biased variance of t over the plane in fp64
  D        the longest chain of fp32 additions the statistics may use (depth(): a declared contract, not a measurement)
  delta    the allowance on the normalised value BEFORE it is rounded to storage
  lo, hi   round16(y - delta), round16(y + delta): rounding is monotone, so a correct kernel's normalised value is one of the 16-bit
           values in [lo, hi]; for most elements lo == hi and the demand is bit for bit"""
import numpy as np
import torch

from operator_bounds_util import EPS, linear_bound, stored

EPS_NORM = float(np.float32(1e-5))          # InstanceNorm2d's eps as the fp32 value the wrapper hands to the kernel


def threads_of(HW):
    """threads of the one-workgroup kernel (pvo_bias_norm_act)"""
    return 1024 if HW >= 16384 else (512 if HW >= 2048 else 256)


def slices_of(HW):
    """slices per plane of the split form (pvo_bias_norm_act_slices); 0: the plane keeps the one-workgroup kernel"""
    return 16 if HW >= 16384 else (4 if HW >= 8192 else 0)


def depth(HW):
    """D = ceil(HW / threads) + 22, the declared depth of the statistics' summation (test module docstring)"""
    return -(-HW // threads_of(HW)) + 22


# ------------------------------------------------------------------------------------------------ reference and interval
def biased(x, bias):
    """t = round16(fp32(x) + fp32(bias[c])): the sum of two 16-bit values is rounded to fp32 and then to storage by torch exactly as
    by the kernel"""
    t = x.float()
    if bias is not None:
        t = t + bias.float().view(1, -1, 1, 1)
    return t.to(x.dtype)


def norm_interval(t, eps=EPS_NORM):
    """(lo, hi, y, delta) of the instance norm of t [N,C,H,W] (16-bit): lo / hi in t's dtype, y / delta fp64.
    delta = 2 [ (D + 1) EPS mean|t| / sqrt(var + eps) + |y| ((D + 4) / 2 + 7) EPS ]  (derived in the test module's docstring), with two
    terms that vanish on tiny planes taken as what they are: a sum of HW terms has HW - 1 roundings in any tree, so D counts as
    min(D, HW - 1), and the division by HW = 1 is exact, so the + 1 beside D is dropped there.  (Never a wider interval; at HW = 1 it
    makes delta = 0, as it must be: t - t / 1 is exactly 0 in fp32, whereas the plain formula leaves every element two-valued.)"""
    N, C, H, W = t.shape
    HW = H * W
    td = t.double().reshape(N, C, HW)
    mean = td.mean(2, keepdim=True)
    var = ((td - mean) ** 2).mean(2, keepdim=True)
    s = (var + eps).sqrt()
    y = (td - mean) / s
    D, div = min(depth(HW), HW - 1), (0 if HW == 1 else 1)
    delta = 2.0 * ((D + div) * EPS * td.abs().mean(2, keepdim=True) / s + y.abs() * ((D + 4) / 2.0 + 7.0) * EPS)
    lo, hi = (y - delta).to(t.dtype), (y + delta).to(t.dtype)
    return lo.view(t.shape), hi.view(t.shape), y.view(t.shape), delta.view(t.shape)


def finish(v, residual, relu_inner, relu_outer):
    """the rest of the chain behind the (normalised) 16-bit value v, as fp32 torch on the CPU does it: relu_inner, round16(residual + .),
    relu_outer.  Monotone non-decreasing in v for a fixed residual."""
    t = v.float()
    if relu_inner:
        t = torch.relu(t)
    if residual is not None:
        t = (residual.float() + t).to(v.dtype).float()
    if relu_outer:
        t = torch.relu(t)
    return t.to(v.dtype)


def epilogue_interval(x, bias, residual, norm, relu_inner, relu_outer, eps=EPS_NORM, stats=None):
    """(f(lo), f(hi), share of elements with lo != hi) of bias_norm_act on the CPU; stats = norm_interval(biased(x, bias), eps) if the
    caller has it already.  Without normalisation lo == hi == t: the check is bit for bit."""
    if norm:
        lo, hi = (stats if stats is not None else norm_interval(biased(x, bias), eps))[:2]
    else:
        lo = hi = biased(x, bias)
    share = float((lo != hi).double().mean()) if lo.numel() else 0.0
    return finish(lo, residual, relu_inner, relu_outer), finish(hi, residual, relu_inner, relu_outer), share


def assert_inside(got, flo, fhi, what):
    """f(lo) <= got <= f(hi) element by element (bit for bit where the two coincide, +0 and -0 being one value); NaN fails"""
    assert got.shape == flo.shape and got.dtype == flo.dtype, (what, tuple(got.shape), tuple(flo.shape), got.dtype, flo.dtype)
    g, a, b = got.double(), flo.double(), fhi.double()
    bad = ~((a <= g) & (g <= b))
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements outside the interval (%d of them where it is one value); first at %s: got %r, interval [%r, %r]"
                             % (what, int(bad.sum()), bad.numel(), int((bad & (a == b)).sum()), i, float(g[i]), float(a[i]), float(b[i])))


def spacing(v, dtype):
    """the distance from |v| to the next 16-bit value above it (fp64 tensor of 16-bit values)"""
    mant, emin = {torch.float16: (10, -24), torch.bfloat16: (7, -133)}[dtype]
    e = torch.frexp(v.abs().clamp_min(2.0 ** -140))[1].double()            # |v| = m 2^e, m in [0.5, 1)
    return torch.exp2((e - 1 - mant).clamp_min(emin))


def least_error(got, y, delta):
    """max over the elements of (the least |normalised value - y| that is consistent with the rounded output) / delta: 0 where got is
    the rounding of y itself, else the distance from y to the edge of got's rounding interval.  A measurement for the record (the
    kernel's value before its rounding cannot be observed), not a threshold."""
    g = got.double()
    least = ((g - y).abs() - 0.5 * spacing(g, got.dtype)).clamp_min(0.0)
    return float((least / delta).max()) if g.numel() else 0.0


# ------------------------------------------------------------------------------------------------ the 1 x 1 convolution
def conv1x1_ref(x, w, bias, stride):
    """(ref0, A0) of the bias-free strided 1 x 1 convolution in fp64, and the bias as fp64 [1,Cout,1,1] (zero without one)"""
    xd = x.double()[:, :, ::stride, ::stride]
    wd = w.double().reshape(w.shape[0], -1)
    ref0 = torch.einsum("oc,nchw->nohw", wd, xd)
    A0 = torch.einsum("oc,nchw->nohw", wd.abs(), xd.abs())
    b = torch.zeros(1, w.shape[0], 1, 1, dtype=torch.float64) if bias is None else bias.double().view(1, -1, 1, 1)
    return ref0, A0, b


def conv1x1_bound(ref0, A0, b, K, dtype):
    """(ref, bound) of y = round16(fl32(round16(acc) + bias)), acc = K products added in fp32:
      v = round16(acc):      |v - ref0| <= b1 = u |ref0| + 2 K EPS A0 + FLOOR                              (linear_bound)
      z = fl32(v + bias):    two 16-bit values; their sum is rounded once to fp32: |z - (v + bias)| <= EPS |v + bias|, so with
                             ref = ref0 + bias: |z - ref| <= err = b1 + EPS (|ref| + b1)
      y = round16(z):        |y - ref| <= err + u (|ref| + err) + FLOOR                                    (stored)"""
    _, b1 = linear_bound(ref0, A0, K, dtype)
    ref = ref0 + b
    err = b1 + EPS * (ref.abs() + b1)
    return ref, stored(ref, err, dtype)


# ------------------------------------------------------------------------------------------------ CPU stand-in and its mutations
MUTATIONS = ("variance_over_hw_minus_1", "last_element_of_odd_plane_skipped", "bias_of_next_channel", "short_slice_tail_skipped",
             "eps_omitted", "relu_outer_before_residual")
f32 = np.float32


def _workgroup_sum(v, threads, pairs=False):
    """fp32 sum of v [P, n] as a workgroup of `threads` adds it: per-thread partial sums over a stride of `threads` (two adjacent values
    first where `pairs`), the 64-lane tree of pvo_wave_sum (xor 1, xor 2, half-row mirror, row mirror, (r0 + r1) + (r2 + r3)), then
    the waves' partial sums in index order.  Returns [P] float32."""
    v = np.asarray(v, dtype=f32)
    P = v.shape[0]
    if pairs:
        v = (v[:, 0::2] + v[:, 1::2]).astype(f32)
    n = v.shape[1]
    rows = max(-(-n // threads), 1)
    pad = np.zeros((P, rows * threads), dtype=f32)
    pad[:, :n] = v
    pad = pad.reshape(P, rows, threads)
    s = np.zeros((P, threads), dtype=f32)
    for r in range(rows):
        s = (s + pad[:, r]).astype(f32)
    lane = np.arange(threads)
    for partner in (lane ^ 1, lane ^ 2, lane ^ 7, lane ^ 15):
        s = (s + s[:, partner]).astype(f32)
    w = s.reshape(P, threads // 64, 64)
    red = ((w[:, :, 0] + w[:, :, 16]).astype(f32) + (w[:, :, 32] + w[:, :, 48]).astype(f32)).astype(f32)
    tot = np.zeros(P, dtype=f32)
    for k in range(red.shape[1]):
        tot = (tot + red[:, k]).astype(f32)
    return tot


def _two_pass(t, threads, pairs, n_used=None):
    """(mean, sum of squared deviations about it) of t [P, n] in fp32, two passes; n_used: only the first n_used values enter the sums"""
    n = t.shape[1]
    u = t if n_used is None else t[:, :n_used]
    mean = (_workgroup_sum(u, threads, pairs) / f32(n)).astype(f32)
    d = (u - mean[:, None]).astype(f32)
    return mean, _workgroup_sum((d * d).astype(f32), threads, pairs)


def standin_bias_norm_act(x, bias=None, residual=None, eps=EPS_NORM, relu_inner=False, relu_outer=False, split=False, mutation=None,
                          one_pass=False, return_normalised=False):
    """bias_norm_act(norm=True) in fp32 numpy in the kernels' own order of operations - what a correct kernel computes -, one workgroup
    per plane (split=False) or in slices with Chan's combination (split=True: pvo_bias_norm_act_split), or one of six ways it goes wrong:
      variance_over_hw_minus_1           the sum of squared deviations divided by HW - 1
      last_element_of_odd_plane_skipped  the statistics of a plane of odd HW never see its last element
      bias_of_next_channel               bias[(c + 1) % C]
      short_slice_tail_skipped           split form: the last (shorter) slice's statistics stop at its last whole 256 elements
      eps_omitted                        1 / sqrt(var)
      relu_outer_before_residual         relu_outer(residual + t) computed as residual + relu_outer(t)
    one_pass: the variance as E[t^2] - E[t]^2 (one walk over the plane).  return_normalised: the fp32 value before its rounding."""
    assert mutation in (None,) + MUTATIONS
    dtype = x.dtype
    N, C, H, W = x.shape
    HW, P = H * W, N * C
    b = bias
    if mutation == "bias_of_next_channel":
        b = bias[(torch.arange(C) + 1) % C]
    t = biased(x, b).float().reshape(P, HW).numpy()
    odd_skip = mutation == "last_element_of_odd_plane_skipped" and HW % 2 == 1
    if not split:
        threads, pairs = threads_of(HW), HW % 2 == 0
        if one_pass:
            mean = (_workgroup_sum(t, threads, pairs) / f32(HW)).astype(f32)
            q = ((_workgroup_sum((t * t).astype(f32), threads, pairs) / f32(HW)).astype(f32) - (mean * mean).astype(f32)).astype(f32) * f32(HW)
        else:
            mean, q = _two_pass(t, threads, pairs and not odd_skip, HW - 1 if odd_skip else None)
    else:
        S = slices_of(HW)
        assert S > 0, "the split form starts at HW = 8192"
        L = -(-HW // S)
        mean, q, cnt = np.zeros(P, dtype=f32), np.zeros(P, dtype=f32), f32(0)
        for k in range(S):
            lo, hi = k * L, min(HW, (k + 1) * L)
            if hi <= lo:
                continue
            sl = t[:, lo:hi]
            used = None
            if mutation == "short_slice_tail_skipped" and hi - lo < L:
                used = (hi - lo) // 256 * 256
            if odd_skip and hi == HW:
                used = hi - lo - 1
            mk, qk = _two_pass(sl, 256, False, used)
            nk = f32(hi - lo)
            tot = f32(cnt + nk)
            dl = (mk - mean).astype(f32)
            mean = (mean + (dl * f32(nk / tot)).astype(f32)).astype(f32)
            q = (q + (qk + ((dl * dl).astype(f32) * f32(f32(cnt * nk) / tot)).astype(f32)).astype(f32)).astype(f32)
            cnt = tot
    div = f32(HW - 1) if mutation == "variance_over_hw_minus_1" else f32(HW)
    var = (q / div).astype(f32)
    if mutation != "eps_omitted":
        var = (var + f32(eps)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        invstd = (f32(1) / np.sqrt(var).astype(f32)).astype(f32)
        yn = ((t - mean[:, None]).astype(f32) * invstd[:, None]).astype(f32)
    yn = torch.from_numpy(yn).view(N, C, H, W)
    if return_normalised:
        return yn
    v = yn.to(dtype)
    if mutation == "relu_outer_before_residual":
        v = finish(v, None, relu_inner, relu_outer)
        return v if residual is None else (residual.float() + v.float()).to(dtype)
    return finish(v, residual, relu_inner, relu_outer)
