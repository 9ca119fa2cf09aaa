"""Helpers of tests/test_operator_bounds.py: fp64 references of the update operator's layers, error bounds built from the number
formats alone, the exact-integer comparison, NaN-guarded buffers, and the mutated CPU stand-ins that prove the checks can fail.

Vocabulary (all tensors on the CPU, NCHW, float64 unless said otherwise):
  ref    the fp64 evaluation of the operation on the kernel's own 16-bit operands
  A      the same evaluation of the absolute values (|x|, |w|, |bias|): the scale an accumulation error is relative to
  u      one rounding to storage: 2^-11 (fp16), 2^-8 (bf16)
  EPS    2^-24, the unit roundoff of one fp32 operation
  K      the number of terms added in fp32 (bias included): any order of K additions errs by at most K EPS A to first order,
         doubled for matrix-core accumulators that truncate -> 2 K EPS A
  FLOOR  2^-24: the spacing of fp16 subnormals, the least a 16-bit output can resolve"""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
FLOOR = 2.0 ** -24


def unit(dtype):
    return {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]


# ------------------------------------------------------------------------------------------------ references
def conv_ref(x, w, b=None, pad=1):
    """(ref, A) of conv2d(x, w) + b with zero padding"""
    xd, wd = x.double(), w.double()
    bd = None if b is None else b.double()
    ref = F.conv2d(xd, wd, bd, padding=pad)
    A = F.conv2d(xd.abs(), wd.abs(), None if bd is None else bd.abs(), padding=pad)
    return ref, A


def accum(K, A):
    """K fp32 additions in any order on accumulators that may truncate"""
    return 2.0 * K * EPS * A


def stored(value, err, dtype):
    """error bound of a 16-bit output: `err` before the rounding, one rounding of a value that lies within err of `value`, the floor"""
    return err + unit(dtype) * (value.abs() + err) + FLOOR


def linear_bound(ref, A, K, dtype, relu=False):
    """|y - ref| <= u |ref| + 2 K EPS A + FLOOR for y = round(act(fp32 sum)): ReLU is 1-Lipschitz, so the accumulation error passes
    through it unchanged and the rounding acts on the activated value.  Returns (reference output, bound)."""
    out = torch.relu(ref) if relu else ref
    return out, unit(dtype) * out.abs() + accum(K, A) + FLOOR


def sigmoid_allowance(x):
    """absolute error of s = rcp(1 + exp2(c x)) with c = -log2(e) against sigmoid(x), x the fp32 pre-activation:
      t = c x: the constant and the product are rounded once each, |dt| <= 2 EPS |t|, so 2^t is off by the factor ln2 |dt| = 2 EPS |x|;
      v_exp_f32 within 1 ulp = 2 EPS: e = exp(-x) (1 + de), |de| <= 2 EPS (|x| + 1);
      1 + e rounded once (EPS), v_rcp_f32 within 1 ulp (2 EPS): s = sigma (1 + ds), |ds| <= (1 - sigma) |de| + 3 EPS
      (d ln(1/(1+e)) / d ln(e) = -e / (1 + e) = -(1 - sigma)).
    |s - sigma| <= sigma (1 - sigma) 2 EPS (|x| + 1) + 3 EPS sigma <= (0.45 + 0.5 + 3) EPS < 4 EPS: u / 2048 (fp16), u / 16384 (bf16) of
    the output scale 1.  Flushed subnormals of exp move s by less than 2^-126."""
    s = torch.sigmoid(x)
    return s * (1 - s) * 2 * EPS * (x.abs() + 1) + 3 * EPS * s


def tanh_allowance(x):
    """absolute error of th = 1 - 2 rcp(1 + exp2(c x)), c = 2 log2(e), against tanh(x):
      e = exp(2x) (1 + de), |de| <= 2 EPS (2 |x| + 1) (as above, the exponent is 2x);
      r = rcp(1 + e) = r0 (1 + dr), r0 = (1 - tanh) / 2, |dr| <= (e / (1 + e)) |de| + 3 EPS = ((1 + tanh) / 2) |de| + 3 EPS;
      2 r is exact, 1 - 2 r is rounded once: |th - tanh| <= (1 - tanh) |dr| + EPS |tanh|.
    The term (1 - tanh) 3 EPS does not shrink with tanh (the cancellation in 1 - 2 / (1 + e)): it is the absolute part.
    Everywhere <= (0.9 + 1 + 6 + 1) EPS < 9 EPS: u / 900 (fp16), u / 7000 (bf16) of the output scale 1."""
    t = torch.tanh(x)
    de = 2 * EPS * (2 * x.abs() + 1)
    return (1 - t) * ((1 + t) / 2 * de + 3 * EPS) + EPS * t.abs()


# ------------------------------------------------------------------------------------------------ checks
def assert_within(y, ref, bound, what):
    """every element of y within `bound` of `ref` (NaN fails); prints the worst err / bound"""
    y = y.double()
    assert y.shape == ref.shape, (what, tuple(y.shape), tuple(ref.shape))
    err = (y - ref).abs()
    ratio = err / bound
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("%s: max err / bound = %.3g, max |err| = %.3g" % (what, worst, float(err.max()) if err.numel() else 0.0))
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements over the bound, worst err / bound = %.3f; first at %s: got %r, ref %r, bound %.3g"
                             % (what, int(bad.sum()), bad.numel(), worst, i, float(y[i]), float(ref[i]), float(bound[i])))
    return worst


def exact_want(ref, A, dtype):
    """the bits a kernel must return on integer operands: every partial sum is an integer below 2^24, hence exact in fp32 in any order,
    and the only rounding is the one to storage"""
    assert float(A.max()) < 2.0 ** 24, "partial sums must stay exact in fp32"
    assert bool((ref == ref.round()).all()), "operands are not integers"
    want = ref.to(dtype)
    assert bool(torch.isfinite(want).all()), "the exact result overflows the storage type"
    return want


def assert_bits(y, want, what):
    """bit for bit, and says which element is wrong"""
    assert y.shape == want.shape and y.dtype == want.dtype, (what, tuple(y.shape), tuple(want.shape), y.dtype, want.dtype)
    it = {2: torch.int16, 4: torch.int32}[y.element_size()]
    bad = y.contiguous().view(it) != want.contiguous().view(it)
    bad &= ~((y == 0) & (want == 0))                       # (+0 and -0 are the same exact value)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (what, int(bad.sum()), bad.numel(), i, float(y[i]), float(want[i])))


def int_tensor(gen, shape, lo, hi, dtype):
    """integers in [lo, hi] stored in `dtype`"""
    return torch.randint(lo, hi + 1, shape, generator=gen).to(dtype)


# ------------------------------------------------------------------------------------------------ guards
class Guarded:
    """a flat buffer of `numel` elements between two guards of `guard` elements, everything NaN"""

    def __init__(self, numel, dtype, device, guard):
        guard = (max(int(guard), 4096) + 63) // 64 * 64       # (whole 128-byte lines: the inner pointer keeps the allocation's alignment)
        self.numel, self.guard = numel, guard
        self.buf = torch.full((numel + 2 * guard,), float("nan"), dtype=dtype, device=device)

    @property
    def inner(self):
        return self.buf[self.guard:self.guard + self.numel]

    def view(self, *shape):
        return self.inner.view(*shape)

    def guards_untouched(self):
        return bool(torch.isnan(self.buf[:self.guard]).all()) and bool(torch.isnan(self.buf[self.guard + self.numel:]).all())


def guarded_copy(t, guard):
    """a copy of the contiguous tensor t inside a NaN-filled allocation"""
    g = Guarded(t.numel(), t.dtype, t.device, guard)
    g.inner.copy_(t.reshape(-1))
    return g.view(*t.shape)


# ------------------------------------------------------------------------------------------------ CPU stand-in and its mutations
MUTATIONS = ("dropped_product_last_column", "swapped_channels_one_tap", "skipped_last_chunk", "halo_from_wrong_row")


def drop_product(y, x, w, channel):
    """remove the product of tap (1, 0) and input channel `channel` from every fp32 sum of the last image column (that tap reads column W - 2)"""
    y[:, :, :, -1] -= w.float()[None, :, channel, 1, 0, None] * x.float()[:, None, channel, :, -2]
    return y


def standin_conv3x3(x, w, b, dtype, relu=True, mutation=None):
    """an fp32 CPU convolution rounded once - what a correct kernel computes - or one of four ways a tiled kernel goes wrong:
      dropped_product_last_column  one product (tap (1, 0), input channel 5: it reads column W - 2) missing from every output of the last image column
      swapped_channels_one_tap     input channels 3 and 4 exchanged in tap (0, 1)
      skipped_last_chunk           the last 32 input channels never accumulated
      halo_from_wrong_row          the halo row below the image holds image row H - 2 instead of zeros"""
    assert mutation in (None,) + MUTATIONS
    xf, wf = x.float(), w.float()
    if mutation == "swapped_channels_one_tap":
        wf = wf.clone()
        wf[:, 3, 0, 1], wf[:, 4, 0, 1] = w.float()[:, 4, 0, 1], w.float()[:, 3, 0, 1]
    if mutation == "skipped_last_chunk":
        xf, wf = xf[:, :-32], wf[:, :-32]
    xp = F.pad(xf, (1, 1, 1, 1))
    if mutation == "halo_from_wrong_row":
        xp[:, :, -1, 1:-1] = xf[:, :, max(xf.shape[2] - 2, 0)]
    y = F.conv2d(xp, wf, b)
    if mutation == "dropped_product_last_column":
        y = drop_product(y, x, w, 5)
    return (torch.relu(y) if relu else y).to(dtype)
