"""The update operator's matrix-core kernels against fp64 references of their own 16-bit operands, held to error bounds that are
built from the number formats, the number of accumulated terms and stated instruction accuracies (operator_bounds_util.py); on
small-integer operands, where fp32 arithmetic is exact, bit for bit; with every output and every input between NaN guards; at the
bench and driver map sizes, degenerate maps and the widths / heights around the tile edges.  No element is exempt from a bound and
no bound is tuned: each test's docstring derives its own.

The GPU tests carry the gpu mark one by one, because the module also holds the CPU tests which prove that the two checks fail on
a stand-in kernel that drops a product, swaps two channels, skips a chunk or reads a wrong halo row."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import operator_bounds_util as B
from operator_bounds_util import EPS, FLOOR

gpu = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
BENCH = [(1, 48, 64), (1, 30, 101), (1, 47, 156)]                       # bench (S-B) and the two driver map sizes
# degenerate maps; then widths 16 k - 1, 16 k, 16 k + 1, 16 k + 8, 16 k + 9 for k = 1, 2 (the wide convolution's two main-loop
# instantiations are chosen by x0 + 8 >= W) on heights 8 k +- 1; several edges at these small sizes only
SMALL = [(2, 1, 1), (2, 1, 40), (2, 33, 1), (3, 2, 2), (2, 7, 15), (1, 9, 16), (2, 7, 17), (1, 9, 24), (2, 15, 25), (1, 17, 31),
         (1, 7, 32), (1, 9, 33), (1, 15, 40), (2, 7, 41)]
SHAPES = BENCH + SMALL


def _id(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return None


# ------------------------------------------------------------------------------------------------ CPU: the checks can fail
def _standin_case(dtype, integer):
    g = torch.Generator().manual_seed(320)
    E, Cin, H, W, Cout = 1, 320, 13, 17, 256
    if integer:
        x, w = B.int_tensor(g, (E, Cin, H, W), -3, 3, dtype), B.int_tensor(g, (Cout, Cin, 3, 3), -2, 2, dtype)
        b = B.int_tensor(g, (Cout,), -4, 4, torch.float32)
    else:                                                                # the operands of tests/test_update_operator.py
        x = torch.randn(E, Cin, H, W, generator=g).to(dtype)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (0.5 / (9 * Cin) ** 0.5)).to(dtype)
        b = torch.randn(Cout, generator=g)
    ref, A = B.conv_ref(x, w, b)
    return x, w, b, ref, A, 9 * Cin + 1


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_bound_check_passes_clean_and_fails_every_mutation(dtype):
    x, w, b, ref, A, K = _standin_case(dtype, integer=False)
    out, bound = B.linear_bound(ref, A, K, dtype, relu=True)
    worst = B.assert_within(B.standin_conv3x3(x, w, b, dtype), out, bound, "clean %s" % dtype)
    assert worst < 1.0
    for m in B.MUTATIONS:
        with pytest.raises(AssertionError, match="over the bound"):
            B.assert_within(B.standin_conv3x3(x, w, b, dtype, mutation=m), out, bound, "%s %s" % (m, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_exact_check_passes_clean_and_fails_every_mutation(dtype):
    x, w, b, ref, A, K = _standin_case(dtype, integer=True)
    want = B.exact_want(torch.relu(ref), A, dtype)
    assert float(A.max()) < 2.0 ** 14 and float(ref.abs().max()) > 100          # far inside fp32's exact integers, far outside bf16's
    B.assert_bits(B.standin_conv3x3(x, w, b, dtype), want, "clean %s" % dtype)
    for m in B.MUTATIONS:
        with pytest.raises(AssertionError, match="elements differ"):
            B.assert_bits(B.standin_conv3x3(x, w, b, dtype, mutation=m), want, "%s %s" % (m, dtype))


def test_old_bf16_tolerance_accepts_a_dropped_product_on_the_last_column():
    """the gap this module closes.  A bf16 convolution loses ONE product (tap (1, 0) of one input channel) on the last image column, once
    for each of the 320 input channels: the derived bound rejects all 320 kernels; allclose(atol = rtol = 3e-2) with the mean-error check of
    tests/test_update_operator.py accepts 75 of them (a product of two unit-scale operands is about 0.01 here, the tolerance 0.03 (1 + |ref|))."""
    dtype = torch.bfloat16
    x, w, b, ref, A, K = _standin_case(dtype, integer=False)
    out, bound = B.linear_bound(ref, A, K, dtype, relu=True)
    y32 = F.conv2d(x.float(), w.float(), b, padding=1)
    old_ref = torch.relu(y32)
    accepted_by_old, caught = 0, 0
    for ci in range(x.shape[1]):
        y = torch.relu(B.drop_product(y32.clone(), x, w, ci)).to(dtype)
        old = torch.allclose(y.float(), old_ref, atol=3e-2, rtol=3e-2) and (y.float() - old_ref).abs().mean().item() < 3e-2 / 8
        accepted_by_old += int(old)
        over = (y.double() - out).abs() > bound
        assert not bool(over[..., :-1].any())
        caught += int(bool(over[..., -1].any()))
    print("dropped product: the old tolerance accepts %d of 320 mutants, the derived bound rejects %d" % (accepted_by_old, caught))
    assert caught == 320 and accepted_by_old >= 32


# ------------------------------------------------------------------------------------------------ GPU plumbing
_CODE = {torch.float16: 1, torch.bfloat16: 2}


def call(name, *args):
    """the C entry point `name` on the current stream with tensors passed as their pointers"""
    from pvo_amd import _lib
    conv = [ctypes.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args]
    rc = getattr(_lib.load(), name)(*conv, None)
    assert rc == 0, (name, rc)


def nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def nchw(t):
    return t.cpu().permute(0, 3, 1, 2)


class Job:
    """one prepared kernel call: device inputs `ins` (every floating tensor of it can move between guards), the outputs' shapes
    and dtypes, and launch(ins, outs)"""

    def __init__(self, ins, specs, launch, dev, in_guard):
        self.ins, self.specs, self.launch, self.dev, self.in_guard = ins, specs, launch, dev, in_guard

    def run(self, ins=None):
        outs = [torch.empty(s, dtype=d, device=self.dev) for s, d in self.specs]
        self.launch(self.ins if ins is None else ins, outs)
        torch.cuda.synchronize()
        return outs


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def check_guards(job, what):
    """outputs between NaN guards: everything written, nothing else touched, same bits; inputs between NaN guards (two image rows +
    two pixels of all channels at least): no NaN reaches an output, same bits"""
    plain = job.run()
    for p in plain:
        assert not bool(torch.isnan(p).any()), what
    gs = [B.Guarded(_numel(s), d, job.dev, 4096) for s, d in job.specs]
    job.launch(job.ins, [g.view(*s) for g, (s, d) in zip(gs, job.specs)])
    torch.cuda.synchronize()
    for i, (g, p) in enumerate(zip(gs, plain)):
        assert not bool(torch.isnan(g.inner).any()), "%s: output %d has unwritten elements" % (what, i)
        assert g.guards_untouched(), "%s: output %d written outside its extent" % (what, i)
        B.assert_bits(g.view(*p.shape), p, "%s: output %d between guards" % (what, i))
    gins = [B.guarded_copy(t, job.in_guard) if torch.is_tensor(t) and t.is_floating_point() else t for t in job.ins]
    for i, (o, p) in enumerate(zip(job.run(gins), plain)):
        assert not bool(torch.isnan(o).any()), "%s: output %d read outside an input" % (what, i)
        B.assert_bits(o, p, "%s: output %d with guarded inputs" % (what, i))


def _rand(g, shape, dtype, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _seed(*v):
    s = 17
    for x in v:
        s = (s * 1000003 + int(x)) % (2 ** 31)
    return torch.Generator().manual_seed(s)


# ------------------------------------------------------------------------------------------------ linear kernels
# every maker returns (job, reference): reference() -> (ref, A, K, relu) on the CPU in fp64, NCHW
def make_conv3x3(dev, dt, E, H, W, integer, Cin=320, Cout=256, relu=True, bias=True, entry="pvo_conv3x3", ystride=0, yoff=0):
    from pvo_amd import droid_backends as db
    g = _seed(E, H, W, Cin, Cout, integer)
    if integer:
        x, w = B.int_tensor(g, (E, Cin, H, W), -3, 3, dt), B.int_tensor(g, (Cout, Cin, 3, 3), -2, 2, dt)
        b = B.int_tensor(g, (Cout,), -4, 4, torch.float32) if bias else None
    else:
        x, w = _rand(g, (E, Cin, H, W), dt), _rand(g, (Cout, Cin, 3, 3), dt, 0.5 / (9 * Cin) ** 0.5)
        b = torch.randn(Cout, generator=g) if bias else None
    wide = entry == "pvo_conv3x3"
    wt = (db.conv3x3_weights if wide else db.conv3x3_c128_weights)(w.to(dev), dt)
    ins = [nhwc(x, dev), wt, None if b is None else b.to(dev)]

    def launch(i, o):
        dims = (E, H, W, Cin, Cout) if wide else (E, H, W, Cout)
        call(entry, i[0], i[1], i[2], o[0], *dims, 1 if relu else 0, ystride, yoff, _CODE[dt])

    job = Job(ins, [((E, H, W, ystride or Cout), dt)], launch, dev, (2 * W + 2) * max(Cin, Cout))
    return job, lambda: B.conv_ref(x, w, b) + (9 * Cin + (1 if bias else 0), relu)


def make_conv3x3_c128(dev, dt, E, H, W, integer, Cout=64, **kw):
    return make_conv3x3(dev, dt, E, H, W, integer, Cin=128, Cout=Cout, entry="pvo_conv3x3_c128", **kw)


def make_conv7x7(dev, dt, E, H, W, integer):
    from pvo_amd import droid_backends as db
    g = _seed(E, H, W, 7, integer)
    if integer:
        x, w, b = B.int_tensor(g, (E, 8, H, W), -3, 3, dt), B.int_tensor(g, (128, 8, 7, 7), -2, 2, dt), B.int_tensor(g, (128,), -4, 4, torch.float32)
    else:
        x, w, b = _rand(g, (E, 8, H, W), dt), _rand(g, (128, 8, 7, 7), dt, 0.08), torch.randn(128, generator=g)
    ins = [nhwc(x, dev), db.conv7x7_c8_weights(w.to(dev), dt), b.to(dev)]
    job = Job(ins, [((E, H, W, 128), dt)], lambda i, o: call("pvo_conv7x7_c8", i[0], i[1], i[2], o[0], E, H, W, _CODE[dt]), dev, (2 * W + 2) * 128)
    return job, lambda: B.conv_ref(x, w, b, pad=3) + (393, True)


def make_conv1x1(dev, dt, E, H, W, integer, Cout=576, relu=False):
    g = _seed(E, H, W, Cout, 1, integer)
    if integer:
        x, w, b = B.int_tensor(g, (E, 128, H, W), -3, 3, dt), B.int_tensor(g, (Cout, 128), -2, 2, dt), B.int_tensor(g, (Cout,), -4, 4, torch.float32)
    else:
        x, w, b = _rand(g, (E, 128, H, W), dt), _rand(g, (Cout, 128), dt, 0.08), torch.randn(Cout, generator=g)
    ins = [nhwc(x, dev), w.to(dev), b.to(dev)]
    job = Job(ins, [((E, H, W, Cout), dt)], lambda i, o: call("pvo_conv1x1_c128", i[0], i[1], i[2], o[0], E * H * W, Cout, 1 if relu else 0, _CODE[dt]),
              dev, (2 * W + 2) * Cout)
    return job, lambda: B.conv_ref(x, w[:, :, None, None], b, pad=0) + (129, relu)


def make_corr_encode(dev, dt, E, H, W, integer):
    from pvo_amd import droid_backends as db
    g = _seed(E, H, W, 196, integer)
    if integer:
        x, w, b = B.int_tensor(g, (E, 196, H, W), -3, 3, dt), B.int_tensor(g, (128, 196, 1, 1), -2, 2, dt), B.int_tensor(g, (128,), -4, 4, torch.float32)
    else:
        x, w, b = _rand(g, (E, 196, H, W), dt), _rand(g, (128, 196, 1, 1), dt, 0.07), torch.randn(128, generator=g)
    ins = [nhwc(x, dev), db.corr_encoder_weights(w.to(dev), dt), b.to(dev)]
    job = Job(ins, [((E, H, W, 128), dt)], lambda i, o: call("pvo_corr_encode", i[0], i[1], i[2], o[0], E * H * W, _CODE[dt]), dev, (2 * W + 2) * 196)
    return job, lambda: B.conv_ref(x, w, b, pad=0) + (197, True)


def run_linear(make, dev, dt, dims, integer, **kw):
    job, reference = make(dev, dt, *dims, integer, **kw)
    ref, A, K, relu = reference()
    what = " ".join([make.__name__[5:], str(dims)] + ["%s=%s" % kv for kv in kw.items()] + [_id(dt)])
    if integer:
        want = B.exact_want(torch.relu(ref) if relu else ref, A, dt)     # the two conditions, asserted before the launch
        B.assert_bits(nchw(job.run()[0]), want, what + " exact")
    else:
        out, bound = B.linear_bound(ref, A, K, dt, relu)
        B.assert_within(nchw(job.run()[0]), out, bound, what)


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("Cout", [128, 256, 512])
@pytest.mark.parametrize("Cin", [32, 96, 128, 320])
def test_conv3x3_bound_every_channel_count(cuda, Cin, Cout, dt):
    """pvo_conv3x3, K = 9 Cin + 1 (the f32 bias is one more fp32 addition): u |ref| + 2 K 2^-24 A + 2^-24, through the ReLU.
    Every Cin x Cout on a ragged map with a half right-most tile, with and without bias / ReLU."""
    run_linear(make_conv3x3, cuda, dt, (2, 9, 25), False, Cin=Cin, Cout=Cout)
    run_linear(make_conv3x3, cuda, dt, (1, 7, 17), False, Cin=Cin, Cout=Cout, relu=False, bias=False)


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", SHAPES, ids=_id)
def test_conv3x3_bound_and_exact_every_shape(cuda, dims, dt):
    """pvo_conv3x3 at the ConvGRU's Cin = 320 (K = 2881; Cout = 256 on the bench map and the small maps, 128 on the two driver maps):
    the derived bound on random operands, and bit-exact on integers (x in [-3, 3], w in [-2, 2], bias in [-4, 4]: max A about
    6 x 10^3 < 2^24, so fp32 sums are exact in any order and the only rounding is the one to storage)"""
    cout = 128 if dims in BENCH[1:] else 256
    run_linear(make_conv3x3, cuda, dt, dims, False, Cout=cout)
    run_linear(make_conv3x3, cuda, dt, dims, True, Cout=cout)


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", SHAPES, ids=_id)
def test_conv3x3_c128_bound_and_exact_every_shape(cuda, dims, dt):
    """pvo_conv3x3_c128, K = 9 x 128 + 1 = 1153, every Cout it serves (the encoders' 64 on every map; 128, 256, 512 on the small ones)"""
    for cout in (64,) if dims in BENCH else (64, 128, 256, 512):
        run_linear(make_conv3x3_c128, cuda, dt, dims, False, Cout=cout)
        run_linear(make_conv3x3_c128, cuda, dt, dims, True, Cout=cout)
    run_linear(make_conv3x3_c128, cuda, dt, dims, False, Cout=64, relu=False, bias=False)


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", SHAPES, ids=_id)
def test_conv7x7_c8_bound_and_exact_every_shape(cuda, dims, dt):
    """pvo_conv7x7_c8: K = 49 x 8 + 1 = 393, ReLU"""
    run_linear(make_conv7x7, cuda, dt, dims, False)
    run_linear(make_conv7x7, cuda, dt, dims, True)


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", SHAPES, ids=_id)
def test_conv1x1_and_corr_encode_bound_and_exact_every_shape(cuda, dims, dt):
    """pvo_conv1x1_c128 (K = 129; Cout = 576 and 192, with and without ReLU) and pvo_corr_encode (K = 196 + 1 = 197, ReLU): rows =
    E H W against their 64-row tiles"""
    for integer in (False, True):
        run_linear(make_conv1x1, cuda, dt, dims, integer, Cout=576)
        run_linear(make_conv1x1, cuda, dt, dims, integer, Cout=192, relu=True)
        run_linear(make_corr_encode, cuda, dt, dims, integer)


# ------------------------------------------------------------------------------------------------ segment mean
def make_segment_mean(dev, dt, E, H, W, integer, in_bias=False, C=128):
    """segments of 0, 1, 3 and the remaining edges on random operands; of 0, 1, 2 and 4 (exact reciprocals) on integers"""
    g = _seed(E, H, W, C, in_bias, integer)
    sizes = [0, 1, 2, 4] if integer else [0, 1, 3, 5]
    n = sum(sizes)
    x = B.int_tensor(g, (n, C, H, W), -3, 3, dt) if integer else _rand(g, (n, C, H, W), dt)
    b = None if not in_bias else (B.int_tensor(g, (C,), -2, 2, torch.float32) if integer else torch.randn(C, generator=g) * 0.5)
    idx = torch.randperm(n, generator=g).int()
    ptr = torch.tensor([0] + sizes).cumsum(0).int()
    Kseg = len(sizes)
    ins = [nhwc(x, dev), ptr.to(dev), idx.to(dev), None if b is None else b.to(dev)]
    job = Job(ins, [((Kseg, H, W, C), dt)], lambda i, o: call("pvo_segment_mean", i[0], i[1], i[2], i[3], o[0], Kseg, H * W, C, _CODE[dt]), dev, (2 * W + 2) * C)

    def reference():
        """(ref, bound): term t = relu(x + b) when there is a bias, which the kernel adds in fp32 (EPS (|x| + |b|)) and rounds to storage
        (B.stored) as a separate pass would; the n terms are added in fp32 and multiplied by the rounded 1 / n: n + 2 roundings"""
        xd = x.double()
        if b is None:
            t, dterm = xd, torch.zeros_like(xd)
        else:
            bd = b.double().view(1, -1, 1, 1)
            t = torch.relu(xd + bd)
            dterm = B.stored(t, EPS * (xd.abs() + bd.abs()), dt)
        ref, err = torch.zeros(Kseg, C, H, W, dtype=torch.float64), torch.zeros(Kseg, C, H, W, dtype=torch.float64)
        for k, s in enumerate(sizes):
            sel = idx[ptr[k]:ptr[k + 1]].long()
            if s:
                ref[k] = t[sel].sum(0) / s
                err[k] = dterm[sel].sum(0) / s + B.accum(s + 2, (t[sel].abs() + dterm[sel]).sum(0) / s)
        return ref, B.stored(ref, err, dt) if b is not None else B.unit(dt) * ref.abs() + err + FLOOR
    return job, reference


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("in_bias", [False, True])
@pytest.mark.parametrize("dims", SHAPES, ids=_id)
def test_segment_mean_bound_and_exact(cuda, dims, in_bias, dt):
    """pvo_segment_mean: out[k] = mean over the segment's edges of x (or of round(relu(x + in_bias))).  Without a bias the linear bound
    with K = n + 2; with one, each term carries EPS (|x| + |b|) + one storage rounding into the mean first.  Integers: bit-exact."""
    for integer in (False, True):
        job, reference = make_segment_mean(cuda, dt, *dims, integer, in_bias=in_bias)
        ref, bound = reference()
        if integer:
            B.exact_want(ref * 4, ref.abs() * 4 + 32, dt)                 # sums of at most 4 integers <= 5, exact reciprocals: multiples of 1/4
            B.assert_bits(nchw(job.run()[0]), ref.to(dt), "segment_mean exact %s bias=%s %s" % (dims, in_bias, _id(dt)))
        else:
            B.assert_within(nchw(job.run()[0]), ref, bound, "segment_mean %s bias=%s %s" % (dims, in_bias, _id(dt)))


# ------------------------------------------------------------------------------------------------ fused lookup + encoder
def make_lookup_encode(dev, dt, H, W, integer=False, N=2, cap=4):
    """the volume pool's radius-3 lookup fused with corr_encoder[0]; unused pool slots hold NaN.  integer: 64 features in [-2, 2], so the
    volume (the dot product of f1 / 4 and f2 / 4) holds multiples of 1/16 and its 2 x 2-averaged levels, rounded or not, of 1/1024; coordinates that are
    multiples of 8, hence integers at all four levels and bilinear weights of 0 and 1; integer filter and bias"""
    from pvo_amd import droid_backends as db
    from pvo_amd.modules.corr import CorrVolumePool
    g = _seed(H, W, 196)
    if integer:
        f1, f2 = B.int_tensor(g, (N, H, W, 64), -2, 2, dt).to(dev), B.int_tensor(g, (N, H, W, 64), -2, 2, dt).to(dev)
    else:
        f1, f2 = _rand(g, (N, H, W, 64), dt).to(dev), _rand(g, (N, H, W, 64), dt).to(dev)
    pool = CorrVolumePool(cap, H, W, dev, dt)
    assert pool.tiled
    for lv in pool.levels:
        lv.fill_(float("nan"))
    pool.add(f1, f2)
    coords = (torch.rand(N, H, W, 2, generator=g) * torch.tensor([W + 8.0, H + 8.0]) - 4.0)
    w, b = _rand(g, (128, 196, 1, 1), dt, 0.05), torch.randn(128, generator=g)
    if integer:
        coords = (coords / 8).round() * 8
        w, b = B.int_tensor(g, (128, 196, 1, 1), -2, 2, dt), B.int_tensor(g, (128,), -4, 4, torch.float32)
    coords = coords.to(dev)
    slots = pool.slots_tensor()
    ins = list(pool.levels) + [coords, db.corr_encoder_weights(w.to(dev), dt), b.to(dev), slots]

    def launch(i, o):
        ptrs = (ctypes.c_void_p * 4)(*[lv.data_ptr() for lv in i[:4]])
        call("pvo_corr_lookup_encode_tiled", ptrs, i[4], i[5], i[6], o[0], N, H, W, _CODE[dt], i[7], cap)

    job = Job(ins, [((N, H, W, 128), dt)], launch, dev, (2 * W + 2) * 196)
    looked_up = lambda: db.corr_pyramid_lookup_tiled(pool.levels, coords, channels_last=True, slots=slots)
    return job, lambda: B.conv_ref(looked_up().cpu(), w, b, pad=0) + (197, True)


LOOKUP_SHAPES = [(48, 64), (30, 101), (47, 156), (8, 8), (9, 17), (15, 25), (17, 9)]        # (the tiled pool needs H, W >= 8)


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("hw", LOOKUP_SHAPES, ids=_id)
def test_lookup_encode_bound_and_guards(cuda, hw, dt):
    """pvo_corr_lookup_encode_tiled as a GEMM of the pool's own looked-up tensor (pvo_corr_pyramid_lookup_tiled, pinned bit-exact against
    the CPU oracle by tests/test_corr_build.py): K = 196 + 1 = 197, ReLU, the linear bound.  Unused pool slots hold NaN.
    Integers: with features in [-2, 2] and coordinates that are multiples of 8 every looked-up value is a stored multiple of 1/1024 (asserted),
    so with an integer filter and bias every partial sum is a whole number of 1/1024 below 2^24 of them, exact in fp32: bit for bit."""
    job, reference = make_lookup_encode(cuda, dt, *hw)
    ref, A, K, relu = reference()
    assert bool(torch.isfinite(ref).all())
    out, bound = B.linear_bound(ref, A, K, dt, relu)
    B.assert_within(nchw(job.run()[0]), out, bound, "lookup_encode %s %s" % (hw, _id(dt)))
    check_guards(job, "lookup_encode %s" % (hw,))
    job, reference = make_lookup_encode(cuda, dt, *hw, integer=True)
    ref, A, K, relu = reference()
    B.exact_want(torch.relu(ref) * 1024, A * 1024, dt)                      # the two conditions, in units of 1/1024, before the launch
    assert float(ref.abs().max()) >= 4                                   # (and the case is not trivially zero)
    B.assert_bits(nchw(job.run()[0]), torch.relu(ref).to(dt), "lookup_encode exact %s %s" % (hw, _id(dt)))


# ------------------------------------------------------------------------------------------------ ConvGRU gates and candidate
def gru_operands(dt, E, H, W, C=192, seed=0):
    g = _seed(E, H, W, C, seed)
    r = lambda *s, sc=1.0: _rand(g, s, dt, sc)
    o = dict(net=torch.tanh(r(E, 128, H, W).float()).to(dt), cf=torch.relu(r(E, C, H, W)), P_zr=r(E, 256, H, W, sc=0.3), P_q=r(E, 128, H, W, sc=0.3),
             gg=torch.randn(E, 384, generator=g) * 0.3, wzr=r(256, 128 + C, 3, 3, sc=0.02), wq=r(128, 128 + C, 3, 3, sc=0.02))
    o["perm"] = torch.randperm(E + 3, generator=g)[:E].int()
    return o


def make_gates(dev, dt, E, H, W, o, slots=False):
    from pvo_amd import droid_backends as db
    C = o["cf"].shape[1]
    P = nhwc(o["P_zr"], dev)
    sl = None
    if slots:                                                            # the static term in a slot pool; unused slots hold NaN
        pool = torch.full((E + 3, H, W, 256), float("nan"), dtype=dt, device=dev)
        sl = o["perm"].to(dev)
        pool[sl.long()] = P
        P = pool
    ins = [nhwc(o["net"], dev), nhwc(o["cf"], dev), db.conv3x3_weights(o["wzr"].to(dev), dt), o["gg"].to(dev), P, sl]
    launch = lambda i, out: call("pvo_gru_conv_gates", i[0], i[1], C, i[2], i[3], i[4], i[5], out[0], out[1], E, H, W, _CODE[dt])
    return Job(ins, [((E, H, W, 128), dt)] * 2, launch, dev, (2 * W + 2) * 256)


def make_candidate(dev, dt, E, H, W, o, RN, Z, slots=False):
    from pvo_amd import droid_backends as db
    C = o["cf"].shape[1]
    P = nhwc(o["P_q"], dev)
    sl = None
    if slots:
        pool = torch.full((E + 3, H, W, 128), float("nan"), dtype=dt, device=dev)
        sl = o["perm"].to(dev)
        pool[sl.long()] = P
        P = pool
    ins = [RN, nhwc(o["cf"], dev), db.conv3x3_weights(o["wq"].to(dev), dt), o["gg"].to(dev), P, sl, Z, nhwc(o["net"], dev)]
    launch = lambda i, out: call("pvo_gru_conv_candidate", i[0], i[1], C, i[2], i[3], i[4], i[5], i[6], i[7], out[0], E, H, W, _CODE[dt])
    return Job(ins, [((E, H, W, 128), dt)], launch, dev, (2 * W + 2) * 256)


def gates_bounds(o, dt):
    """-> (Z ref, Z bound, RN ref, RN bound)"""
    Cin = 128 + o["cf"].shape[1]
    pre, A = B.conv_ref(torch.cat([o["net"], o["cf"]], 1), o["wzr"])
    gz = o["gg"][:, :256, None, None].double()
    pre, A = pre + gz + o["P_zr"].double(), A + gz.abs() + o["P_zr"].double().abs()
    d = B.accum(9 * Cin + 2, A)
    e = d / 4 + B.sigmoid_allowance(pre)
    s, n = torch.sigmoid(pre), o["net"].double()
    z_ref, rn_ref = s[:, :128], s[:, 128:] * n
    return z_ref, B.stored(z_ref, e[:, :128], dt), rn_ref, B.stored(rn_ref, n.abs() * e[:, 128:] + EPS * rn_ref.abs(), dt)


def candidate_bounds(o, dt, RN, Z):
    Cin = 128 + o["cf"].shape[1]
    q, A = B.conv_ref(torch.cat([RN, o["cf"]], 1), o["wq"])
    gq = o["gg"][:, 256:, None, None].double()
    q, A = q + gq + o["P_q"].double(), A + gq.abs() + o["P_q"].double().abs()
    d = B.accum(9 * Cin + 2, A)
    z, n, t = Z.double(), o["net"].double(), torch.tanh(q)
    ref = (1 - z) * n + z * t
    e = z.abs() * (d + B.tanh_allowance(q)) + 3 * EPS * ((1 - z).abs() * n.abs() + z.abs() * t.abs())
    return ref, B.stored(ref, e, dt)




@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", SHAPES, ids=_id)
def test_gru_gates_and_candidate_bounds(cuda, dims, dt):
    """pvo_gru_conv_gates / pvo_gru_conv_candidate over [net | cf] (Cin = 320), dense static terms and a slot pool.
    Pre-activation p = conv + g + P: K = 9 Cin + 2 fp32 terms, |p - ref_p| <= d = 2 K 2^-24 A with A = conv(|x|, |w|) + |g| + |P|.
      Z  = round(s(p)):       sigmoid is 1/4-Lipschitz: d / 4, + the evaluation allowance of rcp(1 + exp2(c p)) (sigmoid_allowance: < 4 x 2^-24
                              from 1 ulp each of v_exp_f32 / v_rcp_f32 and the three fp32 roundings around them), then one storage rounding;
      RN = round(s(p) net):   |net| times the same, + 2^-24 |ref| for the fp32 product, then one storage rounding;
      h' = round((1 - Z) net + Z tanh(q)), q the candidate's pre-activation over [RN | cf] with the kernel's own rounded RN and Z:
                              tanh is 1-Lipschitz: |Z| (d_q + tanh_allowance (< 9 x 2^-24, with the absolute part (1 - tanh) 3 x 2^-24 of the
                              cancellation in 1 - 2 / (1 + e))), + 3 x 2^-24 (|1 - Z| |net| + |Z| |tanh|) for the blend's fp32 operations,
                              then one storage rounding.
    Both allowances stay below u / 16 of the output scale 1 (u / 16 = 2^-15 fp16, 2^-12 bf16) on any input.  The slot-pool form must
    return the dense form's bits with NaN in every unused slot."""
    E, H, W = dims
    o = gru_operands(dt, E, H, W)
    what = "%s %s" % (dims, _id(dt))
    Zd, RNd = make_gates(cuda, dt, E, H, W, o).run()
    z_ref, z_b, rn_ref, rn_b = gates_bounds(o, dt)
    assert float(B.sigmoid_allowance(torch.linspace(-30, 30, 6001, dtype=torch.float64)).max()) <= B.unit(dt) / 16
    assert float(B.tanh_allowance(torch.linspace(-30, 30, 6001, dtype=torch.float64)).max()) <= B.unit(dt) / 16
    B.assert_within(nchw(Zd), z_ref, z_b, "gates Z " + what)
    B.assert_within(nchw(RNd), rn_ref, rn_b, "gates RN " + what)
    out = make_candidate(cuda, dt, E, H, W, o, RNd, Zd).run()[0]
    ref, bound = candidate_bounds(o, dt, nchw(RNd), nchw(Zd))
    B.assert_within(nchw(out), ref, bound, "candidate " + what)
    Zs, RNs = make_gates(cuda, dt, E, H, W, o, slots=True).run()
    B.assert_bits(Zs, Zd, "gates Z through p_slots " + what)
    B.assert_bits(RNs, RNd, "gates RN through p_slots " + what)
    B.assert_bits(make_candidate(cuda, dt, E, H, W, o, RNd, Zd, slots=True).run()[0], out, "candidate through p_slots " + what)


# ------------------------------------------------------------------------------------------------ permutation filters
PERM_STRIDE = 1013                                                        # prime, so p -> 1013 p is a bijection of the 2880 (tap, channel) pairs


def _perm_filter(launch_no, Cin, Cout, dt):
    """output channel co reads the single pair p = 1013 (launch_no Cout + co) mod 9 Cin, p = tap Cin + ci"""
    p = (PERM_STRIDE * (launch_no * Cout + torch.arange(Cout))) % (9 * Cin)
    tap, ci = p // Cin, p % Cin
    w = torch.zeros(Cout, Cin, 3, 3, dtype=dt)
    w[torch.arange(Cout), ci, tap // 3, tap % 3] = 1
    return w, tap, ci


def _shifted(x, tap, ci):
    """[E, Cout, H, W]: plane ci[co] of x shifted by tap[co] with zero padding"""
    H, W = x.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1))
    return torch.stack([xp[:, c, t // 3:t // 3 + H, t % 3:t % 3 + W] for t, c in zip(tap.tolist(), ci.tolist())], 1)


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", [(1, 9, 25), (2, 7, 41)], ids=_id)
def test_conv3x3_permutation_filters_return_the_shifted_planes(cuda, dims, dt):
    """every output channel of pvo_conv3x3 (Cin = 320, Cout = 256) has a single 1 at its own (tap, input channel): the output is that
    input plane, shifted and zero padded, bit for bit.  12 launches x 256 channels visit all 2880 pairs: the fragment order
    [Cout/128][Cin/32][9][2][4][64][8] element by element, on a half and a full right-most tile."""
    from pvo_amd import droid_backends as db
    E, H, W = dims
    Cin, Cout = 320, 256
    x = _rand(_seed(E, H, W, 3), (E, Cin, H, W), dt)
    xd, seen = nhwc(x, cuda), set()
    for n in range(12):
        w, tap, ci = _perm_filter(n, Cin, Cout, dt)
        seen.update((tap * Cin + ci).tolist())
        y = torch.empty(E, H, W, Cout, dtype=dt, device=cuda)
        call("pvo_conv3x3", xd, db.conv3x3_weights(w.to(cuda), dt), None, y, E, H, W, Cin, Cout, 0, 0, 0, _CODE[dt])
        B.assert_bits(nchw(y), _shifted(x, tap, ci), "launch %d" % n)
    assert len(seen) == 9 * Cin


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", [(1, 9, 25), (2, 7, 41)], ids=_id)
def test_gate_kernel_permutation_filters_return_the_gated_shifted_planes(cuda, dims, dt):
    """the same filters through pvo_gru_conv_gates with g = 0 and P = 0: the pre-activation of channel co is exactly v = the shifted
    plane of [net | cf] (one product, zeros elsewhere), so Z = round(s(v)) and RN = round(s(v) net) up to the evaluation allowance alone:
    sigmoid_allowance(v) (+ 2^-24 |ref| for RN's product) and one storage rounding.  Pins the [net | cf] split at channel 128 and the
    fragment order of the segmented main loop element by element: a wrong element is off by the difference of two random values."""
    from pvo_amd import droid_backends as db
    E, H, W = dims
    g = _seed(E, H, W, 4)
    net, cf = torch.tanh(_rand(g, (E, 128, H, W), dt).float()).to(dt), _rand(g, (E, 192, H, W), dt)
    x = torch.cat([net, cf], 1)
    zero_g, zero_P = torch.zeros(E, 384, device=cuda), torch.zeros(E, H, W, 256, dtype=dt, device=cuda)
    nd, cd, seen = nhwc(net, cuda), nhwc(cf, cuda), set()
    for n in range(12):
        w, tap, ci = _perm_filter(n, 320, 256, dt)
        seen.update((tap * 320 + ci).tolist())
        Z, RN = torch.empty(E, H, W, 128, dtype=dt, device=cuda), torch.empty(E, H, W, 128, dtype=dt, device=cuda)
        call("pvo_gru_conv_gates", nd, cd, 192, db.conv3x3_weights(w.to(cuda), dt), zero_g, zero_P, None, Z, RN, E, H, W, _CODE[dt])
        v = _shifted(x, tap, ci).double()
        s, a = torch.sigmoid(v), B.sigmoid_allowance(v)
        B.assert_within(nchw(Z), s[:, :128], B.stored(s[:, :128], a[:, :128], dt), "launch %d %s Z" % (n, _id(dt)))
        rn = s[:, 128:] * net.double()
        B.assert_within(nchw(RN), rn, B.stored(rn, net.double().abs() * a[:, 128:] + EPS * rn.abs(), dt), "launch %d %s RN" % (n, _id(dt)))
    assert len(seen) == 9 * 320


# ------------------------------------------------------------------------------------------------ the output heads
def heads_operands(dt, E, H, W, integer):
    g = _seed(E, H, W, 512, integer)
    if integer:
        # first stage: one weight in 24 is +-1, x in [-2, 2], bias in [-2, 2]: A1 is about 60, asserted <= 256 so that the hidden
        # value is an integer both storage types hold exactly; second stage w2 in [-1, 1], bias in [-4, 4]
        x = B.int_tensor(g, (E, 128, H, W), -2, 2, dt)
        w1 = (B.int_tensor(g, (512, 128, 3, 3), -1, 1, dt).float() * (torch.rand(512, 128, 3, 3, generator=g) < 1 / 16)).to(dt)
        b1, b2 = B.int_tensor(g, (512,), -2, 2, torch.float32), B.int_tensor(g, (8,), -4, 4, torch.float32)
        w2 = B.int_tensor(g, (8, 128, 3, 3), -1, 1, dt)
    else:
        x = torch.tanh(torch.randn(E, 128, H, W, generator=g)).to(dt)
        w1, b1 = _rand(g, (512, 128, 3, 3), dt, 0.03), torch.randn(512, generator=g) * 0.1
        w2, b2 = _rand(g, (8, 128, 3, 3), dt, 0.05), torch.randn(8, generator=g)
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2)            # w2 [head * 2 + out][channel][3][3]


def _w2_taps(w2):
    """[8,128,3,3] -> [4 heads][2 outputs][9 taps][128 channels]"""
    return w2.reshape(4, 2, 128, 9).permute(0, 1, 3, 2).contiguous()


def make_heads_fused(dev, dt, E, H, W, o):
    from pvo_amd import droid_backends as db
    ins = [nhwc(o["x"], dev), db.conv3x3_weights(o["w1"].to(dev), dt), o["b1"].to(dev), db.heads2_fragments(_w2_taps(o["w2"]).to(dev), dt), o["b2"].to(dev)]

    def launch(i, out):                                                  # out = [z (the fp32 tap contributions), y]
        call("pvo_conv3x3_heads", i[0], i[1], i[2], i[3], out[0], E, H, W, _CODE[dt])
        call("pvo_heads_gather", out[0], i[4], out[1], E, H, W, _CODE[dt])

    return Job(ins, [((E, H, W, 4, 18), torch.float32), ((E, H, W, 8), dt)], launch, dev, (2 * W + 2) * 512)


def make_heads_out(dev, dt, E, H, W, o, h1):
    ins = [nhwc(h1, dev), o["b1"].to(dev), _w2_taps(o["w2"]).to(dev), o["b2"].to(dev)]
    return Job(ins, [((E, H, W, 8), dt)], lambda i, out: call("pvo_heads_out", i[0], i[1], i[2], i[3], out[0], E, H, W, _CODE[dt]), dev, (2 * W + 2) * 512)


def heads_stage2(h, dh, o, dt):
    """second stage from the exact hidden value h >= 0 and the bound dh of the kernel's hidden value against it:
    ref = conv(h, w2) + b2; the hidden error is carried through sum |w2| dh; the kernel's own K = 9 x 128 + 1 fp32 terms are bounded
    on what it really adds, A2 = conv(h + dh, |w2|) + |b2|; then one storage rounding.  -> (ref, A2, bound)"""
    w2, b2 = o["w2"].double(), o["b2"].double()
    ref = F.conv2d(h, w2, b2, padding=1, groups=4)
    carry = F.conv2d(dh, w2.abs(), None, padding=1, groups=4)
    A2 = F.conv2d(h + dh, w2.abs(), b2.abs(), padding=1, groups=4)
    return ref, A2, B.stored(ref, carry + B.accum(1153, A2), dt)




@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", SHAPES, ids=_id)
def test_heads_bound_and_exact(cuda, dims, dt):
    """pvo_conv3x3_heads + pvo_heads_gather, and pvo_heads_out from a given first-stage tensor.
    Stage 1: hidden = relu(conv(x, w1) + b1), K1 = 9 x 128 + 1 = 1153: the kernel's fp32 value is within d1 = 2 K1 2^-24 A1 of it and is then
    ROUNDED to the storage type in LDS: |hidden_kernel - hidden| <= dh = d1 + u (hidden + d1) + 2^-24.
    Stage 2 (heads_stage2): |y - ref| <= sum |w2| dh + 2 K2 2^-24 A2 + one storage rounding, K2 = 1153 (nine taps of 128 channels through the
    fp32 z tensor and the gather, + bias).
    pvo_heads_out reads h1 (16-bit, bias-free), adds b1 in fp32 and rounds: dh = 2^-24 (|h1| + |b1|) + u hidden + 2^-24, then the same stage 2.
    Integers: sparse first-stage weights keep hidden <= 256 (exact in bf16 and fp16) and every sum below 2^24: both paths bit-exact."""
    E, H, W = dims
    what = "%s %s" % (dims, _id(dt))
    for integer in (False, True):
        o = heads_operands(dt, E, H, W, integer)
        ref1, A1 = B.conv_ref(o["x"], o["w1"], o["b1"])
        h = torch.relu(ref1)
        if integer:
            assert float(A1.max()) <= 256                                               # both conditions of both stages, before any launch
            ref, A2, _ = heads_stage2(h, torch.zeros_like(h), o, dt)
            want = B.exact_want(ref, A2, dt)
            B.assert_bits(nchw(make_heads_fused(cuda, dt, E, H, W, o).run()[1]), want, "heads exact " + what)
            h1 = (ref1 - o["b1"].double().view(1, -1, 1, 1)).to(dt)                     # the bias-free first stage, exact
            B.assert_bits(nchw(make_heads_out(cuda, dt, E, H, W, o, h1).run()[0]), want, "heads_out exact " + what)
        else:
            dh = B.stored(h, B.accum(1153, A1), dt)
            ref, _, bound = heads_stage2(h, dh, o, dt)
            B.assert_within(nchw(make_heads_fused(cuda, dt, E, H, W, o).run()[1]), ref, bound, "heads " + what)
            h1 = _rand(_seed(E, H, W, 9), (E, 512, H, W), dt, 0.5)
            b1 = o["b1"].double().view(1, -1, 1, 1)
            hh = torch.relu(h1.double() + b1)
            ref, _, bound = heads_stage2(hh, B.stored(hh, EPS * (h1.double().abs() + b1.abs()), dt), o, dt)
            B.assert_within(nchw(make_heads_out(cuda, dt, E, H, W, o, h1).run()[0]), ref, bound, "heads_out " + what)


# ------------------------------------------------------------------------------------------------ fp32 outputs
def make_glo(dev, dt, E, H, W):
    from pvo_amd import _lib
    g = _seed(E, H, W, 11)
    net = torch.tanh(torch.randn(E, 128, H, W, generator=g)).to(dt)
    w, b = _rand(g, (128, 128), dt, 0.1), torch.randn(128, generator=g)
    chunks = _lib.load().pvo_gru_glo_chunks(H * W)
    ins = [nhwc(net, dev), w.to(dev), b.to(dev)]
    job = Job(ins, [((E, chunks, 128), torch.float32)], lambda i, o: call("pvo_gru_glo_fused", i[0], i[1], i[2], o[0], E, H * W, _CODE[dt]), dev, (2 * W + 2) * 128)

    def reference():
        HW = H * W
        chunk = 256
        assert chunks == (HW + 255) // 256
        pre, A = B.conv_ref(net, w[:, :, None, None], b, pad=0)
        es = B.accum(129, A) / 4 + B.sigmoid_allowance(pre)
        n = net.double()
        term, eterm = (torch.sigmoid(pre) * n).reshape(E, 128, HW), (n.abs() * es).reshape(E, 128, HW)
        pad = lambda t: F.pad(t, (0, chunks * chunk - HW)).reshape(E, 128, chunks, chunk)
        ref = pad(term).sum(-1) / HW
        err = (pad(eterm).sum(-1) + B.accum(chunk, pad(term.abs() + eterm).sum(-1))) / HW + 2 * EPS * ref.abs()
        return ref.permute(0, 2, 1), err.permute(0, 2, 1)
    return job, reference


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", SHAPES, ids=_id)
def test_gru_glo_fused_bound(cuda, dims, dt):
    """pvo_gru_glo_fused: part[e, chunk, c] = (1 / HW) sum over the chunk's (at most 256) pixels of s(w . net + b) net, fp32 output (no u).
    Pre-activation: K = 128 + 1, d = 2 x 129 x 2^-24 A; gate: d / 4 + sigmoid_allowance; each term: |net| times that (the product is fused
    into the sum); the sum of at most 256 terms in fp32: 2 x 256 x 2^-24 sum |term|; the rounded 1 / HW and its product: 2 x 2^-24 |ref|."""
    job, reference = make_glo(cuda, dt, *dims)
    ref, bound = reference()
    B.assert_within(job.run()[0].cpu(), ref, bound, "gru_glo_fused %s %s" % (dims, _id(dt)))


def make_gate_context(dev, E, chunks):
    g = _seed(E, chunks, 13)
    part, wg, gb = torch.randn(E, chunks, 128, generator=g) / chunks, torch.randn(128, 384, generator=g) * 0.1, torch.randn(384, generator=g)
    ins = [part.to(dev), wg.to(dev), gb.to(dev)]
    job = Job(ins, [((E, 384), torch.float32)], lambda i, o: call("pvo_gate_context", i[0], i[1], i[2], o[0], E, chunks), dev, 4096)

    def reference():
        ref = part.double().sum(1) @ wg.double() + gb.double()
        A = part.double().abs().sum(1) @ wg.double().abs() + gb.double().abs()
        return ref, B.accum(chunks + 129, A)
    return job, reference


@gpu
@pytest.mark.parametrize("E,chunks", [(1, 1), (3, 12), (2, 16), (5, 17), (2, 29), (36, 12)])
def test_gate_context_bound(cuda, E, chunks):
    """pvo_gate_context: g = (sum over chunks of part) Wg + b, all fp32.  The chunk sum (`chunks` additions) feeds 128 fused products + the
    bias: (1 + chunks 2^-24) (1 + 129 2^-24) - 1 -> K = chunks + 129 on A = (sum |part|) |Wg| + |b|, in the doubled form of the other kernels"""
    job, reference = make_gate_context(cuda, E, chunks)
    ref, bound = reference()
    B.assert_within(job.run()[0].cpu(), ref, bound, "gate_context E=%d chunks=%d" % (E, chunks))


def make_eta(dev, dt, E, H, W):
    g = _seed(E, H, W, 15)
    x = torch.relu(torch.randn(E, 128, H, W, generator=g)).to(dt)
    w, b = _rand(g, (1, 128, 3, 3), dt, 0.05), torch.randn(1, generator=g)
    ins = [nhwc(x, dev), w.permute(0, 2, 3, 1).reshape(9, 128).contiguous().to(dev), b.to(dev)]
    job = Job(ins, [((E, H, W), torch.float32)], lambda i, o: call("pvo_eta_head", i[0], i[1], i[2], None, None, None, o[0], E, H, W, 0.0, 0.2, _CODE[dt]),
              dev, (2 * W + 2) * 128)

    def reference():
        v, A = B.conv_ref(x, w, b)
        d = B.accum(1153, A)
        sp = F.softplus(v, threshold=1e9)
        ref = 0.01 * sp
        lib = 4 * EPS                                                    # expf, log1pf: each taken as accurate to 2 ulp = 4 x 2^-24 relative
        err = 0.01 * (d + lib * torch.sigmoid(v) + lib * sp + 2.1e-9) + 2 * EPS * ref
        return ref[:, 0], err[:, 0]
    return job, reference


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", SHAPES, ids=_id)
def test_eta_head_bound(cuda, dims, dt):
    """pvo_eta_head with frame == NULL: eta = 0.01 softplus(v), v = conv(x, w) + b with K = 9 x 128 + 1 = 1153 fp32 terms: d = 2 K 2^-24 A;
    softplus is 1-Lipschitz.  The kernel evaluates log1pf(expf(v)) (v for v > 20, which is within exp(-20) = 2.1e-9 of softplus) with the
    library's functions, each taken as accurate to 2 ulp = 4 x 2^-24 relative: an error of expf moves log1p by s(v) 4 x 2^-24 (d log1p(E) /
    d ln E = E / (1 + E)), log1pf adds 4 x 2^-24 softplus(v); the rounded constant 0.01 and its product: 2 x 2^-24 |ref|.  fp32 output: no u."""
    job, reference = make_eta(cuda, dt, *dims)
    ref, bound = reference()
    B.assert_within(job.run()[0].cpu(), ref, bound, "eta_head %s %s" % (dims, _id(dt)))


# ------------------------------------------------------------------------------------------------ guards


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", SHAPES, ids=_id)
def test_guards_linear_kernels(cuda, dims, dt):
    """every linear kernel with each output inside a NaN-filled buffer (>= 4096 elements on each side) and, separately, each input inside one
    (>= two image rows + two pixels of all channels): all outputs written, no guard touched, no NaN read, the unguarded call's bits.
    The channel-slice form (ystride, yoff) of the two 3 x 3 kernels: the pixel's other channels are guard as well."""
    E, H, W = dims
    what = "%s %s" % (dims, _id(dt))
    check_guards(make_conv3x3(cuda, dt, E, H, W, False, Cin=320, Cout=256)[0], "conv3x3 " + what)
    check_guards(make_conv3x3(cuda, dt, E, H, W, False, Cin=32, Cout=128, relu=False, bias=False)[0], "conv3x3 32->128 " + what)
    check_guards(make_conv3x3_c128(cuda, dt, E, H, W, False, Cout=64)[0], "conv3x3_c128 " + what)
    check_guards(make_conv7x7(cuda, dt, E, H, W, False)[0], "conv7x7_c8 " + what)
    check_guards(make_conv1x1(cuda, dt, E, H, W, False, Cout=576)[0], "conv1x1_c128 " + what)
    check_guards(make_corr_encode(cuda, dt, E, H, W, False)[0], "corr_encode " + what)
    for in_bias in (False, True):
        check_guards(make_segment_mean(cuda, dt, E, H, W, False, in_bias=in_bias)[0], "segment_mean " + what)
    for make, cout, ys, yo in ((make_conv3x3, 128, 320, 128), (make_conv3x3_c128, 64, 192, 128), (make_conv3x3_c128, 128, 200, 8)):
        dense = make(cuda, dt, E, H, W, False, Cout=cout)[0].run()[0]
        job = make(cuda, dt, E, H, W, False, Cout=cout, ystride=ys, yoff=yo)[0]
        g = B.Guarded(E * H * W * ys, dt, cuda, 4096)
        job.launch(job.ins, [g.view(E, H, W, ys)])
        torch.cuda.synchronize()
        out = g.view(E, H, W, ys)
        B.assert_bits(out[..., yo:yo + cout].contiguous(), dense, "channel slice %d+%d of %d %s" % (yo, cout, ys, what))
        assert g.guards_untouched() and bool(torch.isnan(out[..., :yo]).all()) and bool(torch.isnan(out[..., yo + cout:]).all()), what


@gpu
@pytest.mark.parametrize("dt", DTYPES, ids=_id)
@pytest.mark.parametrize("dims", SHAPES, ids=_id)
def test_guards_gru_heads_and_fp32_kernels(cuda, dims, dt):
    """the same guards around pvo_gru_conv_gates / _candidate (dense and slot-pool static terms, unused slots NaN), pvo_conv3x3_heads +
    pvo_heads_gather (the fp32 z tensor between them counts as an output), pvo_heads_out, pvo_gru_glo_fused, pvo_gate_context, pvo_eta_head"""
    E, H, W = dims
    what = "%s %s" % (dims, _id(dt))
    o = gru_operands(dt, E, H, W, seed=1)
    for slots in (False, True):
        gates = make_gates(cuda, dt, E, H, W, o, slots=slots)
        check_guards(gates, "gates slots=%s %s" % (slots, what))
        Z, RN = gates.run()
        check_guards(make_candidate(cuda, dt, E, H, W, o, RN, Z, slots=slots), "candidate slots=%s %s" % (slots, what))
    ho = heads_operands(dt, E, H, W, False)
    check_guards(make_heads_fused(cuda, dt, E, H, W, ho), "heads " + what)
    check_guards(make_heads_out(cuda, dt, E, H, W, ho, _rand(_seed(E, H, W, 9), (E, 512, H, W), dt, 0.5)), "heads_out " + what)
    check_guards(make_glo(cuda, dt, E, H, W)[0], "gru_glo_fused " + what)
    check_guards(make_eta(cuda, dt, E, H, W)[0], "eta_head " + what)
    if dt == torch.float16:
        check_guards(make_gate_context(cuda, E, 12)[0], "gate_context " + what)
