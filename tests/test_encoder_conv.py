"""pvo_conv_planes (csrc/encoder_conv.hip): the per-frame encoders' 3 x 3 and 7 x 7 convolutions on NCHW planes, on the matrix cores,
deterministic by construction - single layers against exact arithmetic, the epilogue against pvo_bias_norm_act, repeatability, batch
independence, bounds, and what the entry point refuses."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (ksize, stride, Cin, Cout, H, W): every layer class of the encoders at the 240 x 808 stream's map sizes, and ragged maps
LAYERS = [(7, 2, 3, 32, 240, 808), (7, 2, 3, 32, 37, 53),
          (3, 1, 32, 32, 120, 404), (3, 2, 32, 64, 120, 404), (3, 1, 64, 64, 60, 202), (3, 2, 64, 128, 60, 202), (3, 1, 128, 128, 30, 101),
          (3, 1, 32, 32, 7, 9), (3, 2, 32, 64, 7, 9), (3, 1, 64, 64, 1, 1), (3, 2, 64, 128, 1, 1), (3, 1, 32, 32, 2, 33), (3, 2, 32, 32, 2, 33)]


def _operands(layer, n, dtype, seed=0):
    k, s, cin, cout, h, w = layer
    g = torch.Generator().manual_seed(1000 * seed + 7 * cin + cout + h + w + n)
    x = torch.randn(n, cin, h, w, generator=g).to(dtype)
    wt = (torch.randn(cout, cin, k, k, generator=g) * (cin * k * k) ** -0.5).to(dtype)
    return x, wt


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("layer", LAYERS)
def test_single_layer_against_exact_arithmetic(cuda, layer, n, dtype):
    """ref = the fp64 convolution of the same 16-bit operands, A = the same convolution of |x|, |w|.  Every output element:
        |y - ref| <= u |ref| + 2 K 2^-24 A + 2^-24
    u = 2^-11 (fp16) / 2^-8 (bf16): ONE rounding to storage; K = Cin k^2 products added in fp32 in any order (error <= K 2^-24 A to first
    order), doubled for accumulators that truncate.  Derived from the formats, not tuned; no element is exempt."""
    from pvo_amd import droid_backends as db
    k, s, cin, cout, h, w = layer
    x, wt = _operands(layer, n, dtype)
    y = db.conv_planes(x.to(cuda), db.conv_planes_pack(wt.to(cuda)), stride=s)
    ref = torch.nn.functional.conv2d(x.double(), wt.double(), None, s, k // 2)
    A = torch.nn.functional.conv2d(x.double().abs(), wt.double().abs(), None, s, k // 2)
    assert y.shape == ref.shape and y.dtype == dtype and y.is_contiguous()
    u = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    K = cin * k * k
    bound = u * ref.abs() + 2 * K * 2.0 ** -24 * A + 2.0 ** -24
    err = (y.cpu().double() - ref).abs()
    worst = float((err / bound).max())
    print(layer, n, dtype, "max err / bound = %.3f, max |err| = %.3g" % (worst, float(err.max())))
    assert bool((err <= bound).all()), (layer, n, dtype, worst)


# (bias, residual, relu_inner, relu_outer): what the norm-free encoder uses - stem and first convolution of a block (bias + ReLU), second
# convolution of a block (everything) - all off, and the remaining single options
EPILOGUES = [(True, False, True, False), (True, True, True, True), (False, False, False, False), (True, False, False, False),
             (False, True, False, False), (False, True, False, True), (False, False, True, False)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("epi", EPILOGUES)
def test_epilogue_is_bias_norm_act_without_norm(cuda, epi, dtype):
    from pvo_amd import droid_backends as db
    has_b, has_r, ri, ro = epi
    for layer in ((7, 2, 3, 32, 64, 96), (3, 1, 32, 32, 33, 47), (3, 2, 64, 128, 60, 202), (3, 1, 128, 128, 30, 101)):
        k, s, cin, cout, h, w = layer
        x, wt = _operands(layer, 2, dtype, seed=1)
        x, p = x.to(cuda), db.conv_planes_pack(wt.to(cuda))
        bare = db.conv_planes(x, p, stride=s)
        g = torch.Generator().manual_seed(5)
        b = torch.randn(cout, generator=g).to(dtype).to(cuda) if has_b else None
        r = torch.randn(bare.shape, generator=g).to(dtype).to(cuda) if has_r else None
        got = db.conv_planes(x, p, b, r, stride=s, relu_inner=ri, relu_outer=ro)
        want = db.bias_norm_act(bare, b, r, norm=False, relu_inner=ri, relu_outer=ro)
        assert torch.equal(got, want), (layer, epi, dtype)
        if not (has_b or has_r or ri or ro):
            assert torch.equal(got, bare)


@pytest.mark.parametrize("layer", LAYERS)
def test_three_calls_give_identical_bits(cuda, layer):
    from pvo_amd import droid_backends as db
    k, s, cin, cout, h, w = layer
    x, wt = _operands(layer, 2, torch.float16, seed=2)
    x, p = x.to(cuda), db.conv_planes_pack(wt.to(cuda))
    b = torch.linspace(-1, 1, cout).half().to(cuda)
    ys = [db.conv_planes(x, p, b, stride=s, relu_inner=True) for _ in range(3)]
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    assert torch.equal(db.conv_planes_pack(wt.to(cuda)).frag, p.frag)


@pytest.mark.parametrize("layer", [(7, 2, 3, 32, 64, 96), (3, 1, 32, 32, 64, 96), (3, 2, 32, 64, 64, 96), (3, 1, 128, 128, 64, 96)])
def test_batch_of_sixteen_equals_sixteen_single_frames(cuda, layer):
    """(the batch runs the 8 x 16 pixel tile, a single 64 x 96 frame the 4 x 16 one: the sum of an output element does not depend on it)"""
    from pvo_amd import droid_backends as db
    k, s, cin, cout, h, w = layer
    x, wt = _operands(layer, 16, torch.float16, seed=3)
    x, p = x.to(cuda), db.conv_planes_pack(wt.to(cuda))
    y = db.conv_planes(x, p, stride=s)
    for i in range(16):
        assert torch.equal(y[i:i + 1], db.conv_planes(x[i:i + 1].contiguous(), p, stride=s)), i


@pytest.mark.parametrize("layer", LAYERS)
def test_every_output_is_written_and_nothing_else(cuda, layer):
    from pvo_amd import droid_backends as db
    k, s, cin, cout, h, w = layer
    n, guard = 3, 4096
    x, wt = _operands(layer, n, torch.float16, seed=4)
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    count = n * cout * ho * wo
    buf = torch.full((count + 2 * guard,), float("nan"), dtype=torch.float16, device=cuda)
    out = buf[guard:guard + count].view(n, cout, ho, wo)
    y = db.conv_planes(x.to(cuda), db.conv_planes_pack(wt.to(cuda)), stride=s, out=out)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    assert not bool(torch.isnan(out).any())
    assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + count:]).all())
    assert torch.equal(out, db.conv_planes(x.to(cuda), db.conv_planes_pack(wt.to(cuda)), stride=s))


def test_empty_inputs_are_fine(cuda):
    from pvo_amd import droid_backends as db
    p = db.conv_planes_pack(torch.zeros(32, 32, 3, 3, dtype=torch.float16, device=cuda))
    assert db.conv_planes(torch.zeros(0, 32, 8, 8, dtype=torch.float16, device=cuda), p).shape == (0, 32, 8, 8)
    assert db.conv_planes(torch.zeros(2, 32, 0, 8, dtype=torch.float16, device=cuda), p).shape == (2, 32, 0, 8)


def test_refusals(cuda):
    from pvo_amd import droid_backends as db
    from pvo_amd._lib import PvoHipError
    h16 = dict(dtype=torch.float16, device=cuda)

    def run(cin, cout, k, stride, x=None, wdtype=torch.float16, **kw):
        w = torch.zeros(cout, cin, k, k, dtype=wdtype, device=cuda)
        x = torch.zeros(1, cin, 8, 8, **h16) if x is None else x
        return db.conv_planes(x, db.conv_planes_pack(w), stride=stride, **kw)

    for cin, cout, k, stride in ((48, 32, 3, 1), (32, 40, 3, 1), (32, 32, 5, 1), (32, 32, 3, 3), (3, 32, 7, 1), (4, 32, 7, 2)):
        assert not db.conv_planes_supported(k, stride, cin, cout)
        with pytest.raises(PvoHipError):
            run(cin, cout, k, stride)
    for cin, cout, k, stride in ((32, 32, 3, 1), (32, 64, 3, 2), (3, 32, 7, 2), (128, 128, 3, 1)):
        assert db.conv_planes_supported(k, stride, cin, cout)
        assert run(cin, cout, k, stride).shape == (1, cout, 8 // stride, 8 // stride)
    with pytest.raises(PvoHipError):                                           # a non-contiguous x
        run(32, 32, 3, 1, x=torch.zeros(1, 32, 8, 16, **h16)[..., ::2])
    with pytest.raises(PvoHipError):                                           # mixed dtypes: filter bf16, x fp16
        run(32, 32, 3, 1, wdtype=torch.bfloat16)
    with pytest.raises(PvoHipError):                                           # bias of another dtype
        run(32, 32, 3, 1, bias=torch.zeros(32, dtype=torch.bfloat16, device=cuda))
    with pytest.raises(PvoHipError):                                           # a float32 x
        run(32, 32, 3, 1, x=torch.zeros(1, 32, 8, 8, device=cuda))
    x = torch.zeros(1, 32, 8, 8, **h16)
    with pytest.raises(PvoHipError):                                           # y aliasing x
        run(32, 32, 3, 1, x=x, out=x)
    with pytest.raises(PvoHipError):                                           # residual of another shape
        run(32, 32, 3, 1, residual=torch.zeros(1, 32, 4, 4, **h16))
    # the C entry point itself refuses an aliased output too (the binding's check is not the only one)
    from pvo_amd import _lib
    p = db.conv_planes_pack(torch.zeros(32, 32, 3, 3, **h16))
    rc = _lib.load().pvo_conv_planes(x.data_ptr(), p.frag.data_ptr(), None, None, x.data_ptr(), 1, 32, 32, 8, 8, 3, 1, 0, 0, _lib.PVO_F16, None)
    assert rc == 1                                                             # PVO_EINVAL
    rc = _lib.load().pvo_conv_planes(x.data_ptr(), p.frag.data_ptr(), None, None, x.data_ptr() + 2, 1, 32, 32, 8, 8, 3, 1, 0, 0, _lib.PVO_F16, None)
    assert rc == 1                                                             # misaligned
    y = torch.zeros(1, 32, 8, 8, **h16)
    rc = _lib.load().pvo_conv_planes(x.data_ptr(), p.frag.data_ptr(), None, None, y.data_ptr(), 1, 32, 32, 8, 8, 3, 1, 0, 0, 7, None)
    assert rc != 0                                                             # unknown dtype
