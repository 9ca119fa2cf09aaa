"""The volume-free correlation on the GPU (pvo_altcorr_forward / pvo_altcorr_backward through the C ABI and droid_backends, AltCorrBlock
and CorrLayer) against tests/altcorr_reference.py: every branch of altcorr.hip within bounds derived from the number formats, bit for bit
on dyadic operands, every output element written and nothing beyond it, the empty shapes, the refusals, the block's pyramid and its
gradient.  Run with -rP for the worst error / bound of every case (profiles/r28_altcorr_fp64.txt)."""
import ctypes

import numpy as np
import pytest
import torch

import altcorr_reference as R
from operator_bounds_util import Guarded

pytestmark = pytest.mark.gpu

PVO_OK, PVO_EINVAL, PVO_EUNSUPPORTED = 0, 1, 4
# radius-3 cases with C % 4 == 0 run a second time from feature pointers that are 4 bytes off a 16-byte boundary: the entry point then
# takes altcorr_fwd_generic_kernel instead of altcorr_fwd_r3_kernel (whose float4 loads need the alignment)
FORWARD_RUNS = [(c, False) for c in R.CASES] + [(c, True) for c in R.CASES if c[7] == 3 and c[6] % 4 == 0]
FORWARD_IDS = [R.case_id(c) + ("-offset4" if o else "") for c, o in FORWARD_RUNS]


def _dev(a, cuda, offset=False):
    """device copy of a numpy array; offset: as a contiguous view that starts 4 bytes into a larger buffer"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not offset:
        return t.to(cuda)
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=cuda)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else 0)


def _forward(cuda, f1, f2, coords, r, shape=None, expect=PVO_OK, dtype=None):
    """pvo_altcorr_forward into a NaN-filled output between NaN guards -> the output tensor (guards checked)"""
    from pvo_amd import _lib
    from pvo_amd import droid_backends as db
    B, S, H1, W1, H2, W2, C = shape or (f1.shape[0], coords.shape[1], f1.shape[1], f1.shape[2], f2.shape[1], f2.shape[2], f1.shape[3])
    rd = 2 * r + 1
    out = Guarded(B * S * rd * rd * H1 * W1, torch.float32, cuda, 4096)
    rc = _lib.load().pvo_altcorr_forward(_p(f1), _p(f2), _p(coords), ctypes.c_void_p(out.inner.data_ptr()), B, S, H1, W1, H2, W2, C, r,
                                         _lib.PVO_F32 if dtype is None else dtype, db._stream(cuda))
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert out.guards_untouched()
    return out.view(B, S, rd * rd, H1, W1)


def _backward(cuda, f1, f2, coords, grad, r, shape=None, expect=PVO_OK):
    """pvo_altcorr_backward into NaN-filled fmap1_grad / fmap2_grad between NaN guards -> (g1, g2)"""
    from pvo_amd import _lib
    from pvo_amd import droid_backends as db
    B, S, H1, W1, H2, W2, C = shape or (f1.shape[0], coords.shape[1], f1.shape[1], f1.shape[2], f2.shape[1], f2.shape[2], f1.shape[3])
    g1, g2 = Guarded(B * H1 * W1 * C, torch.float32, cuda, 4096), Guarded(B * H2 * W2 * C, torch.float32, cuda, 4096)
    rc = _lib.load().pvo_altcorr_backward(_p(f1), _p(f2), _p(coords), _p(grad), ctypes.c_void_p(g1.inner.data_ptr()),
                                          ctypes.c_void_p(g2.inner.data_ptr()), B, S, H1, W1, H2, W2, C, r, _lib.PVO_F32, db._stream(cuda))
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert g1.guards_untouched() and g2.guards_untouched()
    return g1.view(B, H1, W1, C), g2.view(B, H2, W2, C)


# ------------------------------------------------------------------------------------------------ kernels against the reference
@pytest.mark.parametrize("cfg,offset", FORWARD_RUNS, ids=FORWARD_IDS)
def test_forward_is_within_the_bound_and_exact_on_dyadic_operands(cuda, cfg, offset):
    """|got - ref| <= (C + 8) U magnitude, U = 2^-24: C roundings of the fma chain, two for 1 - dx and 1 - dy, one for their product, one
    for s w, three for the four-term sum, one of slack for second-order terms; exactly +-0 where all four taps are outside.  On dyadic
    operands (features k/4, coordinates on quarters) every product and sum is exact in fp32: the fp64 reference bit for bit, after
    asserting that it is representable and magnitude 2^8 < 2^24.  Every output element is written, nothing beyond them"""
    from pvo_amd import droid_backends as db
    label = FORWARD_IDS[FORWARD_RUNS.index((cfg, offset))]
    C, r = cfg[6], cfg[7]
    for exact in (False, True):
        c = R.reference(cfg, exact)
        f1, f2, coords = _dev(c["f1"], cuda, offset), _dev(c["f2"], cuda, offset), _dev(c["coords"], cuda)
        got = _forward(cuda, f1, f2, coords, r)
        assert not bool(torch.isnan(got).any()), "an output element was not written"
        if exact:
            R.assert_equal(got, R.exact_want(c["value"], c["magnitude"], label), label + " forward, exact")
        else:
            assert R.assert_within(got.cpu(), c["value"], R.forward_bound(c["magnitude"], C), label + " forward") < 1
        bound, = db.altcorr_forward(f1, f2, coords, r)                        # (the binding's own allocation: the same bits)
        assert torch.equal(bound.view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("cfg", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_backward_is_within_the_bounds_and_exact_on_dyadic_operands(cuda, cfg):
    """g1: (T + 8) U magnitude, T = S (2r+2)^2 fma terms plus the seven roundings that form g and one of slack, magnitude
    sum |grad| w |f2|.  g2: (K + 8) U magnitude per target pixel, K the number of (pixel, sample, window tap) contributions that land on
    it - the atomics may add in any order - magnitude sum |grad| w |f1|.  Both buffers are handed over full of NaN, as torch.empty may:
    fmap1_grad is fully written, fmap2_grad zeroed before the accumulation.  On dyadic operands (gradients integers in [-2, 2]) every
    partial sum is exact whatever order the atomics take: bit for bit, after asserting the premise"""
    label, r = R.case_id(cfg), cfg[7]
    for exact in (False, True):
        c = R.reference(cfg, exact)
        g1, g2 = _backward(cuda, *(_dev(c[k], cuda) for k in ("f1", "f2", "coords", "grad")), r)
        assert not bool(torch.isnan(g1).any()) and not bool(torch.isnan(g2).any())
        if exact:
            R.assert_equal(g1, R.exact_want(c["bwd"]["g1"], c["bwd"]["g1_mag"], label), label + " g1, exact")
            R.assert_equal(g2, R.exact_want(c["bwd"]["g2"], c["bwd"]["g2_mag"], label), label + " g2, exact")
        else:
            assert R.assert_within(g1.cpu(), c["bwd"]["g1"], R.g1_bound(c["bwd"]), label + " g1") < 1
            assert R.assert_within(g2.cpu(), c["bwd"]["g2"], R.g2_bound(c["bwd"]), label + " g2") < 1


# ------------------------------------------------------------------------------------------------ empty shapes
def test_backward_without_source_pixels_returns_a_zeroed_fmap2_grad(cuda):
    """H1 W1 == 0 with a non-empty fmap2: there is nothing to accumulate, and fmap2_grad - NaN on entry, torch.empty_like in the binding -
    comes back all zero, as the header promises"""
    from pvo_amd import droid_backends as db
    f2 = torch.randn(2, 3, 4, 8, device=cuda)
    for h1, w1 in ((0, 5), (5, 0)):
        g1, g2 = _backward(cuda, None, f2, None, None, 3, shape=(2, 1, h1, w1, 3, 4, 8))
        assert g1.numel() == 0 and g2.numel() == 2 * 3 * 4 * 8
        assert bool((g2 == 0).all())
        b1, b2, bc = db.altcorr_backward(torch.empty(2, h1, w1, 8, device=cuda), f2, torch.empty(2, 1, h1, w1, 2, device=cuda),
                                         torch.empty(2, 1, 49, h1, w1, device=cuda), 3)
        assert bool((b2 == 0).all()) and b1.numel() == 0 and bc.numel() == 0


def test_backward_without_samples_returns_zero_gradients(cuda):
    f1, f2 = torch.randn(1, 3, 5, 8, device=cuda), torch.randn(1, 3, 4, 8, device=cuda)
    g1, g2 = _backward(cuda, f1, f2, None, None, 3, shape=(1, 0, 3, 5, 3, 4, 8))
    assert bool((g1 == 0).all()) and bool((g2 == 0).all())


def test_empty_batch_and_empty_target_touch_nothing_they_should_not(cuda):
    """B == 0: PVO_OK, no element exists and the guards stay NaN.  H2 W2 == 0: every tap is outside, so the outputs the header calls
    fully written are all zero (fmap2_grad has no element), again nothing beyond them is touched - with null fmap2 pointers"""
    f1 = torch.randn(1, 3, 5, 8, device=cuda)
    coords = torch.rand(1, 2, 3, 5, 2, device=cuda) * 4
    grad = torch.randn(1, 2, 49, 3, 5, device=cuda)
    assert _forward(cuda, None, None, None, 3, shape=(0, 2, 3, 5, 3, 4, 8)).numel() == 0
    g1, g2 = _backward(cuda, None, None, None, None, 3, shape=(0, 2, 3, 5, 3, 4, 8))
    assert g1.numel() == 0 and g2.numel() == 0
    for h2, w2 in ((0, 4), (4, 0)):
        out = _forward(cuda, f1, None, coords, 3, shape=(1, 2, 3, 5, h2, w2, 8))
        assert bool((out == 0).all())
        g1, g2 = _backward(cuda, f1, None, coords, grad, 3, shape=(1, 2, 3, 5, h2, w2, 8))
        assert bool((g1 == 0).all()) and g2.numel() == 0
    # the forward's own empty shapes: no sample, no source pixel
    assert _forward(cuda, f1, f1, None, 3, shape=(1, 0, 3, 5, 3, 5, 8)).numel() == 0
    assert _forward(cuda, None, f1, None, 3, shape=(1, 2, 0, 5, 3, 5, 8)).numel() == 0


# ------------------------------------------------------------------------------------------------ refusals (none of these launches)
def test_more_than_65535_grid_rows_are_refused_before_any_write(cuda):
    """B S = 65536 (forward) and B = 65536 (backward) index the grid's y dimension: PVO_EUNSUPPORTED, outputs still NaN"""
    from pvo_amd import _lib
    from pvo_amd import droid_backends as db
    n = 65536
    f = torch.zeros(n, 1, 1, 4, device=cuda)
    coords, grad = torch.zeros(n, 1, 1, 1, 2, device=cuda), torch.zeros(n, 1, 49, 1, 1, device=cuda)
    assert bool(torch.isnan(_forward(cuda, f, f, coords, 3, expect=PVO_EUNSUPPORTED)).all())
    assert bool(torch.isnan(_forward(cuda, f[:256], f[:256], coords.view(256, 256, 1, 1, 2), 3, expect=PVO_EUNSUPPORTED)).all())
    g1, g2 = _backward(cuda, f, f, coords, grad, 3, expect=PVO_EUNSUPPORTED)
    assert bool(torch.isnan(g1).all()) and bool(torch.isnan(g2).all())
    with pytest.raises(_lib.PvoHipError):
        db.altcorr_forward(f, f, coords, 3)
    with pytest.raises(_lib.PvoHipError):
        db.altcorr_backward(f, f, coords, grad, 3)
    # one fewer is served
    assert not bool(torch.isnan(_forward(cuda, f[:n - 1], f[:n - 1], coords[:n - 1], 3)).any())
    g1, g2 = _backward(cuda, f[:n - 1], f[:n - 1], coords[:n - 1], grad[:n - 1], 3)
    assert bool((g1 == 0).all()) and bool((g2 == 0).all())


def test_wrong_types_shapes_and_null_pointers_are_refused(cuda):
    from pvo_amd import _lib
    from pvo_amd import droid_backends as db
    c = R.reference(R.CASES[0])
    f1, f2, coords, grad = (_dev(c[k], cuda) for k in ("f1", "f2", "coords", "grad"))
    for bad in ((f1.half(), f2.half(), coords), (f1, f2.half(), coords), (f1.double(), f2.double(), coords), (f1, f2, coords.double())):
        with pytest.raises(_lib.PvoHipError):
            db.altcorr_forward(*bad, 3)
    for bad in ((f1.half(), f2.half(), coords, grad), (f1, f2, coords.double(), grad), (f1, f2, coords, grad.half())):
        with pytest.raises(_lib.PvoHipError):
            db.altcorr_backward(*bad, 3)
    with pytest.raises(_lib.PvoHipError):                                      # C == 0
        db.altcorr_forward(f1[..., :0].contiguous(), f2[..., :0].contiguous(), coords, 3)
    with pytest.raises(_lib.PvoHipError):
        db.altcorr_backward(f1[..., :0].contiguous(), f2[..., :0].contiguous(), coords, grad, 3)
    with pytest.raises(_lib.PvoHipError):                                      # negative radius
        db.altcorr_forward(f1, f2, coords, -1)
    with pytest.raises(_lib.PvoHipError):
        db.altcorr_backward(f1, f2, coords, grad[:, :, :1].contiguous(), -1)
    with pytest.raises(RuntimeError, match="must be contiguous"):
        db.altcorr_forward(f1.transpose(1, 2), f2, coords, 3)
    with pytest.raises(_lib.PvoHipError):                                      # CPU tensors: there is no fall-back
        db.altcorr_forward(f1.cpu(), f2.cpu(), coords.cpu(), 3)
    # the C ABI itself: other element types are unsupported, null pointers invalid, and neither writes
    assert bool(torch.isnan(_forward(cuda, f1, f2, coords, 3, expect=PVO_EUNSUPPORTED, dtype=_lib.PVO_F16)).all())
    assert bool(torch.isnan(_forward(cuda, None, f2, coords, 3, shape=(2, 2, 5, 7, 6, 9, 32), expect=PVO_EINVAL)).all())
    assert bool(torch.isnan(_forward(cuda, f1, None, coords, 3, shape=(2, 2, 5, 7, 6, 9, 32), expect=PVO_EINVAL)).all())
    assert bool(torch.isnan(_forward(cuda, f1, f2, None, 3, shape=(2, 2, 5, 7, 6, 9, 32), expect=PVO_EINVAL)).all())
    for args in ((None, f2, coords, grad), (f1, None, coords, grad), (f1, f2, None, grad), (f1, f2, coords, None)):
        g1, g2 = _backward(cuda, *args, 3, shape=(2, 2, 5, 7, 6, 9, 32), expect=PVO_EINVAL)
        assert bool(torch.isnan(g1).all()) and bool(torch.isnan(g2).all())


# ------------------------------------------------------------------------------------------------ AltCorrBlock
def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
                                                                      b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


@pytest.mark.parametrize("S", [0, 2], ids=["coords5", "coords6-S2"])
@pytest.mark.parametrize("edges", sorted(R.BLOCK_EDGES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("maps", R.BLOCK_MAPS, ids=["%dx%d" % m for m in R.BLOCK_MAPS])
def test_altcorrblock_pyramid_and_lookup(cuda, maps, dtype, edges, S):
    """the stored pyramid: level 0 is fmaps / 4 (exact; fp16 up to half a subnormal step, 2^-25), each further level the 2 x 2 mean of the
    stored level below - fp32: one rounding, U |mean| (the fp64 sum of four fp32 values adds 2^-50 at most); fp16:
    (2^-11 + 2^-22) |mean| + 2^-25, one fp32-accumulated mean and one rounding to half.  The call: every level within the forward bound
    (C + 8) U magnitude of block(...) evaluated on those stored tensors.  Planar and channels-last maps give identical bits"""
    from pvo_amd.modules.corr import AltCorrBlock
    frames, ii, jj = R.BLOCK_EDGES[edges]
    H, W = maps
    C = R.BLOCK_CHANNELS
    fmaps, coords = R.block_inputs(frames, H, W, len(ii), S)
    fm = fmaps.to(cuda).to(dtype)
    iit, jjt = torch.tensor(ii, device=cuda), torch.tensor(jj, device=cuda)
    label = "block %dx%d %s %s %s" % (H, W, "fp16" if dtype == torch.float16 else "fp32", edges, "S2" if S else "S1")
    with torch.no_grad():
        blk = AltCorrBlock(fm)
        blk_cl = AltCorrBlock(fm.permute(0, 1, 3, 4, 2).contiguous(), channels_last=True)
        out, out_cl = blk(coords.to(cuda), iit, jjt), blk_cl(coords.to(cuda), iit, jjt)
    assert len(blk.pyramid) == len(blk_cl.pyramid) == 4
    pyramid = [p.cpu() for p in blk.pyramid]
    for l, p in enumerate(pyramid):
        assert tuple(p.shape) == (1, frames, H >> l, W >> l, C) and p.dtype == dtype
        assert _bits_equal(blk.pyramid[l], blk_cl.pyramid[l])
    level0 = fm.cpu().double().permute(0, 1, 3, 4, 2) / 4
    if dtype == torch.float32:
        assert torch.equal(pyramid[0].double(), level0)
    else:
        assert float((pyramid[0].double() - level0).abs().max()) <= 2.0 ** -25
    for l in range(3):
        mean = R.pooled_mean(pyramid[l])
        bound = (R.U + 2.0 ** -50) * mean.abs() if dtype == torch.float32 else (2.0 ** -11 + 2.0 ** -22) * mean.abs() + 2.0 ** -25
        R.assert_within(pyramid[l + 1], mean, bound, "%s pyramid level %d" % (label, l + 1))
    assert tuple(out.shape) == (1, len(ii), 196, H, W) + ((S,) if S else ()) and out.dtype == torch.float32 and out.is_contiguous()
    assert _bits_equal(out, out_cl)
    value, magnitude = R.block(pyramid, coords, ii, jj, 3)
    got = out.cpu()
    for l in range(4):
        k = slice(49 * l, 49 * (l + 1))
        assert R.assert_within(got[:, :, k], value[:, :, k], R.forward_bound(magnitude[:, :, k], C), "%s level %d" % (label, l)) < 1


@pytest.mark.parametrize("S", [0, 2], ids=["coords5", "coords6-S2"])
def test_altcorrblock_gradient_is_exact_on_dyadic_operands(cuda, S):
    """autograd through AltCorrBlock and CorrLayer (the only consumer of pvo_altcorr_backward): integer features in [-3, 3], coordinates on
    the half grid, a sparse output weight in {-1, 0, 1}.  Features are then multiples of 2^-2 4^-l at level l, weights of 2^-2 4^-l,
    and every contribution to d / d fmaps a multiple of 2^-18; with the gradient's magnitude (the same gradient over absolute values)
    below 2^6 every partial sum - in the kernel's atomics, in the pooling's and the gather's backward - is exact in fp32, so the result
    equals the fp64 autograd of a pure-torch formulation on the CPU bit for bit.  The premise is asserted first"""
    from pvo_amd.modules.corr import AltCorrBlock
    frames, ii, jj = R.BLOCK_EDGES["mono"]
    H, W = R.BLOCK_MAPS[0]
    fmaps, coords = R.block_inputs(frames, H, W, len(ii), S, exact=True)
    g = np.random.default_rng(7)
    shape = (1, len(ii), 196, H, W) + ((S,) if S else ())
    weight = torch.from_numpy((g.integers(-1, 2, shape) * (g.random(shape) < 0.25)).astype(np.float32))
    want, magnitude = R.block_gradient(fmaps, coords, ii, jj, weight)
    label = "block gradient %s" % ("S2" if S else "S1")
    want = R.exact_want(want, magnitude, label, bits=18)
    assert float((want != 0).float().mean()) > 0.9
    x = fmaps.to(cuda).requires_grad_(True)
    out = AltCorrBlock(x)(coords.to(cuda), torch.tensor(ii, device=cuda), torch.tensor(jj, device=cuda))
    (out * weight.to(cuda)).sum().backward()
    R.assert_equal(x.grad, want, label)
    print("%s: bit-equal, max magnitude %.3g" % (label, float(magnitude.max())))
