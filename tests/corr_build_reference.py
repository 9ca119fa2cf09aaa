"""Helpers of tests/test_corr_build_bounds.py: the contract of pvo_corr_build, pvo_corr_build_tiled and pvo_corr_build_tiled_rows
(include/pvo_hip.h, header comment of pvo_amd/csrc/corr_build.hip) restated in plain torch on the CPU, the error bounds that follow
from the number formats alone, and the mutated stand-ins that prove the checks can fail.

The contract.  Features are [N, H, W, C] here (channels-last; the NCHW call form holds the same numbers).
  level 0     [N, HW, H, W]: level0[n, p1, p2] = sum_c (f1[n, p1, c] / 4) (f2[n, p2, c] / 4), accumulated in fp32 (fp64 for fp64
              features) and rounded ONCE to the feature type
  level l+1   [N, HW, H >> (l+1), W >> (l+1)]: the 2x2 mean of the STORED level l: ((a + b) + c) + d in the accumulate type in
              ATen's window order (kh, kw), times 0.25, one rounding; partial windows at the right / bottom border are dropped
  out_slots   edge n is written to slot out_slots[n] of level tensors that hold more slots; no other slot is touched
  tiled       level l is [slots, H, W, ceil(Hl / 8), ceil(Wl / 8), 8, 8] with (Hl, Wl) = (H >> l, W >> l): element (y, x) of a plane
              lies at [y / 8, x / 8, y % 8, x % 8].  Elements of an existing tile beyond (Hl, Wl) are unspecified padding
  rows        edge n reads frame rows1[n] of the first buffer and frame rows2[n] of the second

The level-0 bound (level0_bound), ref and A in fp64 on the operands as stored (level0_ref):
  16-bit output   u |ref| + 2 C 2^-24 A + 2^-24 (operator_bounds_util.linear_bound with K = C): the C products of two 16-bit numbers
                  are exact in fp32; adding them in any order on accumulators that may truncate errs by at most 2 C 2^-24 A; the
                  factor 1/16 is exact; one rounding to storage (u = 2^-11 fp16, 2^-8 bf16); 2^-24 is the spacing of fp16 subnormals
  fp32 output     2 C 2^-24 A: the operands / 4 are exact, a chain of C fused multiply-adds errs by at most C 2^-24 A to first
                  order (doubled for the higher orders), and the output is the accumulator itself: no storage term
  fp64 output     2 C 2^-53 A, the same chain in fp64
No element is exempt.  Pooled levels are held to equality with pool_exact of the stored level below."""
import torch

import operator_bounds_util as B

MUTATIONS = ("truncated_rounding", "dropped_product_last_column", "swapped_channels_f2", "transposed_pixels", "edge_reads_edge0",
             "pooled_from_unrounded", "window_shifted")
LEVEL0_MUTATIONS, POOL_MUTATIONS = MUTATIONS[:5], MUTATIONS[5:]
CPU_CASES = [(128, 8, 64), (16, 5, 7), (64, 11, 19), (32, 8, 40)]          # (C, H, W), two edges each
SENTINEL = 0x7e01                                                         # fp16: a NaN with a payload; bf16: 2.7e37 - nothing a build writes


# ------------------------------------------------------------------------------------------------ operands
def features(seed, N, H, W, C, dtype, integer=False):
    """two distinct feature maps [N, H, W, C] that differ per edge: unit normal, or integers in [-8, 8]"""
    g = torch.Generator().manual_seed(seed)
    if integer:
        return B.int_tensor(g, (N, H, W, C), -8, 8, dtype), B.int_tensor(g, (N, H, W, C), -8, 8, dtype)
    return torch.randn(N, H, W, C, generator=g).to(dtype), torch.randn(N, H, W, C, generator=g).to(dtype)


# ------------------------------------------------------------------------------------------------ references
def level0_ref(f1, f2):
    """(ref, A), both [N, HW, HW] float64: ref = sum_c f1 f2 / 16 and A = sum_c |f1| |f2| / 16 on the operands as stored"""
    a, b = f1.double().flatten(1, 2), f2.double().flatten(1, 2)
    ref = torch.einsum("npc,nqc->npq", a, b) / 16.0
    A = torch.einsum("npc,nqc->npq", a.abs(), b.abs()) / 16.0
    return ref, A


def level0_bound(ref, A, C, dtype):
    """the bound of the module docstring for an output of type `dtype`"""
    if dtype in (torch.float16, torch.bfloat16):
        return B.linear_bound(ref, A, C, dtype)[1]
    return 2.0 * C * {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}[dtype] * A


def pool_exact(level, dtype):
    """level l+1 from the stored level l [..., h, w]: ((a + b) + c) + d in the accumulate type (fp64 for fp64, else fp32) in ATen's window
    order, times 0.25, one rounding to `dtype`, floor sizes"""
    v = level.to(torch.float64 if dtype == torch.float64 else torch.float32)
    h, w = v.shape[-2] // 2, v.shape[-1] // 2
    v = v[..., :2 * h, :2 * w]
    s = ((v[..., 0::2, 0::2] + v[..., 0::2, 1::2]) + v[..., 1::2, 0::2]) + v[..., 1::2, 1::2]
    return (s * 0.25).to(dtype)


def untile(level, Hl, Wl):
    """[slots, H, W, th, tw, 8, 8] -> the row-major planes [slots, H, W, Hl, Wl]"""
    S, H, W, th, tw = level.shape[:5]
    return level.transpose(-3, -2).reshape(S, H, W, th * 8, tw * 8)[..., :Hl, :Wl].contiguous()


def inside_mask(H, W, l):
    """[th, tw, 8, 8] bool: the elements of level l's tiles that lie inside (H >> l, W >> l); the rest is padding"""
    Hl, Wl = H >> l, W >> l
    th, tw = (Hl + 7) // 8, (Wl + 7) // 8
    m = torch.zeros(th * 8, tw * 8, dtype=torch.bool)
    m[:Hl, :Wl] = True
    return m.view(th, 8, tw, 8).transpose(1, 2).contiguous()


def int_want(f1, f2, dtype, nlev=4):
    """the bits a build must return on integer features: with 16 max A < 2^24 every fp32 partial sum is an exact integer in any order,
    sum / 16 is exact, and the only rounding of level 0 is the one to storage; the pooled sums of four stored values are exact in fp32
    too (asserted), so every level is the fp64 value rounded once, level l+1 taken from the rounded level l.  Shapes as a dense build."""
    N, H, W, C = f1.shape
    ref, A = level0_ref(f1, f2)
    assert float(A.max()) * 16 < 2.0 ** 24, "partial sums must stay exact in fp32"
    assert bool((ref * 16 == (ref * 16).round()).all()), "operands are not integers"
    out = [ref.to(dtype).view(N, H, W, H, W)]
    assert bool(torch.isfinite(out[0]).all())
    for l in range(1, nlev):
        v = out[-1].double()
        h, w = v.shape[-2] // 2, v.shape[-1] // 2
        v = v[..., :2 * h, :2 * w]
        s = (v[..., 0::2, 0::2] + v[..., 0::2, 1::2] + v[..., 1::2, 0::2] + v[..., 1::2, 1::2]) * 0.25
        assert bool((s.float().double() == s).all()), "the pooled sums must stay exact in fp32"
        out.append(s.to(dtype))
    return out


# ------------------------------------------------------------------------------------------------ checks
def check_level0(l0, f1, f2, what):
    """level 0 [N, H, W, H, W] (any device) within the bound of its type on every element; prints and returns the worst err / bound"""
    N, H, W, C = f1.shape
    ref, A = level0_ref(f1, f2)
    return B.assert_within(l0.cpu().reshape(N, H * W, H * W), ref, level0_bound(ref, A, C, l0.dtype), what)


def _same_bits(y, want, what):
    it = {2: torch.int16, 4: torch.int32, 8: torch.int64}[y.element_size()]
    assert y.shape == want.shape and y.dtype == want.dtype, (what, tuple(y.shape), tuple(want.shape), y.dtype, want.dtype)
    bad = y.contiguous().view(it) != want.contiguous().view(it)
    bad &= ~((y == 0) & (want == 0))                       # (+0 and -0 are the same exact value)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (what, int(bad.sum()), bad.numel(), i, float(y[i]), float(want[i])))


def assert_bits(y, want, what):
    """bit for bit (operator_bounds_util.assert_bits, for 8-byte types and empty levels as well)"""
    _same_bits(y.cpu(), want.cpu(), what)


def check_pooled(levels, what):
    """every level above 0 equals pool_exact of the stored level below, bit for bit"""
    for l in range(1, len(levels)):
        below = levels[l - 1].cpu()
        assert_bits(levels[l], pool_exact(below, below.dtype), "%s: level %d from the stored level %d" % (what, l, l - 1))


def check_shapes(levels, N, H, W):
    assert [tuple(x.shape) for x in levels] == [(N, H, W, H >> l, W >> l) for l in range(len(levels))]


# ------------------------------------------------------------------------------------------------ CPU stand-in and its mutations
def _round_toward_zero(x, dtype):
    """fp32 -> 16-bit, truncated: the nearest value, stepped one unit toward zero where it is larger in magnitude"""
    y = x.to(dtype)
    over = y.float().abs() > x.abs()
    bits = y.view(torch.int16)
    return torch.where(over, bits - 1, bits).view(dtype)          # (sign-magnitude: one less is one step toward zero, either sign)


def _pool32(v):
    h, w = v.shape[-2] // 2, v.shape[-1] // 2
    v = v[..., :2 * h, :2 * w]
    return (((v[..., 0::2, 0::2] + v[..., 0::2, 1::2]) + v[..., 1::2, 0::2]) + v[..., 1::2, 1::2]) * 0.25


def standin_build(f1, f2, dtype, nlev=4, mutation=None):
    """what a correct kernel computes - an fp32 matmul, times 0.0625, one round-to-nearest-even, then pool_exact - or one of the ways
    this kernel can go wrong:
      truncated_rounding            level 0 rounded toward zero
      dropped_product_last_column   channel 5 missing from every sum whose target pixel lies in image column W - 1
      swapped_channels_f2           channels 3 and 4 of f2 exchanged (they share the first 16-channel k step; the others are untouched)
      transposed_pixels             p1 and p2 exchanged
      edge_reads_edge0              edge n > 0 reads f2 of edge 0
      pooled_from_unrounded         level l+1 from the fp32 level l before its rounding
      window_shifted                the 2x2 window of level 1 starts at column 1 (the columns wrap, so the sizes stay)"""
    assert mutation in (None,) + MUTATIONS
    N, H, W, C = f1.shape
    a, b = f1.float().flatten(1, 2), f2.float().flatten(1, 2).clone()
    if mutation == "dropped_product_last_column":
        b.view(N, H, W, C)[:, :, W - 1, 5] = 0
    if mutation == "swapped_channels_f2":
        b[..., 3], b[..., 4] = f2.float().flatten(1, 2)[..., 4], f2.float().flatten(1, 2)[..., 3]
    if mutation == "edge_reads_edge0":
        b = b[:1].expand(N, -1, -1)
    acc = torch.matmul(a, b.transpose(1, 2))
    if mutation == "transposed_pixels":
        acc = acc.transpose(1, 2)
    raw = (acc * 0.0625).reshape(N, H, W, H, W)
    levels = [_round_toward_zero(raw, dtype) if mutation == "truncated_rounding" else raw.to(dtype)]
    for l in range(1, nlev):
        if mutation == "pooled_from_unrounded":
            raw = _pool32(raw)
            levels.append(raw.to(dtype))
        elif mutation == "window_shifted" and l == 1:
            levels.append(pool_exact(torch.roll(levels[0], -1, dims=-1), dtype))
        else:
            levels.append(pool_exact(levels[-1], dtype))
    return levels
