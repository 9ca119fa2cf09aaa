"""Helpers of tests/test_altcorr_fp64_host.py and tests/test_altcorr_fp64_gpu.py: an fp64 reference of the volume-free correlation
(pvo_altcorr_forward / pvo_altcorr_backward, AltCorrBlock) that uses no product code and no oracle, the inputs both modules share,
error bounds built from the number formats alone, the exact comparison on dyadic operands, and fp32 stand-ins with named mutations that
prove the checks can fail.

Vocabulary (torch tensors on the CPU, float64 unless said otherwise):
  f1 [B,H1,W1,C], f2 [B,H2,W2,C]   channels-last feature maps; coords [B,S,H1,W1,2] float32 (x, y); r the radius, rd = 2 r + 1
  value      [B,S,rd^2,H1,W1], channel iy + rd ix: the explicit volume einsum("bhwc,byxc->bhwyx") sampled bilinearly at the four
             taps (floor + offset, + 1) of each window cell; a tap outside the target contributes 0
  magnitude  the same expression over |f1|, |f2| (|grad| in the backward): the scale an accumulation error is relative to
  U          2^-24, the unit roundoff of one fp32 operation
dx = x - floor(x) of an fp32 coordinate is exact in fp64, and in fp32 too except for x in (-1, 0) with bits below 2^-24 (1 + x is then
rounded once, by at most 2^-25: visible against the weight 1 - dx only where the complementary tap lies outside the target).  floor(x) is
carried as int64, so 3e9 stays 3e9 (far outside any target), which is also where the kernels' clamp puts it."""
import numpy as np
import torch

U = 2.0 ** -24

# (B, S, H1, W1, H2, W2, C, r): the smallest shapes that reach each branch of altcorr.hip
CASES = [
    (2, 2, 5, 7, 6, 9, 32, 3),        # B > 1 and S > 1
    (1, 3, 9, 13, 4, 6, 128, 3),      # workload C, target smaller than the source
    (1, 1, 8, 16, 8, 16, 64, 3),      # H1 W1 = 128: two full pixel groups, no tail
    (1, 2, 6, 11, 2, 3, 130, 3),      # target smaller than the window, tail channel group, C % 4 != 0
    (2, 1, 7, 10, 6, 7, 100, 3),      # B > 1, tail channel group
    (1, 2, 5, 13, 9, 7, 6, 3),        # C < 64, C % 4 != 0
    (1, 2, 6, 11, 6, 6, 16, 2),       # generic kernel
    (1, 1, 3, 5, 7, 9, 4, 0),         # radius 0
    (1, 1, 5, 9, 6, 8, 20, 1),        # radius 1
]
EXACT_HOST_CASES = [CASES[0], CASES[3], CASES[6], CASES[7]]
ZERO_SHARE_CAP = 0.60
ZERO_SHARE_CAP_2X3 = 0.85

MUTATIONS = ("dropk", "tail", "batch", "border", "sample0", "trunc", "swapd", "chan", "corner", "dirty")
FORWARD_MUTATIONS = ("dropk", "batch", "border", "sample0", "trunc", "swapd", "chan")
BACKWARD_MUTATIONS = MUTATIONS


def case_id(cfg):
    return "B%d-S%d-%dx%d-%dx%d-C%d-r%d" % tuple(cfg)


def applicable(mutation, cfg):
    """whether `mutation` can change a value of this case at all"""
    B, S, _, _, _, _, C, r = cfg
    return {"batch": B > 1, "sample0": S > 1, "chan": r > 0, "trunc": r > 0, "tail": C % 64 != 0}.get(mutation, True)


# ------------------------------------------------------------------------------------------------ inputs
def specials(H2, W2):
    """the coordinates placed deliberately, (x, y): exact integers, -0.0, the last pixel, windows that leave the target partly, windows
    that leave it by exactly one tap on each side (at radius 3, floor == -4 puts the last tap at -1 and floor == W2 + 3 the first at
    W2) and by a hair less, values beyond the int range, and half-way points astride the border"""
    return np.array([(0.0, 0.0), (-0.0, -0.0), (W2 - 1, H2 - 1), (-3.25, 1.5), (1.5, -3.25), (W2 + 2.5, 1.25), (1.25, H2 + 2.5),
                     (-4.0, -4.0), (-3.999, -3.999), (W2 + 3, H2 + 3), (W2 + 2.999, H2 + 2.999), (3e9, -3e9), (2.0, 3.0), (-1.0, -2.0),
                     (-0.5, -0.5), (W2 - 0.5, H2 - 0.5)], np.float32)


def special_pixels(H1, W1):
    n = min(16, (H1 * W1) // 2)
    return (np.arange(n) * (H1 * W1)) // n


def _grid(H1, W1, H2, W2):
    """the source grid mapped onto the target"""
    xs = np.arange(W1, dtype=np.float64) * (W2 - 1) / max(W1 - 1, 1)
    ys = np.arange(H1, dtype=np.float64) * (H2 - 1) / max(H1 - 1, 1)
    return np.stack(np.meshgrid(xs, ys), -1)                                   # [H1,W1,2] (x, y)


def inputs(cfg):
    """(f1, f2, coords, grad) float32 numpy: features standard_normal / 4, coordinates the mapped grid + uniform jitter in +-2.5 with
    the special list written over min(16, H1 W1 / 2) evenly spaced pixels of every (b, s) plane, rotated by the plane index"""
    B, S, H1, W1, H2, W2, C, r = cfg
    g = np.random.default_rng([2028] + list(cfg))
    f1 = (g.standard_normal((B, H1, W1, C)) / 4).astype(np.float32)
    f2 = (g.standard_normal((B, H2, W2, C)) / 4).astype(np.float32)
    coords = (_grid(H1, W1, H2, W2)[None, None] + g.uniform(-2.5, 2.5, (B, S, H1, W1, 2))).astype(np.float32)
    sp, pix = specials(H2, W2), special_pixels(H1, W1)
    flat = coords.reshape(B * S, H1 * W1, 2)
    for p in range(B * S):
        flat[p, pix] = sp[(np.arange(len(pix)) + p) % len(sp)]
    grad = g.standard_normal((B, S, (2 * r + 1) ** 2, H1, W1)).astype(np.float32)
    return f1, f2, coords, grad


def exact_inputs(cfg):
    """dyadic operands: features k / 4 (|k| <= 3), coordinates round(grid) + k / 4 (|k| <= 12), gradients integers in [-2, 2].  Weights
    are multiples of 1/16 and every product and partial sum a multiple of 2^-8 (forward) or 2^-6 (backward) far below 2^24 of them: exact
    in fp32 in any order, with or without fma"""
    B, S, H1, W1, H2, W2, C, r = cfg
    g = np.random.default_rng([2029] + list(cfg))
    f1 = (g.integers(-3, 4, (B, H1, W1, C)) / 4).astype(np.float32)
    f2 = (g.integers(-3, 4, (B, H2, W2, C)) / 4).astype(np.float32)
    coords = (np.round(_grid(H1, W1, H2, W2))[None, None] + g.integers(-12, 13, (B, S, H1, W1, 2)) / 4).astype(np.float32)
    grad = g.integers(-2, 3, (B, S, (2 * r + 1) ** 2, H1, W1)).astype(np.float32)
    return f1, f2, coords, grad


def specials_present(coords, H2, W2):
    """every special of the list is in the plane coords [H1,W1,2], sign of zero included"""
    have = {(float(x), float(y), bool(np.signbit(x)), bool(np.signbit(y))) for x, y in coords.reshape(-1, 2)}
    return all((float(x), float(y), bool(np.signbit(x)), bool(np.signbit(y))) in have for x, y in specials(H2, W2))


# ------------------------------------------------------------------------------------------------ fp64 reference
def _t(a, dtype=torch.float64):
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return a.to(dtype)


def _frac(coords):
    c = _t(coords)
    assert coords.dtype in (np.float32, torch.float32), "coordinates are fp32: that is what makes dx, dy exact"
    fl = torch.floor(c)
    d = c - fl
    return fl[..., 0].long(), fl[..., 1].long(), d[..., 0], d[..., 1]


def _cell_taps(coords, r, H2, W2):
    """for each window cell and each of its four taps: (channel, inside [B,S,H1,W1], flat target index (clamped where outside), weight)"""
    rd = 2 * r + 1
    fx, fy, dx, dy = _frac(coords)
    for ix in range(rd):
        for iy in range(rd):
            for ty in (0, 1):
                for tx in (0, 1):
                    h2, w2 = fy - r + iy + ty, fx - r + ix + tx
                    ok = (h2 >= 0) & (h2 < H2) & (w2 >= 0) & (w2 < W2)
                    idx = h2.clamp(0, max(H2 - 1, 0)) * W2 + w2.clamp(0, max(W2 - 1, 0))
                    yield iy + rd * ix, ok, idx, (dy if ty else 1 - dy) * (dx if tx else 1 - dx)


def sample(volume, coords, r):
    """the bilinear window lookup of an explicit volume [B,H1,W1,H2,W2] -> [B,S,rd^2,H1,W1]; differentiable in `volume`"""
    B, S, H1, W1, _ = coords.shape
    H2, W2 = volume.shape[-2:]
    rd = 2 * r + 1
    out = [torch.zeros(B, S, H1, W1, dtype=torch.float64) for _ in range(rd * rd)]
    if H2 * W2 > 0:
        flat = volume.reshape(B, 1, H1, W1, H2 * W2).expand(B, S, H1, W1, H2 * W2)
        for ch, ok, idx, w in _cell_taps(coords, r, H2, W2):
            v = flat.gather(-1, idx.unsqueeze(-1)).squeeze(-1)
            out[ch] = out[ch] + torch.where(ok, v * w, torch.zeros_like(w))
    return torch.stack(out, 2)


def forward(f1, f2, coords, r):
    """(value, magnitude), both [B,S,rd^2,H1,W1]"""
    a, b = _t(f1), _t(f2)
    return (sample(torch.einsum("bhwc,byxc->bhwyx", a, b), coords, r),
            sample(torch.einsum("bhwc,byxc->bhwyx", a.abs(), b.abs()), coords, r))


def backward(f1, f2, coords, grad, r):
    """dict(g1, g2, g1_mag, g2_mag, T, K): the adjoint of forward() written as the scatter of grad w into the volume's gradient,
    g1 = G f2, g2 = G^T f1; magnitudes sum |grad| w |f2| and sum |grad| w |f1|; T = S (2r+2)^2 is the number of terms of a g1 element,
    K [B,H2,W2] counts the (pixel, sample, window tap) triples whose tap is that target pixel (one atomic each)"""
    a, b, go = _t(f1), _t(f2), _t(grad)
    B, S, H1, W1, _ = coords.shape
    H2, W2 = b.shape[1:3]
    n2 = max(H2 * W2, 1)
    G, Ga = torch.zeros(B, H1, W1, n2, dtype=torch.float64), torch.zeros(B, H1, W1, n2, dtype=torch.float64)
    K = torch.zeros(B, n2, dtype=torch.float64)
    if H2 * W2 > 0:
        for ch, ok, idx, w in _cell_taps(coords, r, H2, W2):
            gw = torch.where(ok, go[:, :, ch] * w, torch.zeros_like(w))
            G.scatter_add_(-1, idx.permute(0, 2, 3, 1), gw.permute(0, 2, 3, 1))
            Ga.scatter_add_(-1, idx.permute(0, 2, 3, 1), gw.abs().permute(0, 2, 3, 1))
        fx, fy, _, _ = _frac(coords)
        for iy in range(2 * r + 2):
            for ix in range(2 * r + 2):
                h2, w2 = fy - r + iy, fx - r + ix
                ok = (h2 >= 0) & (h2 < H2) & (w2 >= 0) & (w2 < W2)
                K.scatter_add_(-1, (h2.clamp(0, H2 - 1) * W2 + w2.clamp(0, W2 - 1)).reshape(B, -1), ok.double().reshape(B, -1))
    G, Ga, K = G[..., :H2 * W2], Ga[..., :H2 * W2], K[:, :H2 * W2]
    bf, af = b.reshape(B, H2 * W2, -1), a
    return dict(g1=torch.einsum("bhwt,btc->bhwc", G, bf), g2=torch.einsum("bhwt,bhwc->btc", G, af).reshape(b.shape),
                g1_mag=torch.einsum("bhwt,btc->bhwc", Ga, bf.abs()), g2_mag=torch.einsum("bhwt,bhwc->btc", Ga, af.abs()).reshape(b.shape),
                T=S * (2 * r + 2) ** 2, K=K.reshape(B, H2, W2))


def block(pyramid, coords, ii, jj, r):
    """AltCorrBlock.__call__ in fp64 on the block's own stored pyramid tensors [B,N,H_l,W_l,C]: level l correlates pyramid[0][:, ii]
    with pyramid[l][:, jj] at coords / 2^l (exact in fp32), rd^2 channels per level, concatenated in order.  coords [B,E,H,W,2] or
    [B,E,H,W,S,2].  Returns (value, magnitude), [B,E,L rd^2,H,W] or [B,E,L rd^2,H,W,S]"""
    coords = coords.detach().cpu().float()
    squeeze = coords.dim() == 5
    if squeeze:
        coords = coords.unsqueeze(-2)
    B, E, H, W, S, _ = coords.shape
    c = coords.permute(0, 1, 4, 2, 3, 5).reshape(B * E, S, H, W, 2)
    ii, jj = torch.as_tensor(ii).cpu().long(), torch.as_tensor(jj).cpu().long()
    vals, mags = [], []
    for l, level in enumerate(pyramid):
        f1 = _t(pyramid[0])[:, ii].reshape((B * E,) + tuple(pyramid[0].shape[2:]))
        f2 = _t(level)[:, jj].reshape((B * E,) + tuple(level.shape[2:]))
        cl = c / 2 ** l
        assert torch.equal(cl * 2 ** l, c)
        d = cl.double() - torch.floor(cl.double())
        assert torch.equal(d.float().double(), d), "level %d: dx or dy is not exact in fp32 (see block_inputs)" % l
        v, m = forward(f1, f2, cl, r)
        vals.append(v.view(B, E, S, -1, H, W).permute(0, 1, 3, 4, 5, 2))
        mags.append(m.view(B, E, S, -1, H, W).permute(0, 1, 3, 4, 5, 2))
    v, m = torch.cat(vals, 2), torch.cat(mags, 2)
    return (v.squeeze(-1), m.squeeze(-1)) if squeeze else (v, m)


# ------------------------------------------------------------------------------------------------ bounds and checks
def forward_bound(magnitude, C):
    """(C + 8) U magnitude: C roundings of the fma chain; two for 1 - dx and 1 - dy, one for their product, one for s w; three for the
    four-term sum; one of slack for second-order terms.  0 where all four taps are outside: the output is then exactly +-0"""
    return (C + 8) * U * magnitude


def g1_bound(ref):
    """(T + 8) U magnitude: T fma terms, the seven roundings that form g (two per weight product pair and the sum), one of slack"""
    return (ref["T"] + 8) * U * ref["g1_mag"]


def g2_bound(ref):
    """(K + 8) U magnitude per target pixel: K atomic additions in any order, the seven roundings of g and the product g f1"""
    return (ref["K"].unsqueeze(-1) + 8) * U * ref["g2_mag"]


def zero_share(magnitude):
    return float((magnitude == 0).double().mean())


def assert_within(got, want, bound, label):
    """every element of got within `bound` of `want` (NaN fails; a zero bound demands +-0 exactly); prints and returns the worst
    error / bound"""
    got, want, bound = _t(got), _t(want), _t(bound)
    assert got.shape == want.shape == bound.shape, (label, tuple(got.shape), tuple(want.shape), tuple(bound.shape))
    err = (got - want).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("%s: max err / bound = %.3g, max |err| = %.3g" % (label, worst, float(err.max()) if err.numel() else 0.0))
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements over the bound, worst err / bound = %.3f; first at %s: got %r, ref %r, bound %.3g"
                             % (label, int(bad.sum()), bad.numel(), worst, i, float(got[i]), float(want[i]), float(bound[i])))
    return worst


def exact_want(ref, magnitude, label, bits=8):
    """the fp32 bits a kernel must return on dyadic operands.  Asserts the premise: the reference is representable in fp32 and
    magnitude 2^bits < 2^24, so that every partial sum (a multiple of 2^-bits bounded by the magnitude) is exact in fp32 in any order"""
    ref, magnitude = _t(ref), _t(magnitude)
    want = ref.float()
    assert bool((want.double() == ref).all()), "%s: the reference is not representable in fp32" % label
    assert bool((ref * 2.0 ** bits == (ref * 2.0 ** bits).round()).all()), "%s: the operands are not dyadic" % label
    assert float(magnitude.max()) * 2.0 ** bits < 2.0 ** 24 if magnitude.numel() else True, "%s: partial sums may round" % label
    return want


def assert_equal(got, want, label):
    """bit for bit (+0 and -0 are the same exact value), and says which element is wrong"""
    got = got.detach().cpu() if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape, (label, got.dtype, tuple(got.shape), tuple(want.shape))
    bad = got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)
    bad &= ~((got == 0) & (want == 0))
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r" % (label, int(bad.sum()), bad.numel(), i, float(got[i]), float(want[i])))


# ------------------------------------------------------------------------------------------------ fp32 stand-ins and their mutations
def _standin_window(f2, coords, r, mutation):
    """the (2r+2)^2 tap window of every (b, s, pixel) as the kernels form it: (inside, row index into f2.reshape(-1, C), dx, dy)"""
    B, S, H1, W1, _ = coords.shape
    _, H2, W2, _ = f2.shape
    if mutation == "sample0":
        coords = np.broadcast_to(coords[:, :1], coords.shape)
    cx, cy = coords[..., 0], coords[..., 1]
    dx, dy = cx - np.floor(cx), cy - np.floor(cy)
    if mutation == "swapd":
        dx, dy = dy, dx
    to_int = np.trunc if mutation == "trunc" else np.floor
    x0 = np.clip(to_int(cx), -2.0 ** 30, 2.0 ** 30).astype(np.int64) - r
    y0 = np.clip(to_int(cy), -2.0 ** 30, 2.0 ** 30).astype(np.int64) - r
    t = np.arange(2 * r + 2)
    h2 = y0[..., None, None] + t[:, None]                                     # [B,S,H1,W1,iy,ix]
    w2 = x0[..., None, None] + t[None, :]
    over = 1 if mutation == "border" else 0
    ok = (h2 >= 0) & (h2 < H2 + over) & (w2 >= 0) & (w2 < W2 + over)
    b = (np.arange(B) + (1 if mutation == "batch" else 0)) % B
    row = (b[:, None, None, None, None, None] * H2 + h2) * W2 + w2
    row = np.where(ok, row % max(B * H2 * W2, 1), 0)                          # (the off-by-one guard reads the next row of memory)
    assert dx.dtype == dy.dtype == np.float32
    return ok, row, dx, dy


def standin(f1, f2, coords, r, mutation=None):
    """pvo_altcorr_forward in plain fp32 numpy, in the kernels' order (channel chain, then the four weighted taps; fma-free), or one of
    the ways such a kernel goes wrong:
      dropk    the last channel is lost            batch    fmap2 of the wrong batch entry
      border   right and bottom guards off by one  sample0  every sample uses sample 0's coordinates
      trunc    truncation instead of floor         swapd    dx and dy exchanged
      chan     channel ix + rd iy"""
    assert mutation is None or mutation in FORWARD_MUTATIONS, mutation
    f1, f2, coords = (np.ascontiguousarray(a, np.float32) for a in (f1, f2, coords))
    B, S, H1, W1, _ = coords.shape
    C, rd = f1.shape[-1], 2 * r + 1
    if f2.shape[1] * f2.shape[2] == 0:
        return np.zeros((B, S, rd * rd, H1, W1), np.float32)
    ok, row, dx, dy = _standin_window(f2, coords, r, mutation)
    rows = f2.reshape(-1, C)[row]                                             # [B,S,H1,W1,iy,ix,C]
    a = f1[:, None, :, :, None, None, :]
    s = np.zeros(ok.shape, np.float32)
    for k in range(C - 1 if mutation == "dropk" else C):
        s = s + a[..., k] * rows[..., k]
    s = np.where(ok, s, np.float32(0))
    one = np.float32(1)
    w = lambda v: v[..., None, None]
    o = s[..., :rd, :rd] * w((one - dy) * (one - dx))
    o = o + s[..., :rd, 1:] * w((one - dy) * dx)
    o = o + s[..., 1:, :rd] * w(dy * (one - dx))
    o = o + s[..., 1:, 1:] * w(dy * dx)                                        # [B,S,H1,W1,iy,ix]
    o = o.transpose(0, 1, 4, 5, 2, 3) if mutation == "chan" else o.transpose(0, 1, 5, 4, 2, 3)
    assert o.dtype == np.float32
    return np.ascontiguousarray(o).reshape(B, S, rd * rd, H1, W1)


def standin_backward(f1, f2, coords, grad, r, mutation=None):
    """pvo_altcorr_backward in plain fp32 numpy -> (g1, g2): per tap the scalar g from its four cells, g1 a chain over samples and taps,
    g2 added tap by tap onto a zeroed buffer.  The forward's mutations, and:
      tail     channels at or beyond 64 (C // 64) are lost    corner  tap (rd, rd) skipped
      dirty    fmap2_grad accumulated onto a buffer that was not zeroed"""
    assert mutation is None or mutation in BACKWARD_MUTATIONS, mutation
    f1, f2, coords, grad = (np.ascontiguousarray(a, np.float32) for a in (f1, f2, coords, grad))
    B, S, H1, W1, _ = coords.shape
    C, rd = f1.shape[-1], 2 * r + 1
    g1 = np.zeros_like(f1)
    g2 = np.full((max(f2.shape[0] * f2.shape[1] * f2.shape[2], 1), C), 1 if mutation == "dirty" else 0, np.float32)
    if f2.shape[1] * f2.shape[2] == 0:
        return g1, np.zeros_like(f2)
    ok, row, dx, dy = _standin_window(f2, coords, r, mutation)
    if mutation == "corner":
        ok = ok.copy()
        ok[..., rd, rd] = False
    cell = grad.reshape(B, S, rd, rd, H1, W1)
    cell = cell.transpose(0, 1, 4, 5, 2, 3) if mutation == "chan" else cell.transpose(0, 1, 4, 5, 3, 2)     # [B,S,H1,W1,iy,ix]
    P = np.zeros((B, S, H1, W1, rd + 2, rd + 2), np.float32)                  # P[iy + 1, ix + 1] = cell (iy, ix); zeros around it
    P[..., 1:rd + 1, 1:rd + 1] = cell
    one = np.float32(1)
    w = lambda v: v[..., None, None]
    g = P[..., :rd + 1, :rd + 1] * w(dy) * w(dx)
    g = g + P[..., :rd + 1, 1:] * w(dy) * w(one - dx)
    g = g + P[..., 1:, :rd + 1] * w(one - dy) * w(dx)
    g = g + P[..., 1:, 1:] * w(one - dy) * w(one - dx)
    keep = np.ones(C, bool)
    if mutation == "dropk":
        keep[C - 1] = False
    if mutation == "tail":
        keep[64 * (C // 64):] = False
    f2rows = f2.reshape(-1, C)
    for n in range(S):
        for iy in range(rd + 1):
            for ix in range(rd + 1):
                m = ok[:, n, :, :, iy, ix]
                gt, rt = g[:, n, :, :, iy, ix, None], row[:, n, :, :, iy, ix]
                g1 = g1 + np.where(m[..., None] & keep, gt * f2rows[rt], np.float32(0))
                np.add.at(g2, rt[m], (np.where(keep, gt * f1, np.float32(0)))[m])
    assert g1.dtype == g2.dtype == np.float32
    return g1, g2[:f2.shape[0] * f2.shape[1] * f2.shape[2]].reshape(f2.shape)


# ------------------------------------------------------------------------------------------------ shared evaluations
_cache = {}


def reference(cfg, exact=False):
    """dict(f1, f2, coords, grad [float32 numpy], value, magnitude, bwd) of a case, computed once and shared (do not modify)"""
    key = (tuple(cfg), bool(exact))
    if key not in _cache:
        f1, f2, coords, grad = (exact_inputs if exact else inputs)(cfg)
        value, magnitude = forward(f1, f2, coords, cfg[7])
        _cache[key] = dict(f1=f1, f2=f2, coords=coords, grad=grad, value=value, magnitude=magnitude, bwd=backward(f1, f2, coords, grad, cfg[7]))
    return _cache[key]


# ------------------------------------------------------------------------------------------------ AltCorrBlock
BLOCK_MAPS = [(11, 19), (16, 24)]          # odd maps whose pooled levels floor (5 x 9, 2 x 4, 1 x 2), and the suite's even shape
BLOCK_FRAMES, BLOCK_CHANNELS = 4, 128
# (frames in the block, ii, jj): a repeated source and two self edges; the stereo block [left | right] of 2 x 4 frames, where the
# self edge (i, i) looks up frame i + 4, exactly the index list FactorGraph.update_lowmem builds
BLOCK_EDGES = {"mono": (4, [0, 0, 1, 2, 3, 2], [1, 2, 1, 3, 0, 2]),
               "stereo": (8, [0, 0, 1, 2, 3, 3], [1, 2, 1 + 4, 0, 3 + 4, 2])}


def block_inputs(frames, H, W, E, S, exact=False):
    """(fmaps [1,frames,C,H,W] float32, coords [1,E,H,W,2] (S == 0) or [1,E,H,W,S,2]): the kernel cases' generators on same-size maps,
    specials included;
    exact: integer features in [-3, 3] (the block divides by 4) and coordinates on the half grid (level 3 then samples at eighths)"""
    s = max(S, 1)
    g = np.random.default_rng([2030, frames, H, W, E, S, int(exact)])
    if exact:
        fmaps = g.integers(-3, 4, (1, frames, BLOCK_CHANNELS, H, W)).astype(np.float32)
        coords = (_grid(H, W, H, W)[None, None] + g.integers(-8, 9, (E, s, H, W, 2)) / 2).astype(np.float32)
    else:
        fmaps = g.standard_normal((1, frames, BLOCK_CHANNELS, H, W)).astype(np.float32)
        # rounded to multiples of 2^-16 (3e9 is one): x / 2^l - floor is then exact in fp32 at all four levels, which the forward bound
        # presumes.  A coordinate just below 0 with finer bits has 1 + x rounded (by up to 2^-25), which the weight 1 - dx = -x magnifies
        # without limit relative to itself; the pooled levels divide coordinates towards 0, so free jitter meets that at every run
        coords = (np.round(inputs((E, s, H, W, H, W, 1, 3))[2].astype(np.float64) * 2.0 ** 16) / 2.0 ** 16).astype(np.float32)
    coords = torch.from_numpy(coords).permute(0, 2, 3, 1, 4)[None]            # [1,E,H,W,S,2]
    return torch.from_numpy(fmaps), (coords.squeeze(-2) if S == 0 else coords).contiguous()


def pooled_mean(level):
    """the 2 x 2 mean (stride 2, floor) of a stored level [B,N,H,W,C], fp64"""
    x = _t(level)
    H, W = x.shape[2] // 2, x.shape[3] // 2
    x = x[:, :, :2 * H, :2 * W]
    return (x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2] + x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2]) / 4


def block_gradient(fmaps, coords, ii, jj, weight, r=3, num_levels=4):
    """d <weight, AltCorrBlock(fmaps)(coords, ii, jj)> / d fmaps by fp64 autograd of a pure-torch formulation (divide by 4, 2 x 2 mean
    pyramid, explicit volume per edge and level, bilinear window), and the same gradient over |fmaps|, |weight| (the magnitude)"""
    coords = coords.detach().cpu().float()
    if coords.dim() == 5:
        coords, weight = coords.unsqueeze(-2), weight.unsqueeze(-1)
    B, E, H, W, S, _ = coords.shape
    assert B == 1
    c = coords.permute(0, 1, 4, 2, 3, 5).reshape(E, S, H, W, 2)
    ii, jj = torch.as_tensor(ii).long(), torch.as_tensor(jj).long()
    grads = []
    for x, w in ((_t(fmaps), _t(weight)), (_t(fmaps).abs(), _t(weight).abs())):
        x = x.clone().requires_grad_(True)
        f = f0 = x[0] / 4.0                                                    # [N,C,H,W]
        total = 0.0
        for l in range(num_levels):
            vol = torch.einsum("echw,ecyx->ehwyx", f0[ii], f[jj])
            out = sample(vol, c / 2 ** l, r)                                   # [E,S,49,H,W]
            total = total + (out.permute(0, 2, 3, 4, 1)[None] * w[:, :, 49 * l:49 * (l + 1)]).sum()
            if l + 1 < num_levels:
                f = torch.nn.functional.avg_pool2d(f, 2, stride=2)
        total.backward()
        grads.append(x.grad)
    return grads[0], grads[1]
