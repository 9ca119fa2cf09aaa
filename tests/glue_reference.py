"""The graph glue's yardstick (tests/test_glue_fp64_host.py, tests/test_glue_fp64_gpu.py): pvo_graph_motion (and the motion half of
pvo_reproject_motion), pvo_graph_post and pvo_segment_hist (pvo_amd/csrc/graph_glue.hip, graph_post.h, operator_small.hip) restated in
numpy.  Everything starts from the SAME 16-bit head values the kernel reads (decoded to fp32, which is exact).

What is held to equality, and why it can be:
  motion      every feature is one or two IEEE fp32 additions / subtractions of fp32 inputs (t - x0, (t - x0) + dd, t - c1), a clamp to
              +-64 and ONE round-to-nearest-even to fp16 / bf16: numpy fp32 does the same operations, so the 16-bit patterns are equal
  raw_mask    raw + delta_mask, one fp32 addition                       target, target_ba   coords1 + delta, one fp32 addition
  delta_dy    delta_dy_raw * (1 - bin): the raw value or a zero         full_flow           (coords1 + delta_dy) - coords0, two fp32 ops
  the vote    dyn / max(tot, 1) > thresh: one correctly rounded fp32 division of two small integers
  segment_hist  integer counts
"Equal" means equal as numbers (a product with the zero of 1 - bin may be -0).

What carries a bound: weight = 1 / (1 + expf(-x)) with x = w + 10 (1 - bin) (one fp32 addition, restated exactly), against the fp64
sigmoid s of that same x.  expf is documented to 1 ulp (EXPF_ULP; 1 ulp <= 2 EPS relative, EPS = 2^-24), the sum 1 + e and the division
round once each:  e' = e (1 + 2 EXPF_ULP EPS),  ds = s^2 e 2 EXPF_ULP EPS + 2 EPS s = EPS s (2 EXPF_ULP (1 - s) + 2),
plus TINY = 2^-126 for a result below the smallest normal, which may be flushed.  The same bound serves the static / dynamic decision
sigmoid(raw_mask') >= dy_thresh: it is SETTLED when |s - dy_thresh| exceeds the bound.  raw_mask' == 0 is settled as well: expf(-0) is
exactly 1, 1 + 1 and 1 / 2 are exact, so the kernel's sigmoid is exactly 0.5 and the decision is 0.5 >= dy_thresh.
delta_dy, weight and full_flow of a pixel are compared only where its two decisions are settled (or the vote forces the segment, which
settles both); raw_mask, target and target_ba everywhere."""
import numpy as np

EPS = 2.0 ** -24
EXPF_ULP = 1.0
TINY = 2.0 ** -126
UNSETTLED_CAP = 0.01
MUTANTS = ("bin_swapped", "no_plus10", "flow_from_target", "vote_seg0")

# (E, H, W): E*HW = 105 and HW = 35 - a wave straddles two edges, nothing is a multiple of 64; 522 = 2 * 256 + 10; 320 = 5 * 64
SHAPES = ((3, 5, 7), (2, 9, 29), (5, 8, 8))
SEGMENTS = (1, 2, 16, 70)
DY_THRESH = (0.3, 0.5, 0.7)


def to_bits(x, bf16):
    """fp32 -> the 16-bit pattern, round to nearest even"""
    x = np.ascontiguousarray(x, np.float32)
    if not bf16:
        return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bits(b, bf16):
    b = np.ascontiguousarray(b, np.uint16)
    return b.view(np.float16).astype(np.float32) if not bf16 else (b.astype(np.uint32) << 16).view(np.float32)


def _grid(H, W):
    y, x = np.divmod(np.arange(H * W), W)
    return x.astype(np.float32).reshape(H, W), y.astype(np.float32).reshape(H, W)


def motion(target, coords1, delta_dy, raw_mask, bf16, clamp=64.0):
    """[E,H,W,2] fp32 each -> uint16 [E,H,W,8]: clamp(t - c0 | t - c0 + dd | t - c1 | raw_mask, +-64) rounded once"""
    t, c1, dd, m = [np.asarray(a, np.float32).reshape(-1, *np.asarray(a).shape[-3:]) for a in (target, coords1, delta_dy, raw_mask)]
    x0, y0 = _grid(t.shape[1], t.shape[2])
    c0 = np.stack([x0, y0], -1)[None]
    a = t - c0
    f = np.concatenate([a, a + dd, t - c1, m], -1).astype(np.float32)
    lim = np.float32(clamp)
    return to_bits(np.minimum(np.maximum(f, -lim), lim), bf16)


def sigmoid(x):
    """(fp64 sigmoid of the fp32 x, bound on the kernel's fp32 sigmoid)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
    return s, EPS * s * (2.0 * EXPF_ULP * (1.0 - s) + 2.0) + TINY


def decide(x, thresh):
    """static (True) / dynamic of the updated mask logit x (fp32) -> (decision, settled)"""
    s, e = sigmoid(x)
    t = np.float64(np.float32(thresh))
    zero = np.asarray(x) == 0
    return np.where(zero, 0.5 >= t, s >= t), zero | (np.abs(s - t) > e)


def segment_hist(segm, raw_mask, heads, S, dy_thresh):
    """segm int [E,H,W], raw_mask fp32 [E,H,W,2] (before the update), heads fp32 [E,H,W,8] (the decoded 16-bit values) ->
    tot, dyn int32 [E,S], settled bool [E,H,W]; ids < 0 count as 0, ids >= S as S - 1"""
    segm = np.clip(np.asarray(segm, np.int64), 0, S - 1)
    E = segm.shape[0]
    rm = (np.asarray(raw_mask, np.float32).reshape(E, *segm.shape[1:], 2) + np.asarray(heads, np.float32)[..., 6:8]).astype(np.float32)
    b, s = decide(rm, dy_thresh)
    d = ~b[..., 0] | ~b[..., 1]
    tot, dyn = np.zeros((E, S), np.int32), np.zeros((E, S), np.int32)
    for e in range(E):
        tot[e] = np.bincount(segm[e].reshape(-1), minlength=S)
        dyn[e] = np.bincount(segm[e].reshape(-1), weights=d[e].reshape(-1), minlength=S).astype(np.int32)
    return tot, dyn, s.all(-1)


def forced(segm, tot, dyn, thresh, S, seg0=False):
    """bool [E,H,W]: the pixel's segment (id != 0) is voted dynamic on its edge: fp32 dyn / max(tot, 1) > thresh"""
    sg = np.clip(np.asarray(segm, np.int64), 0, S - 1)
    E = sg.shape[0]
    frac = np.asarray(dyn, np.float32) / np.maximum(np.asarray(tot, np.float32), np.float32(1.0))
    over = frac > np.float32(thresh)
    f = over[np.arange(E)[:, None, None], sg]
    return f if seg0 else f & (sg != 0)


def post(coords1, heads, raw_mask, dy_thresh, vote=None, mutant=None):
    """coords1, raw_mask fp32 [E,H,W,2], heads fp32 [E,H,W,8] (delta | delta_dy | weight logits | delta_mask),
    vote = (segm [E,H,W], tot, dyn [E,S], thresh) -> dict of the seven outputs (weight / weight_ba in fp64 with weight_bound), and
    settled bool [E,H,W,2]"""
    c1, h, raw = np.asarray(coords1, np.float32), np.asarray(heads, np.float32), np.asarray(raw_mask, np.float32)
    E, H, W, _ = c1.shape
    raw = raw.reshape(E, H, W, 2)
    x0, y0 = _grid(H, W)
    c0 = np.stack([x0, y0], -1)[None]
    rm = (raw + h[..., 6:8]).astype(np.float32)
    b, settled = decide(rm, dy_thresh)
    if vote is not None:
        segm, tot, dyn, vth = vote
        f = forced(segm, tot, dyn, vth, np.asarray(tot).shape[1], seg0=(mutant == "vote_seg0"))[..., None]
        b, settled = b & ~f, settled | f
    one_minus = (b if mutant == "bin_swapped" else ~b).astype(np.float32)          # 1 - bin: 1 where dynamic
    target = (c1 + h[..., 0:2]).astype(np.float32)
    ddy = (h[..., 2:4] * one_minus).astype(np.float32)
    x = h[..., 4:6] if mutant == "no_plus10" else (h[..., 4:6] + one_minus * np.float32(10.0)).astype(np.float32)
    weight, wb = sigmoid(x)
    flow = ((target if mutant == "flow_from_target" else (c1 + ddy).astype(np.float32)) - c0).astype(np.float32)
    ba = lambda a: np.ascontiguousarray(np.moveaxis(a, -1, 1))
    return dict(raw_mask=rm, target=target, delta_dy=ddy, weight=weight, weight_bound=wb, full_flow=flow, target_ba=ba(target),
                weight_ba=ba(weight), settled=settled, static=b)


def check_post(got, ref, cap=UNSETTLED_CAP):
    """got: dict of the kernel's seven outputs ([E,H,W,2], the two BA layouts [E,2,H,W]) -> (ok, dict(worst = max weight err / bound,
    unsettled, mismatches))"""
    s = ref["settled"]
    s_ba = np.moveaxis(s, -1, 1)
    g = {k: np.asarray(v, np.float64).reshape(ref[k].shape) for k, v in got.items()}
    bad = 0
    for k in ("raw_mask", "target", "target_ba"):
        bad += int(np.count_nonzero(g[k] != ref[k]))
    for k in ("delta_dy", "full_flow"):
        bad += int(np.count_nonzero((g[k] != ref[k]) & s))
    worst = 0.0
    for k, m, bound in (("weight", s, ref["weight_bound"]), ("weight_ba", s_ba, np.moveaxis(ref["weight_bound"], -1, 1))):
        ratio = np.abs(g[k] - ref[k]) / bound
        ratio = np.where(np.isnan(ratio), np.inf, ratio)[m]
        if ratio.size:
            worst = max(worst, float(ratio.max()))
        bad += int(np.count_nonzero(ratio > 1.0))
    rep = dict(worst=worst, unsettled=1.0 - float(np.mean(s)) if s.size else 0.0, mismatches=bad)
    return bad == 0 and rep["unsettled"] <= cap, rep


def case(E, H, W, bf16, seed=0, S=16):
    """random inputs for one shape: coords1 near the pixel grid, head values ALREADY ROUNDED to the 16-bit type, a mask logit that the
    update takes to exactly 0 on every 17th pixel, targets and masks that reach both clamps of the motion features, segment ids from
    -2 to S + 1 (S = 70: one id per lane of a wave, 64 ballot rounds).  Returns a dict of numpy arrays."""
    rng = np.random.default_rng(seed + 131 * E + 17 * H + W + (7 if bf16 else 0))
    x0, y0 = _grid(H, W)
    c0 = np.stack([x0, y0], -1)[None]
    coords1 = (c0 + rng.normal(0, 2.0, (E, H, W, 2))).astype(np.float32)
    heads = rng.normal(0, 1.0, (E, H, W, 8)) * np.array([2.0, 2.0, 1.0, 1.0, 3.0, 3.0, 1.0, 1.0])
    heads = from_bits(to_bits(heads.astype(np.float32), bf16), bf16)
    raw = rng.normal(0, 1.5, (E, H, W, 2)).astype(np.float32)
    flat = raw.reshape(-1, 2)
    flat[::17, 0] = -heads.reshape(-1, 8)[::17, 6]
    target = (c0 + rng.normal(0, 40.0, (E, H, W, 2))).astype(np.float32)
    ddy = rng.normal(0, 30.0, (E, H, W, 2)).astype(np.float32)
    raw_motion = rng.normal(0, 40.0, (E, H, W, 2)).astype(np.float32)
    if S == 70:
        segm = (np.arange(E * H * W) % 70).reshape(E, H, W)
    else:
        segm = rng.integers(-2, S + 2, (E, H, W))
    segm = segm.astype(np.int32)
    segm.reshape(-1)[3], segm.reshape(-1)[5] = -3, S + 5
    return dict(coords1=coords1, heads=heads, raw_mask=raw, target=target, delta_dy=ddy, raw_motion=raw_motion, segm=segm)
