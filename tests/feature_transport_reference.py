"""pvo_feature_transport's contract (include/pvo_hip.h) restated in numpy: every fp32 operation of the contract is one np.float32
operation here, rounded on its own, so the native call has to give the same bytes.  Host only; the winner is found by sorting, not
by the library's atomic key, so the two share no construction.

    transport(ref, cur, flow, ...)   lists of [H,W,C] arrays per level -> (outs, srcs)
"""
import os

import numpy as np

F = np.float32
NEAREST, REFERENCE = 0, 1
_golden = {}


def golden(case):
    """one case of tests/golden/feature_transport.npz (what the reference's own methods returned: tests/golden/gen_transport_golden.py)
    as a dict, {} if the generator dropped it"""
    if not _golden:
        with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_transport.npz")) as z:
            _golden.update({k: z[k] for k in z.files})
    pre = case + "/"
    return {k[len(pre):]: v for k, v in _golden.items() if k.startswith(pre)}


def _axis(n_in, n_out, idx):
    """one axis of the align_corners resize: (i0, i1, l, h) for the cells idx of an n_out grid over an n_in map"""
    r = F(n_in - 1) / F(n_out - 1) if n_out > 1 else F(0)
    p = r * idx.astype(F)
    i0 = np.minimum(p.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l = p - i0.astype(F)
    return i0, i1, l, F(1) - l


def bilinear(A, H, W):
    """A [Ha,Wa] float32 -> [H,W]: the contract's resize"""
    A = np.ascontiguousarray(A, dtype=F)
    Ha, Wa = A.shape
    y0, y1, ly, hy = [v[:, None] for v in _axis(Ha, H, np.arange(H))]
    x0, x1, lx, hx = [v[None, :] for v in _axis(Wa, W, np.arange(W))]
    with np.errstate(invalid="ignore", over="ignore"):
        top = hx * A[y0, x0] + lx * A[y0, x1]
        bot = hx * A[y1, x0] + lx * A[y1, x1]
        return (hy * top + ly * bot).astype(F)


def transport_depth(depth, rel_pose, intrinsics):
    """the depth map carried into the current camera, at its own resolution"""
    depth = np.asarray(depth, dtype=F)
    rel = np.asarray(rel_pose, dtype=F).reshape(12)
    fx, fy, cx, cy = [F(v) for v in np.asarray(intrinsics, dtype=F).reshape(4)]
    Hd, Wd = depth.shape
    u = np.arange(Wd).astype(F)[None, :]
    v = np.arange(Hd).astype(F)[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        X = (u - cx) / fx * depth
        Y = (v - cy) / fy * depth
        return (((rel[8] * X + rel[9] * Y) + rel[10] * depth) + rel[11]).astype(F)


def resolve(flow, H, W, sx=1.0, sy=1.0, depth=None, order=1, mode=NEAREST):
    """src int32 [H,W]: the source cell that wins each target cell of one level, or -1"""
    flow = np.asarray(flow, dtype=F)
    fx = bilinear(flow[..., 0], H, W)
    fy = bilinear(flow[..., 1], H, W)
    x = np.broadcast_to(np.arange(W).astype(F)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H).astype(F)[:, None], (H, W))
    keep = np.isfinite(fx) & np.isfinite(fy)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == NEAREST:
            rx = np.floor((x + fx * F(sx)) + F(0.5))
            ry = np.floor((y + fy * F(sy)) + F(0.5))
        else:
            qx, qy = np.trunc(fx), np.trunc(fy)
            keep &= ~((qx <= F(-1)) | (qy <= F(-1)) | (np.abs(fx) >= F(32768)) | (np.abs(fy) >= F(32768)))
            rx, ry = x + qx, y + qy
        keep &= (rx >= 0) & (rx <= F(W - 1)) & (ry >= 0) & (ry <= F(H - 1))
        if depth is not None:
            d = bilinear(depth, H, W)
            keep &= np.isfinite(d) & (d > 0)
        else:
            d = np.zeros((H, W), F)
    src = np.full(H * W, -1, np.int32)
    s = np.flatnonzero(keep.reshape(-1))
    if s.size:
        t = ry.reshape(-1)[s].astype(np.int64) * W + rx.reshape(-1)[s].astype(np.int64)
        key = d.reshape(-1)[s].astype(np.float64) * (1.0 if order > 0 else -1.0)
        # per target: the smallest key first, ties to the largest s
        o = np.lexsort((-s, key, t))
        t, s = t[o], s[o]
        first = np.ones(t.size, bool)
        first[1:] = t[1:] != t[:-1]
        src[t[first]] = s[first]
    return src.reshape(H, W)


def f32_to_bf16_bits(v):
    """round to nearest even (finite inputs and infinities)"""
    b = np.ascontiguousarray(v, dtype=F).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(F)


def gather(ref, cur, src, alpha=1.0, bf16=False):
    """one level's out: [cur | alpha * ref[src]] ([H,W,2C]) or alpha * ref[src] ([H,W,C]).  ref / cur: float16, float32, or uint16
    holding bfloat16 bits with bf16=True; the result has their type"""
    H, W, C = ref.shape
    rows = ref.reshape(H * W, C)
    flat = src.reshape(-1)
    moved = np.zeros_like(rows)
    won = flat >= 0
    moved[won] = rows[flat[won]]
    if F(alpha) != F(1):
        with np.errstate(invalid="ignore", over="ignore"):
            if bf16:
                scaled = f32_to_bf16_bits(bf16_bits_to_f32(moved) * F(alpha))
            else:
                scaled = (moved.astype(F) * F(alpha)).astype(ref.dtype)
        scaled[~won] = 0
        moved = scaled
    moved = moved.reshape(H, W, C)
    return moved if cur is None else np.concatenate([cur, moved], axis=2)


def transport(ref, cur, flow, scales=None, depth=None, order=1, rel_pose=None, intrinsics=None, alpha=1.0, mode=NEAREST, bf16=False):
    """all levels: ref / cur lists of [H,W,C] (cur or its entries may be None); scales a list of (sx, sy).  Returns (outs, srcs)."""
    if rel_pose is not None:
        depth = transport_depth(depth, rel_pose, intrinsics)
    outs, srcs = [], []
    for l, r in enumerate(ref):
        H, W, _ = r.shape
        sx, sy = (1.0, 1.0) if scales is None else scales[l]
        src = resolve(flow, H, W, sx, sy, depth, order, mode) if H * W else np.zeros((H, W), np.int32)
        c = None if cur is None else cur[l]
        outs.append(gather(r, c, src, alpha, bf16))
        srcs.append(src)
    return outs, srcs
