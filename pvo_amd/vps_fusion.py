"""The VO -> VPS link: the odometry's flow and depth carry the previous frame's feature pyramid into the current frame, and one
convolution fuses it with the current frame's features - the paper's "VO-enhanced VPS" input, which the reference builds on the host
(VPS_Module/detectron2/modeling/meta_arch/panoptic_fpn.py:199-210,310-431: numpy index arrays, a dict sorted by depth, an indexed
assignment per pyramid level).  Here everything stays on the device: droid_backends.feature_transport (include/pvo_hip.h
pvo_feature_transport) followed by droid_backends.conv3x3.

    FeatureFusion(C)            the module a panoptic network calls in place of flow_transport_feature[_with_depth] + fusion_module
    from_graph(graph, e, ...)   flow, disparity key and scales of one factor-graph edge, without a file or a host round trip
    transport_labels(l, src)    an int32 label plane carried through a level's src: panoptic ids for a frame that has none

The panoptic network itself (backbone, heads, trackers) is not part of this library."""
import torch

from . import droid_backends as db

_I64_MAX = (1 << 63) - 1


def _axis(n_in, n_out, dev):
    f32 = torch.float32
    idx = torch.arange(n_out, device=dev)
    r = (torch.tensor(float(n_in - 1), dtype=f32, device=dev) / torch.tensor(float(n_out - 1), dtype=f32, device=dev)) if n_out > 1 \
        else torch.zeros((), dtype=f32, device=dev)
    p = r * idx.to(f32)
    i0 = torch.clamp(p.to(torch.int64), max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l = p - i0.to(f32)
    return i0, i1, l, 1.0 - l


def _bilinear(A, H, W):
    """the contract's resize of A [Ha,Wa] float32 onto an H x W grid, every operation rounded on its own"""
    y0, y1, ly, hy = [v[:, None] for v in _axis(A.shape[0], H, A.device)]
    x0, x1, lx, hx = [v[None, :] for v in _axis(A.shape[1], W, A.device)]
    top = hx * A[y0, x0] + lx * A[y0, x1]
    bot = hx * A[y1, x0] + lx * A[y1, x1]
    return hy * top + ly * bot


def transport_torch(ref_feats, cur_feats, flow, scales=None, depth=None, order=1, rel_pose=None, intrinsics=None, alpha=1.0,
                    mode="nearest"):
    """pvo_feature_transport's contract in plain torch operations (any device, any float dtype): what FeatureFusion runs where the
    native call does not apply.  Same arguments and results as droid_backends.feature_transport."""
    f32 = torch.float32
    dev = flow.device
    if rel_pose is not None:
        rel = rel_pose.reshape(12)
        fx, fy, cx, cy = intrinsics.reshape(4).unbind(0)
        u = torch.arange(depth.shape[1], device=dev).to(f32)[None, :]
        v = torch.arange(depth.shape[0], device=dev).to(f32)[:, None]
        X = (u - cx) / fx * depth
        Y = (v - cy) / fy * depth
        depth = ((rel[8] * X + rel[9] * Y) + rel[10] * depth) + rel[11]
    outs, srcs = [], []
    for l, ref in enumerate(ref_feats):
        _, C, H, W = ref.shape
        sx, sy = (1.0, 1.0) if scales is None else scales[l]
        fx_, fy_ = _bilinear(flow[..., 0], H, W), _bilinear(flow[..., 1], H, W)
        x = torch.arange(W, device=dev).to(f32)[None, :].expand(H, W)
        y = torch.arange(H, device=dev).to(f32)[:, None].expand(H, W)
        keep = torch.isfinite(fx_) & torch.isfinite(fy_)
        if mode == "nearest":
            rx = torch.floor((x + fx_ * torch.tensor(sx, dtype=f32, device=dev)) + 0.5)
            ry = torch.floor((y + fy_ * torch.tensor(sy, dtype=f32, device=dev)) + 0.5)
        else:
            qx, qy = torch.trunc(fx_), torch.trunc(fy_)
            keep &= ~((qx <= -1) | (qy <= -1) | (fx_.abs() >= 32768) | (fy_.abs() >= 32768))
            rx, ry = x + qx, y + qy
        keep &= (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
        hi = torch.zeros(H, W, dtype=torch.int64, device=dev)
        if depth is not None:
            d = _bilinear(depth, H, W)
            keep &= torch.isfinite(d) & (d > 0)
            bits = d.contiguous().view(torch.int32).to(torch.int64)          # positive floats order as their bits
            hi = bits if order > 0 else 0x7FFFFFFF - bits
        s = torch.arange(H * W, device=dev)
        key = (hi.reshape(-1) << 32) | (0xFFFFFFFF - s)                       # the smallest key first, ties to the largest s
        keep = keep.reshape(-1)
        t = (ry.reshape(-1).clamp(0, max(H - 1, 0)).to(torch.int64) * W + rx.reshape(-1).clamp(0, max(W - 1, 0)).to(torch.int64))
        best = torch.full((H * W,), _I64_MAX, dtype=torch.int64, device=dev)
        best.scatter_reduce_(0, t[keep], key[keep], "amin", include_self=True)
        src = torch.where(best == _I64_MAX, torch.full_like(best, -1), 0xFFFFFFFF - (best & 0xFFFFFFFF))
        rows = ref[0].permute(1, 2, 0).reshape(H * W, C)
        moved = rows[src.clamp(min=0)]
        if alpha != 1.0:
            moved = (moved.to(f32) * alpha).to(ref.dtype)
        moved = torch.where((src >= 0)[:, None], moved, torch.zeros_like(moved)).reshape(1, H, W, C)
        cur = None if cur_feats is None else cur_feats[l]
        if cur is not None:
            moved = torch.cat([cur.permute(0, 2, 3, 1), moved], dim=3)
        outs.append(moved.permute(0, 3, 1, 2))
        srcs.append(src.to(torch.int32).reshape(H, W))
    return outs, srcs


class FeatureFusion(torch.nn.Module):
    """[cur | alpha * transported] -> C channels through one 3x3 convolution.  `fusion_conv1` is the reference's name
    (panoptic_fpn.py:410-414), so its checkpoint key loads.  On a GPU, with 16-bit channels-last features and C % 128 == 0, the forward
    is the native transport followed by the native convolution (inference; the weights are packed once per dtype - call
    `repack()` after loading new ones); otherwise a plain torch formulation of the same contract."""

    def __init__(self, channels=256, alpha=1.0, mode="nearest"):
        super().__init__()
        self.channels, self.alpha, self.mode = int(channels), float(alpha), mode
        self.fusion_conv1 = torch.nn.Conv2d(2 * self.channels, self.channels, 3, padding=1)
        self._packed = {}

    def repack(self):
        self._packed = {}

    def _native(self, feats, flow):
        t = feats[0]
        return flow.is_cuda and t.is_cuda and t.dtype in (torch.float16, torch.bfloat16) and self.channels % 128 == 0 and \
            len(feats) <= 8 and all(f.dim() == 4 and f.is_contiguous(memory_format=torch.channels_last) for f in feats)

    def _weights(self, dtype, dev):
        key = (dtype, dev)
        if key not in self._packed:
            w = db.conv3x3_weights(self.fusion_conv1.weight.to(dev), dtype)
            self._packed[key] = (w, self.fusion_conv1.bias.detach().to(dev, torch.float32).contiguous())
        return self._packed[key]

    def forward(self, ref_feats, cur_feats, flow, depth=None, scales=None, order=1, rel_pose=None, intrinsics=None):
        """ref_feats, cur_feats: dicts of [1,C,H,W] under the same keys (a pyramid's levels); the rest as
        droid_backends.feature_transport (scales: a dict under the same keys, or a list in their order).  Returns a dict of [1,C,H,W]."""
        names = list(ref_feats)
        ref, cur = [ref_feats[k] for k in names], [cur_feats[k] for k in names]
        if isinstance(scales, dict):
            scales = [scales[k] for k in names]
        kw = dict(scales=scales, depth=depth, order=order, rel_pose=rel_pose, intrinsics=intrinsics, alpha=self.alpha, mode=self.mode)
        if self._native(ref + cur, flow):
            with torch.no_grad():
                fused, _ = db.feature_transport(ref, cur, flow, **kw)
                w, b = self._weights(ref[0].dtype, ref[0].device)
                return {k: db.conv3x3(x, w, b) for k, x in zip(names, fused)}
        fused, _ = transport_torch(ref, cur, flow, **kw)
        return {k: self.fusion_conv1(x) for k, x in zip(names, fused)}


def from_graph(graph, e, level_shapes):
    """The transport's operands from one edge of a factor graph, device tensors only (the VO -> VPS path without a file): the flow of
    edge e (graph.full_flow[0, e], in 1/8-resolution pixels, from frame ii[e] to frame jj[e]), the source keyframe's inverse depth as the
    key with order = -1 (the larger disparity is the nearer surface), and per level (H_l, W_l) the scales (W_l / wd, H_l / ht).
    Returns the keyword arguments of droid_backends.feature_transport / FeatureFusion.forward."""
    ht, wd = graph.ht, graph.wd
    flow = graph.full_flow[0, e].contiguous()
    disp = torch.index_select(graph.video.disps, 0, graph.ii[e:e + 1])[0].contiguous()       # (an index on the device: no synchronisation)
    return dict(flow=flow, depth=disp, order=-1, scales=[(W / wd, H / ht) for H, W in level_shapes])


def transport_labels(labels, src):
    """labels int32 [H,W] of the reference frame carried through src int32 [H,W] (a level's winners): labels[src] where a cell was
    reached, 0 where src is -1"""
    if labels.dtype != torch.int32 or src.dtype != torch.int32 or labels.shape != src.shape:
        raise ValueError("transport_labels: labels and src must be int32 tensors of one shape")
    flat = labels.reshape(-1)
    got = flat[src.reshape(-1).clamp(min=0).long()]
    return torch.where(src.reshape(-1) >= 0, got, torch.zeros_like(got)).reshape(src.shape)
