"""Convex 8x upsampling of the training path in libpvo_hip (pvo_cvx_upsample / pvo_cvx_upsample_vjp).

`cvx_upsample`, `upsample_dim_1` and `upsample_dim_x` have the signatures and semantics of the functions of the same names in
`pvo_amd.droid_net` (the reference's droid_net.py:23-54), which stay the specification: one autograd Function whose forward is one
HIP kernel and whose backward is two (pvo_amd/csrc/cvx_upsample.hip).  The backward keeps only `data` and `mask` - the softmax is
recomputed - where the PyTorch chain keeps the softmax, the product and permuted copies of a [B, 576, h, w] tensor per call.

Domain: device tensors, data and mask both fp32 or both fp64, data [B,H,W,D] with D = 1 or 2, mask [B,576,H,W] contiguous or
channels-last.  Anything else raises ValueError - there is no fallback.  Forward and backward are bit-identical from call to call.
"""
import torch
from torch.autograd.function import once_differentiable


def _unsupported(what):
    raise ValueError("pvo_amd.geom.upsample_native: " + what + "; pvo_amd.droid_net.cvx_upsample handles it")


class _CvxUpsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, mask):
        from .. import droid_backends as db
        ctx.save_for_backward(data, mask)
        return db.cvx_upsample(data, mask)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        from .. import droid_backends as db
        data, mask = ctx.saved_tensors
        gmask, gdata = db.cvx_upsample_vjp(data, mask, gout.contiguous())
        return (gdata if ctx.needs_input_grad[0] else None), (gmask if ctx.needs_input_grad[1] else None)


def cvx_upsample(data, mask):
    """droid_net.cvx_upsample(data [B,H,W,D], mask [B,576,H,W]) -> [B,8H,8W,D], differentiable in both"""
    if not (isinstance(data, torch.Tensor) and isinstance(mask, torch.Tensor)):
        _unsupported("data and mask must be tensors")
    if data.dtype != mask.dtype or data.dtype not in (torch.float32, torch.float64):
        _unsupported("needs data and mask both fp32 or both fp64; got %s and %s" % (data.dtype, mask.dtype))
    if data.dim() != 4 or data.shape[-1] not in (1, 2):
        _unsupported("data must be [B,H,W,D] with D = 1 or 2")
    if mask.dim() != 4 or mask.shape[1] != 576 or mask.shape[0] != data.shape[0] or tuple(mask.shape[2:]) != tuple(data.shape[1:3]):
        _unsupported("mask must be [B,576,H,W] for data [B,H,W,D]")
    if not (data.is_cuda and mask.is_cuda):
        _unsupported("needs device tensors")
    if not (mask.is_contiguous() or mask.permute(0, 2, 3, 1).is_contiguous()):
        mask = mask.contiguous()
    return _CvxUpsample.apply(data.contiguous(), mask)


def upsample_dim_1(disp, mask):
    batch, num, ht, wd = disp.shape
    up = cvx_upsample(disp.reshape(batch * num, ht, wd, 1), mask.reshape(batch * num, -1, ht, wd))
    return up.view(batch, num, 8 * ht, 8 * wd)


def upsample_dim_x(flow, mask):
    batch, num, ht, wd, dim = flow.shape
    up = cvx_upsample(flow.reshape(batch * num, ht, wd, dim), mask.reshape(batch * num, -1, ht, wd))
    return up.view(batch, num, 8 * ht, 8 * wd, dim)
