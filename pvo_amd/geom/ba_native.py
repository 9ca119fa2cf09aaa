"""Differentiable dense bundle adjustment of the training path in libpvo_hip (pvo_ba_train / pvo_ba_train_vjp).

`BA` has the signature, return values and semantics of `pvo_amd.geom.ba.BA` (the reference's geom/ba.py:31-106 with
geom/chol.py:5-73), which stays the specification and the path for everything outside this one's domain: one Gauss-Newton
step, built as one autograd Function whose forward and backward each run as a handful of HIP kernels
(pvo_amd/csrc/ba_train.hip) with no host synchronisation.  Poses come in and go out as SE3; their gradients are in the 7 ambient
coordinates, as the SE3 operations' own.

Domain: device tensors, all fp32 or all fp64 (the arithmetic, the Cholesky included, is done in that type); rig 1; 0 <= fixedp <= P
with at most 16 free poses (P - fixedp; 0 is a depth-only step); any batch B sharing one ii / jj; per-frame intrinsics [B,P,4]
that do not require grad; ii / jj on the host or on the device.  Anything else raises ValueError - there is no fallback.

The keyframes of the graph (torch.unique(ii)) and the edges of each keyframe form the `plan`; `make_plan` builds it (one host
synchronisation, for the number of keyframes).  A caller that steps the same graph many times - DroidNet.forward's 2 x 15 steps -
builds it once and passes it in.
"""
import torch
from torch.autograd.function import once_differentiable

from .se3 import SE3

MAX_FREE_POSES = 16
_FALLBACK = "; pvo_amd.geom.ba.BA handles it"


def _unsupported(what):
    raise ValueError("pvo_amd.geom.ba_native.BA: " + what + _FALLBACK)


def make_plan(ii, device=None):
    """(kx, kk, kptr, kedge) int32 on ii's device (or `device`): the keyframes in ascending order, each edge's keyframe, and the
    edges of every keyframe in edge order as a CSR (kptr [M+1], kedge [N])"""
    ii = torch.as_tensor(ii, dtype=torch.long, device=device)
    if ii.device.type != "cuda":
        _unsupported("the plan lives on the GPU; got ii on %s" % ii.device)
    kx, kk = torch.unique(ii, return_inverse=True)
    kedge = torch.argsort(kk, stable=True)
    kptr = torch.zeros(kx.shape[0] + 1, dtype=torch.long, device=ii.device)
    kptr[1:] = torch.cumsum(torch.bincount(kk, minlength=kx.shape[0]), 0)
    return tuple(t.to(torch.int32).contiguous() for t in (kx, kk, kptr, kedge))


def check_supported(target, weight, eta, poses, disps, intrinsics, fixedp=1, rig=1):
    """raise ValueError unless these inputs are in the native BA's domain (see the module docstring).  Every condition has a
    message of its own; where the tensors live is checked last, so that the other conditions are checked for host tensors too."""
    if rig != 1:
        _unsupported("rig = %s is not supported (rig 1 only)" % rig)
    pdata = poses.data if isinstance(poses, SE3) else poses
    ts = (target, weight, eta, pdata, disps, intrinsics)
    if not all(isinstance(t, torch.Tensor) for t in ts):
        _unsupported("target, weight, eta, disps, intrinsics must be tensors and poses an SE3")
    if len({t.dtype for t in ts}) != 1 or disps.dtype not in (torch.float32, torch.float64):
        _unsupported("needs all tensors fp32 or all fp64; got %s" % sorted({str(t.dtype) for t in ts}))
    if intrinsics.requires_grad:
        _unsupported("has no intrinsics gradient (intrinsics requires grad)")
    if disps.dim() != 4:
        _unsupported("disps must be [B,P,H,W]")
    B, P, ht, wd = disps.shape
    if pdata.shape != (B, P, 7) or intrinsics.shape != (B, P, 4):
        _unsupported("poses must be [B,P] SE3 and intrinsics [B,P,4] (per-frame)")
    if target.dim() != 5 or target.shape[0] != B or target.shape[2:] != (ht, wd, 2) or weight.shape != target.shape:
        _unsupported("target and weight must be [B,N,H,W,2]")
    if not 0 <= fixedp <= P:
        _unsupported("needs 0 <= fixedp <= P; got P = %d, fixedp = %d" % (P, fixedp))
    if P - fixedp > MAX_FREE_POSES:
        _unsupported("supports at most %d free poses; got P - fixedp = %d" % (MAX_FREE_POSES, P - fixedp))
    if not all(t.is_cuda for t in ts):
        _unsupported("needs device tensors")
    if len({t.device for t in ts}) != 1:
        _unsupported("all tensors must live on one device")


class _BATrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, target, weight, eta, pdata, disps, intrinsics, ii, jj, plan, fixedp):
        from .. import droid_backends as db
        pout, dout, dx, ws = db.ba_train(pdata, disps, intrinsics, target, weight, eta, ii, jj, plan, fixedp)
        ctx.save_for_backward(target, weight, pdata, disps, intrinsics, ii, jj)
        ctx.plan, ctx.fixedp, ctx.ws, ctx.eta_shape = plan, fixedp, ws, eta.shape      # ws: this call's own state
        ctx.mark_non_differentiable(dx)
        return pout, dout, dx

    @staticmethod
    @once_differentiable
    def backward(ctx, g_poses, g_disps, _g_dx):
        from .. import droid_backends as db
        target, weight, pdata, disps, intrinsics, ii, jj = ctx.saved_tensors
        g_poses = torch.zeros_like(pdata) if g_poses is None else g_poses
        g_disps = torch.zeros_like(disps) if g_disps is None else g_disps
        gt, gw, ge, gp, gd = db.ba_train_vjp(pdata, disps, intrinsics, target, weight, ii, jj, ctx.plan, ctx.fixedp, ctx.ws,
                                             g_poses, g_disps)
        return gt, gw, ge.view(ctx.eta_shape), gp, gd, None, None, None, None, None


def step(target, weight, eta, poses, disps, intrinsics, ii, jj, fixedp=1, rig=1, plan=None):
    """`BA` that also returns the pose update dx [B, 6 (P - fixedp)] (zero where the reduced system is not SPD)"""
    check_supported(target, weight, eta, poses, disps, intrinsics, fixedp, rig)
    dev = disps.device
    ii = torch.as_tensor(ii, dtype=torch.long, device=dev).contiguous()
    jj = torch.as_tensor(jj, dtype=torch.long, device=dev).contiguous()
    if plan is None:
        plan = make_plan(ii)
    if jj.shape != ii.shape or ii.shape[0] != target.shape[1]:
        _unsupported("ii and jj must list the N edges of target / weight")
    B, P, ht, wd = disps.shape
    M = plan[0].shape[0]
    if eta.numel() != B * M * ht * wd:
        _unsupported("eta must hold [B, M, H, W] with M = %d keyframes" % M)
    pdata, d, dx = _BATrain.apply(target.contiguous(), weight.contiguous(), eta.reshape(B, M, ht, wd).contiguous(),
                                  poses.data.contiguous(), disps.contiguous(), intrinsics.contiguous(), ii, jj, plan, int(fixedp))
    return SE3(pdata), d, dx


def BA(target, weight, eta, poses, disps, intrinsics, ii, jj, fixedp=1, rig=1, plan=None):
    """One Gauss-Newton step over poses and inverse depths: pvo_amd.geom.ba.BA in libpvo_hip"""
    poses, disps, _ = step(target, weight, eta, poses, disps, intrinsics, ii, jj, fixedp, rig, plan)
    return poses, disps
