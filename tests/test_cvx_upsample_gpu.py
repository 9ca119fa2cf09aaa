"""Convex 8x upsampling on the device: pvo_cvx_upsample / pvo_cvx_upsample_vjp (pvo_amd/csrc/cvx_upsample.hip) alone, with row tables,
under autograd, inside pvo_graph_update, through a tracked sequence and in DroidNet's training unroll.

The forward bound.  u = 2^-24 (half an ulp of fp32), X = max |data|.  Per output the kernel computes, from logits converted EXACTLY to
fp32, m = max_k l_k, x_k = l_k - m <= 0, e_k = exp(x_k), s = sum_k e_k, acc = sum_k e_k n_k (tap order, n_k the neighbour), out = acc / s.
Every e_k and s is positive, |n_k| <= X, and the true value is sum_k w_k n_k with w_k = exp(x_k) / sum exp(x_j), sum w_k = 1:
  * the subtraction x_k rounds once: |dx_k| <= u |x_k|, which changes exp(x_k) by the factor (1 + |x_k| u).  Weighted by w_k:
    sum_k w_k |x_k| <= sum_{k != max} |x_k| exp(x_k) <= 8 / e < 3 (s >= 1 because the maximum contributes exp(0) = 1) - 3 u in the
    numerator and 3 u in the denominator:                                                                     6 u X
  * exp: the device library's expf is accurate to 1 ulp = 2 u, numerator and denominator:                       4 u X
  * nine products and eight additions of the numerator (no cancellation in |.|: bounded by sum e_k |n_k|):       9 u X
  * eight additions of the denominator:                                                                         8 u X
  * one division, whose rounding is the one rounding on store:                                                  1 u X
  28 u X in first order; C_FWD = 32 leaves the second-order terms room.  The issue's condition is c <= 64; an indexing mistake (a tap
  rotated, dy / dx transposed) costs 1.7-2.2 absolute on these inputs, seven orders above 32 u X = 4.2e-6.
The same derivation with u = 2^-53 bounds the fp64 kernel (exp there: the library's 1 ulp as well)."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C_FWD = 32.0
U32, U64 = 2.0 ** -24, 2.0 ** -53
SIZES = [(8, 48, 64), (26, 30, 101), (6, 25, 50), (2, 11, 19), (1, 1, 1), (3, 47, 156)]
SCALES = [1.0, 4.0, 8.0, 20.0]
GOLD = os.path.join(os.path.dirname(__file__), "golden", "droidnet_forward.npz")


def _spec64(data, mask):
    """droid_net.cvx_upsample evaluated in fp64 on the operands as they are stored"""
    from pvo_amd.droid_net import cvx_upsample
    return cvx_upsample(data.double(), mask.double().contiguous())


def _operands(dev, B, H, W, D, scale, dtype, layout, seed):
    g = torch.Generator().manual_seed(seed)
    data = (torch.rand(B, H, W, D, generator=g) * 2.0 + 0.2).to(dev)                     # [0.2, 2.2]
    mask = (torch.randn(B, 576, H, W, generator=g) * scale).to(dev).to(dtype)            # rounded to the storage type: the operand
    if layout == "channels_last":
        mask = mask.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return data, mask


def _neighbours(data):
    """the nine zero-padded neighbours [B,9,H,W,D] by slicing a padded copy (not F.unfold: an independent formulation)"""
    B, H, W, D = data.shape
    pad = torch.zeros(B, H + 2, W + 2, D, dtype=data.dtype, device=data.device)
    pad[:, 1:-1, 1:-1] = data
    return torch.stack([pad[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], 1)


def _fine(t):
    """[B,H,W,D] per coarse pixel -> [B,8H,8W,D] per fine pixel"""
    return t.repeat_interleave(8, 1).repeat_interleave(8, 2)


@pytest.mark.parametrize("layout", ["planar", "channels_last"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_forward_within_the_derived_bound_of_the_fp64_evaluation(cuda, dtype, layout):
    from pvo_amd import droid_backends as db
    worst = 0.0
    for n, (B, H, W) in enumerate(SIZES):
        for D in (1, 2):
            for scale in SCALES:
                data, mask = _operands(cuda, B, H, W, D, scale, dtype, layout, seed=1000 * n + 10 * D + int(scale))
                out = db.cvx_upsample(data, mask)
                assert out.shape == (B, 8 * H, 8 * W, D) and out.dtype == torch.float32
                ref = _spec64(data, mask)
                X = float(data.abs().max())
                err = float((out.double() - ref).abs().max())
                worst = max(worst, err / (U32 * X))
                print("%s %s %dx%dx%d D=%d scale %g: max error %.3e = %.2f u X (bound %.0f)" % (dtype, layout, B, H, W, D, scale, err, err / (U32 * X), C_FWD))
                assert err <= C_FWD * U32 * X, (dtype, layout, B, H, W, D, scale, err / (U32 * X))
                # every output inside [min, max] of its nine zero-padded neighbours
                nb = _neighbours(data.double())
                lo, hi = _fine(nb.min(1).values), _fine(nb.max(1).values)
                assert bool(((out.double() >= lo - C_FWD * U32 * X) & (out.double() <= hi + C_FWD * U32 * X)).all())
    print("worst case over all sizes: %.2f u X" % worst)


def test_forward_fp64_operands(cuda):
    from pvo_amd import droid_backends as db
    for layout in ("planar", "channels_last"):
        for D in (1, 2):
            data, mask = _operands(cuda, 2, 11, 19, D, 4.0, torch.float64, layout, seed=5 + D)
            data = data.double()
            out = db.cvx_upsample(data, mask)
            err = float((out - _spec64(data, mask)).abs().max())
            print("fp64 %s D=%d: %.3e = %.2f u64 X" % (layout, D, err, err / (U64 * float(data.abs().max()))))
            assert out.dtype == torch.float64 and err <= C_FWD * U64 * float(data.abs().max())


@pytest.mark.parametrize("layout", ["planar", "channels_last"])
def test_reference_fixture_constant_field_and_zero_padded_border(cuda, layout):
    from pvo_amd import droid_backends as db
    cl = (lambda m: m.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)) if layout == "channels_last" else (lambda m: m)
    z = np.load(GOLD)
    data, mask = torch.from_numpy(z["cvx_data"]).to(cuda), cl(torch.from_numpy(z["cvx_mask"]).to(cuda))
    assert data.shape[-1] == 3                                  # the fixture's field has three channels, the kernel takes one or two: in two calls
    for sl in (slice(0, 2), slice(2, 3)):
        up = db.cvx_upsample(data[..., sl].contiguous(), mask)
        assert torch.allclose(up.cpu(), torch.from_numpy(z["cvx_up"])[..., sl], atol=1e-6)    # as tests/test_droidnet.py holds the PyTorch form
    # a constant field stays constant in the interior
    g = torch.Generator().manual_seed(3)
    for D in (1, 2):
        const = torch.full((2, 11, 19, D), 2.5, device=cuda)
        m = cl((torch.randn(2, 576, 11, 19, generator=g) * 8).to(cuda).half())
        c = db.cvx_upsample(const, m)
        assert float((c[:, 8:-8, 8:-8] - 2.5).abs().max()) <= C_FWD * U32 * 2.5
        assert float(c.min()) >= 0.0 and float(c[:, :8].min()) < 2.4                          # the border mixes in the zero padding
        # border pixels: against an explicit zero-padded evaluation (padded copy, slices, einsum), compared on the border itself
        data, mask = _operands(cuda, 3, 11, 19, D, 4.0, torch.float16, layout, seed=40 + D)
        out = db.cvx_upsample(data, mask).double()
        w = torch.softmax(mask.double().contiguous().view(3, 9, 8, 8, 11, 19), 1)              # [B,k,dy,dx,H,W]
        ref = torch.einsum("bkyxhw,bkhwd->bhywxd", w, _neighbours(data.double())).reshape(3, 88, 152, D)
        border = torch.ones(88, 152, dtype=torch.bool, device=cuda)
        border[8:-8, 8:-8] = False
        err = float((out - ref)[:, border].abs().max())
        print("%s D=%d border error %.3e" % (layout, D, err))
        assert err <= C_FWD * U32 * float(data.abs().max())
        assert float((out - ref).abs().max()) <= C_FWD * U32 * float(data.abs().max())


@pytest.mark.parametrize("layout", ["planar", "channels_last"])
def test_row_tables_update_named_frames_in_place(cuda, layout):
    from pvo_amd import droid_backends as db
    g = torch.Generator().manual_seed(9)
    F, H, W = 64, 30, 101
    rows_in, rows_out = [40, 3, 17, 63, 9, 22], [5, 61, 0, 33, 12, 48]
    K = len(rows_in)
    buf = (torch.rand(F, H, W, 1, generator=g) + 0.2).to(cuda)
    _, mask = _operands(cuda, K, H, W, 1, 4.0, torch.float16, layout, seed=10)
    sentinel = torch.randn(F, 8 * H, 8 * W, 1, generator=g).to(cuda)
    out = sentinel.clone()
    r = db.cvx_upsample(buf, mask, out=out, in_rows=torch.tensor(rows_in, device=cuda), out_rows=torch.tensor(rows_out, device=cuda))
    assert r.data_ptr() == out.data_ptr()
    direct = db.cvx_upsample(buf[rows_in].contiguous(), mask)
    assert torch.equal(out[rows_out], direct)
    rest = [k for k in range(F) if k not in rows_out]
    assert torch.equal(out[rest], sentinel[rest])                                             # bit for bit untouched
    out2 = sentinel.clone()
    db.cvx_upsample(buf, mask, out=out2, in_rows=rows_in, out_rows=rows_out)                  # host sequences: the same call
    assert torch.equal(out, out2)
    # in place on the same frames, as DepthVideo.upsample uses it
    out3 = sentinel.clone()
    db.cvx_upsample(buf, mask, out=out3, in_rows=rows_in, out_rows=rows_in)
    assert torch.equal(out3[rows_in], direct) and torch.equal(out3[[k for k in range(F) if k not in rows_in]], sentinel[[k for k in range(F) if k not in rows_in]])
    with pytest.raises(db.PvoHipError):
        db.cvx_upsample(buf, mask, out=out3, in_rows=[0, 1, 2, 3, 4, F], out_rows=rows_in)   # a row outside the buffer


@pytest.mark.parametrize("layout", ["planar", "channels_last"])
@pytest.mark.parametrize("D", [1, 2])
def test_gradcheck_fp64(cuda, layout, D):
    from pvo_amd.geom import upsample_native as un
    g = torch.Generator().manual_seed(20 + D)
    data = (torch.rand(2, 5, 7, D, generator=g, dtype=torch.float64) + 0.2).to(cuda).requires_grad_()
    mask = (torch.randn(2, 576, 5, 7, generator=g, dtype=torch.float64) * 2).to(cuda)
    if layout == "channels_last":
        mask = mask.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    mask.requires_grad_()
    assert torch.autograd.gradcheck(un.cvx_upsample, (data, mask), eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=0.0)


@pytest.mark.parametrize("layout", ["planar", "channels_last"])
@pytest.mark.parametrize("D", [1, 2])
def test_backward_fp32_against_fp64_autograd_with_pytorch_fp32_as_the_yardstick(cuda, layout, D):
    """gmask and gdata at 6 x 25x50 against PyTorch autograd of droid_net.cvx_upsample in fp64; the native error, relative to the largest
    gradient magnitude, may be at most 4 x the error of PyTorch's own fp32 autograd on the same operands (both computed here; the factor
    covers another summation order and exp).  Two backward calls are bit-identical."""
    from pvo_amd.droid_net import cvx_upsample
    from pvo_amd.geom import upsample_native as un
    B, H, W = 6, 25, 50
    data, mask = _operands(cuda, B, H, W, D, 4.0, torch.float32, layout, seed=30 + D)
    gout = torch.randn(B, 8 * H, 8 * W, D, generator=torch.Generator().manual_seed(31)).to(cuda)

    def grads(fn, d, m, go):
        d, m = d.detach().clone().requires_grad_(), m.detach().clone().requires_grad_()
        fn(d, m).backward(go)
        return m.grad, d.grad
    gm64, gd64 = grads(cvx_upsample, data.double(), mask.double().contiguous(), gout.double())
    gm_pt, gd_pt = grads(cvx_upsample, data, mask.contiguous(), gout)
    gm, gd = grads(un.cvx_upsample, data, mask, gout)
    assert gm.stride() == mask.stride()
    for name, nat, pt, ref in (("gmask", gm, gm_pt, gm64), ("gdata", gd, gd_pt, gd64)):
        top = float(ref.abs().max())
        e_nat, e_pt = float((nat.double() - ref).abs().max()) / top, float((pt.double() - ref).abs().max()) / top
        print("%s %s D=%d: native %.3e, PyTorch fp32 %.3e of the largest gradient (ratio %.2f, allowed 4)" % (name, layout, D, e_nat, e_pt, e_nat / e_pt))
        assert e_nat <= 4.0 * e_pt, (name, e_nat, e_pt)
    gm2, gd2 = grads(un.cvx_upsample, data, mask, gout)
    assert torch.equal(gm, gm2) and torch.equal(gd, gd2)


def _window(cuda, size):
    import bench
    from test_chained_updates import structured_operator
    if size == "sb":
        video, graph = bench.make_window(cuda, seed=3)
    else:                                                              # a real frontend window: 26 keyframes of 30 x 101
        video, graph = bench.make_window(cuda, seed=3, H8=30, W8=101, NKF=26, buffer=32, intr=(60.0, 60.0, 50.5, 15.0))
    structured_operator(graph.update_op, 0.1)
    return video, graph


def _two_updates(cuda, size, upsample, supply_mask=True):
    """two native updates; the second writes its upsampling mask to a tensor of ours (pvo_operator_args.upmask)"""
    video, graph = _window(cuda, size)
    graph.upsample = upsample
    if upsample:
        video.ensure_disps_up().fill_(-7.0)
    graph.update(None, None, use_inactive=True)
    st = graph._cache["fused"]
    K = int(st["seg"][2])
    mask = torch.zeros(K, graph.ht, graph.wd, 576, dtype=torch.float16, device=cuda)
    if supply_mask:
        st["args"].op.upmask = mask.data_ptr()
    graph.update(None, None, use_inactive=True)
    assert graph._cache["fused"] is st                                  # the same cached call: our pointer was used
    torch.cuda.synchronize()
    return video, graph, mask.permute(0, 3, 1, 2)


@pytest.mark.parametrize("size", ["sb", "window"])
def test_inside_the_native_update(cuda, size):
    from pvo_amd import droid_backends as db
    from pvo_amd.droid_net import cvx_upsample
    video, graph, mask = _two_updates(cuda, size, True)
    src = sorted(set(graph._ii_h))
    assert float(mask.float().abs().max()) > 0
    # bit for bit what the stand-alone kernel gives for the update's own mask and the depths the BA left (clamp included)
    alone = db.cvx_upsample(video.disps[src].unsqueeze(-1).contiguous(), mask).squeeze(-1)
    assert torch.equal(video.disps_up[src], alone)
    ref = cvx_upsample(video.disps[src].double().unsqueeze(-1), mask.double().contiguous()).squeeze(-1)
    X = float(video.disps[src].abs().max())
    err = float((video.disps_up[src].double() - ref).abs().max())
    print("%s: disps_up against the PyTorch form of the same mask and the post-BA depths: %.3e = %.2f u X" % (size, err, err / (U32 * X)))
    assert err <= C_FWD * U32 * X
    rest = [k for k in range(video.disps.shape[0]) if k not in src]
    assert rest and bool((video.disps_up[rest] == -7.0).all())          # rows outside unique(ii) untouched
    # the switch observes, it never perturbs
    v0, g0, _ = _two_updates(cuda, size, False, supply_mask=False)
    assert v0.disps_up is None
    assert torch.equal(video.poses, v0.poses) and torch.equal(video.disps, v0.disps)
    assert torch.equal(graph.net, g0.net) and torch.equal(graph.target_cam, g0.target_cam) and torch.equal(graph.weight, g0.weight)
    # the mask computed as a launch of its own instead of inside the first pose solve: the same disps_up
    db.debug_config("no_riders", True)
    try:
        v1, g1, mask1 = _two_updates(cuda, size, True)
    finally:
        db.debug_config("no_riders", False)
    assert torch.equal(mask1, mask) and torch.equal(v1.disps_up, video.disps_up)
    # a motion-only update leaves disps_up alone
    before = video.disps_up.clone()
    graph.update(None, None, use_inactive=True, motion_only=True)
    torch.cuda.synchronize()
    assert torch.equal(video.disps_up, before)


def _interpolating_logits():
    """[576] logits whose softmax is the bilinear weight of each of the nine coarse neighbours at the centre of fine pixel (dy, dx) -
    what a trained upsampling head approximates: the fine field interpolates the coarse one, so an 8 x 8 block's mean is the coarse
    value wherever the field is locally linear (the weights of the two outer taps are equal over a block)"""
    o = (torch.arange(8).float() + 0.5) / 8 - 0.5                                             # offset of a fine pixel from the coarse centre
    w1 = torch.stack([(-o).clamp(min=0), 1 - o.abs(), o.clamp(min=0)])                       # [tap -1 | 0 | +1][fine index]
    w = torch.einsum("ay,bx->abyx", w1, w1).reshape(9, 8, 8)                                   # k = 3 ky + kx
    return torch.log(w + 1e-4).reshape(576)


class _MaskedOracleOperator:
    """pvo_amd.synthetic.OracleFlowOperator that also hands back an upsampling mask (interpolating logits + seeded noise of 0.1, another
    draw in every call; channels-last fp16 as the native operator writes them), so the PyTorch formulation of FactorGraph.update has one"""

    def __init__(self, inner):
        self.inner, self.calls = inner, 0

    def __getattr__(self, name):
        return getattr(self.inner, name)

    def __call__(self, net, inp, corr, motn, ii, jj, flag=False, **kw):
        out = list(self.inner(net, inp, corr, motn, ii, jj, flag, **kw))
        K, (h, w) = out[3].shape[1], out[3].shape[2:]
        g = torch.Generator().manual_seed(1000 + self.calls)
        self.calls += 1
        m = (_interpolating_logits() + 0.1 * torch.randn(K, h, w, 576, generator=g)).half().to(out[3].device).permute(0, 3, 1, 2)
        out[4] = {"disp": m[None], "flow": None, "dy_mask": None}
        return tuple(out)


def _track(cuda, upsample):
    from pvo_amd import droid_backends as db
    from pvo_amd.droid import Droid, default_args
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.synthetic import OracleFlowOperator, PlaneScene, run_sequence
    scene = PlaneScene(ht=24, wd=32, n_frames=14, seed=0)
    torch.manual_seed(0)
    droid = Droid(default_args(device=str(cuda), image_size=[scene.ht * 8, scene.wd * 8], buffer=32, upsample=upsample))
    op = _MaskedOracleOperator(OracleFlowOperator(scene, droid.video, lambda p, d, k, i, j: db.reproject(p, d, k, i, j)[0]))
    droid.frontend = DroidFrontend(op, droid.video, device=cuda, warmup=8, keyframe_thresh=0.5, frontend_thresh=16.0, frontend_window=20,
                                   frontend_radius=2, frontend_nms=1, upsample=bool(getattr(droid.args, "upsample", False)))
    run_sequence(scene, droid.video, droid.frontend, op)
    return droid, scene


def test_tracked_sequence_yields_full_resolution_depth(cuda):
    droid, scene = _track(cuda, True)
    n, v = droid.video.counter, droid.video
    depth = droid.get_depth(convex=True)
    assert depth.shape == (n, scene.ht * 8, scene.wd * 8) and n >= 10
    assert bool(torch.isfinite(depth).all()) and float(depth.min()) > 0
    blocks = depth.view(n, scene.ht, 8, scene.wd, 8).mean((2, 4))
    rel = ((blocks - v.disps[:n]).abs() / v.disps[:n])[:, 1:-1, 1:-1]
    print("8x8 block means against the 1/8-resolution depths, interior: max relative gap %.4f" % float(rel.max()))
    assert float(rel.max()) < 0.05
    assert droid.get_depth().shape == depth.shape                       # the bilinear default is still there
    off, _ = _track(cuda, False)
    assert off.video.disps_up is None
    with pytest.raises(RuntimeError):
        off.get_depth(convex=True)
    assert off.video.counter == n and torch.equal(off.video.poses[:n], v.poses[:n]) and torch.equal(off.video.disps[:n], v.disps[:n])
    assert np.array_equal(off.get_traj(), droid.get_traj())


def test_training_unroll_with_native_upsampling(cuda):
    """DroidNet.forward(native_upsample=True) against False on the 4-frame graph of tests/test_droidnet.py, in one process on the same
    seeded weights and inputs.  disp_list: each form is within its bound of the fp64 value of the same operands (PyTorch's fp32 chain: 8 u X,
    measured on the host for the issue; the kernel: C_FWD u X), so the two are within (C_FWD + 8) u X of each other; the kernel's own
    bound is asserted per step on the operands captured from the run.  Gradients of update.agg.upmask_disp (they flow through the mask
    alone): the criterion of the backward test - against the fp64 gradient computed from the captured operands, the native run's error
    may be at most 4 x the PyTorch run's."""
    import pvo_amd.droid_net as dn
    from pvo_amd.geom import upsample_native as un
    from pvo_amd.geom.se3 import SE3
    from test_droidnet import _inputs
    z = np.load(GOLD)
    N, H, W = [int(v) for v in z["shape"]]
    steps = 2
    images, Gs, disps, intr = _inputs(N, H, W)
    graph = OrderedDict((i, [j for j in range(N) if j != i and abs(i - j) <= 2]) for i in range(N))
    g = torch.Generator().manual_seed(77)
    R = [torch.randn(1, N, H, W, generator=g).to(cuda) for _ in range(steps)]
    captured = []
    real = un.upsample_dim_1

    def spy(d, m):
        captured.append((d.detach().clone(), m.detach().clone()))
        return real(d, m)

    def run(native):
        torch.manual_seed(0)
        net = dn.DroidNet().train().to(cuda)
        feats = []
        hook = net.update.agg.upmask_disp.register_forward_hook(lambda mod, inp, out: feats.append(inp[0].detach().clone()))
        res = net(SE3(Gs.data.clone().to(cuda)), images.to(cuda), disps.to(cuda), intr.to(cuda), graph, num_steps=steps, fixedp=2,
                  native_upsample=native)
        hook.remove()
        loss = sum((d * r).sum() for d, r in zip(res[1], R))
        loss.backward()
        up = net.update.agg.upmask_disp[0]
        return [d.detach() for d in res[1]], up.weight.grad.clone(), up.bias.grad.clone(), feats, up.weight.detach().clone(), up.bias.detach().clone()

    det = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        un.upsample_dim_1 = spy
        try:
            d_nat, gw_nat, gb_nat, feats, w0, b0 = run(True)
        finally:
            un.upsample_dim_1 = real
        d_pt, gw_pt, gb_pt, _, _, _ = run(False)
    finally:
        torch.use_deterministic_algorithms(det)
    assert len(captured) == steps and len(feats) == steps
    for s in range(steps):
        dd, mm = captured[s]
        X = float(dd.abs().max())
        ref = dn.upsample_dim_1(dd.double(), mm.double())
        e_nat = float((d_nat[s].double() - ref).abs().max())
        e_two = float((d_nat[s] - d_pt[s]).abs().max())
        print("step %d: native against fp64 of its operands %.2f u X; native against the PyTorch run %.2f u X" % (s, e_nat / (U32 * X), e_two / (U32 * X)))
        assert e_nat <= C_FWD * U32 * X
        assert e_two <= (C_FWD + 8.0) * U32 * X
    # fp64 gradient of the 1 x 1 mask convolution's parameters from the captured operands
    w64, b64 = w0.double().requires_grad_(), b0.double().requires_grad_()
    loss = 0.0
    for s in range(steps):
        dd, mm = captured[s]
        m64 = torch.nn.functional.conv2d(feats[s].double(), w64, b64).view(mm.shape)
        assert float((m64.detach() - mm.double()).abs().max()) < 1e-3 * max(1.0, float(mm.abs().max()))    # the hook saw this mask's input
        loss = loss + (dn.upsample_dim_1(dd.double(), m64) * R[s].double()).sum()
    loss.backward()
    for name, nat, pt, ref in (("weight", gw_nat, gw_pt, w64.grad), ("bias", gb_nat, gb_pt, b64.grad)):
        top = float(ref.abs().max())
        e_nat, e_pt = float((nat.double() - ref).abs().max()) / top, float((pt.double() - ref).abs().max()) / top
        print("upmask_disp %s gradient: native run %.3e, PyTorch run %.3e of the largest entry (ratio %.2f, allowed 4)" % (name, e_nat, e_pt, e_nat / e_pt))
        assert e_nat <= 4.0 * e_pt, (name, e_nat, e_pt)
