"""pvo_amd.geom.ba_native.BA - the training path's bundle adjustment in libpvo_hip (pvo_amd/csrc/ba_train.hip) - against the
PyTorch BA it mirrors (pvo_amd.geom.ba.BA, the specification) and the reference's fixtures: values and gradients in fp64 and
fp32, gradcheck, per-element failure of the reduced system, the depth-only step, repeatability, DroidNet's and tools/train.py's
`native_ba` switch, and the inputs it refuses."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

from pvo_amd.geom import ba_native
from pvo_amd.geom import projective_ops as pops
from pvo_amd.geom.ba import BA as torch_BA
from pvo_amd.geom.se3 import SE3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")


def _scene(B, P, ht, wd, seed=0, dtype=torch.float64, noise=0.5):
    """P frames moving forward along a gentle curve, depths in (0.3, 1.0), per-frame intrinsics, edges |i - j| in {1, 2} both ways
    plus one edge i == j; target = the true reprojection plus noise, positive weights"""
    g = torch.Generator().manual_seed(seed)
    xi = torch.zeros(B, P, 6, dtype=torch.float64)
    xi[..., 2] = -0.05 * torch.arange(P, dtype=torch.float64)
    xi[..., :6] += 0.01 * torch.randn(B, P, 6, generator=g, dtype=torch.float64)
    poses = SE3.exp(xi).data
    disps = 0.3 + 0.7 * torch.rand(B, P, ht, wd, generator=g, dtype=torch.float64)
    intr = torch.tensor([0.9 * wd, 0.9 * wd, wd / 2.0, ht / 2.0], dtype=torch.float64).repeat(B, P, 1)
    intr = intr * (1 + 0.02 * torch.rand(B, P, 4, generator=g, dtype=torch.float64))
    ii, jj = [], []
    for i in range(P):
        for j in range(P):
            if i != j and abs(i - j) <= 2:
                ii.append(i); jj.append(j)
    ii.append(P // 2); jj.append(P // 2)
    ii, jj = torch.tensor(ii), torch.tensor(jj)
    c, _ = pops.projective_transform(SE3(poses), disps, intr, ii, jj)
    target = c + noise * torch.randn(c.shape, generator=g, dtype=torch.float64)
    weight = torch.rand(c.shape, generator=g, dtype=torch.float64)
    M = int(torch.unique(ii).numel())
    eta = 1e-3 + 1e-2 * torch.rand(B, M, ht, wd, generator=g, dtype=torch.float64)
    # start away from the truth
    p0 = SE3.exp(0.02 * torch.randn(B, P, 6, generator=g, dtype=torch.float64)).mul(SE3(poses)).data
    d0 = disps * (1 + 0.1 * torch.randn(disps.shape, generator=g, dtype=torch.float64)).clamp(0.5, 1.5)
    t = dict(target=target, weight=weight, eta=eta, poses=p0, disps=d0, intr=intr)
    return {k: v.to(dtype) for k, v in t.items()}, ii, jj


def _run(fn, s, ii, jj, fixedp, steps=2, dev="cuda:0", seed=1, **kw):
    """`steps` chained BA steps; returns poses, disps and the gradients of a fixed random linear function of them with respect
    to target, weight, eta, poses and disps"""
    leaves = {k: s[k].to(dev).clone().requires_grad_(True) for k in ("target", "weight", "eta", "poses", "disps")}
    intr = s["intr"].to(dev)
    G, d = SE3(leaves["poses"]), leaves["disps"]
    for _ in range(steps):
        G, d = fn(leaves["target"], leaves["weight"], leaves["eta"], G, d, intr, ii, jj, fixedp=fixedp, **kw)
    g = torch.Generator().manual_seed(seed)
    cp = torch.randn(G.data.shape, generator=g, dtype=torch.float64).to(dev, G.data.dtype)
    cd = torch.randn(d.shape, generator=g, dtype=torch.float64).to(dev, d.dtype)
    grads = torch.autograd.grad((G.data * cp).sum() + (d * cd).sum(), list(leaves.values()))
    return G.data.detach(), d.detach(), dict(zip(leaves, grads))


def _close_grads(got, ref, rel, abs_):
    for k in ref:
        scale = ref[k].abs().max().item()
        err = (got[k] - ref[k]).abs().max().item()
        assert err <= rel * scale + abs_, (k, err, scale)


# ---- refused inputs (no GPU needed) ------------------------------------------------------------------------------------------------

def _refused_args(case, dev):
    """the arguments of one refused call: a valid fp32 call on `dev` with one thing changed; returns (args, kwargs)"""
    s, ii, jj = _scene(1, 18 if case == "too_many_free_poses" else 4, 6, 7, dtype=torch.float32)
    s = {k: v.to(dev) for k, v in s.items()}
    args = [s["target"], s["weight"], s["eta"], SE3(s["poses"]), s["disps"], s["intr"], ii, jj]
    kw = {"fixedp": 1}
    if case == "rig":
        kw["rig"] = 2
    elif case == "mixed_dtype":
        args[1] = args[1].double()
    elif case == "intrinsics_grad":
        args[5] = args[5].clone().requires_grad_(True)
    elif case == "fixedp_out_of_range":
        kw["fixedp"] = 5
    return args, kw


# each refusal is told apart by its own message; all of them name the PyTorch BA as the path that handles the input
REFUSALS = {
    "rig": r"rig = 2 is not supported",
    "mixed_dtype": r"all tensors fp32 or all fp64",
    "intrinsics_grad": r"no intrinsics gradient",
    "too_many_free_poses": r"at most 16 free poses; got P - fixedp = 17",
    "fixedp_out_of_range": r"0 <= fixedp <= P; got P = 4, fixedp = 5",
}


@pytest.mark.parametrize("case", sorted(REFUSALS) + ["cpu"])
def test_unsupported_inputs_raise_value_error_naming_the_torch_ba(case):
    """host tensors: every condition but the device is checked first, so each case meets its own check"""
    args, kw = _refused_args(case, "cpu")
    with pytest.raises(ValueError, match=REFUSALS.get(case, r"needs device tensors") + r".*pvo_amd\.geom\.ba\.BA handles it"):
        ba_native.BA(*args, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_unsupported_device_inputs_raise_value_error_naming_the_torch_ba(case):
    args, kw = _refused_args(case, "cuda:0")
    with pytest.raises(ValueError, match=REFUSALS[case] + r".*pvo_amd\.geom\.ba\.BA handles it"):
        ba_native.BA(*args, **kw)


def test_a_plan_that_does_not_fit_the_graph_is_refused():
    """droid_backends.ba_train reads the plan as int32 CSR: another dtype or lengths that do not fit the edges raise"""
    from pvo_amd import droid_backends as db
    from pvo_amd._lib import PvoHipError
    ii = torch.tensor([0, 1, 1, 2, 2])
    kx, kk = torch.unique(ii, return_inverse=True)
    plan = (kx.int(), kk.int(), torch.tensor([0, 1, 3, 5], dtype=torch.int32), torch.arange(5, dtype=torch.int32))
    assert db._check_ba_plan(plan, 5, 3) == 3
    with pytest.raises(PvoHipError, match="int32"):
        db._check_ba_plan((kx, kk) + plan[2:], 5, 3)                          # int64, as torch.unique returns it
    with pytest.raises(PvoHipError, match="does not fit"):
        db._check_ba_plan(plan, 6, 3)                                         # built for another edge list
    with pytest.raises(PvoHipError, match="does not fit"):
        db._check_ba_plan(plan, 5, 2)                                         # more keyframes than frames


def test_droidnet_native_ba_refuses_cpu_tensors():
    from pvo_amd import droid_net as dn
    from test_droidnet import _inputs
    images, Gs, disps, intr = _inputs(3, 64, 64, seed=5)
    net = dn.DroidNet().train()
    graph = OrderedDict((i, [j for j in range(3) if j != i]) for i in range(3))
    with pytest.raises(ValueError, match=r"pvo_amd\.geom\.ba\.BA"):
        net(SE3(Gs.data[:, :3]), images, disps, intr, graph, num_steps=1, fixedp=2, native_ba=True)


def test_train_parse_args_native_ba_switch():
    import train as T
    assert T.parse_args([]).native_ba is False
    assert T.parse_args(["--native_ba", "True"]).native_ba is True
    assert T.parse_args(["--native_ba", "False"]).native_ba is False


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------

CASES = [  # B, P, fixedp, ht, wd
    (1, 3, 1, 8, 10),
    (2, 5, 2, 8, 10),
    (1, 8, 0, 16, 16),
    (2, 4, 0, 25, 50),
    (1, 6, 1, 25, 50),
    (2, 7, 2, 16, 16),
    (1, 16, 0, 6, 7),            # 16 free poses: the largest reduced system (96 x 96; in fp64 beyond 48 KB of LDS)
    (2, 17, 1, 6, 7),
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,P,fixedp,ht,wd", CASES)
def test_fp64_two_steps_match_torch_ba(B, P, fixedp, ht, wd):
    s, ii, jj = _scene(B, P, ht, wd, seed=P + 10 * B)
    Gr, dr, gr = _run(torch_BA, s, ii, jj, fixedp)
    Gn, dn_, gn = _run(ba_native.BA, s, ii, jj, fixedp)
    assert (Gn - Gr).abs().max().item() < 1e-9
    assert (dn_ - dr).abs().max().item() < 1e-9
    _close_grads(gn, gr, 1e-8, 1e-12)


@pytest.mark.gpu
def test_host_and_device_edge_lists_and_a_given_plan_agree():
    s, ii, jj = _scene(1, 5, 8, 10, seed=3)
    a = _run(ba_native.BA, s, ii, jj, 1)
    b = _run(ba_native.BA, s, ii.cuda(), jj.cuda(), 1, plan=ba_native.make_plan(ii.cuda()))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _load(name):
    z = np.load(os.path.join(GOLD, "ba_python_%s.npz" % name))
    t = {k: torch.from_numpy(z[k]) for k in z.files}
    t["intr_all"] = t["intr"][None, None].repeat(1, t["poses"].shape[0], 1)
    t["fixedp"] = int(z["fixedp"])
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b"])
def test_fp32_matches_reference_fixtures(name):
    t = _load(name)
    dev = torch.device("cuda:0")
    leaves = {k: t[k][None].clone().to(dev).requires_grad_(True) for k in ("target", "weight", "eta", "disps")}
    Gs, disps = SE3(t["poses"][None].clone().to(dev)), leaves["disps"]
    intr = t["intr_all"].to(dev)
    for it in (1, 2):
        Gs, disps = ba_native.BA(leaves["target"], leaves["weight"], leaves["eta"] - 1e-7, Gs, disps, intr, t["ii"], t["jj"],
                                 fixedp=t["fixedp"])
        ep = (Gs.data[0].detach().cpu() - t["ba_poses_%d" % it]).abs().max().item()
        ed = (disps[0].detach().cpu() - t["ba_disps_%d" % it]).abs().max().item()
        print("fixture %s step %d: max |poses - ref| %.3g, max |disps - ref| %.3g" % (name, it, ep, ed))
        assert ep < 1e-5 and ed < 1e-4
    ((Gs.data[0] * t["grad_cp"].to(dev)).sum() + (disps[0] * t["grad_cd"].to(dev)).sum()).backward()
    for k, v in leaves.items():
        ref = t["grad_" + k]
        scale = ref.abs().max().item()
        err = (v.grad[0].cpu() - ref).abs().max().item()
        print("fixture %s grad_%s: max error %.3g of max |ref| %.3g" % (name, k, err, scale))
        assert err <= 1e-3 * scale + 1e-7, k


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 2])
def test_gradcheck_fp64(steps):
    s, ii, jj = _scene(1, 4, 6, 7, seed=21, noise=0.3)
    dev = torch.device("cuda:0")
    intr = s["intr"].to(dev)
    assert (s["disps"] > 0.2).all() and (s["disps"] < 2).all()

    def f(target, weight, eta, poses, disps):
        G, d = SE3(poses), disps
        for _ in range(steps):
            G, d = ba_native.BA(target, weight, eta, G, d, intr, ii, jj, fixedp=1)
        return G.data, d

    inputs = tuple(s[k].to(dev).clone().requires_grad_(True) for k in ("target", "weight", "eta", "poses", "disps"))
    # (nondet_tol: the pose / depth gradients through the Jacobians are summed with fp atomics - pvo_proj_transform_vjp)
    assert torch.autograd.gradcheck(f, inputs, eps=1e-6, atol=1e-6, rtol=1e-4, nondet_tol=1e-12)


@pytest.mark.gpu
def test_non_spd_system_fails_per_batch_element():
    s, ii, jj = _scene(2, 5, 8, 10, seed=4)
    s["weight"][1] = -s["weight"][1]                           # batch element 1: the reduced system is not SPD
    dev = torch.device("cuda:0")
    _, _, dx = ba_native.step(*[s[k].to(dev) for k in ("target", "weight", "eta")], SE3(s["poses"].to(dev)), s["disps"].to(dev),
                              s["intr"].to(dev), ii, jj, fixedp=1)
    assert torch.equal(dx[1], torch.zeros_like(dx[1])) and dx[0].abs().max() > 0
    Gr, dr, gr = _run(torch_BA, s, ii, jj, 1, steps=1)
    Gn, dn_, gn = _run(ba_native.BA, s, ii, jj, 1, steps=1)
    assert torch.equal(Gn[1], s["poses"][1].to(dev))
    assert (Gn - Gr).abs().max().item() < 1e-9 and (dn_ - dr).abs().max().item() < 1e-9
    _close_grads(gn, gr, 1e-8, 1e-12)


@pytest.mark.gpu
def test_depth_only_step_matches_torch_ba():
    s, ii, jj = _scene(2, 4, 8, 10, seed=5)
    Gr, dr, gr = _run(torch_BA, s, ii, jj, 4)
    Gn, dn_, gn = _run(ba_native.BA, s, ii, jj, 4)
    assert torch.equal(Gn, Gr) and (dn_ - dr).abs().max().item() < 1e-9
    _close_grads(gn, gr, 1e-8, 1e-12)
    from test_torch_ba import _depth_only_case
    c = _depth_only_case()
    dev = torch.device("cuda:0")
    args = (c["target"][None].to(dev), c["weight"][None].to(dev), c["eta"][None].to(dev) - 1e-7)
    intr = c["intr"][None, None].repeat(1, 2, 1).to(dev)
    Gt, dt = torch_BA(*args, SE3(c["poses"][None].to(dev)), c["d0"][None].to(dev), intr, c["ii"], c["jj"], fixedp=2)
    Gn, dn_ = ba_native.BA(*args, SE3(c["poses"][None].to(dev)), c["d0"][None].to(dev), intr, c["ii"], c["jj"], fixedp=2)
    assert torch.equal(Gn.data, Gt.data) and (dn_ - dt).abs().max().item() < 1e-5
    assert (dn_[0].cpu() - c["d0"]).abs().max() > 0.05


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_forward_is_bitwise_repeatable(dtype):
    s, ii, jj = _scene(2, 7, 25, 50, seed=6, dtype=dtype)
    dev = torch.device("cuda:0")
    args = [s[k].to(dev) for k in ("target", "weight", "eta")]
    outs = [ba_native.BA(*args, SE3(s["poses"].to(dev)), s["disps"].to(dev), s["intr"].to(dev), ii, jj, fixedp=1) for _ in range(2)]
    assert torch.equal(outs[0][0].data, outs[1][0].data) and torch.equal(outs[0][1], outs[1][1])


def _group_cos(na, nb):
    ga = {k: p.grad for k, p in na.named_parameters() if p.grad is not None}
    gb = {k: p.grad for k, p in nb.named_parameters() if p.grad is not None}
    assert set(ga) == set(gb)
    out = {}
    for group in ("fnet.", "cnet.", "update.gru.", "update.corr_encoder."):
        a = torch.cat([ga[k].flatten() for k in sorted(ga) if k.startswith(group)])
        b = torch.cat([gb[k].flatten() for k in sorted(gb) if k.startswith(group)])
        assert torch.isfinite(a).all()
        out[group] = (float(torch.dot(a, b) / (a.norm() * b.norm())), float(a.norm() / b.norm()))
    return out


@pytest.mark.gpu
def test_small_training_step_native_ba_matches_torch_ba():
    from pvo_amd import droid_net as dn
    from test_droidnet import _inputs
    dev = "cuda:0"
    images, Gs, disps, intr = _inputs(3, 128, 128, seed=5)
    graph = OrderedDict((i, [j for j in range(3) if j != i]) for i in range(3))
    runs = {}
    for native in (False, True):
        torch.manual_seed(0)
        net = dn.DroidNet().train().to(dev)
        res = net(SE3(Gs.data[:, :3].to(dev)), images.to(dev), disps.to(dev), intr.to(dev), graph, num_steps=2, fixedp=2, native_ba=native)
        Gs_l, disp_l, resid_l, _ = res
        loss = sum(r.abs().mean() for r in resid_l) + sum(d.mean() for d in disp_l) + sum((g.data ** 2).sum() for g in Gs_l)
        loss.backward()
        runs[native] = (net, res, float(loss))
    (nt, rt, lt), (nn_, rn, ln) = runs[False], runs[True]
    assert abs(ln - lt) < 1e-3 * abs(lt), (ln, lt)
    for a, b in zip(rn[0], rt[0]):
        assert (a.data - b.data).abs().max() < 1e-4
    for group, (cos, ratio) in _group_cos(nn_, nt).items():
        assert cos >= 0.995 and 0.98 <= ratio <= 1.02, (group, cos, ratio)


@pytest.mark.gpu
def test_st_training_step_native_ba_matches_torch_ba():
    import train as T
    from pvo_amd.droid_net import DroidNet
    from pvo_amd.geom import losses as L
    from pvo_amd.geom.graph_utils import build_frame_graph
    from pvo_amd.synthetic import TrainClips
    dev = torch.device("cuda:0")
    args = T.parse_args(["--device", "cuda"])
    images, poses, disps, intr, gt_masks, gt_vals, segments = [x[None].to(dev) for x in TrainClips(6, (200, 400))[3]]
    graph = build_frame_graph(poses, disps, intr, num=20, need_inv=False)
    runs = {}
    for native in (False, True):
        torch.manual_seed(0)
        net = DroidNet().to(dev).train()
        Ps = SE3(poses)
        Gs = SE3.IdentityLike(Ps)
        Gs.data[:, 0] = Ps.data[:, 0]; Gs.data[:, 1:] = Ps.data[:, [1]]
        out = net(Gs, images, torch.ones_like(disps[:, :, 3::8, 3::8]), intr / 8.0, graph, num_steps=15, fixedp=2, ret_flow=True,
                  downsample=True, segments=segments, corr_dtype=torch.bfloat16, native_ba=native)
        loss, _ = T.objective(args, L, out, (images, Ps, disps, intr, gt_masks, gt_vals), graph, L.SSIM().to(dev), 0)
        loss.backward()
        runs[native] = (net, float(loss))
    (nt, lt), (nn_, ln) = runs[False], runs[True]
    assert np.isfinite(ln) and abs(ln - lt) < 1e-2 * abs(lt), (ln, lt)
    for group, (cos, _) in _group_cos(nn_, nt).items():
        assert cos >= 0.99, (group, cos)


def _gpu_worker(rank, argv, report):
    import train as T
    T.train(rank, T.parse_args(argv), report)


@pytest.mark.gpu
def test_train_driver_native_ba_two_steps(tmp_path):
    import torch.multiprocessing as mp
    argv = ["--gpus", "0", "--device", "cuda", "--native_ba", "True", "--steps", "2", "--iters", "3", "--n_frames", "4", "--edges", "10",
            "--crop_size", "128", "192", "--log_every", "1", "--out_dir", str(tmp_path), "--port", "29547", "--restart_prob", "0.0"]
    report = mp.get_context("spawn").Manager().dict()
    mp.spawn(_gpu_worker, args=(argv, report), nprocs=1, join=True)
    assert report[0]["steps"] == 2 and np.isfinite(report[0]["loss"])
    ckpt = os.path.join(str(tmp_path), "vkitti2_dy_train_final.pth")
    state = torch.load(ckpt, map_location="cpu")
    from pvo_amd.droid_net import DroidNet
    net = DroidNet()
    sd = state.get("model", state) if isinstance(state, dict) else state
    net.load_state_dict({k.replace("module.", "", 1): v for k, v in sd.items()})
