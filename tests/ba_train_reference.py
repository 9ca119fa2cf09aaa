"""Cases and the fp64 host evaluation that the training path's native bundle adjustment (pvo_amd/csrc/ba_train.hip with
proj_fwd_kernel / proj_vjp_kernel of se3_ops.hip) is held to.

The reference is the specification itself: pvo_amd.geom.ba.BA on CPU tensors in fp64 (CPU tensors always take the PyTorch
formulation of SE3 and projective_transform) and autograd for the five gradients of a fixed random linear function of the
outputs.  `ba_step` is the same step written out on the same helpers, so that it can return the intermediate cut (Z, coordinates,
validity, Ji / Jj / Jz, the pre-mask disparities d1, dx) and so that single terms can be mutated; unmutated it equals BA bit for bit
(tests/test_ba_train_fp64_host.py checks that).

A case is a seeded scene in which every mask of the step fires and every index path is taken:
  * one frame (`push`) displaced 1.6 forward: the other frames' near points fall at Z < 0.2 and at Z < 0.1 in it;
  * row 1 of every frame starts just under 10 with targets that pull its even columns over 10 (every other one of them from further
    away and more damped, so that it crosses in a second step) and its odd columns away; row 2 starts just over 0 with targets that
    pull its even columns under 0; row 3 has eta and weights so small that the 1e-7 of the depth block matters;
  * the last frame has no out-edges (M = P - 1), one edge has i == j, one edge is listed twice, the edge list is shuffled so that
    keyframes' edges are not contiguous, and the intrinsics differ per frame.
All inputs are exactly representable in fp32, so the fp64 reference and every fp32 evaluation read the same numbers.

Admission (a condition, not a measurement): in the fp64 reference, in every step, each of the four masks (Z < 0.2, Z < 0.1, d1 > 10,
d1 < 0) fires on at least 4 samples and leaves at least 4 samples of the same frame alone, and no Z lies within a band of 0.1 / 0.2
and no d1 within a band of 0 / 10, the band being 64 times the largest deviation of PyTorch's fp32 CPU evaluation of that quantity
from fp64 in the case.  The builder clears the bands itself by nudging the offending input disparities (a pixel that the first of
two steps masked to 0 no longer feels its input disparity: there the targets of its edges are moved), and takes the first of eight
seeds whose scene is admitted.  With the bands clear, the validity and zero patterns of a correct fp32 implementation equal the
reference's exactly.

The yardstick e_pt of an output is the error of PyTorch's own fp32 evaluation against fp64, relative to the largest fp64 magnitude;
`accept` is the rule the GPU tests apply (error at most FACTOR * e_pt, zero patterns exact)."""
import functools

import torch

from pvo_amd.geom import ba as tba
from pvo_amd.geom import projective_ops as pops
from pvo_amd.geom.chol import schur_solve
from pvo_amd.geom.se3 import SE3

CASES = [  # B, P, fixedp, ht, wd, steps
    (2, 5, 1, 6, 7, 1),          # HW = 42, under one wave
    (2, 5, 1, 6, 7, 2),
    (1, 4, 0, 16, 16, 1),        # HW = 256, exactly one chunk, free gauge
    (1, 4, 1, 9, 29, 1),         # HW = 261, a second chunk of 5 pixels
    (2, 6, 2, 17, 16, 1),        # edges between two fixed frames
    (1, 4, 4, 6, 7, 1),          # depth-only, Pf = 0, with masks
    (1, 5, 4, 6, 7, 1),          # one free pose
    (2, 17, 1, 6, 7, 1),         # 16 free poses: the 96 x 96 system
    (2, 17, 1, 6, 7, 2),
    (1, 16, 0, 6, 7, 1),
]
CASE_IDS = ["B%d-P%d-fix%d-%dx%d-steps%d" % c for c in CASES]
LEAVES = ("target", "weight", "eta", "poses", "disps")
FACTOR = 4.0                     # tests/test_cvx_upsample_gpu.py's: another summation order, the LDS Cholesky
BAND = 64.0
MIN_FIRE = 4
MUTANTS = ("valid_above_0.1", "mask_grad_passed_above_10", "lm_dropped", "c_1e-7_dropped", "self_edge_cross_blocks_dropped",
           "sink_frame_stepped", "keyframe_edge_missing")


def layout(P, fixedp):
    """the frames with a role: (push, sink, self-edge frame)"""
    return P // 2, P - 1, min(max(fixedp, 1), P - 2)


def _edges(P, fixedp, g):
    push, sink, same = layout(P, fixedp)
    e = [(i, j) for i in range(P) for j in range(P) if i != sink and i != j and abs(i - j) <= 2]
    e.append((same, same))
    e.append((0, 1))                                                            # a duplicate
    perm = torch.randperm(len(e), generator=g).tolist()
    ii, jj = torch.tensor([e[k][0] for k in perm]), torch.tensor([e[k][1] for k in perm])
    kk = torch.unique(ii, return_inverse=True)[1]
    assert any(((kk == m).nonzero().flatten().diff() > 1).any() for m in range(P - 1))      # some keyframe's edges are apart
    return ii, jj


def _scene(B, P, fixedp, ht, wd, seed):
    assert ht >= 4 and P >= 4
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *sh: torch.rand(*sh, generator=g, dtype=torch.float64)
    push, sink, _ = layout(P, fixedp)
    xi = torch.zeros(B, P, 6, dtype=torch.float64)
    xi[..., 2] = -0.05 * torch.arange(P, dtype=torch.float64)
    xi += 0.01 * torch.randn(B, P, 6, generator=g, dtype=torch.float64)
    xi[:, push, 2] -= 1.6
    poses = SE3.exp(xi).data
    true = 0.3 + 0.7 * rnd(B, P, ht, wd)
    intr = torch.tensor([0.9 * wd, 0.9 * wd, wd / 2.0, ht / 2.0], dtype=torch.float64).repeat(B, P, 1)
    intr = intr * (1 + 0.02 * rnd(B, P, 4))
    ii, jj = _edges(P, fixedp, g)
    d0 = true * (1 + 0.1 * torch.randn(true.shape, generator=g, dtype=torch.float64)).clamp(0.5, 1.5)
    # rows that the step carries over 10 and under 0 (even columns: pulled across; odd columns: pulled away).  Of the even columns
    # of row 1 every other one starts lower and more damped, to cross 10 in a second step
    col = torch.arange(wd)
    even, late = (col % 2 == 0).to(torch.float64), (col % 4 == 2).to(torch.float64)
    d0[:, :, 1] = even * (1 - late) * (9.9 + 0.09 * rnd(B, P, wd)) + late * (9.55 + 0.3 * rnd(B, P, wd)) + (1 - even) * (9.5 + 0.4 * rnd(B, P, wd))
    true[:, :, 1] = d0[:, :, 1] + even * (1.0 + 2.0 * rnd(B, P, wd)) - (1 - even) * (1.0 + 2.0 * rnd(B, P, wd))
    d0[:, :, 2] = 0.01 + 0.04 * rnd(B, P, wd)
    true[:, :, 2] = d0[:, :, 2] - even * (2.0 + 4.0 * rnd(B, P, wd)) + (1 - even) * (0.1 + 0.4 * rnd(B, P, wd))
    p0 = SE3.exp(0.02 * torch.randn(B, P, 6, generator=g, dtype=torch.float64)).mul(SE3(poses)).data
    c, _ = pops.projective_transform(SE3(poses), true, intr, ii, jj)
    target = c + 0.5 * torch.randn(c.shape, generator=g, dtype=torch.float64)
    # (row 1 sees its pull alone: at disparity 10 the error of the starting poses would outweigh it)
    c0, _ = pops.projective_transform(SE3(p0), true, intr, ii, jj)
    target[:, :, 1] = c0[:, :, 1] + 0.1 * torch.randn(c[:, :, 1].shape, generator=g, dtype=torch.float64)
    weight = rnd(*c.shape)
    M = int(torch.unique(ii).numel())
    assert M == P - 1
    eta = 1e-3 + 1e-2 * rnd(B, M, ht, wd)
    eta[:, :, 1] *= (0.1 + 0.9 * late)                                          # (row 1 is to move)
    weight[:, :, 3] *= 1e-3                                                     # row 3: C of the order of the 1e-7 added to it
    eta[:, :, 3] = 2e-7 * (1 + rnd(B, M, wd))
    s = dict(target=target, weight=weight, eta=eta, poses=p0, disps=d0, intr=intr)
    return {k: v.float().double() for k, v in s.items()}, ii, jj


def depth_in_target(poses, disps, intr, ii, jj):
    """Z of every sample in its edge's frame j [B,N,H,W]: what `valid` and the guarded inverse test"""
    X0, _ = pops.iproj(disps[:, ii], intr[:, ii])
    Gij = poses[:, jj] * poses[:, ii].inv()
    return (Gij[:, :, None, None] * X0)[..., 2]


def ba_step(target, weight, eta, poses, disps, intr, ii, jj, fixedp, mutant=None):
    """pvo_amd.geom.ba.BA written out on its own helpers -> (poses, disps, cut); `mutant` changes one term (MUTANTS)"""
    assert mutant is None or mutant in MUTANTS
    B, P, ht, wd = disps.shape
    N, HW, D = ii.shape[0], ht * wd, 6
    Z = depth_in_target(poses, disps, intr, ii, jj)
    if mutant == "valid_above_0.1":
        coords, valid, (Ji, Jj, Jz) = pops.projective_transform(poses, disps, intr, ii, jj, jacobian=True)
        valid = (Z > 0.1).to(valid.dtype).unsqueeze(-1)
        r = (target - coords).reshape(B, N, -1)
        w = 0.001 * (valid * weight).reshape(B, N, -1)
        Ji, Jj = Ji.reshape(B, N, -1, D), Jj.reshape(B, N, -1, D)
    else:
        r, w, Ji, Jj, Jz = tba._linearise(target, weight, poses, disps, intr, ii, jj)
    kx, kk = torch.unique(ii, return_inverse=True)
    M, Pf = kx.shape[0], P - fixedp
    pi, pj = ii - fixedp, jj - fixedp
    if mutant == "self_edge_cross_blocks_dropped":
        wJi, wJj = w[..., None] * Ji, w[..., None] * Jj
        blk = lambda a, b: torch.einsum("bnrd,bnre->bnde", a, b)
        cross = (ii != jj).to(Ji.dtype).view(1, N, 1, 1)
        H = (tba._scatter_blocks(blk(wJi, Ji), pi, pi, Pf, Pf) + tba._scatter_blocks(blk(wJi, Jj) * cross, pi, pj, Pf, Pf) +
             tba._scatter_blocks(blk(wJj, Ji) * cross, pj, pi, Pf, Pf) + tba._scatter_blocks(blk(wJj, Jj), pj, pj, Pf, Pf))
        H = H.view(B, Pf, Pf, D, D)
        v = (tba._scatter_rows(torch.einsum("bnrd,bnr->bnd", wJi, r), pi, Pf) +
             tba._scatter_rows(torch.einsum("bnrd,bnr->bnd", wJj, r), pj, Pf))
    else:
        H, v, wJi, wJj = tba._pose_system(Ji, Jj, w, r, pi, pj, Pf)
    Jz2 = Jz.reshape(B, N, HW, 2)
    Ei = torch.einsum("bnhcd,bnhc->bndh", wJi.view(B, N, HW, 2, D), Jz2)
    Ej = torch.einsum("bnhcd,bnhc->bndh", wJj.view(B, N, HW, 2, D), Jz2)
    w2, r2 = w.view(B, N, HW, 2), r.view(B, N, HW, 2)
    wk = (w2 * r2 * Jz2).sum(-1)
    Ck = (w2 * Jz2 * Jz2).sum(-1)
    if mutant == "keyframe_edge_missing":                                       # the last edge of the second keyframe is not summed
        keep = torch.ones(N, dtype=Ck.dtype)
        keep[int((kk == 1).nonzero().flatten()[-1])] = 0
        keep = keep.to(Ck.device)
        Ei, Ej, wk, Ck = Ei * keep.view(1, N, 1, 1), Ej * keep.view(1, N, 1, 1), wk * keep.view(1, N, 1), Ck * keep.view(1, N, 1)
    E = (tba._scatter_blocks(Ei, pi, kk, Pf, M) + tba._scatter_blocks(Ej, pj, kk, Pf, M)).view(B, Pf, M, D, HW)
    C = tba._scatter_rows(Ck, kk, M) + eta.reshape(B, M, HW)
    if mutant != "c_1e-7_dropped":
        C = C + 1e-7
    wz = tba._scatter_rows(wk, kk, M)
    dx, dz = schur_solve(H, E, C, v, wz, lm=0.0 if mutant == "lm_dropped" else 0.0001)
    pout = tba.pose_retr(poses, dx, torch.arange(Pf) + fixedp)
    d1 = tba.disp_retr(disps, dz.view(B, -1, ht, wd), kx)
    if mutant == "sink_frame_stepped":                                          # the frame without out-edges takes the last keyframe's step
        add = torch.zeros_like(d1)
        add[:, P - 1] = dz.view(B, -1, ht, wd)[:, M - 1]
        d1 = d1 + add
    if mutant == "mask_grad_passed_above_10":
        dout = torch.where(d1 > 10, d1 - d1.detach(), d1).clamp(min=0.0)
    else:
        dout = torch.where(d1 > 10, torch.zeros_like(d1), d1).clamp(min=0.0)
    cut = dict(Z=Z, d1=d1, dx=dx.reshape(B, Pf * D))
    return pout, dout, cut


def projection_cut(s, ii, jj, dtype=torch.float64, dev="cpu"):
    """coordinates, validity and the three Jacobians of the case's first linearisation (PyTorch formulation on `dev` tensors that
    take it), and the pose / depth gradients of a fixed random linear function of coordinates and Jacobians"""
    poses = s["poses"].to(dev, dtype).clone().requires_grad_(True)
    disps = s["disps"].to(dev, dtype).clone().requires_grad_(True)
    x1, valid, (Ji, Jj, Jz) = pops.projective_transform(SE3(poses), disps, s["intr"].to(dev, dtype), ii, jj, jacobian=True)
    cot = projection_cotangents(x1.shape[:4])
    loss = sum((o * cot[k].to(dev, dtype)).sum() for k, o in (("x1", x1), ("Ji", Ji), ("Jj", Jj), ("Jz", Jz)))
    gp, gd = torch.autograd.grad(loss, [poses, disps])
    out = dict(x1=x1, Ji=Ji, Jj=Jj, Jz=Jz, g_poses=gp, g_disps=gd)
    return {k: v.detach().double().cpu() for k, v in out.items()}, valid.detach().cpu()


def projection_cotangents(bnhw, seed=2):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *t: torch.randn(*bnhw, *t, generator=g, dtype=torch.float64)
    return dict(x1=rn(2), Ji=rn(2, 6), Jj=rn(2, 6), Jz=rn(2, 1))


def cotangents(B, P, ht, wd, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, P, 7, generator=g, dtype=torch.float64), torch.randn(B, P, ht, wd, generator=g, dtype=torch.float64))


def run_chain(step, s, ii, jj, fixedp, steps, dtype, dev="cpu", grads=True):
    """`steps` chained calls of step(target, weight, eta, SE3, disps, intr, ii, jj, fixedp) -> (SE3, disps, dx | None, cut | None)
    -> (outputs as fp64 CPU tensors: poses, disps, dx<k>, g_<leaf>; the cuts)"""
    leaves = {k: s[k].to(dev, dtype).clone().requires_grad_(grads) for k in LEAVES}
    intr = s["intr"].to(dev, dtype)
    G, d, out, cuts = SE3(leaves["poses"]), leaves["disps"], {}, []
    for k in range(steps):
        G, d, dx, cut = step(leaves["target"], leaves["weight"], leaves["eta"], G, d, intr, ii, jj, fixedp)
        if dx is not None:
            out["dx%d" % k] = dx.detach()
        cuts.append(cut)
    out["poses"], out["disps"] = G.data.detach(), d.detach()
    if grads:
        cp, cd = cotangents(*d.shape)
        gs = torch.autograd.grad((G.data * cp.to(dev, dtype)).sum() + (d * cd.to(dev, dtype)).sum(), list(leaves.values()))
        out.update({"g_" + k: g for k, g in zip(LEAVES, gs)})
    return {k: v.double().cpu() for k, v in out.items()}, cuts


def _spec_step(*a):
    G, d = tba.BA(*a[:8], fixedp=a[8])
    return G, d, None, None


def _cut_step(mutant=None):
    def step(*a):
        G, d, cut = ba_step(*a, mutant=mutant)
        return G, d, cut["dx"], {k: v.detach().double().cpu() for k, v in cut.items()}
    return step


def evaluate_torch(s, ii, jj, fixedp, steps, dtype, dev="cpu"):
    """the specification (geom.ba.BA + autograd) in `dtype` on `dev`, with dx and the cut from ba_step -> (outputs, cuts)"""
    out, _ = run_chain(_spec_step, s, ii, jj, fixedp, steps, dtype, dev)
    with torch.no_grad():
        o2, cuts = run_chain(_cut_step(), s, ii, jj, fixedp, steps, dtype, dev, grads=False)
    out.update({k: v for k, v in o2.items() if k.startswith("dx")})
    out["_cut_poses"], out["_cut_disps"] = o2["poses"], o2["disps"]
    return out, cuts


def evaluate_mutant(s, ii, jj, fixedp, steps, mutant, dtype=torch.float32):
    return run_chain(_cut_step(mutant), s, ii, jj, fixedp, steps, dtype)[0]


# ---- admission ---------------------------------------------------------------------------------------------------------------------

def _cuts_only(s, ii, jj, fixedp, steps, dtype):
    with torch.no_grad():
        return run_chain(_cut_step(), s, ii, jj, fixedp, steps, dtype, grads=False)[1]


def _fires_and_spares(fired, frame_axis_index, nframes):
    """fired [B, F or N, ...] bool, frame of every entry of axis 1 -> (samples fired, whether a frame in which it fires has
    >= MIN_FIRE samples left alone)"""
    ok = False
    for f in range(nframes):
        sel = fired[:, frame_axis_index == f]
        if sel.numel() and int(sel.sum()) >= 1 and int((~sel).sum()) >= MIN_FIRE:
            ok = True
    return int(fired.sum()), ok


def admission(s, ii, jj, fixedp, steps):
    """-> dict(ok, counts per step and mask, bands, offenders): see the module docstring.  Steps are judged in order, and a step
    only once the steps before it are clear (beyond a sample inside a band the fp32 evaluation may take another branch, and the
    deviations after it are no longer rounding)."""
    P = s["disps"].shape[1]
    c64, c32 = _cuts_only(s, ii, jj, fixedp, steps, torch.float64), _cuts_only(s, ii, jj, fixedp, steps, torch.float32)
    rep = dict(ok=True, counts=[], band_Z=0.0, band_d1=0.0, offenders=None, inside=0)
    frames = torch.arange(P)
    for k in range(steps):
        Z, d1 = c64[k]["Z"], c64[k]["d1"]
        bz = BAND * float((c32[k]["Z"] - Z).abs().max())
        rep["band_Z"] = max(rep["band_Z"], bz)
        inZ = ((Z - 0.1).abs() <= bz) | ((Z - 0.2).abs() <= bz)
        if inZ.any():
            rep.update(ok=False, offenders=("Z", k, inZ), inside=int(inZ.sum()))
            return rep
        bd = BAND * float((c32[k]["d1"] - d1).abs().max())
        rep["band_d1"] = max(rep["band_d1"], bd)
        ind = (d1.abs() <= bd) | ((d1 - 10).abs() <= bd)
        if ind.any():
            rep.update(ok=False, offenders=("d1", k, ind), inside=int(ind.sum()))
            return rep
        cnt = {}
        for name, fired, idx in (("Z<0.2", Z <= 0.2, jj), ("Z<0.1", Z < 0.1, jj), ("d1>10", d1 > 10, frames), ("d1<0", d1 < 0, frames)):
            n, spared = _fires_and_spares(fired, idx, P)
            cnt[name] = (n, fired.numel())
            if n < MIN_FIRE or not spared:
                rep["ok"] = False
        rep["counts"].append(cnt)
    return rep


def _nudge(s, ii, rep, cuts64, it):
    """move the input disparities behind the offending samples off the band (positive, exact in fp32); `it` varies the size"""
    what, k, mask = rep["offenders"]
    d = s["disps"].clone()
    if what == "Z":                                                             # sample (b, edge, pixel) -> disparity (b, ii[edge], pixel)
        hit = torch.zeros_like(d, dtype=torch.bool)
        for e in mask.any(dim=0).flatten(1).any(1).nonzero().flatten().tolist():
            hit[:, ii[e]] |= mask[:, e]
        step = (0.02 * d + 0.003) * (1 + it % 3)
        d = torch.where(hit, d + step, d)
    else:
        d1 = cuts64[k]["d1"]
        away = torch.where(d1 > 5, torch.where(d1 > 10, 1.0, -1.0), torch.where(d1 > 0, 1.0, -1.0)).to(d.dtype)   # from the threshold it is near
        step = (8 * rep["band_d1"] + 1e-3) * (1 + it % 3)
        moved = d + away * step
        d = torch.where(mask, torch.where(moved < 1e-3, d + 2 * step, moved), d)      # (an input disparity stays positive)
        if k > 0:                                                               # a pixel that the step before masked to 0 does not feel its input
            prev = cuts64[k - 1]["d1"]                                          # disparity any more: move the targets of its edges instead
            stuck = mask & ((prev > 10) | (prev <= 0))
            if stuck.any():
                s = dict(s)
                tgt = s["target"].clone()
                for e in range(ii.shape[0]):
                    tgt[:, e, :, :, 0] += stuck[:, ii[e]].to(tgt.dtype) * (1.0 + it % 3)
                s["target"] = tgt.float().double()
    s = dict(s)
    s["disps"] = d.float().double()
    return s


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(B, P, fixedp, ht, wd, steps):
    """the admitted case with its fp64 reference and the CPU fp32 yardstick"""
    base = 100 * P + 10 * B + fixedp + ht * wd
    for seed in range(base, base + 8):                                          # the first seed whose scene is admitted
        s, ii, jj = _scene(B, P, fixedp, ht, wd, seed)
        nudges = 0
        for it in range(40):
            rep = admission(s, ii, jj, fixedp, steps)
            if rep["offenders"] is None:
                break
            nudges += rep["inside"]
            s = _nudge(s, ii, rep, _cuts_only(s, ii, jj, fixedp, steps, torch.float64), it)
        if rep["ok"]:
            break
    c = Case()
    c.shape, c.s, c.ii, c.jj, c.fixedp, c.steps, c.admission, c.nudged, c.seed = (B, P, fixedp, ht, wd, steps), s, ii, jj, fixedp, steps, rep, nudges, seed
    c.ref, c.cuts = evaluate_torch(s, ii, jj, fixedp, steps, torch.float64)
    c.pt32, _ = evaluate_torch(s, ii, jj, fixedp, steps, torch.float32)
    c.e_pt = errors(c.pt32, c.ref)
    return c


# ---- the acceptance rule -------------------------------------------------------------------------------------------------------------

def outputs_of(ref):
    return [k for k in ref if not k.startswith("_")]


def scale_of(ref, k):
    return float(ref[k].abs().max()) if ref[k].numel() else 0.0


def errors(got, ref):
    """per output: max |got - ref| relative to the largest |ref| (absolute where the reference is all zero or empty)"""
    out = {}
    for k in outputs_of(ref):
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        err = float((got[k] - ref[k]).abs().max()) if ref[k].numel() else 0.0
        if err != err:
            err = float("inf")
        out[k] = err / (scale_of(ref, k) or 1.0)
    return out


def accept(got, ref, e_pt, factor=FACTOR):
    """-> (ratio of the error to e_pt per output, list of what fails): every error at most factor * e_pt; the zero pattern of disps
    and the rejected systems of dx (all-zero rows) exact"""
    err, ratios, bad = errors(got, ref), {}, []
    for k, e in err.items():
        ratios[k] = e / e_pt[k] if e_pt[k] > 0 else (0.0 if e == 0 else float("inf"))
        if not e <= factor * e_pt[k]:
            bad.append("%s: error %.3g of the largest, %.3g x e_pt %.3g" % (k, e, ratios[k], e_pt[k]))
    if not torch.equal(got["disps"] == 0, ref["disps"] == 0):
        bad.append("disps: zero pattern differs at %d samples" % int(((got["disps"] == 0) != (ref["disps"] == 0)).sum()))
    for k in ref:
        if k.startswith("dx") and ref[k].numel():
            rej_r, rej_g = (ref[k] == 0).all(dim=1), (got[k] == 0).all(dim=1)
            if not torch.equal(rej_r, rej_g):
                bad.append("%s: rejected systems differ" % k)
    return ratios, bad


def larger(a, b):
    return {k: max(a[k], b[k]) for k in a}
