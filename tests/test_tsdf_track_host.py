"""Frame-to-model tracking, the yardstick held to itself (CPU, seconds): tests/tsdf_track_reference.py's Jacobian against finite
differences, the conditions the GPU tests rely on (a positive definite H, every start ending at one pose, a falling energy, at most 1 % of
the pixels flagged), the derived bounds against the contract restated in fp32 arithmetic, four deliberately wrong references that the
check must reject, and the binding's struct mirrors against the header."""
import ctypes
import os
import re

import numpy as np
import pytest

import tsdf_reference as R
import tsdf_track_reference as T

_cache = {}
FRAME = 2                                  # the middle camera


def _volume():
    if "vol" not in _cache:
        _cache["vol"] = T.fused_volume()
    return _cache["vol"]


def _scene(size=(24, 32)):
    if ("scene", size) not in _cache:
        _cache[("scene", size)] = T.scene(*size)
    return _cache[("scene", size)]


def _track(size=(24, 32), nstarts=6, mutant=None, **kw):
    """the reference tracker on frame FRAME from the fixed list of starts (and the true pose last)"""
    key = ("track", size, nstarts, mutant, tuple(sorted(kw.items())))
    if key not in _cache:
        poses, disps, intr, weight = _scene(size)
        start = np.stack([T.perturbed(poses[FRAME], xi) for xi in T.starts(nstarts)] + [poses[FRAME]])
        args = dict(T.PARAMS)
        args.update(kw)
        _cache[key] = (T.track_reference(_volume(), start, disps, intr, [FRAME] * len(start), weight=weight, mutant=mutant, **args), start)
    return _cache[key]


def test_jacobian_against_finite_differences():
    """J against central differences of S under Exp(xi) G, on pixels whose cell does not change"""
    poses, disps, intr, weight = _scene()
    vol = _volume()
    pose = T.perturbed(poses[FRAME], T.starts(2)[1] * 0.3)
    e0 = T.evaluate(vol, disps[FRAME], weight[FRAME], intr, pose)
    s64 = vol["tsdf"].astype(np.float64)
    h, worst = 1e-4, 0.0
    cell0 = np.floor(_p(vol, disps[FRAME], intr, pose.astype(np.float64)))
    for i in range(6):
        xi = np.zeros(6)
        xi[i] = h
        S = []
        same = e0["votes"] & ~e0["flagged"]
        for sign in (1, -1):
            p = _p(vol, disps[FRAME], intr, _retract64(sign * xi, pose))          # (the perturbed pose stays fp64: fp32 would cost EPS / h)
            same &= (np.floor(p) == cell0).all(-1)
            cell = np.where(same[..., None], cell0, 0).astype(np.int64).reshape(-1, 3)
            S.append(T.V._trilinear(T.V._corners(s64, cell), p.reshape(-1, 3) - cell)[0].reshape(same.shape))
        assert same.sum() > 100
        fd = (S[0] - S[1]) / (2 * h)
        err, scale = np.abs(fd - e0["J"][..., i])[same], np.abs(e0["J"][..., i])[same].max()
        worst = max(worst, err.max() / scale)
        assert err.max() <= 1e-3 * scale, (i, err.max(), scale)               # (S is trilinear in p, p nearly linear in xi: second order in h)
    print("J against central differences: worst error %.2e of the largest |J_i|" % worst)


def _retract64(xi, pose):
    """Exp(xi) pose in fp64"""
    pose = np.asarray(pose, np.float64)
    dt, dq = T.se3_exp(xi)
    return np.concatenate([R.rotation(dq) @ pose[:3] + dt, T._qmul(dq, pose[3:])])


def _p(vol, disp, intr, pose):
    """voxel coordinates [ht,wd,3] of the frame's pixels at `pose` (fp64)"""
    pose = np.asarray(pose, np.float64)
    ht, wd = disp.shape
    fx, fy, cx, cy = [np.float64(v) for v in intr]
    Rm, t = R.rotation(pose[3:]), pose[:3]
    vv, uu = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    with np.errstate(all="ignore"):
        z = 1.0 / disp.astype(np.float64)
    Xc = np.stack([z * (uu - cx) / fx, z * (vv - cy) / fy, z], -1)
    return ((Xc - t) @ Rm - np.asarray(vol["origin"], np.float32).astype(np.float64)) / np.float64(np.float32(vol["voxel"]))


def test_the_scene_is_well_posed():
    """asserted on the reference ALONE: H positive definite, the starts end at one pose, E falls after the first step"""
    poses, disps, intr, weight = _scene()
    e = T.evaluate(_volume(), disps[FRAME], weight[FRAME], intr, poses[FRAME])
    Hs = e["H"].copy()
    Hs[3:] *= 0.5
    Hs[:, 3:] *= 0.5                                                       # rotations scaled by 0.5 (a lever arm of half a metre)
    ev = np.linalg.eigvalsh(Hs)
    print("H at the true pose: %d of %d pixels contribute, eigenvalues %.3g .. %.3g, condition number %.1f, E %.3f"
          % (e["count"], e["votes"].size, ev[0], ev[-1], ev[-1] / ev[0], e["E"]))
    assert ev[0] > 0 and ev[-1] / ev[0] < 500 and e["count"] > 0.4 * e["votes"].size
    for band in (0.9, 0.6):
        ref, start = _track(band=band)
        final, truth = ref["poses"], poses[FRAME]
        assert np.all(ref["info"][:, :, 3] == 0)
        to_truth = np.array([T.pose_difference(p, truth) for p in final])
        spread = max(T.pose_difference(a, b) for a in final for b in final)
        off = np.array([T.pose_difference(p, truth) for p in start])
        print("band %.1f: starts %.4f .. %.4f from the truth end %.5f .. %.5f from it, %.2e from each other; E %.3f -> %.3f; final pose %s"
              % (band, off[:-1].min(), off.max(), to_truth.min(), to_truth.max(), spread, ref["info"][0, 0, 0], ref["info"][0, -1, 0],
                 np.array2string(final[0], precision=5)))
        assert spread <= 0.01 * to_truth.min()
        E = ref["info"][:, :, 0]
        assert np.all(E[:-1, -1] < E[:-1, 0])
        # monotone after the first step: the energy over a FIXED set of pixels, those that vote at the final pose (the info rows' E is
        # over the votes of its own evaluation: while the pose moves pixels enter the band and bring their energy, so with band 0.6 it
        # rises once, 4.6 -> 4.7 at most, although every pixel's residual falls)
        vol = _volume()
        for s_ in range(len(final)):
            fixed, seq = ref["votes"][s_], []
            for e_ in range(ref["trail"].shape[1]):
                ev_ = T.evaluate(vol, disps[FRAME], weight[FRAME], intr, ref["trail"][s_, e_], band=1.0)
                seq.append((ev_["weight"] * ev_["S"] ** 2)[fixed & ev_["valid"]].sum())
            seq = np.array(seq)
            assert np.all(seq[2:] <= seq[1:-1] * (1 + 1e-12)), (band, s_, seq)
        if band == 0.9:                      # (there the rows' own E is monotone as well)
            assert np.all(E[:, 2:] <= E[:, 1:-1] * (1 + 1e-12)), E


@pytest.mark.parametrize("size", T.SIZES)
def test_few_pixels_are_flagged(size):
    poses, disps, intr, weight = _scene(size)
    flagged = total = 0
    for band, huber in ((0.9, 0.0), (0.6, 0.3)):
        for f in range(T.NFRAMES):
            for xi in np.concatenate([np.zeros((1, 6)), T.starts(3)]):
                e = T.evaluate(_volume(), disps[f], weight[f], intr, T.perturbed(poses[f], xi), band=band, huber=huber)
                flagged, total = flagged + e["nflag"], total + e["flagged"].size
    print("%dx%d: %d of %d pixel evaluations flagged (%.3f %%)" % (size[0], size[1], flagged, total, 100.0 * flagged / total))
    assert flagged <= 0.01 * total


# ------------------------------------------------------------------------------------------------ the contract in fp32 arithmetic
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _lerp(a, b, t):
    return _fma(t, b - a, a)


def evaluate_fp32(vol, disp, weight, intr, pose, band, huber):
    """include/pvo_hip.h's evaluation with every operation rounded to fp32 and every multiply-add fused, pixel by pixel: residual (NaN =
    no vote), jac and the 28 sums (summed in fp64: the tree is test_tsdf_track_gpu's matter)"""
    f = np.float32
    tsdf, wsum = vol["tsdf"], vol["wsum"]
    nz, ny, nx = tsdf.shape
    n = np.array([nx, ny, nz])
    o, voxel = np.asarray(vol["origin"], f), f(vol["voxel"])
    x, y, z, w = [f(v) for v in pose[3:]]
    t = np.asarray(pose[:3], f)
    two, one = f(2), f(1)
    r = np.array([one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w),
                  two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w),
                  two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)], f)
    M = np.zeros(9, f)
    p0 = np.zeros(3, f)
    for i in range(3):
        for j in range(3):
            M[3 * i + j] = r[3 * j + i] / voxel
        c = -_fma(r[6 + i], t[2], _fma(r[3 + i], t[1], r[i] * t[0]))
        p0[i] = (c - o[i]) / voxel
    ht, wd = disp.shape
    fx, fy, cx, cy = [f(v) for v in intr]
    vv, uu = np.meshgrid(np.arange(ht, dtype=f), np.arange(wd, dtype=f), indexing="ij")
    rx, ry = ((uu - cx) / fx).reshape(-1), ((vv - cy) / fy).reshape(-1)
    d = disp.reshape(-1)
    wt = np.ones_like(d) if weight is None else weight.reshape(-1)
    with np.errstate(all="ignore"):
        ok = np.isfinite(d) & (d > 0) & np.isfinite(wt) & (wt > 0)
        zz = (one / np.where(ok, d, one)).astype(f)
    g = [_fma(M[3 * i], rx, _fma(M[3 * i + 1], ry, np.full_like(rx, M[3 * i + 2]))) for i in range(3)]
    p = np.stack([_fma(zz, g[i], np.full_like(rx, p0[i])) for i in range(3)], 1)
    inbox = ok & np.all((p >= 0) & (p <= (n - 1).astype(f)), 1)
    cell = np.minimum(np.floor(np.where(inbox[:, None], p, 0)).astype(np.int64), n - 2)
    valid = inbox & T.V._corners(wsum >= f(1.0), cell).all(1)
    fr = (p - cell.astype(f)).astype(f)
    s = T.V._corners(tsdf, cell)
    fx_, fy_, fz_ = fr[:, 0], fr[:, 1], fr[:, 2]
    b0 = _lerp(_lerp(s[:, 0], s[:, 1], fx_), _lerp(s[:, 2], s[:, 3], fx_), fy_)
    b1 = _lerp(_lerp(s[:, 4], s[:, 5], fx_), _lerp(s[:, 6], s[:, 7], fx_), fy_)
    S = _lerp(b0, b1, fz_)
    gr = [_lerp(_lerp(s[:, 1] - s[:, 0], s[:, 3] - s[:, 2], fy_), _lerp(s[:, 5] - s[:, 4], s[:, 7] - s[:, 6], fy_), fz_),
          _lerp(_lerp(s[:, 2] - s[:, 0], s[:, 3] - s[:, 1], fx_), _lerp(s[:, 6] - s[:, 4], s[:, 7] - s[:, 5], fx_), fz_),
          _lerp(_lerp(s[:, 4] - s[:, 0], s[:, 5] - s[:, 1], fx_), _lerp(s[:, 6] - s[:, 2], s[:, 7] - s[:, 3], fx_), fy_)]
    a = np.abs(S)
    votes = valid & (a < f(band))
    gc = [_fma(np.full_like(rx, M[i]), gr[0], _fma(np.full_like(rx, M[3 + i]), gr[1], M[6 + i] * gr[2])) for i in range(3)]
    X = [zz * rx, zz * ry, zz]
    J = np.stack([-gc[0], -gc[1], -gc[2], -_fma(X[1], gc[2], -(X[2] * gc[1])), -_fma(X[2], gc[0], -(X[0] * gc[2])),
                  -_fma(X[0], gc[1], -(X[1] * gc[0]))], 1)
    h = f(huber)
    with np.errstate(all="ignore"):
        quad = (h == 0) | (a <= h)
        k = np.where(quad, one, h / a).astype(f)
        rho = np.where(quad, S * S, h * _fma(np.full_like(a, two), a, np.full_like(a, -h))).astype(f)
    wk = (wt * k).astype(f)
    terms = []
    for i in range(6):
        wj = wk * J[:, i]
        terms += [wj * J[:, j] for j in range(i, 6)]
    for i in range(6):
        terms.append(wk * J[:, i] * S)
    terms.append(wt * rho)
    terms = np.stack(terms, 1).astype(np.float64)
    terms = np.concatenate([terms[:, :21], terms[:, 21:27], terms[:, 27:]], 1)
    sums = np.where(votes[:, None], terms, 0.0).sum(0)
    return (np.where(votes, S, np.nan).reshape(ht, wd).astype(f), np.where(votes[:, None], J, 0).reshape(ht, wd, 6).astype(f), sums,
            int(votes.sum()))


@pytest.mark.parametrize("size", T.SIZES)
def test_the_bounds_hold_for_the_contract_in_fp32(size):
    """every output of the fp32 restatement within the derived bounds of the fp64 reference, through the same check the kernel gets"""
    poses, disps, intr, weight = _scene(size)
    vol = _volume()
    start = np.stack([T.perturbed(poses[f], xi) for f, xi in zip((0, 2, 4), T.starts(3) * 0.5)])
    for band, huber in ((0.9, 0.0), (0.6, 0.3)):
        ref = T.track_reference(vol, start, disps, intr, [0, 2, 4], weight=weight, iters=0, band=band, huber=huber)
        got = dict(poses=start, info=np.zeros((3, 1, 4), np.float32), residual=np.zeros((3,) + size, np.float32),
                   jac=np.zeros((3,) + size + (6,), np.float32), system=np.zeros((3, 27)))
        for s, f in enumerate((0, 2, 4)):
            res, jac, sums, count = evaluate_fp32(vol, disps[f], weight[f], intr, start[s], band, huber)
            got["residual"][s], got["jac"][s], got["system"][s] = res, jac, sums[:27]
            got["info"][s, 0] = (sums[27], count, 0.0, 0.0 if count >= T.PARAMS["min_count"] else 1.0)
            ok, worst = T.reduction_check(sums[:27], got["info"][s, 0], res, jac, weight[f], huber)
            assert ok, worst
        ok, report = T.track_matches(got, ref)
        print("%dx%d band %.1f huber %.1f: %s" % (size[0], size[1], band, huber, report))
        assert ok, report


def _outer(mutant, iters):
    """the reference tracker on the two outer cameras (the poses farthest from the identity) from full-extent starts"""
    key = ("outer", mutant, iters)
    if key not in _cache:
        poses, disps, intr, weight = _scene()
        xs = T.starts(4)
        start = np.stack([T.perturbed(poses[f], x) for f, x in zip((0, 4, 4, 0), xs)])
        _cache[key] = T.track_reference(_volume(), start, disps, intr, [0, 4, 4, 0], weight=weight, mutant=mutant, **dict(T.PARAMS, iters=iters))
    return _cache[key]


@pytest.mark.parametrize("mutant", T.MUTANTS)
def test_the_check_rejects_a_wrong_reference(mutant):
    """the checks the kernel gets - an evaluation alone (iters = 0: per pixel) and one step (iters = 1: the pose) - pass on the
    reference itself and fail, one or the other, against each wrong reference"""
    verdicts = []
    for iters in (0, 1):
        good = _outer(None, iters)
        ok, report = T.track_matches(T.as_got(good), good)
        assert ok, report                                                  # the reference passes its own check
        ok, report = T.track_matches(T.as_got(good), _outer(mutant, iters))
        print(mutant, "iters", iters, report)
        verdicts.append(ok)
    assert not all(verdicts)
    if mutant == "right_retraction":
        assert verdicts[0]                                                 # (an evaluation alone cannot tell: it takes the step)


def test_the_struct_mirrors_follow_the_header():
    from pvo_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvo_hip.h")).read()
    for name, mirror in (("pvo_tsdf_track_args", _lib.TsdfTrackArgs), ("pvo_tsdf_sparse_track_args", _lib.TsdfSparseTrackArgs)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        fields = []
        for line in body.split(";"):
            line = line.strip()
            if not line:
                continue
            names = line.split(",")
            names[0] = names[0].split()[-1]
            fields += [re.sub(r"[\*\s]|\[\d+\]", "", v) for v in names]
        assert fields == [f[0] for f in mirror._fields_], name
        assert mirror.__doc__ == name
    assert ctypes.sizeof(_lib.TsdfSparseTrackArgs) >= ctypes.sizeof(_lib.TsdfTrackArgs)
    assert _lib.TSDF_TRACK_MAX_ITERS == int(re.search(r"#define PVO_TSDF_TRACK_MAX_ITERS (\d+)", header).group(1))
