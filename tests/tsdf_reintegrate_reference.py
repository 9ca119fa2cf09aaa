"""The live volume's yardstick (tests/test_tsdf_reintegrate_host.py, tests/test_tsdf_reintegrate_gpu.py): the contract of
pvo_tsdf_reintegrate (include/pvo_hip.h) restated in numpy on top of tests/tsdf_reference.py.  As there, geometry and averages are
evaluated in fp64 on the fp32 inputs, and the weight sum is the contract's fp32 number on both sides (Wn = W + w or W - w rounded to
fp32), held to EQUALITY.  The emptying decision !(Wn > w_floor) compares two fp32 numbers that are the same on both sides, so it cannot
flip.

A state (dict) is a volume with the bound it has accumulated: tsdf f64, wsum f32, rgb f64 [..,3] or None, bound / bound_rgb f64 (the
kernel's error against this reference, per voxel), touched bool (some call wrote the voxel), flagged bool (sticky: some decision of some
slot of some call was within rounding of flipping), emptied bool (the voxel's LAST write emptied it).  reintegrate_reference maps a
state to the next one, so a whole remove-then-add history carries its bound along.

Bound of one slot (EPS = 2^-24, first order, the kernel in fp32 with contraction, which only removes roundings; E_val from
tsdf_reference's derivation, the observation being formed by the same expressions):
  ADD     tsdf_reference's:  E_T' = (E_T W + E_val w) / Wn + K_AVG EPS,  E_C' = E_C W / Wn + 255 K_AVG EPS
  REMOVE  T' = clamp((T W - val w) / Wn, -1, 1), Wn = W - w the same fp32 number on both sides.
          Incoming errors: the numerator moves by at most E_T W + E_val w, the quotient by that over Wn - the incoming bound times W / Wn.
          Own roundings, with |T|, |val| <= 1: the product T W: EPS W; the product val w: EPS w; their difference, of magnitude
          <= W + w: EPS (W + w); the division, one ulp = 2 EPS of a quotient of magnitude <= (W + w) / Wn.  Over Wn the first three
          give 2 EPS (W + w) / Wn, with the division 4 EPS (W + w) / Wn; K_UN = 5 absorbs the second order, as K_AVG does.  The clamp
          is 1-Lipschitz and both sides lie in [-1, 1], hence the cap at 2:
              E_T' = min(2, (E_T W + E_val w) / Wn + K_UN EPS (W + w) / Wn)
          Colours (<= 255, the pixel's colour exact on both sides, clamp to [0, 255]):
              E_C' = min(255, E_C W / Wn + 255 K_UN EPS (W + w) / Wn)
          An emptied voxel is exactly zero on both sides: E_T' = E_C' = 0.
Unlike an addition, a removal AMPLIFIES what came in by W / Wn > 1: the bound says something only while that ratio stays small, which
the tests secure through their inputs (weights in [0.25, 1]: at most 14.5 when four of five frames go) and print.

Flags are tsdf_reference's decision flags, evaluated for the operands of BOTH sets (a removal decides by the same tests)."""
import numpy as np

import tsdf_reference as R

EPS, K_CAM, K_AVG, PIXEL_BAND = R.EPS, R.K_CAM, R.K_AVG, R.PIXEL_BAND
K_UN = 5
W_FLOOR = 2.0 ** -10
PUSH = (0.031, -0.017, 0.023)          # the move of a keyframe the tests use (a camera-frame translation): off every optical axis


def empty_state(dims, colours=True):
    dims = tuple(dims)
    return dict(tsdf=np.zeros(dims), wsum=np.zeros(dims, np.float32), rgb=np.zeros(dims + (3,)) if colours else None,
                bound=np.zeros(dims), bound_rgb=np.zeros(dims), touched=np.zeros(dims, bool), flagged=np.zeros(dims, bool),
                emptied=np.zeros(dims, bool), hits=0, max_ratio=1.0)


def observe(dims, origin, voxel, trunc, pose, disp, intr, weight=None, image=None, img_stride=8, img_offset=3, z_near=0.0):
    """what ONE frame (pose [7], disp [ht,wd], weight [ht,wd] or None, image uint8 [3,IH,IW] or None) contributes to every voxel:
    dict(ok bool, val f64, w f32 (0 where not ok), col f64 [..,3] or None, E_val f64, flagged bool) - pvo_tsdf_integrate's tests in
    their order, tsdf_reference.integrate_reference's expressions"""
    nz, ny, nx = dims
    ht, wd = disp.shape
    o = np.asarray(origin, np.float32).astype(np.float64)
    voxel, trunc, z_near = np.float64(np.float32(voxel)), np.float64(np.float32(trunc)), np.float64(np.float32(z_near))
    fx, fy, cx, cy = [np.float64(v) for v in np.asarray(intr, np.float32)]
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    X = o + voxel * np.stack([xx, yy, zz], -1).astype(np.float64)
    ksum = voxel * (xx + yy + zz)
    pose = np.asarray(pose, np.float32)
    Rm, t = R.rotation(pose[3:]), pose[:3].astype(np.float64)
    Xc = X @ Rm.T + t
    xc, yc, zc = Xc[..., 0], Xc[..., 1], Xc[..., 2]
    E_c = K_CAM * EPS * (ksum + np.abs(o).sum() + np.abs(t).sum())
    flagged = np.abs(zc - z_near) <= E_c
    ok = zc > z_near
    with np.errstate(all="ignore"):
        qx, qy = xc / zc, yc / zc
        u, v = fx * qx + cx, fy * qy + cy
        ru, rv = np.floor(u + 0.5), np.floor(v + 0.5)
        E_u = fx * ((1 + np.abs(qx)) * E_c / zc + 3 * EPS * np.abs(qx)) + 2 * EPS * (np.abs(fx * qx) + abs(cx) + 0.5)
        E_v = fy * ((1 + np.abs(qy)) * E_c / zc + 3 * EPS * np.abs(qy)) + 2 * EPS * (np.abs(fy * qy) + abs(cy) + 0.5)
        near = ok & (ru >= -1) & (ru <= wd) & (rv >= -1) & (rv <= ht)
        du, dv = np.abs(u + 0.5 - np.round(u + 0.5)), np.abs(v + 0.5 - np.round(v + 0.5))
        flagged |= near & ((du <= np.maximum(PIXEL_BAND, E_u)) | (dv <= np.maximum(PIXEL_BAND, E_v)))
    ok &= np.isfinite(ru) & np.isfinite(rv) & (ru >= 0) & (ru < wd) & (rv >= 0) & (rv < ht)
    ui = np.where(ok, ru, 0).astype(np.int64)
    vi = np.where(ok, rv, 0).astype(np.int64)
    d32 = np.asarray(disp, np.float32)[vi, ui]
    w32 = np.ones(dims, np.float32) if weight is None else np.asarray(weight, np.float32)[vi, ui]
    with np.errstate(all="ignore"):
        ok &= np.isfinite(d32) & (d32 > 0) & np.isfinite(w32) & (w32 > 0)
        d = np.where(ok, d32, 1).astype(np.float64)
        sdf = 1.0 / d - zc
        E_s = 2 * EPS / d + E_c + EPS * np.abs(sdf)
        flagged |= ok & (np.abs(sdf + trunc) <= E_s)
        ok &= ~(sdf < -trunc)
        val = np.minimum(1.0, sdf / trunc)
        E_val = E_s / trunc + 2 * EPS
    col = None
    if image is not None:
        im = np.asarray(image)
        col = np.stack([im[c][img_stride * vi + img_offset, img_stride * ui + img_offset] for c in (2, 1, 0)], -1).astype(np.float64)
    return dict(ok=ok, val=val, w=np.where(ok, w32, np.float32(0)).astype(np.float32), col=col, E_val=E_val, flagged=flagged)


MUTANTS = ("new_poses", "unit_removal", "keep_emptied", "keep_colours")


def reintegrate_reference(state, origin, voxel, trunc, intr, remove=None, add=None, images=None, img_stride=8, img_offset=3, z_near=0.0,
                          w_max=0.0, w_floor=W_FLOOR, mutant=None):
    """pvo_tsdf_reintegrate on `state` (not modified); returns the next state.  remove / add: (poses [nframes,7], disps [nframes,ht,wd],
    ix, weight [nframes,ht,wd] or None) or None.  mutant: None or one of MUTANTS - a removal projected with the ADD set's poses, a
    removal that ignores w (takes 1), an emptied voxel left with its last tsdf and wsum, colours not de-integrated: deliberately wrong
    variants the tests must be able to tell apart."""
    s = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}
    dims = s["tsdf"].shape
    colours = s["rgb"] is not None and images is not None
    T, W, C, E_T, E_C = s["tsdf"], s["wsum"], s["rgb"], s["bound"], s["bound_rgb"]
    w_floor32, w_max32 = np.float32(w_floor), np.float32(w_max)

    def frames(fs):
        if fs is None:
            return
        poses, disps, ix, weight = fs
        nf = np.asarray(disps).shape[0]
        for f in [int(v) for v in np.asarray(ix).reshape(-1)]:
            if 0 <= f < nf:
                yield f, poses, disps, weight

    for f, poses, disps, weight in frames(remove):
        if mutant == "new_poses" and add is not None:
            poses = add[0]
        ob = observe(dims, origin, voxel, trunc, poses[f], disps[f], intr, None if weight is None else weight[f],
                     images[f] if colours else None, img_stride, img_offset, z_near)
        ok, w32 = ob["ok"], ob["w"]
        if mutant == "unit_removal":
            w32 = np.where(ok, np.float32(1), np.float32(0)).astype(np.float32)
        s["flagged"] |= ob["flagged"]
        Wn32 = (W - w32).astype(np.float32)                                  # the contract's fp32 difference
        gone = ok & ~(Wn32 > w_floor32)
        live = ok & ~gone
        Wd, wd64, Wn = W.astype(np.float64), w32.astype(np.float64), np.where(live, Wn32, 1).astype(np.float64)
        s["max_ratio"] = max(s["max_ratio"], float((Wd / Wn)[live].max()) if live.any() else 1.0)
        Tn = np.clip((T * Wd - ob["val"] * wd64) / Wn, -1.0, 1.0)
        E_Tn = np.minimum(2.0, (E_T * Wd + ob["E_val"] * wd64) / Wn + K_UN * EPS * (Wd + wd64) / Wn)
        if colours:
            if mutant != "keep_colours":
                Cn = np.clip((C * Wd[..., None] - ob["col"] * wd64[..., None]) / Wn[..., None], 0.0, 255.0)
                C = np.where(live[..., None], Cn, C)
            E_C = np.where(live, np.minimum(255.0, E_C * Wd / Wn + 255 * K_UN * EPS * (Wd + wd64) / Wn), E_C)
        T, E_T = np.where(live, Tn, T), np.where(live, E_Tn, E_T)
        W = np.where(live, Wn32, W).astype(np.float32)
        if mutant != "keep_emptied":
            T, W = np.where(gone, 0.0, T), np.where(gone, np.float32(0), W).astype(np.float32)
            if C is not None:
                C = np.where(gone[..., None], 0.0, C)
        E_T, E_C = np.where(gone, 0.0, E_T), np.where(gone, 0.0, E_C)
        s["touched"] |= ok
        s["emptied"] = (s["emptied"] & ~live) | gone
        s["hits"] += int(ok.sum())

    for f, poses, disps, weight in frames(add):
        ob = observe(dims, origin, voxel, trunc, poses[f], disps[f], intr, None if weight is None else weight[f],
                     images[f] if colours else None, img_stride, img_offset, z_near)
        ok, w32 = ob["ok"], ob["w"]
        s["flagged"] |= ob["flagged"]
        Wn32 = (W + w32).astype(np.float32)                                  # the contract's fp32 sum
        Wd, wd64, Wn = W.astype(np.float64), w32.astype(np.float64), np.where(ok, Wn32, 1).astype(np.float64)
        T = np.where(ok, (T * Wd + ob["val"] * wd64) / Wn, T)
        E_T = np.where(ok, (E_T * Wd + ob["E_val"] * wd64) / Wn + K_AVG * EPS, E_T)
        if colours:
            C = np.where(ok[..., None], (C * Wd[..., None] + ob["col"] * wd64[..., None]) / Wn[..., None], C)
            E_C = np.where(ok, E_C * Wd / Wn + 255 * K_AVG * EPS, E_C)
        if w_max32 > 0:
            s["flagged"] |= ok & (Wn32 != w_max32) & (np.abs(Wn32.astype(np.float64) - np.float64(w_max32)) <= 2 * EPS * np.float64(w_max32))
            Wn32 = np.where(Wn32 > w_max32, w_max32, Wn32).astype(np.float32)
        W = np.where(ok, Wn32, W).astype(np.float32)
        s["touched"] |= ok
        s["emptied"] &= ~ok
        s["hits"] += int(ok.sum())

    s.update(tsdf=T, wsum=W, rgb=C, bound=E_T, bound_rgb=E_C)
    return s


def state_matches(got_tsdf, got_wsum, got_rgb, ref):
    """the check of the re-integration tests, on the voxels that are not flagged: wsum EQUAL (hence the emptied set equal), tsdf / rgb
    within the carried bound, and every voxel the reference holds empty (never touched, or emptied) bit-for-bit zero.
    Returns (ok, report); the report has the measured share of the bound."""
    un = ~ref["flagged"]
    w_ok = np.array_equal(got_wsum[un], ref["wsum"][un])
    e_ok = np.array_equal((got_wsum == 0)[un], (ref["wsum"] == 0)[un])
    err = np.abs(got_tsdf.astype(np.float64) - ref["tsdf"])
    t_ok = bool(np.all(err[un] <= ref["bound"][un]))
    rest = un & (ref["wsum"] == 0) & ((ref["tsdf"] == 0) | ~ref["touched"])
    z_ok = not got_tsdf.view(np.uint32)[rest].any() and not got_wsum.view(np.uint32)[rest].any()
    c_ok, cerr, cshare = True, 0.0, 0.0
    live = un & (ref["bound"] > 0)
    if got_rgb is not None:
        ce = np.abs(got_rgb.astype(np.float64) - ref["rgb"]).max(-1)
        c_ok = bool(np.all(ce[un] <= ref["bound_rgb"][un])) and not got_rgb.view(np.uint32)[rest].any()
        cerr = float(ce[un].max())
        cshare = float((ce[live] / ref["bound_rgb"][live]).max()) if live.any() else 0.0
    report = ("wsum equal %s, emptied set equal %s, tsdf max err %.3e (max err / bound %.3f, max bound %.3e), rgb max err %.3e (max err / "
              "bound %.3f, max bound %.3e), empty voxels zero %s" % (
                  w_ok, e_ok, err[un].max(), (err[live] / ref["bound"][live]).max() if live.any() else 0.0, ref["bound"][un].max(),
                  cerr, cshare, ref["bound_rgb"][un].max(), z_ok))
    return w_ok and e_ok and t_ok and z_ok and c_ok, report


# ------------------------------------------------------------------------------------------------------------ inputs
def nondyadic_weights(shape, seed=11):
    """weights uniform in [0.25, 1): sums of them are NOT exact in fp32, unlike the scene's multiples of 1/64"""
    return (0.25 + 0.75 * np.random.default_rng(seed).random(shape)).astype(np.float32)


_cases = {}


def case(name, weights="scene"):
    """the inputs of the tests on a scene of tsdf_reference.SCENES, computed once and never modified: weights "scene" (multiples of
    1/64, whose sums are exact), "nondyadic" or "unit" (weight None).  A dict: dims, origin, voxel, trunc, nf, k (the middle keyframe),
    poses, disps, intr, images, weight, and poses2 / disps2 with keyframe k pushed; rest = the keyframes other than k"""
    key = (name, weights)
    if key not in _cases:
        nf, ht, wd, dims, origin, voxel, trunc = R.SCENES[name]
        poses, disps, intr, images, weight, hit = R.scene(nf, ht, wd)
        w = {"scene": weight, "nondyadic": nondyadic_weights(weight.shape), "unit": None}[weights]
        k = nf // 2
        poses2, disps2 = pushed(poses, disps, k)
        _cases[key] = dict(dims=dims, origin=origin, voxel=voxel, trunc=trunc, nf=nf, k=k, poses=poses, disps=disps, intr=intr, images=images,
                           weight=w, poses2=poses2, disps2=disps2, rest=[f for f in range(nf) if f != k])
    return _cases[key]


def run(c, state, remove=None, add=None, moved=False, colours=True, **kw):
    """reintegrate_reference on a case: remove / add are lists of keyframes; remove reads the case's original frames, add the original
    ones or with moved=True the pushed ones"""
    rm = None if remove is None else (c["poses"], c["disps"], remove, c["weight"])
    ad = None if add is None else ((c["poses2"], c["disps2"]) if moved else (c["poses"], c["disps"])) + (add, c["weight"])
    return reintegrate_reference(state, c["origin"], c["voxel"], c["trunc"], c["intr"], remove=rm, add=ad,
                                 images=c["images"] if colours else None, img_stride=1, img_offset=0, **kw)


def pushed(poses, disps, k, push=PUSH, seed=5, rel=0.01):
    """the scene with keyframe k moved: its camera-frame translation pushed by `push` and its depths perturbed by up to rel (1 %)"""
    poses, disps = np.array(poses, np.float32), np.array(disps, np.float32)
    poses[k, :3] += np.asarray(push, np.float32)
    disps[k] *= (1.0 + rel * (2.0 * np.random.default_rng(seed).random(disps[k].shape) - 1.0)).astype(np.float32)
    return poses, disps
