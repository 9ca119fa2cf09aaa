"""The panoptic surface reconstruction's yardstick (tests/test_tsdf_panoptic_host.py, tests/test_tsdf_panoptic_gpu.py): the label vote
of pvo_tsdf_integrate_panoptic and the vertex-label rule of pvo_tsdf_mesh_panoptic (include/pvo_hip.h) restated in numpy, on top of
tests/tsdf_reference.py, which is imported and not changed.

The vote.  Which (voxel, frame) pairs contribute, and with which pixel, are the decisions of tsdf_reference.integrate_reference; its loop
keeps them to itself, so integrate_panoptic_reference walks the frames with the same fp64 formulae and then REQUIRES that its weight
sum, its touched set and its flags are that function's (an assertion on every call).  The vote itself is the contract's sequence in
np.float32, one rounded operation each - lconf + w, w - lconf, lconf - w involve no product, so the kernel's multiply-add contraction
cannot touch them: on voxels whose decisions are safe, label and lconf are held to EQUALITY.

Flags.  The vote adds one decision to the reference's: sdf <= trunc.  The kernel's sdf differs from the exact one by at most the
reference's counted E_s = 2 EPS / d + E_c + EPS |sdf| (tsdf_reference's docstring), so a voxel is also flagged when for some
contributing frame |sdf - trunc| <= E_s.  L > 0, label == L, lconf < w and lconf > w_max compare numbers that are the same on both
sides and cannot flip.

The vertex label is comparisons on the fp32 volume: exact."""
import numpy as np

import tsdf_reference as R

EPS = R.EPS
PLANE_ID = (1 << 24) + 5                  # above 2^24: a float could not carry them
SPHERE_ID = (1 << 25) + 3
OTHER_ID = (1 << 24) + 7                  # what the disagreeing frame calls the plane
MUTANTS = ("free_space", "unweighted", "last_wins", "never_switch")


def label_maps(hit, div=1, odd_frame=1, patches=True):
    """per-frame id maps int32 [nf, ceil(ht/div), ceil(wd/div)] for tsdf_reference.scene's `hit` (the pixel sees the sphere), sampled at
    the centre pixel of each div x div cell: the sphere SPHERE_ID, the plane PLANE_ID; frame odd_frame disagrees (it calls the plane
    OTHER_ID and the sphere PLANE_ID), so votes switch there and switch back later; a patch of 0 and a patch of negative ids in
    every frame, at places that move with the frame.  odd_frame=-1, patches=False: every frame agrees and every pixel has an id"""
    nf, ht, wd = hit.shape
    c = div // 2
    h = hit[:, c::div, c::div]
    lab = np.where(h, SPHERE_ID, PLANE_ID).astype(np.int32)
    if 0 <= odd_frame < nf:
        lab[odd_frame] = np.where(h[odd_frame], PLANE_ID, OTHER_ID)
    lh, lw = lab.shape[1:]
    for f in range(nf if patches else 0):
        y0, x0 = (f + lh // 3) % lh, (2 * f + lw // 4) % lw
        lab[f, y0:y0 + max(1, lh // 4), x0:x0 + max(1, lw // 5)] = 0
        y1, x1 = (f + (2 * lh) // 3) % lh, (3 * f + lw // 2) % lw
        lab[f, y1:y1 + max(1, lh // 5), x1:x1 + max(1, lw // 4)] = -7 - f
    return lab


def integrate_panoptic_reference(dims, origin, voxel, trunc, poses, disps, intr, ix, labels, label_div=1, weight=None, z_near=0.0,
                                 w_max=0.0, mutant=None, check=True):
    """pvo_tsdf_integrate_panoptic's label volumes from ZEROED ones.  Returns dict(label int32, lconf f32, wsum f32, touched bool,
    flagged bool (the reference's flags and the vote's), flagged_base bool, switches int: how often each voxel's label changed from
    one positive id to another, voters: the number of pairs that voted).
    mutant: None or one of MUTANTS - "free_space" (sdf > trunc votes as well), "unweighted" (every vote weighs 1), "last_wins"
    (the latest label replaces the held one), "never_switch" (the first label stays; a disagreeing vote only lowers lconf, not below
    0) - deliberately wrong variants the tests must tell apart."""
    poses, disps, intr = np.asarray(poses, np.float32), np.asarray(disps, np.float32), np.asarray(intr, np.float32)
    labels = np.asarray(labels)
    assert labels.dtype == np.int32
    nf, ht, wd = disps.shape
    nz, ny, nx = dims
    o = np.asarray(origin, np.float32).astype(np.float64)
    voxel, trunc = np.float64(np.float32(voxel)), np.float64(np.float32(trunc))
    z_near, w_max = np.float64(np.float32(z_near)), np.float32(w_max)
    fx, fy, cx, cy = [np.float64(v) for v in intr]
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    X = o + voxel * np.stack([xx, yy, zz], -1).astype(np.float64)
    ksum = voxel * (xx + yy + zz)
    W = np.zeros(dims, np.float32)
    label, lconf = np.zeros(dims, np.int32), np.zeros(dims, np.float32)
    touched, flagged, band = np.zeros(dims, bool), np.zeros(dims, bool), np.zeros(dims, bool)
    switches = np.zeros(dims, int)
    voters = 0
    one = np.float32(1)
    for f in [int(v) for v in np.asarray(ix).reshape(-1)]:
        if not 0 <= f < nf:
            continue
        # ---- tsdf_reference.integrate_reference's decisions, formula for formula
        Rm, t = R.rotation(poses[f, 3:]), poses[f, :3].astype(np.float64)
        Xc = X @ Rm.T + t
        xc, yc, zc = Xc[..., 0], Xc[..., 1], Xc[..., 2]
        E_c = R.K_CAM * EPS * (ksum + np.abs(o).sum() + np.abs(t).sum())
        flagged |= np.abs(zc - z_near) <= E_c
        ok = zc > z_near
        with np.errstate(all="ignore"):
            qx, qy = xc / zc, yc / zc
            u, v = fx * qx + cx, fy * qy + cy
            ru, rv = np.floor(u + 0.5), np.floor(v + 0.5)
            E_u = fx * ((1 + np.abs(qx)) * E_c / zc + 3 * EPS * np.abs(qx)) + 2 * EPS * (np.abs(fx * qx) + abs(cx) + 0.5)
            E_v = fy * ((1 + np.abs(qy)) * E_c / zc + 3 * EPS * np.abs(qy)) + 2 * EPS * (np.abs(fy * qy) + abs(cy) + 0.5)
            near = ok & (ru >= -1) & (ru <= wd) & (rv >= -1) & (rv <= ht)
            du, dv = np.abs(u + 0.5 - np.round(u + 0.5)), np.abs(v + 0.5 - np.round(v + 0.5))
            flagged |= near & ((du <= np.maximum(R.PIXEL_BAND, E_u)) | (dv <= np.maximum(R.PIXEL_BAND, E_v)))
        ok &= np.isfinite(ru) & np.isfinite(rv) & (ru >= 0) & (ru < wd) & (rv >= 0) & (rv < ht)
        ui = np.where(ok, ru, 0).astype(np.int64)
        vi = np.where(ok, rv, 0).astype(np.int64)
        d32 = disps[f][vi, ui]
        w32 = np.ones(dims, np.float32) if weight is None else np.asarray(weight, np.float32)[f][vi, ui]
        with np.errstate(all="ignore"):
            ok &= np.isfinite(d32) & (d32 > 0) & np.isfinite(w32) & (w32 > 0)
            d = np.where(ok, d32, 1).astype(np.float64)
            sdf = 1.0 / d - zc
            E_s = 2 * EPS / d + E_c + EPS * np.abs(sdf)
            flagged |= ok & (np.abs(sdf + trunc) <= E_s)
            ok &= ~(sdf < -trunc)
        w32 = np.where(ok, w32, np.float32(0)).astype(np.float32)
        Wn32 = (W + w32).astype(np.float32)
        if w_max > 0:
            flagged |= ok & (Wn32 != w_max) & (np.abs(Wn32.astype(np.float64) - np.float64(w_max)) <= 2 * EPS * np.float64(w_max))
            Wn32 = np.where(Wn32 > w_max, w_max, Wn32).astype(np.float32)
        W = np.where(ok, Wn32, W).astype(np.float32)
        touched |= ok
        # ---- the vote: the added decision, then the contract's sequence in fp32
        band |= ok & (np.abs(sdf - trunc) <= E_s)
        L = labels[f][vi // label_div, ui // label_div]
        vote = ok & (L > 0)
        if mutant != "free_space":
            vote &= sdf <= trunc
        w = np.where(vote, one if mutant == "unweighted" else w32, np.float32(0)).astype(np.float32)
        same = vote & (label == L)
        if mutant == "last_wins":
            take, lose = vote & ~same, np.zeros(dims, bool)
            new = np.where(same, lconf + w, np.where(take, w, lconf))
        elif mutant == "never_switch":
            take, lose = vote & (label == 0), vote & ~same & (label != 0)
            new = np.where(same, lconf + w, np.where(take, w, np.where(lose, np.maximum(lconf - w, np.float32(0)), lconf)))
        else:
            take, lose = vote & ~same & (lconf < w), vote & ~same & ~(lconf < w)
            new = np.where(same, lconf + w, np.where(take, w - lconf, np.where(lose, lconf - w, lconf)))
        assert new.dtype == np.float32
        switches += take & (label > 0)
        label = np.where(take, L, label).astype(np.int32)
        lconf = new
        if w_max > 0:
            lconf = np.where(vote & (lconf > w_max), w_max, lconf).astype(np.float32)
        voters += int(vote.sum())
    out = dict(label=label, lconf=lconf, wsum=W, touched=touched, flagged=flagged | band, flagged_base=flagged, switches=switches,
               voters=voters)
    if check:                       # the decisions above ARE the reference's
        ref = R.integrate_reference(dims, origin, voxel, trunc, poses, disps, intr, ix, weight=weight, z_near=z_near, w_max=w_max)
        assert np.array_equal(ref["wsum"], W) and np.array_equal(ref["touched"], touched) and np.array_equal(ref["flagged"], flagged)
    return out


def labels_match(got_label, got_lconf, ref):
    """the check of the integration tests: on unflagged touched voxels label and lconf EQUAL (lconf by its bytes); unflagged untouched
    voxels bit-for-bit zero.  Returns (ok, report)."""
    un = ~ref["flagged"]
    live, rest = un & ref["touched"], un & ~ref["touched"]
    l_ok = np.array_equal(got_label[live], ref["label"][live])
    c_ok = np.array_equal(got_lconf.view(np.uint32)[live], ref["lconf"].view(np.uint32)[live])
    z_ok = not got_label[rest].any() and not got_lconf.view(np.uint32)[rest].any()
    report = "label differs at %d, lconf at %d of %d voxels; untouched zero %s" % (
        (got_label[live] != ref["label"][live]).sum(), (got_lconf.view(np.uint32)[live] != ref["lconf"].view(np.uint32)[live]).sum(),
        live.sum(), z_ok)
    return l_ok and c_ok and z_ok, report


def vertex_labels(tsdf, label, cells):
    """pvo_tsdf_mesh_panoptic's rule for the cells [V,3] = (cz,cy,cx): the label of the corner with the smallest |tsdf| among the
    corners with label > 0, ties to the lowest j = 4 dz + 2 dy + dx, 0 without any.  int32 [V]"""
    tsdf, label = np.asarray(tsdf, np.float32), np.asarray(label, np.int32)
    out = np.zeros(len(cells), np.int32)
    for k, (cz, cy, cx) in enumerate(np.asarray(cells).reshape(-1, 3)):
        best, dist = 0, np.float32(0)
        for j in range(8):
            at = (cz + (j >> 2), cy + ((j >> 1) & 1), cx + (j & 1))
            L, dj = label[at], np.abs(tsdf[at])
            if L > 0 and (best == 0 or dj < dist):
                best, dist = L, dj
        out[k] = best
    return out
