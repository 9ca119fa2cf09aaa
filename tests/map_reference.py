"""The map export's yardstick (tests/test_map_points_host.py, tests/test_map_points_gpu.py): pvo_map_points' contract
(include/pvo_hip.h) restated in numpy, given a votes array.  Selection is integer and fp32 arithmetic stated explicitly; the world
points are evaluated in fp64 on the fp32 inputs.  tests/test_map_points_host.py qualifies this file against the recorded kernel-text
fixtures (tests/golden/geom_kernels.npz) before anything is held to it.

Error bound of the kernel's points (map_points.hip world_point, compiled without multiply-add contraction, so every operation below
rounds once; EPS = 2^-24; first order in EPS; s_i = |Xc_i| + |t_i|, S = |t|_1 + |Xc|_1 = s_0 + s_1 + s_2):
  Xc_i = ((pix - c) / f) / d          3 roundings (Zc = 1 / d: one)                      |err| <= 3 EPS |Xc_i|
  v_i  = Xc_i - t_i                   1 rounding of a value of magnitude <= s_i          |err| <= 4 EPS s_i
  r_ij   entry of R(q)^T:  1 - 2 (a a + b b): two products, a sum, the exact doubling, a difference  |err| <= 4 EPS (a a + b b) + EPS <= 5 EPS
                           2 (a b +- c d):    two products and a sum, doubled: <= 4 EPS (|a b| + |c d|) <= 2 EPS for a unit q
                           |r_ij| <= 1
  r_ij v_j                            error of the factors (4 + 5) EPS s_j, 1 rounding of the product: <= 10 EPS s_j
  (r_i0 v_0 + r_i1 v_1) + r_i2 v_2    2 roundings, of magnitudes <= s_0 + s_1 and <= S:  <= 2 EPS S
  => |p_i - exact| <= K_POINT EPS S with K_POINT = 4 + 5 + 1 + 2 = 12 dependent roundings.
The reference below evaluates the SAME algebraic form (the matrix of the quaternion as stored, not normalised again), so a stored
quaternion's distance from unit norm (a few EPS) enters only at second order.  On the scenes of the tests S < 9, so the bound stays
below 12 * 2^-24 * 9 = 6.5e-6 - tighter everywhere than the rtol 1e-5 / atol 1e-5 the iproj tests grant."""
import numpy as np

EPS = 2.0 ** -24
K_POINT = 12


def frame_means(disps, ix):
    """fp32 [N]: per exported frame the mean inverse depth, summed in fp64 and rounded to fp32 once (0 for a frame id out of range)"""
    nf = disps.shape[0]
    out = np.zeros(len(ix), np.float32)
    with np.errstate(all="ignore"):
        for b, f in enumerate(ix):
            if 0 <= f < nf:
                out[b] = np.float32(np.sum(disps[f].astype(np.float64).reshape(-1)) / float(disps[f].size))
    return out


def rotation_T(q):
    """fp64 R(q)^T of a quaternion (x, y, z, w) as stored"""
    x, y, z, w = [np.float64(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y + z * w), 2 * (x * z - y * w)],
                     [2 * (x * y - z * w), 1 - 2 * (x * x + z * z), 2 * (y * z + x * w)],
                     [2 * (x * z + y * w), 2 * (y * z - x * w), 1 - 2 * (x * x + y * y)]])


def map_reference(poses, disps, intr, ix, votes, min_votes=2, mean_frac=0.5, images=None, img_stride=8, img_offset=3,
                  labels=None, label_div=1, reject=None):
    """poses [nf,7] f32, disps [nf,ht,wd] f32, intr [4] f32, ix [N] ints, votes [N,ht,wd] (pvo_depth_filter's for ix) ->
    dict(src int32 [n,2], frame_start int32 [N+1], total, alpha uint8 [n], xyz f64 [n,3], bound f64 [n], rgb uint8 [n,3] / label
    int32 [n] where images / labels are given)"""
    poses, disps, intr = np.asarray(poses, np.float32), np.asarray(disps, np.float32), np.asarray(intr, np.float32)
    nf, ht, wd = disps.shape
    ix = [int(v) for v in np.asarray(ix).reshape(-1)]
    means = frame_means(disps, ix)
    src, alpha, xyz, bound, rgb, lab = [], [], [], [], [], []
    frame_start = np.zeros(len(ix) + 1, np.int32)
    fx, fy, cx, cy = [np.float64(v) for v in intr]
    count = 0
    for b, f in enumerate(ix):
        frame_start[b] = count                                     # (a frame id out of range: an empty slot)
        if not 0 <= f < nf:
            continue
        d = disps[f].reshape(-1)
        v = np.asarray(votes[b], np.float32).reshape(-1)
        with np.errstate(all="ignore"):
            keep = (v >= np.float32(min_votes)) & (d > np.float32(mean_frac) * means[b]) & np.isfinite(d) & (d > 0)
        yy, xx = np.divmod(np.arange(ht * wd), wd)
        if reject is not None:
            keep &= np.asarray(reject)[f][yy // label_div, xx // label_div] == 0
        k = np.nonzero(keep)[0]                                    # raster order
        y, x = yy[k], xx[k]
        dd = d[k].astype(np.float64)
        Xc = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones(len(k))], 1) / dd[:, None]
        t = poses[f, :3].astype(np.float64)
        xyz.append((Xc - t) @ rotation_T(poses[f, 3:]).T)
        bound.append(K_POINT * EPS * (np.abs(t).sum() + np.abs(Xc).sum(1)))
        src.append(np.stack([np.full(len(k), f), k], 1))
        alpha.append(v[k].astype(np.uint8))
        if images is not None:
            im = np.asarray(images)[f]
            rgb.append(np.stack([im[c][img_stride * y + img_offset, img_stride * x + img_offset] for c in (2, 1, 0)], 1))
        if labels is not None:
            lab.append(np.asarray(labels)[f][y // label_div, x // label_div])
        count += len(k)
    cat = lambda parts, shape, dt: (np.concatenate(parts) if parts else np.zeros(shape, dt)).astype(dt)
    out = dict(src=cat(src, (0, 2), np.int32), alpha=cat(alpha, (0,), np.uint8), xyz=cat(xyz, (0, 3), np.float64),
               bound=cat(bound, (0,), np.float64))
    frame_start[len(ix)] = count
    out.update(frame_start=frame_start, total=count)
    if images is not None:
        out["rgb"] = cat(rgb, (0, 3), np.uint8)
    if labels is not None:
        out["label"] = cat(lab, (0,), np.int32)
    return out


def scene(seed, nframes, ht, wd, noise):
    """constant-twist poses and a bilinear 6 x 8 inverse-depth field (the recipe of the geometry tests), every frame's field under
    multiplicative noise, ROUNDED TO MULTIPLES OF 1/4096: the fp64 sum of a frame is then exact in any order, so the mean cannot
    depend on a kernel's reduction order.  Returns torch CPU tensors poses [nframes,7], disps [nframes,ht,wd], intr [4]."""
    import torch
    from pvo_amd.geom.se3 import SE3
    g = torch.Generator().manual_seed(seed)
    intr = torch.tensor([wd * 0.625, wd * 0.625, wd / 2.0, ht / 2.0])
    xi = torch.tensor([0.05, 0.0, 0.02, 0.0, 0.01, 0.0])
    poses = torch.stack([SE3.exp(k * xi).data for k in range(nframes)], 0).float()
    low = torch.rand(1, 1, 6, 8, generator=g) * 0.8 + 0.2
    field = torch.nn.functional.interpolate(low, size=(ht, wd), mode="bilinear", align_corners=True)[0, 0]
    disps = field[None].repeat(nframes, 1, 1) * (1.0 + noise * torch.randn(nframes, ht, wd, generator=g))
    disps = (torch.round(disps * 4096.0) / 4096.0).clamp_(min=1.0 / 4096.0)
    return poses.contiguous(), disps.float().contiguous(), intr


# (nframes, ht, wd, noise): 13 x 17 = 221 pixels, one partial workgroup; 30 x 101 = 3030 = 47 * 64 + 22, a partial last wave and a
# partial last workgroup; 24 x 40 x 8 frames, where the votes reach 5; 9 x 12 x 3 frames, whose frames 0 and 1 have fewer than two
# neighbours and keep NOTHING - the empty-frame path of the scan
SCENES = {"13x17x7": (7, 13, 17, 0.02), "30x101x5": (5, 30, 101, 0.1), "24x40x8": (8, 24, 40, 0.02), "9x12x3": (3, 9, 12, 0.0)}
SEED = 5
THRESHOLDS = (0.05, 0.2)
