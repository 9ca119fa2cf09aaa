"""The brick volume's yardstick (tests/test_tsdf_sparse_host.py, tests/test_tsdf_sparse_gpu.py): the marking rule of
pvo_tsdf_sparse_allocate (include/pvo_hip.h) restated in fp64 on the fp32 inputs, the raster-order slot assignment, and the scatter /
gather between brick and dense layouts.  The integration's and the mesh's yardsticks are the dense kernels and tests/tsdf_reference.py.

A brick index is floor((c + 0.5) / 8) of a corner coordinate c = p +- margin, p the sample's position in voxels.  The kernel computes p
in fp32, so a coordinate within rounding of a brick face may land on either side.  Error bound of the kernel's p (EPS = 2^-24, first
order; r = (|rx|, |ry|, 1) the ray, Z = 1/d + trunc >= every sample depth, Mx = |r|_1 Z + |t|_1 a bound on |Xc - t|_1):
  rx = (ui - cx) / fx                  a difference and a division                                     2 EPS |rx|
  z = 1 / d, lo = max(z_near, z - trunc), hi = z + trunc, z_k = lo + (hi - lo) (k / (S-1)): the division, two sums, the difference, the
      fraction, the product and the sum, all of magnitude <= Z                                          |err| <= 6 EPS Z
  a_i = r_i z_k - t_i                  r_i's 2 EPS, z_k's 6 EPS, the product and the sum (or their contraction): summed over i
                                                                                                       |err|_1 <= 10 EPS Mx
  X_j = sum_i R_ij a_i                 entries of R(q) within 5 EPS (tests/tsdf_reference.py), three products and two sums <= 3 EPS,
                                       and a's own error, all times |a|_1 <= Mx                        |err| <= 18 EPS Mx
  p_j = (X_j - o_j) / voxel            the difference EPS (Mx + |o_j|), the division EPS                |err| <= 21 EPS (Mx + |o|_1) / voxel
  h = p_j + 0.5, h +- margin           two sums of magnitude <= |p_j| + 8.5;  * 0.125 is exact          |err| <= 2 EPS (|p_j| + 8.5)
  E = K_MARK EPS ((Mx + |o|_1) / voxel + 9), K_MARK = 32 (21 + 2 + the second order).
A corner whose h is within E of a multiple of 8 is AMBIGUOUS: the MAY set takes both bricks, the MUST set neither.  A sample whose own
p + 0.5 is within E of the grid's boundary is ambiguous as a whole (may: it marks; must: it does not).  Validity of a pixel (d, w
finite and > 0) compares fp32 inputs and cannot flip; hi >= lo can only flip where 1/d + trunc is within 6 EPS Z of z_near: may only."""
import numpy as np

import tsdf_reference as R

EPS = R.EPS
K_MARK = 32
BRICK = 8

# (nframes, ht, wd, (gz, gy, gx) bricks, origin, voxel, trunc): the analytic scenes of tsdf_reference.scene at three sizes.  Origins off
# the cameras' axes (tsdf_reference.SCENES says why) and placed so that bricks straddle all four sides of the frustums (the worlds are
# wider and taller than the cameras see at the near depths), the z_near plane the tests use (Z_NEAR, inside the first layer of bricks)
# and, in the 2 x 2 x 2 world, zfar + trunc (zfar <= 2.32 there, so its voxels at z = 2.68 and 2.80 lie beyond it).
SCENES = {
    "5x24x32": (5, 24, 32, (3, 3, 5), (-1.013, -0.617, 0.953), 0.05, 0.15),
    "3x12x16": (3, 12, 16, (2, 2, 2), (-0.913, -0.917, 1.003), 0.12, 0.36),
    "2x9x12": (2, 9, 12, (1, 2, 3), (-2.013, -1.367, 0.903), 0.17, 0.51),
}
Z_NEAR = {"5x24x32": 1.1, "3x12x16": 1.2, "2x9x12": 1.3}


def scene(name, seed=0):
    """tsdf_reference.scene of the named size with ONE MORE frame appended that looks away from the world (a half turn about y, the
    depths of frame 0): no sample of it lies in the grid and no voxel projects into it.  Returns (poses, disps, intr, images, weight,
    hit) with nframes + 1 frames and ix = every frame, the outside one in the middle, and two ids outside [0, nframes + 1)."""
    nf = SCENES[name][0]
    poses, disps, intr, images, weight, hit = R.scene(nf, SCENES[name][1], SCENES[name][2], seed)
    away = np.array([[0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0]], np.float32)
    poses = np.concatenate([poses, away])
    disps, images, weight, hit = [np.concatenate([a, a[:1]]) for a in (disps, images, weight, hit)]
    ix = list(range(nf // 2)) + [-3, nf] + list(range(nf // 2, nf)) + [nf + 1]
    return (poses, disps, intr, images, weight, hit), ix


def mark_reference(grid_dims, origin, voxel, trunc, poses, disps, intr, ix, weight=None, z_near=0.0, margin=2.0):
    """pvo_tsdf_sparse_allocate's marks.  Returns (must, may) bool [gz,gy,gx]: the bricks the kernel must mark, and may mark."""
    poses, disps, intr = np.asarray(poses, np.float32), np.asarray(disps, np.float32), np.asarray(intr, np.float32)
    nf, ht, wd = disps.shape
    gz, gy, gx = grid_dims
    dims = np.array([gx, gy, gz])
    o = np.asarray(origin, np.float32).astype(np.float64)
    voxel, trunc = np.float64(np.float32(voxel)), np.float64(np.float32(trunc))
    z_near, margin = np.float64(np.float32(z_near)), np.float64(np.float32(margin))
    S = int(np.ceil(np.float32(trunc) / np.float32(voxel))) + 1
    fx, fy, cx, cy = [np.float64(v) for v in intr]
    vv, uu = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    must, may = np.zeros((gz, gy, gx), bool), np.zeros((gz, gy, gx), bool)
    for f in [int(v) for v in np.asarray(ix).reshape(-1)]:
        if not 0 <= f < nf:
            continue
        d32 = disps[f]
        w32 = np.ones_like(d32) if weight is None else np.asarray(weight, np.float32)[f]
        with np.errstate(all="ignore"):
            ok = np.isfinite(d32) & (d32 > 0) & np.isfinite(w32) & (w32 > 0)
        if not ok.any():
            continue
        d = d32[ok].astype(np.float64)
        rx, ry = (uu[ok] - cx) / fx, (vv[ok] - cy) / fy
        Rm, t = R.rotation(poses[f, 3:]), poses[f, :3].astype(np.float64)
        z = 1.0 / d
        lo, hi = np.maximum(z_near, z - trunc), z + trunc
        Z = hi
        sure = hi - lo > 6 * EPS * Z                                            # the ray has samples whatever the rounding
        maybe = hi - lo >= -6 * EPS * Z
        zk = lo[:, None] + (hi - lo)[:, None] * (np.arange(S) / (S - 1.0))[None]           # [P,S]
        Xc = np.stack([rx[:, None] * zk, ry[:, None] * zk, zk], -1)               # [P,S,3]
        p = ((Xc - t) @ Rm - o) / voxel                                           # R^T (Xc - t), row vectors
        Mx = (np.abs(rx) + np.abs(ry) + 1.0) * Z + np.abs(t).sum()
        E = (K_MARK * EPS * ((Mx + np.abs(o).sum()) / voxel + 9.0))[:, None, None]          # [P,1,1]
        h = p + 0.5
        in_sure = np.all((h > E) & (h < BRICK * dims - E), -1) & sure[:, None]  # [P,S]
        in_may = np.all((h >= -E) & (h <= BRICK * dims + E), -1) & maybe[:, None]
        corner = {}
        for sign in (-1, 1):
            c = h + sign * margin
            b = np.floor(c / BRICK)
            frac = c - BRICK * b
            corner[sign] = (b, frac <= E, BRICK - frac <= E)                     # index, within E of the face below / above
        for j in range(8):                                                       # per axis the lower or the upper coordinate
            pick = [corner[1 if (j >> e) & 1 else -1] for e in range(3)]
            base = np.stack([pick[e][0][..., e] for e in range(3)], -1).astype(np.int64)          # [P,S,3] (x,y,z)
            below = np.stack([pick[e][1][..., e] for e in range(3)], -1)
            above = np.stack([pick[e][2][..., e] for e in range(3)], -1)
            amb = below | above
            # must: no axis ambiguous, the brick inside the grid
            inside = np.all((base >= 0) & (base < dims), -1)
            sel = in_sure & inside & ~amb.any(-1)
            bb = base[sel]
            must[bb[:, 2], bb[:, 1], bb[:, 0]] = True
            # may: every combination of the base index and, where ambiguous, its neighbour
            for k in range(27):
                off = np.array([k % 3 - 1, (k // 3) % 3 - 1, k // 9 - 1])
                allowed = np.all((off == 0) | ((off == -1) & below) | ((off == 1) & above), -1)
                cand = base + off
                sel = in_may & allowed & np.all((cand >= 0) & (cand < dims), -1)
                bb = cand[sel]
                may[bb[:, 2], bb[:, 1], bb[:, 0]] = True
    return must, may


def assign_slots(marked, grid=None):
    """the appending rule: the marked bricks that `grid` (default: all -1) does not hold get the slots n, n + 1, ... in raster order, n
    the number of bricks held.  Returns (grid int32 [gz,gy,gx], coord int32 [n_total,3] = (bz,by,bx))."""
    marked = np.asarray(marked, bool)
    grid = np.full(marked.shape, -1, np.int32) if grid is None else np.array(grid, np.int32)
    n = int((grid >= 0).sum())
    coord = np.zeros((n, 3), np.int32)
    held = np.argwhere(grid >= 0)
    coord[grid[grid >= 0]] = held
    new = np.argwhere(marked & (grid < 0))                                       # raster order
    grid[new[:, 0], new[:, 1], new[:, 2]] = n + np.arange(len(new), dtype=np.int32)
    return grid, np.concatenate([coord, new.astype(np.int32)])


def to_dense(pool, coord, grid_dims):
    """bricks [n,8,8,8(,3)] at coord [n,3] scattered into a zeroed dense [8gz,8gy,8gx(,3)] volume"""
    pool = np.asarray(pool)
    gz, gy, gx = grid_dims
    tail = pool.shape[4:]
    dense = np.zeros((gz, gy, gx, BRICK, BRICK, BRICK) + tail, pool.dtype)
    c = np.asarray(coord, np.int64)
    dense[c[:, 0], c[:, 1], c[:, 2]] = pool[:len(c)]
    perm = (0, 3, 1, 4, 2, 5) + tuple(range(6, 6 + len(tail)))
    return np.ascontiguousarray(dense.transpose(perm).reshape((BRICK * gz, BRICK * gy, BRICK * gx) + tail))


def to_bricks(dense, coord):
    """the bricks at coord [n,3] gathered from a dense [8gz,8gy,8gx(,3)] volume: [n,8,8,8(,3)]"""
    dense = np.asarray(dense)
    gz, gy, gx = [s // BRICK for s in dense.shape[:3]]
    tail = dense.shape[3:]
    v = dense.reshape((gz, BRICK, gy, BRICK, gx, BRICK) + tail)
    perm = (0, 2, 4, 1, 3, 5) + tuple(range(6, 6 + len(tail)))
    c = np.asarray(coord, np.int64)
    return np.ascontiguousarray(v.transpose(perm)[c[:, 0], c[:, 1], c[:, 2]])


def voxel_mask(allocated):
    """bool [8gz,8gy,8gx]: the voxels of the bricks `allocated` bool [gz,gy,gx]"""
    a = np.asarray(allocated, bool)
    return np.repeat(np.repeat(np.repeat(a, BRICK, 0), BRICK, 1), BRICK, 2)
