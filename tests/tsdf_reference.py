"""The surface reconstruction's yardstick (tests/test_tsdf_host.py, tests/test_tsdf_gpu.py): the contracts of pvo_tsdf_integrate and
pvo_tsdf_mesh (include/pvo_hip.h) restated in numpy.  Geometry and averages are evaluated in fp64 on the fp32 inputs; the two things the
contract states in fp32 are done in fp32 here as well: the weight sum (Wn = W + w rounded to fp32, which is also the average's
denominator) and the mesh's classification (wsum >= min_weight, tsdf < 0).

Error bound of the kernel's volume (pvo_amd/csrc/tsdf.hip, fp32 with multiply-add contraction, which only removes roundings;
EPS = 2^-24; first order in EPS; o = origin, |.|_1 the 1-norm):
  r_ij   entry of R(q): as in tests/map_reference.py                                                   |err| <= 5 EPS
  A_ij = voxel r_ij                    one more rounding                                               |err| <= 6 EPS voxel
  b_i  = (r_i0 ox + r_i1 oy) + r_i2 oz + t_i   products (5 + 1) EPS |o_j|, three sums of magnitude <= |o|_1 + |t|_1
                                                                                                       |err| <= 9 EPS (|o|_1 + |t|_1)
  Xc_i = A_i0 x + A_i1 y + A_i2 z + b_i, x, y, z the voxel's integer index (exact in fp32): products 7 EPS voxel k, three sums of
         magnitude <= M = voxel (x + y + z) + |o|_1 + |t|_1                                            |err| <= E_c = K_CAM EPS M,
         K_CAM = 12 (7 and 9 on disjoint parts of M, 3 on all of it)
  u = fx (xc / zc) + cx, then u + 0.5: with q = xc / zc (a division is within one ulp = 2 EPS)
         E_u = fx ((1 + |q|) E_c / zc + 3 EPS |q|) + 2 EPS (|fx q| + |cx| + 0.5)
  sdf = 1 / d - zc                     E_s = 2 EPS / d + E_c + EPS |sdf|
  val = min(1, sdf / trunc)            (min is 1-Lipschitz)  E_val = E_s / trunc + 2 EPS
  T'  = (T W + val w) / Wn             with |T|, |val| <= 1: two products EPS (W + w), the sum EPS (W + w), the division 2 EPS, over
         Wn = (W + w)(1 + <= EPS): 4 EPS at first order, K_AVG = 5 absorbs the factor and the second order
         E_T' = (E_T W + E_val w) / Wn + K_AVG EPS;   colours (<= 255, the pixel's colour exact): E_C' = E_C W / Wn + 255 K_AVG EPS
W itself is the same fp32 sum in the same order on both sides: it is held to EQUALITY.

Decisions.  A voxel is FLAGGED when for some frame a decision of the contract is within rounding of flipping: u + 0.5 or v + 0.5 within
max(2^-12, E_u) of an integer while the pixel is in or next to the map; |zc - z_near| <= E_c; |sdf + trunc| <= E_s.  Wn > w_max
compares two fp32 numbers that are the same on both sides, so it cannot flip; it is flagged only for 0 < |Wn - w_max| <= 2 EPS w_max.
Flagged voxels may be left out of the value comparison; they must stay below 1 % of the touched voxels (test_tsdf_host.py).

Error bound of the kernel's mesh, given the SAME fp32 volume (so the classification, the counts and the faces are held to equality):
  t = sa / (sa - sb), opposite sides, so no cancellation: 3 EPS;  m = (sum of n <= 12 terms in [0, 1]) / n: (n + 4) EPS <= 16 EPS
  vertex_e = o_e + voxel (c_e + m_e)   E_v = EPS (16 voxel + 3 voxel (c_e + 1) + |o_e|)
  gradient component: four differences <= 2 (2 EPS each), sums of magnitude <= 4, 4, 8: E_g = 24 EPS; unit normal:
                                       E_n = sqrt(3) E_g / |g| + 6 EPS (squares, sums, root, division)
  colour: the sum of eight values <= 255 (seven additions of magnitude <= 2040), + 0.5: E_col = EPS (7 * 2040 + 256); the uint8 may
          differ by one only where mean + 0.5 is within E_col of an integer."""
import numpy as np

EPS = 2.0 ** -24
K_CAM = 12
K_AVG = 5
PIXEL_BAND = 2.0 ** -12


# ------------------------------------------------------------------------------------------------------------ scene
PLANE_N = np.array([0.15, 0.08, 1.0]) / np.linalg.norm([0.15, 0.08, 1.0])
PLANE_D = 2.0 * PLANE_N[2]                     # the plane passes through (0, 0, 2)
SPHERE_C = np.array([0.1, 0.05, 1.3])
SPHERE_R = 0.35


def surface_distance(X):
    """distance of the points X [n,3] from the analytic scene's surface (the plane or the sphere, whichever is nearer)"""
    X = np.asarray(X, np.float64)
    return np.minimum(np.abs(X @ PLANE_N - PLANE_D), np.abs(np.linalg.norm(X - SPHERE_C, axis=1) - SPHERE_R))


def scene(nframes, ht, wd, seed=0):
    """camera centres on the line y = z = 0 with a small yaw toward the middle, looking along +z at a tilted plane with a sphere in front;
    the inverse depth of every pixel from the closed-form ray intersections.  Returns numpy: poses [nframes,7] f32 (world-to-camera),
    disps [nframes,ht,wd] f32, intr [4] f32, images uint8 [nframes,3,ht,wd] (BGR, a smooth pattern plus noise), weight f32
    [nframes,ht,wd] in [0.5, 1.5] and hit [nframes,ht,wd] bool: the pixel sees the sphere."""
    rng = np.random.default_rng(seed)
    intr = np.array([0.8 * wd, 0.8 * wd, 0.5 * wd - 0.5, 0.5 * ht - 0.5], np.float32)
    fx, fy, cx, cy = [np.float64(v) for v in intr]
    poses = np.zeros((nframes, 7), np.float32)
    disps = np.zeros((nframes, ht, wd), np.float32)
    hit = np.zeros((nframes, ht, wd), bool)
    yy, xx = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    for k in range(nframes):
        c = np.array([0.15 * (k - 0.5 * (nframes - 1)), 0.0, 0.0])
        yaw = -0.2 * c[0]                                            # camera-to-world: a rotation by yaw about y
        Rcw = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        R = Rcw.T
        poses[k, :3] = -R @ c
        poses[k, 3:] = [0.0, np.sin(-0.5 * yaw), 0.0, np.cos(-0.5 * yaw)]
        dw = np.stack([(xx - cx) / fx, (yy - cy) / fy, np.ones_like(xx, float)], -1) @ Rcw.T     # ray directions, dc.z = 1: s = depth
        s_plane = (PLANE_D - PLANE_N @ c) / (dw @ PLANE_N)
        oc = c - SPHERE_C
        qa, qb, qc = (dw * dw).sum(-1), 2.0 * (dw @ oc), oc @ oc - SPHERE_R ** 2
        disc = qb * qb - 4 * qa * qc
        s_sphere = np.where(disc > 0, (-qb - np.sqrt(np.maximum(disc, 0))) / (2 * qa), np.inf)
        hit[k] = s_sphere < s_plane
        disps[k] = (1.0 / np.minimum(s_plane, s_sphere)).astype(np.float32)
    base = 96 + 64 * np.sin(0.4 * xx)[None, None] * np.cos(0.3 * yy)[None, None] + 20 * np.arange(3)[None, :, None, None]
    images = np.clip(base + rng.integers(-16, 17, (nframes, 3, ht, wd)), 0, 255).astype(np.uint8)
    weight = (0.5 + rng.integers(0, 65, (nframes, ht, wd)) / 64.0).astype(np.float32)
    return poses, disps, intr, images, weight, hit


# (nframes, ht, wd, (nz, ny, nx), origin, voxel, trunc): sizes with tails in every dimension - 26880, 1920 and 693 voxels are no
# multiples of 256, no row is a multiple of 64.  The origins are deliberately off the cameras' axes: with a voxel column on an optical
# axis (x = 0 or y = 0 in a camera without pitch) u + 0.5 is an integer on a whole plane of voxels, a tie by construction
SCENES = {
    "5x24x32": (5, 24, 32, (24, 28, 40), (-1.013, -0.717, 0.953), 0.05, 0.15),
    "3x12x16": (3, 12, 16, (10, 12, 16), (-0.913, -0.717, 0.903), 0.12, 0.36),
    "2x9x12": (2, 9, 12, (7, 9, 11), (-0.813, -0.667, 0.903), 0.17, 0.51),
}


# ------------------------------------------------------------------------------------------------------------ integration
def rotation(q):
    """fp64 R(q) of a quaternion (x, y, z, w) as stored"""
    x, y, z, w = [np.float64(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def integrate_reference(dims, origin, voxel, trunc, poses, disps, intr, ix, weight=None, images=None, img_stride=8, img_offset=3,
                        z_near=0.0, w_max=0.0, mutant=None):
    """pvo_tsdf_integrate into a ZEROED volume of dims (nz,ny,nx).  Returns dict(tsdf f64, wsum f32, rgb f64 [..,3] (with images),
    touched bool, flagged bool, bound f64, bound_rgb f64, hits: the number of voxel-frame pairs fused).
    mutant: None, or one of "floor_u" (floor(u) in place of rounding), "ray_sdf" (sdf along the ray), "unweighted" (an unweighted
    mean of the values) and "no_weight" (weight ignored) - deliberately wrong variants the tests must be able to tell apart."""
    poses, disps, intr = np.asarray(poses, np.float32), np.asarray(disps, np.float32), np.asarray(intr, np.float32)
    nf, ht, wd = disps.shape
    nz, ny, nx = dims
    o = np.asarray(origin, np.float32).astype(np.float64)
    voxel, trunc = np.float64(np.float32(voxel)), np.float64(np.float32(trunc))
    z_near, w_max = np.float64(np.float32(z_near)), np.float32(w_max)
    fx, fy, cx, cy = [np.float64(v) for v in intr]
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    X = o + voxel * np.stack([xx, yy, zz], -1).astype(np.float64)
    ksum = voxel * (xx + yy + zz)
    T = np.zeros(dims)
    W = np.zeros(dims, np.float32)
    C = np.zeros(dims + (3,))
    E_T, E_C = np.zeros(dims), np.zeros(dims)
    touched, flagged = np.zeros(dims, bool), np.zeros(dims, bool)
    count = np.zeros(dims)
    hits = 0
    for f in [int(v) for v in np.asarray(ix).reshape(-1)]:
        if not 0 <= f < nf:
            continue
        R, t = rotation(poses[f, 3:]), poses[f, :3].astype(np.float64)
        Xc = X @ R.T + t
        xc, yc, zc = Xc[..., 0], Xc[..., 1], Xc[..., 2]
        E_c = K_CAM * EPS * (ksum + np.abs(o).sum() + np.abs(t).sum())
        flagged |= np.abs(zc - z_near) <= E_c
        ok = zc > z_near
        with np.errstate(all="ignore"):
            qx, qy = xc / zc, yc / zc
            u, v = fx * qx + cx, fy * qy + cy
            if mutant == "floor_u":
                ru, rv = np.floor(u), np.floor(v)
            else:
                ru, rv = np.floor(u + 0.5), np.floor(v + 0.5)
            E_u = fx * ((1 + np.abs(qx)) * E_c / zc + 3 * EPS * np.abs(qx)) + 2 * EPS * (np.abs(fx * qx) + abs(cx) + 0.5)
            E_v = fy * ((1 + np.abs(qy)) * E_c / zc + 3 * EPS * np.abs(qy)) + 2 * EPS * (np.abs(fy * qy) + abs(cy) + 0.5)
            near = ok & (ru >= -1) & (ru <= wd) & (rv >= -1) & (rv <= ht)
            du, dv = np.abs(u + 0.5 - np.round(u + 0.5)), np.abs(v + 0.5 - np.round(v + 0.5))
            flagged |= near & ((du <= np.maximum(PIXEL_BAND, E_u)) | (dv <= np.maximum(PIXEL_BAND, E_v)))
        ok &= np.isfinite(ru) & np.isfinite(rv) & (ru >= 0) & (ru < wd) & (rv >= 0) & (rv < ht)
        ui = np.where(ok, ru, 0).astype(np.int64)
        vi = np.where(ok, rv, 0).astype(np.int64)
        d32 = disps[f][vi, ui]
        w32 = np.ones(dims, np.float32) if weight is None or mutant == "no_weight" else np.asarray(weight, np.float32)[f][vi, ui]
        with np.errstate(all="ignore"):
            ok &= np.isfinite(d32) & (d32 > 0) & np.isfinite(w32) & (w32 > 0)
            d = np.where(ok, d32, 1).astype(np.float64)
            sdf = 1.0 / d - zc
            if mutant == "ray_sdf":
                sdf = sdf * np.sqrt(qx * qx + qy * qy + 1.0)
            E_s = 2 * EPS / d + E_c + EPS * np.abs(sdf)
            flagged |= ok & (np.abs(sdf + trunc) <= E_s)
            ok &= ~(sdf < -trunc)
            val = np.minimum(1.0, sdf / trunc)
            E_val = E_s / trunc + 2 * EPS
        w32 = np.where(ok, w32, np.float32(0))
        Wn32 = (W + w32).astype(np.float32)                                 # the contract's fp32 sum
        Wd, wd64, Wn = W.astype(np.float64), w32.astype(np.float64), np.where(ok, Wn32, 1).astype(np.float64)
        if mutant == "unweighted":
            Tn = (T * count + val) / (count + 1)
        else:
            Tn = (T * Wd + val * wd64) / Wn
        T = np.where(ok, Tn, T)
        E_T = np.where(ok, (E_T * Wd + E_val * wd64) / Wn + K_AVG * EPS, E_T)
        if images is not None:
            im = np.asarray(images)[f]
            col = np.stack([im[c][img_stride * vi + img_offset, img_stride * ui + img_offset] for c in (2, 1, 0)], -1).astype(np.float64)
            C = np.where(ok[..., None], (C * Wd[..., None] + col * wd64[..., None]) / Wn[..., None], C)
            E_C = np.where(ok, E_C * Wd / Wn + 255 * K_AVG * EPS, E_C)
        if w_max > 0:
            flagged |= ok & (Wn32 != w_max) & (np.abs(Wn32.astype(np.float64) - np.float64(w_max)) <= 2 * EPS * np.float64(w_max))
            Wn32 = np.where(Wn32 > w_max, w_max, Wn32).astype(np.float32)
        W = np.where(ok, Wn32, W).astype(np.float32)
        count += ok
        touched |= ok
        hits += int(ok.sum())
    out = dict(tsdf=T, wsum=W, touched=touched, flagged=flagged, bound=E_T, bound_rgb=E_C, hits=hits)
    if images is not None:
        out["rgb"] = C
    return out


def volume_matches(got_tsdf, got_wsum, got_rgb, ref):
    """the check of the integration tests: on unflagged voxels wsum EQUAL and tsdf / rgb within the derived bound; voxels the reference
    leaves untouched bit-for-bit zero (flagged ones excepted: their decision may have flipped).  Returns (ok, report)."""
    un = ~ref["flagged"]
    w_ok = np.array_equal(got_wsum[un], ref["wsum"][un])
    err = np.abs(got_tsdf.astype(np.float64) - ref["tsdf"])
    t_ok = bool(np.all(err[un] <= ref["bound"][un]))
    rest = un & ~ref["touched"]
    z_ok = not got_tsdf.view(np.uint32)[rest].any() and not got_wsum.view(np.uint32)[rest].any()
    c_ok, cerr = True, 0.0
    if got_rgb is not None:
        ce = np.abs(got_rgb.astype(np.float64) - ref["rgb"]).max(-1)
        c_ok = bool(np.all(ce[un] <= ref["bound_rgb"][un])) and not got_rgb.view(np.uint32)[rest].any()
        cerr = float(ce[un].max())
    live = un & ref["touched"]
    report = "wsum equal %s, tsdf max err %.3e (max err / bound %.3f, max bound %.3e), rgb max err %.3e, untouched zero %s" % (
        w_ok, err[un].max(), (err[live] / ref["bound"][live]).max() if live.any() else 0.0, ref["bound"].max(), cerr, z_ok)
    return w_ok and t_ok and z_ok and c_ok, report


# ------------------------------------------------------------------------------------------------------------ mesh
AXES = ((1, 2), (2, 0), (0, 1))          # the other two axes (b, c') of axis a, cyclically; axes are 0 = x, 1 = y, 2 = z


def mesh_reference(tsdf, wsum, rgb, origin, voxel, min_weight=1.0):
    """pvo_tsdf_mesh: surface nets on the fp32 volume it is given (classification by exact fp32 comparisons).  Returns dict(verts f64
    [V,3], normals f64 [V,3], rgb f64 [V,3] (the means before rounding), faces int32 [F,3], cells int [V,3] = (cz,cy,cx) per vertex,
    bound_v, bound_n f64 [V,3] / [V], E_col, cell_valid bool [nz-1,ny-1,nx-1]: all eight corners valid)"""
    tsdf, wsum = np.asarray(tsdf, np.float32), np.asarray(wsum, np.float32)
    nz, ny, nx = tsdf.shape
    o = np.asarray(origin, np.float32).astype(np.float64)
    voxel = np.float64(np.float32(voxel))
    valid = wsum >= np.float32(min_weight)
    inside = tsdf < np.float32(0)
    empty = dict(verts=np.zeros((0, 3)), normals=np.zeros((0, 3)), rgb=np.zeros((0, 3)), faces=np.zeros((0, 3), np.int32),
                 cells=np.zeros((0, 3), int), bound_v=np.zeros((0, 3)), bound_n=np.zeros(0), E_col=EPS * (7 * 2040 + 256),
                 cell_valid=np.zeros((max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0)), bool))
    if min(nz, ny, nx) < 2:
        return empty
    corner = lambda a, j: a[(j >> 2):nz - 1 + (j >> 2), ((j >> 1) & 1):ny - 1 + ((j >> 1) & 1), (j & 1):nx - 1 + (j & 1)]
    all_valid = np.all([corner(valid, j) for j in range(8)], 0)
    n_in = np.sum([corner(inside, j) for j in range(8)], 0)
    active = all_valid & (n_in > 0) & (n_in < 8)
    index = np.full(active.shape, -1, np.int64)
    cells = np.argwhere(active)                                           # raster order
    index[active] = np.arange(len(cells))
    verts, normals, cols, bound_v, bound_n, faces = [], [], [], [], [], []
    s64 = tsdf.astype(np.float64)
    for cz, cy, cx in cells:
        c = (cx, cy, cz)
        s = [s64[cz + (j >> 2), cy + ((j >> 1) & 1), cx + (j & 1)] for j in range(8)]
        p, n = np.zeros(3), 0
        for a in range(3):
            for j in range(8):
                if j & (1 << a):
                    continue
                sa, sb = s[j], s[j | (1 << a)]
                if (sa < 0) == (sb < 0):
                    continue
                pt = np.array([(j >> e) & 1 for e in range(3)], float)
                pt[a] = sa / (sa - sb)
                p += pt
                n += 1
        verts.append(o + voxel * (np.array(c, float) + p / n))
        bound_v.append(EPS * (16 * voxel + 3 * voxel * (np.array(c, float) + 1) + np.abs(o)))
        g = np.array([sum(s[j | (1 << a)] - s[j] for j in range(8) if not j & (1 << a)) for a in range(3)])
        ln = np.linalg.norm(g)
        normals.append(g / ln if ln > 0 else np.zeros(3))
        bound_n.append(np.sqrt(3.0) * 24 * EPS / ln + 6 * EPS if ln > 0 else np.inf)
        if rgb is not None:
            cols.append(np.mean([np.asarray(rgb[cz + (j >> 2), cy + ((j >> 1) & 1), cx + (j & 1)], np.float64) for j in range(8)], 0))
        # faces: axes x, y, z; A = corner 0, B = A + e_a
        for a, (b, cc) in enumerate(AXES):
            A, B = inside[cz, cy, cx], inside[cz + (a == 2), cy + (a == 1), cx + (a == 0)]
            if A == B or c[b] < 1 or c[cc] < 1:
                continue
            q = []
            for db_, dc_ in ((0, 0), (1, 0), (1, 1), (0, 1)):
                n3 = list(c)
                n3[b] -= db_
                n3[cc] -= dc_
                q.append(index[n3[2], n3[1], n3[0]])
            if min(q) < 0:
                continue
            faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])] if A else [(q[0], q[2], q[1]), (q[0], q[3], q[2])]
    if not len(cells):
        empty["cell_valid"] = all_valid
        return empty
    return dict(verts=np.array(verts), normals=np.array(normals), rgb=np.array(cols) if rgb is not None else np.zeros((len(cells), 3)),
                faces=np.array(faces, np.int32).reshape(-1, 3), cells=cells, bound_v=np.array(bound_v), bound_n=np.array(bound_n),
                E_col=EPS * (7 * 2040 + 256), cell_valid=all_valid)


def sphere_volume(dims, centre, radius, trunc, device):
    """torch f32 [nz,ny,nx] on `device`: the signed distance of every voxel index (x,y,z) to the sphere |p - centre| = radius (all in
    voxels), divided by trunc and clamped to [-1, 1] - a closed surface for the mesh tests that need more cells than a fused scene has"""
    import torch
    nz, ny, nx = dims
    ar = lambda n: torch.arange(n, dtype=torch.float32, device=device)
    z, y, x = torch.meshgrid(ar(nz), ar(ny), ar(nx), indexing="ij")
    d = torch.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return torch.clamp(d / trunc, -1.0, 1.0).contiguous()


def edge_shares(faces):
    """{(i, j) with i < j: the number of triangles that use the edge}"""
    from collections import Counter
    e = Counter()
    for f in np.asarray(faces):
        for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            e[(min(a, b), max(a, b))] += 1
    return e


def interior_vertices(mesh):
    """bool [V]: the 3 x 3 x 3 cells around the vertex's cell all exist and have eight valid corners - the surface cannot end there"""
    cv = np.pad(mesh["cell_valid"], 1, constant_values=False)
    ok = np.ones(len(mesh["cells"]), bool)
    for k, (cz, cy, cx) in enumerate(mesh["cells"]):
        ok[k] = cv[cz:cz + 3, cy:cy + 3, cx:cx + 3].all()
    return ok


def colours_match(got_rgb8, ref):
    """uint8 colours against the fp64 means: floor(mean + 0.5) clamped, off by one allowed only within E_col of a tie"""
    x = ref["rgb"] + 0.5
    want = np.clip(np.floor(x), 0, 255)
    tie = np.abs(x - np.round(x)) <= ref["E_col"]
    diff = np.abs(got_rgb8.astype(np.float64) - want)
    return bool(np.all((diff == 0) | (tie & (diff <= 1))))
