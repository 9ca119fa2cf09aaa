"""The volume render's yardstick (tests/test_tsdf_render_host.py, tests/test_tsdf_render_gpu.py): the contract of pvo_tsdf_render
(include/pvo_hip.h) restated in numpy.  Geometry, interpolation and blends are evaluated in fp64 on the fp32 inputs; what the contract
compares in fp32 is compared in fp32 here as well: wsum >= min_weight, the lattice's end points ceil(z_near / dz) and floor(z_far / dz),
and the label rule (|tsdf| of fp32 corners).

Error bound of the kernel (pvo_amd/csrc/tsdf_ray.h: fp32, every multiply-add one fma; EPS = 2^-24, first order; o = origin, |.|_1 the
1-norm, r1 = |rx| + |ry| + 1, z = z_k):
  R_ij   entry of R(q), as in tests/tsdf_reference.py                                                  |err| <= 5 EPS
  M_ij = R_ji / voxel                  one more rounding                                               |err| <= 6 EPS / voxel
  c_i  = -(R^T t)_i                    products (5 + 1) EPS |t_j|, two roundings of magnitude <= |t|_1   |err| <= 8 EPS |t|_1
  p0_i = (c_i - o_i) / voxel           the difference EPS (|t|_1 + |o_i|), the division                  |err| <= 10 EPS (|t|_1 + |o|_1) / voxel
  rx   = (ui - cx) / fx                a difference and a division                                      |err| <= 2 EPS |rx|
  g_i  = fma(M_i0, rx, fma(M_i1, ry, M_i2))   M's 6, rx's 2, two roundings, all of magnitude <= r1 / voxel   |err| <= 10 EPS r1 / voxel
  z_k  = float(k) dz                   one rounding                                                      |err| <= EPS z
  p_i  = fma(z, g_i, p0_i)             z E_g + EPS z |g_i| (|g_i| <= r1 / voxel: rows of R^T are unit) + E_p0 + the rounding EPS |p_i|
         E_p = EPS (K_RAY z r1 / voxel + K_P0 (|t|_1 + |o|_1) / voxel + |p_i|),   K_RAY = 12 (10 + 1 + second order), K_P0 = 10
  f_i  = p_i - c_i                     exact (p_i in [c_i, c_i + 1])                                    E_f = E_p
  S    = three levels of lerp(a, b, t) = fma(t, b - a, a) on values in [-1, 1]: per level the difference (<= 2 EPS) and the fma
         (<= EPS), errors of a, b pass through a convex combination                                     rounding <= 9 EPS
         E_S = K_TRI EPS + sum_i |dS/df_i| E_p_i,   K_TRI = 10, dS/df the gradient the reference computes anyway
  t    = Sa / (Sa - Sb), Sa >= 0 > Sb, D = Sa - Sb = |Sa| + |Sb|:   E_t = (|Sb| E_Sa + Sa E_Sb) / D^2 + 3 EPS
  depth = (float(k-1) + t) dz          E_d = dz (E_t + 2 EPS k)
  grad_i = two levels of lerp on corner differences (<= 2, 2 EPS each; a level's difference <= 4): rounding <= K_GRAD EPS = 16 EPS;
         d grad_i / d f_j is a second difference, <= 4:   E_grad_i = K_GRAD EPS + 4 sum_{j != i} E_p_j
  v = lerp(grad_a, grad_b, t)          E_v_i = max(E_grad_a_i, E_grad_b_i) + |grad_b_i - grad_a_i| E_t + 12 EPS
  normal = v / |v|                     (the map v -> v / |v| has a Jacobian of norm <= 1 / |v|)         E_n = |E_v|_2 / |v| + 6 EPS
  colour: the same three levels on values <= 255: E_C = 255 K_TRI EPS + sum_i |dC/df_i| E_p_i; the blend max(E_Ca, E_Cb) +
         |Cb - Ca| E_t + 3 * 255 EPS; + 0.5: 256 EPS.  The uint8 may differ by one only where x + 0.5 is within that of an integer.

Decisions.  A pixel is FLAGGED when a decision of its walk, up to and including the sample that ends it, is within rounding of flipping:
|S_j| <= E_S for a valid sample; a component of p(z_j) within E_p of an integer while the cell on the other side differs in validity
(for the ending sample also: in its label pick), or within E_p of a face of the box while the cell there is valid; and, at a hit,
max(E_Sa, E_Sb) / D > 2^-8 (t ill-conditioned: the first-order bound no longer holds).  Flagged pixels are left out of the value
comparison; they must stay below 1 % of a scene's pixels (test_tsdf_render_host.py asserts it on this reference alone)."""
import numpy as np

import tsdf_reference as R

EPS = R.EPS
K_RAY, K_P0, K_TRI, K_GRAD = 12, 10, 10, 16
T_COND = 2.0 ** -8
MUTANTS = ("nearest", "no_interp", "ignore_validity", "ray_depth")

_DX = np.array([j & 1 for j in range(8)])
_DY = np.array([(j >> 1) & 1 for j in range(8)])
_DZ = np.array([j >> 2 for j in range(8)])


def lattice(z_near, z_far, dz):
    """(klo, khi) in fp32, as the kernel's host code computes them"""
    z_near, z_far, dz = np.float32(z_near), np.float32(z_far), np.float32(dz)
    return int(np.ceil(z_near / dz)), int(np.floor(z_far / dz))


def _corners(a, cell):
    """a [nz,ny,nx(,c)] at the eight corners of cell [P,3] = (cx,cy,cz): [P,8(,c)]"""
    return a[cell[:, 2, None] + _DZ, cell[:, 1, None] + _DY, cell[:, 0, None] + _DX]


def _trilinear(s, f):
    """s [P,8(,c)], f [P,3] -> value [P(,c)] and its gradient [P,3(,c)] with respect to f"""
    if s.ndim == 3:
        f = f[..., None]
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    lerp = lambda a, b, t: a + t * (b - a)
    b0 = lerp(lerp(s[:, 0], s[:, 1], fx), lerp(s[:, 2], s[:, 3], fx), fy)
    b1 = lerp(lerp(s[:, 4], s[:, 5], fx), lerp(s[:, 6], s[:, 7], fx), fy)
    gx = lerp(lerp(s[:, 1] - s[:, 0], s[:, 3] - s[:, 2], fy), lerp(s[:, 5] - s[:, 4], s[:, 7] - s[:, 6], fy), fz)
    gy = lerp(lerp(s[:, 2] - s[:, 0], s[:, 3] - s[:, 1], fx), lerp(s[:, 6] - s[:, 4], s[:, 7] - s[:, 5], fx), fz)
    return lerp(b0, b1, fz), np.stack([gx, gy, b1 - b0], 1)


def _label_pick(s32, lab):
    """pvo_tsdf_mesh_panoptic's vertex rule: s32 f32 [P,8], lab int32 [P,8] -> int32 [P]"""
    d = np.where(lab > 0, np.abs(s32), np.float32(np.inf))
    j = np.argmin(d, 1)                                   # the first minimum: ties to the lowest corner
    return np.where((lab > 0).any(1), lab[np.arange(len(j)), j], 0).astype(np.int32)


def render_reference(tsdf, wsum, rgb, label, origin, voxel, poses, intr, ix, ht, wd, dz, z_near, z_far, min_weight=1.0, allocated=None,
                     mutant=None):
    """pvo_tsdf_render of the fp32 volume.  allocated bool [nz/8,ny/8,nx/8] (the brick volume): voxels of other bricks are invalid.
    Returns dict(hit bool [N,ht,wd], depth, normal [..,3], rgb [..,3] (before rounding; None without rgb), label int32, flagged bool,
    bound_d, bound_n, bound_c f64 [N,ht,wd]).  mutant: None or one of MUTANTS - deliberately wrong variants the tests must tell apart."""
    assert mutant is None or mutant in MUTANTS
    tsdf, wsum = np.asarray(tsdf, np.float32), np.asarray(wsum, np.float32)
    nz, ny, nx = tsdf.shape
    n = np.array([nx, ny, nz])
    poses, intr = np.asarray(poses, np.float32), np.asarray(intr, np.float32)
    ix = [int(v) for v in np.asarray(ix).reshape(-1)]
    N = len(ix)
    o = np.asarray(origin, np.float32).astype(np.float64)
    voxel = np.float64(np.float32(voxel))
    dz32 = np.float32(dz)
    klo, khi = lattice(z_near, z_far, dz)
    fx, fy, cx, cy = [np.float64(v) for v in intr]
    valid_vox = wsum >= np.float32(min_weight)
    if mutant == "ignore_validity":
        valid_vox = np.ones_like(valid_vox)
    if allocated is not None:
        valid_vox = valid_vox & np.repeat(np.repeat(np.repeat(np.asarray(allocated, bool), 8, 0), 8, 1), 8, 2)
    s64 = tsdf.astype(np.float64)
    rgb64 = None if rgb is None else np.asarray(rgb, np.float32).astype(np.float64)
    lab = None if label is None else np.asarray(label, np.int32)
    out = dict(hit=np.zeros((N, ht, wd), bool), depth=np.zeros((N, ht, wd)), normal=np.zeros((N, ht, wd, 3)),
               rgb=None if rgb is None else np.zeros((N, ht, wd, 3)), label=np.zeros((N, ht, wd), np.int32),
               flagged=np.zeros((N, ht, wd), bool), bound_d=np.zeros((N, ht, wd)), bound_n=np.zeros((N, ht, wd)),
               bound_c=np.zeros((N, ht, wd)))
    if min(nz, ny, nx) < 2:
        return out
    vv, uu = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    rx, ry = ((uu - cx) / fx).reshape(-1), ((vv - cy) / fy).reshape(-1)
    r1 = np.abs(rx) + np.abs(ry) + 1.0
    P = ht * wd

    def cell_valid(cell):
        return _corners(valid_vox, cell).all(1)

    def sample(k, sel):
        """sample k of the pixels sel: p, cell, frac, in-box, valid, E_p [.,3]"""
        z = np.float64(np.float32(k)) * np.float64(dz32)
        p = z * g[sel] + p0
        E_p = EPS * (K_RAY * z * r1[sel, None] / voxel + K_P0 * m1 / voxel + np.abs(p))
        inbox = np.all((p >= 0) & (p <= n - 1), 1)
        cell = np.minimum(np.floor(np.where(inbox[:, None], p, 0)).astype(np.int64), n - 2)
        return p, cell, p - cell, inbox, E_p

    def value(cell, frac, p):
        s = _corners(s64, cell)
        if mutant == "nearest":
            near = np.clip(np.floor(p + 0.5).astype(np.int64), 0, n - 1)
            S = s64[near[:, 2], near[:, 1], near[:, 0]]
            return s, S, _trilinear(s, frac)[1]
        S, grad = _trilinear(s, frac)
        return s, S, grad

    for b, f in enumerate(ix):
        if not 0 <= f < poses.shape[0]:
            continue
        Rm, t = R.rotation(poses[f, 3:]), poses[f, :3].astype(np.float64)
        M = Rm.T / voxel
        p0 = (-(Rm.T @ t) - o) / voxel
        g = np.stack([rx, ry, np.ones(P)], 1) @ M.T                       # [P,3]
        m1 = np.abs(t).sum() + np.abs(o).sum()
        alive = np.ones(P, bool)
        prev_ok = np.zeros(P, bool)
        flagged = np.zeros(P, bool)
        end_k = np.full(P, -1)
        for k in range(klo, khi + 1):
            sel = np.flatnonzero(alive)
            if not len(sel):
                break
            p, cell, frac, inbox, E_p = sample(k, sel)
            ok = inbox.copy()
            ok[inbox] = cell_valid(cell[inbox])
            # decisions of the position: a face of the box, an integer with a cell of other validity beyond it
            near_face = np.any((np.abs(p) <= E_p) | (np.abs(p - (n - 1)) <= E_p), 1)
            cl = np.clip(np.floor(np.clip(p, 0, n - 1)).astype(np.int64), 0, n - 2)
            nf = np.flatnonzero(near_face)
            if len(nf):
                flagged[sel[nf]] |= cell_valid(cl[nf])
            frac_r = p - np.round(p)
            near_int = inbox[:, None] & (np.abs(frac_r) <= E_p)
            ni = np.flatnonzero(near_int.any(1))
            alt_cells = {}
            if len(ni):
                side = np.where(near_int[ni], np.where(np.round(p[ni]) > cell[ni], 1, -1), 0)     # the cell beyond the integer
                for m in range(1, 8):
                    use = np.array([(m >> e) & 1 for e in range(3)])
                    alt = np.clip(cell[ni] + side * use, 0, n - 2)
                    differs = np.any(alt != cell[ni], 1)
                    flagged[sel[ni]] |= differs & (cell_valid(alt) != ok[ni])
                    alt_cells[m] = (alt, differs)
            vi_ = np.flatnonzero(ok)
            S = np.zeros(len(sel))
            E_S = np.zeros(len(sel))
            if len(vi_):
                s, Sv, grad = value(cell[vi_], frac[vi_], p[vi_])
                S[vi_] = Sv
                E_S[vi_] = K_TRI * EPS + (np.abs(grad) * E_p[vi_]).sum(1)
                flagged[sel[vi_]] |= np.abs(Sv) <= E_S[vi_]
            ends = ok & (S < 0)
            e = np.flatnonzero(ends)
            if len(e):
                pix = sel[e]
                end_k[pix] = k
                alive[pix] = False
                if lab is not None:
                    pick = _label_pick(_corners(tsdf, cell[e]), _corners(lab, cell[e]))
                    out["label"][b].reshape(-1)[pix] = pick
                    pos = {int(q): j for j, q in enumerate(ni)}
                    for j_e, q in enumerate(e):                           # the label pick of the cell beyond a near integer
                        if int(q) in pos:
                            for alt, differs in alt_cells.values():
                                a1 = alt[pos[int(q)]][None]
                                if differs[pos[int(q)]] and _label_pick(_corners(tsdf, a1), _corners(lab, a1))[0] != pick[j_e]:
                                    flagged[sel[q]] = True
                hit = prev_ok[pix]
                h = e[hit]
                if len(h):
                    hp = sel[h]
                    pa, ca, fa, _, E_pa = sample(k - 1, hp)
                    sa, Sa, ga = value(ca, fa, pa)
                    sb, Sb, gb = value(cell[h], frac[h], p[h])
                    E_Sa = K_TRI * EPS + (np.abs(ga) * E_pa).sum(1)
                    E_Sb = E_S[h]
                    D = Sa - Sb
                    with np.errstate(all="ignore"):
                        tt = Sa / D
                        E_t = (np.abs(Sb) * E_Sa + np.abs(Sa) * E_Sb) / (D * D) + 3 * EPS
                        flagged[hp] |= ~(np.maximum(E_Sa, E_Sb) / D <= T_COND)
                    depth = (np.float64(k - 1) + tt) * np.float64(dz32)
                    if mutant == "no_interp":
                        depth = np.full(len(h), np.float64(np.float32(k)) * np.float64(dz32))
                    if mutant == "ray_depth":
                        depth = depth * np.sqrt(rx[hp] ** 2 + ry[hp] ** 2 + 1.0)
                    out["hit"][b].reshape(-1)[hp] = True
                    out["depth"][b].reshape(-1)[hp] = depth
                    out["bound_d"][b].reshape(-1)[hp] = np.float64(dz32) * (E_t + 2 * EPS * k)
                    other = lambda E: E.sum(1, keepdims=True) - E
                    E_ga, E_gb = K_GRAD * EPS + 4 * other(E_pa), K_GRAD * EPS + 4 * other(E_p[h])
                    v = ga + tt[:, None] * (gb - ga)
                    E_v = np.maximum(E_ga, E_gb) + np.abs(gb - ga) * E_t[:, None] + 12 * EPS
                    ln = np.linalg.norm(v, axis=1)
                    with np.errstate(all="ignore"):
                        out["normal"][b].reshape(-1, 3)[hp] = np.where(ln[:, None] > 0, v / ln[:, None], 0.0)
                        out["bound_n"][b].reshape(-1)[hp] = np.where(ln > 0, np.linalg.norm(E_v, axis=1) / ln + 6 * EPS, np.inf)
                    if rgb64 is not None:
                        Ca, dCa = _trilinear(_corners(rgb64, ca), fa)
                        Cb, dCb = _trilinear(_corners(rgb64, cell[h]), frac[h])
                        E_Ca = 255 * K_TRI * EPS + (np.abs(dCa) * E_pa[:, :, None]).sum(1)
                        E_Cb = 255 * K_TRI * EPS + (np.abs(dCb) * E_p[h][:, :, None]).sum(1)
                        out["rgb"][b].reshape(-1, 3)[hp] = Ca + tt[:, None] * (Cb - Ca)
                        E_c = np.maximum(E_Ca, E_Cb) + np.abs(Cb - Ca) * E_t[:, None] + (3 * 255 + 256) * EPS
                        out["bound_c"][b].reshape(-1)[hp] = E_c.max(1)
                # a ray that ends without a hit is a miss: its label is 0 as well
                miss = pix[~hit]
                out["label"][b].reshape(-1)[miss] = 0
            prev_ok[sel] = ok
        out["flagged"][b] = flagged.reshape(ht, wd)
    return out


def render_matches(got, ref):
    """the check of the render tests.  got: dict of numpy depth f32 [N,ht,wd], normal f32 [..,3] or None, rgba uint8 [..,4] or None, label
    int32 or None.  On unflagged pixels: hit / miss EQUAL (depth > 0, and every output of a miss exactly the miss), label EQUAL, depth
    and normal within the bounds, colours off by one only within the bound of a tie.  Returns (ok, report)."""
    un = ~ref["flagged"]
    hit = ref["hit"] & un
    miss = ~ref["hit"] & un
    depth = got["depth"].astype(np.float64)
    h_ok = bool(np.all(depth[hit] > 0)) and not got["depth"].view(np.uint32)[miss].any()
    d_err = np.abs(depth - ref["depth"])
    d_ok = bool(np.all(d_err[hit] <= ref["bound_d"][hit]))
    n_ok, n_err, c_ok, l_ok = True, 0.0, True, True
    if got.get("normal") is not None:
        ne = np.abs(got["normal"].astype(np.float64) - ref["normal"]).max(-1)
        n_ok = bool(np.all(ne[hit] <= ref["bound_n"][hit])) and not got["normal"].view(np.uint32)[miss].any()
        n_err = float(ne[hit].max()) if hit.any() else 0.0
    if got.get("rgba") is not None:
        rgba = got["rgba"]
        c_ok = not rgba[miss].any() and bool(np.all(rgba[hit][:, 3] == 255))
        if ref["rgb"] is None:
            c_ok = c_ok and not rgba[hit][:, :3].any()
        else:
            x = ref["rgb"][hit] + 0.5
            want = np.clip(np.floor(x), 0, 255)
            tie = np.abs(x - np.round(x)) <= ref["bound_c"][hit][:, None]
            diff = np.abs(rgba[hit][:, :3].astype(np.float64) - want)
            c_ok = c_ok and bool(np.all((diff == 0) | (tie & (diff <= 1))))
    if got.get("label") is not None:
        l_ok = np.array_equal(got["label"][un], ref["label"][un])
    with np.errstate(all="ignore"):
        ratio = (d_err[hit] / ref["bound_d"][hit]).max() if hit.any() else 0.0
    report = "hit/miss %s, depth %s (max err %.3e, max err / bound %.3f), normal %s (max err %.3e), colour %s, label %s, flagged %.4f" % (
        h_ok, d_ok, d_err[hit].max() if hit.any() else 0.0, ratio, n_ok, n_err, c_ok, l_ok, ref["flagged"].mean())
    return h_ok and d_ok and n_ok and c_ok and l_ok, report


def as_got(ref):
    """a reference's own outputs in the form render_matches takes (for holding one reference against another)"""
    depth = np.where(ref["hit"], ref["depth"], 0).astype(np.float32)
    rgba = np.zeros(ref["hit"].shape + (4,), np.uint8)
    if ref["rgb"] is not None:
        rgba[..., :3] = np.clip(np.floor(ref["rgb"] + 0.5), 0, 255)
    rgba[..., 3] = 255
    rgba[~ref["hit"]] = 0
    return dict(depth=depth, normal=ref["normal"].astype(np.float32), rgba=rgba, label=ref["label"])


# ------------------------------------------------------------------------------------------------------------ analytic scene
def analytic_view(pose, intr, ht, wd):
    """the closed forms of tsdf_reference's scene seen from `pose` (world-to-camera): depth along the optical axis [ht,wd], the outward
    unit normal [ht,wd,3] and sphere bool [ht,wd] (the ray hits the sphere in front of the plane)"""
    fx, fy, cx, cy = [np.float64(v) for v in np.asarray(intr, np.float32)]
    pose = np.asarray(pose, np.float32)
    Rm, t = R.rotation(pose[3:]), pose[:3].astype(np.float64)
    c = -Rm.T @ t
    yy, xx = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    dw = np.stack([(xx - cx) / fx, (yy - cy) / fy, np.ones_like(xx, float)], -1) @ Rm               # R^T d, row vectors
    with np.errstate(all="ignore"):
        s_plane = (R.PLANE_D - R.PLANE_N @ c) / (dw @ R.PLANE_N)
        oc = c - R.SPHERE_C
        qa, qb, qc = (dw * dw).sum(-1), 2.0 * (dw @ oc), oc @ oc - R.SPHERE_R ** 2
        disc = qb * qb - 4 * qa * qc
        s_sphere = np.where(disc > 0, (-qb - np.sqrt(np.maximum(disc, 0))) / (2 * qa), np.inf)
    s_sphere = np.where(s_sphere > 0, s_sphere, np.inf)
    sphere = s_sphere < s_plane
    depth = np.minimum(s_plane, s_sphere)
    X = c + np.where(np.isfinite(depth), depth, 0)[..., None] * dw
    n_s = (X - R.SPHERE_C) / R.SPHERE_R
    n_p = -R.PLANE_N * np.sign(R.PLANE_N @ dw.reshape(-1, 3).T).reshape(ht, wd, 1)               # toward the camera's side
    return depth, np.where(sphere[..., None], n_s, n_p), sphere


def interior(sphere, margin=2):
    """bool [ht,wd]: pixels at least `margin` pixels from the sphere's silhouette and from the image border"""
    ht, wd = sphere.shape
    ok = np.zeros_like(sphere)
    ok[margin:ht - margin, margin:wd - margin] = True
    pad = np.pad(sphere, margin, mode="edge")
    for dy in range(-margin, margin + 1):
        for dx in range(-margin, margin + 1):
            ok &= pad[margin + dy:margin + dy + ht, margin + dx:margin + dx + wd] == sphere
    return ok


def view_intrinsics(ht, wd):
    """tsdf_reference.scene's intrinsics for an image of ht x wd"""
    return np.array([0.8 * wd, 0.8 * wd, 0.5 * wd - 0.5, 0.5 * ht - 0.5], np.float32)


OWN_SIZE = (40, 56)                      # the scene's own poses are rendered at this size,
EXTRA_SIZE = (13, 19)                    # the three extra views at this one: no multiple of the 8 x 8 tile in either direction
DZ_FACTOR = 0.6                          # dz = 0.6 voxel: incommensurate with the voxel lattice (the z_k land on no voxel plane)
# what test_tsdf_render_host.py measures on the reference's render (24 x 32, the keyframes' size, dz = voxel / 2) of the fused analytic
# scene "5x24x32" (voxel 0.05) against the closed forms, over pixels two or more from the silhouette and the border, rounded up: the
# largest |depth - closed form| (0.0090), the largest per-view mean of it (0.0016) and the largest component of |normal - closed form|
# (0.1716: the gradient of a volume fused from nearest-pixel depths).  The GPU system test allows twice these.
ANALYTIC_DEPTH_ERR = 0.0091
ANALYTIC_DEPTH_MEAN_ERR = 0.0017
ANALYTIC_NORMAL_ERR = 0.1717


def extra_views(scene_poses):
    """poses [3,7] f32: a novel view between the scene's first two cameras with a pitch and a roll; a view that looks away from the
    volume (a half turn about y); a camera at the sphere's centre that looks back at the scene's cameras (every ray starts inside the
    surface and meets the inner side of the observed shell first: a miss by the rule)"""
    c = []
    for p in np.asarray(scene_poses, np.float32)[:2]:
        c.append(-R.rotation(p[3:]).T @ p[:3].astype(np.float64))
    eye = 0.5 * (c[0] + c[1]) + np.array([0.013, -0.21, 0.05])
    novel = look_at(eye, [0.07, 0.04, 1.6], roll=0.3)
    away = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0], np.float32)
    # (looking back at the cameras, through the part of the sphere they observed: R = diag(-1, 1, -1), t = -R c)
    inside = np.array([R.SPHERE_C[0], -R.SPHERE_C[1], R.SPHERE_C[2], 0.0, 1.0, 0.0, 0.0], np.float32)
    return np.stack([novel, away, inside])


def analytic_labels(dims, origin, voxel, sphere_id, plane_id):
    """a label volume int32 [nz,ny,nx] for the analytic scene: the id of the surface the voxel's centre is nearer to"""
    nz, ny, nx = dims
    zz, yy, xx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    X = np.asarray(origin, np.float32).astype(np.float64) + np.float64(np.float32(voxel)) * np.stack([xx, yy, zz], -1)
    d_plane = np.abs(X @ R.PLANE_N - R.PLANE_D)
    d_sphere = np.abs(np.linalg.norm(X - R.SPHERE_C, axis=-1) - R.SPHERE_R)
    return np.where(d_sphere < d_plane, sphere_id, plane_id).astype(np.int32)


def look_at(eye, target, roll=0.0):
    """a world-to-camera pose [7] f32 (t, q = x, y, z, w) of a camera at `eye` looking at `target`, rolled about its axis"""
    eye, target = np.asarray(eye, float), np.asarray(target, float)
    zc = (target - eye) / np.linalg.norm(target - eye)
    xc = np.cross([0.0, 1.0, 0.0], zc)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    cr, sr = np.cos(roll), np.sin(roll)
    xc, yc = cr * xc + sr * yc, -sr * xc + cr * yc
    Rm = np.stack([xc, yc, zc])                                          # world-to-camera rotation
    w = 0.5 * np.sqrt(max(1.0 + np.trace(Rm), 1e-12))
    q = np.array([(Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w), w])
    return np.concatenate([-Rm @ eye, q]).astype(np.float32)
