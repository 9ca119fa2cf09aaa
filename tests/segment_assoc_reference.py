"""The contract of pvo_segment_associate (include/pvo_hip.h) restated in numpy: the yardstick of tests/test_segment_tracks_host.py and
tests/test_segment_assoc_gpu.py.  Integers and exactly stated fp32 operations only, so the tests compare with equality.

    associate(labels, ii, jj, target, S, valid, cls, min_iou, mutant)    the six outputs
    scene(ht, wd, nframes, plain)                                        the fixed scene (SIZES, EDGES, S, MIN_IOU)
    PLANTED                                                              hand-made cases, each with the counts its docstring derives
    MUTANTS                                                              wrong readings of the contract the scene must tell apart

The scene.  Ground-truth ids: 1 the wall (everything not named below), 2 a rectangle moving (+k, 0) pixels per frame, 3 a disc moving
(-k, k - 1) per frame and painted over the rectangle (k = min(ht // 9, wd // 12): 1, 2, 3 at the three sizes), 0 (no segment) in the two
rightmost columns, whose flow (+3, 0) leaves the frame.  Unless plain:
  4  a sliver of the top row whose LABEL moves while the wall under it does not (a segmentation that drifts): columns 0..5 in frame 0,
     3..9 in frame 1, absent later.  On edge (0, 1) n = 3 (columns 3, 4, 5), area_i = 6, area_j = 7, d = 10: n / d = 3 / 10 exactly, and
     MIN_IOU = float32(0.3) = 0.300000011920929 > 3 / 10: no match by the contract, a match for whoever compares in fp32
  5  a 2 x 4 block in the bottom left corner, whole in the even frames and split into halves 5 | 6 in the odd ones: on (0, 1) segment 5
     overlaps both halves with n / d = 4 / 8 (best_j ties), on (1, 2) both halves overlap the whole with 4 / 8 (best_i ties)
Each frame's ids 1..S-1 are then permuted independently; the targets are the painted layer's true shift plus a fixed sub-pixel
pattern within +-0.22 (so that rounding, not truncation, recovers the shift)."""
import numpy as np

f32 = np.float32
SIZES = ((24, 32), (9, 12), (30, 101))
EDGES = ((0, 1), (1, 2), (3, 1), (0, 4), (2, 2))
NFRAMES = 5
S = 8
MIN_IOU = 0.3
OUTPUTS = ("overlap", "area_i", "area_j", "match", "match_n", "match_d")
MUTANTS = ("truncate", "swap_xy", "label_of_source_frame", "no_bounds", "tie_high", "float_iou")


def _ahead(n1, d1, k1, n2, d2, k2, mutant):
    """is (n1 / d1, index k1) ahead of (n2 / d2, k2)?  n2 = 0: there is no second"""
    if n2 == 0:
        return True
    if mutant == "float_iou":
        l, r = f32(n1) / f32(d1), f32(n2) / f32(d2)
    else:
        l, r = int(n1) * int(d2), int(n2) * int(d1)
    if l != r:
        return bool(l > r)
    return k1 > k2 if mutant == "tie_high" else k1 < k2


def associate(labels, ii, jj, target, S, valid=None, cls=None, min_iou=0.25, mutant=None):
    labels = np.asarray(labels)
    nf, ht, wd = labels.shape
    E = len(ii)
    out = dict(overlap=np.zeros((E, S, S), np.int32), area_i=np.zeros((E, S), np.int32), area_j=np.zeros((E, S), np.int32),
               match=np.full((E, S), -1, np.int32), match_n=np.zeros((E, S), np.int32), match_d=np.zeros((E, S), np.int32))
    dense = np.where((labels >= 0) & (labels < S), labels, 0).astype(np.int64)
    half = f32(0.0) if mutant == "truncate" else f32(0.5)
    for e in range(E):
        i, j = int(ii[e]), int(jj[e])
        if not (0 <= i < nf and 0 <= j < nf):
            continue
        t = np.asarray(target[e], f32)
        tx, ty = (t[..., 1], t[..., 0]) if mutant == "swap_xy" else (t[..., 0], t[..., 1])
        with np.errstate(invalid="ignore", over="ignore"):
            rx, ry = np.floor((tx + half).astype(f32)), np.floor((ty + half).astype(f32))
            fin = np.isfinite(tx) & np.isfinite(ty)
            if mutant == "no_bounds":
                rx, ry = np.clip(np.where(fin, rx, 0), 0, wd - 1), np.clip(np.where(fin, ry, 0), 0, ht - 1)
                counted = fin
            else:
                counted = fin & (rx >= f32(0)) & (rx <= f32(wd - 1)) & (ry >= f32(0)) & (ry <= f32(ht - 1))
        if valid is not None:
            counted = counted & (np.asarray(valid[e]) != 0)
        a = dense[i][counted]
        x, y = rx[counted].astype(np.int64), ry[counted].astype(np.int64)
        b = dense[i if mutant == "label_of_source_frame" else j][y, x]
        np.add.at(out["overlap"][e], (a, b), 1)
        out["area_i"][e] = np.bincount(a, minlength=S)
        out["area_j"][e] = np.bincount(dense[j].ravel(), minlength=S)
        ov, ai, aj = out["overlap"][e], out["area_i"][e], out["area_j"][e]
        best_j, best_i = {}, {}                                              # a -> (n, d, b);  b -> (n, d, a)
        for a_, b_ in zip(*np.nonzero(ov)):
            a_, b_ = int(a_), int(b_)
            if a_ == 0 or b_ == 0 or (cls is not None and cls[i][a_] != cls[j][b_]):
                continue
            n = int(ov[a_, b_])
            d = int(ai[a_]) + int(aj[b_]) - n
            pj, pi = best_j.get(a_, (0, 1, 0)), best_i.get(b_, (0, 1, 0))
            if _ahead(n, d, b_, pj[0], pj[1], pj[2], mutant):
                best_j[a_] = (n, d, b_)
            if _ahead(n, d, a_, pi[0], pi[1], pi[2], mutant):
                best_i[b_] = (n, d, a_)
        for a_, (n, d, b_) in best_j.items():
            if best_i[b_][2] != a_:
                continue
            if mutant == "float_iou":
                ok = f32(n) / f32(d) >= f32(min_iou)
            else:
                ok = float(n) >= float(f32(min_iou)) * float(d)                # exact in fp64: n, d < 2^24
            if ok:
                out["match"][e, a_], out["match_n"][e, a_], out["match_d"][e, a_] = b_, n, d
    return out


# ------------------------------------------------------------------------------------------------------------------ the scene
def truth_frame(ht, wd, f, plain=False):
    """(ground-truth ids int32 [ht,wd], the painted layer's motion per frame [ht,wd,2] as (dx, dy)) of frame f"""
    k = min(ht // 9, wd // 12)
    ys, xs = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    ids = np.ones((ht, wd), np.int32)
    vel = np.zeros((ht, wd, 2), np.int64)
    rect = (ys >= 2 * k) & (ys < 4 * k) & (xs >= k + k * f) & (xs < 4 * k + k * f)
    ids[rect], vel[rect] = 2, (k, 0)
    cy, cx = 5 * k + (k - 1) * f, 8 * k - k * f
    disc = 4 * ((ys - cy) ** 2 + (xs - cx) ** 2) <= 9 * k * k
    ids[disc], vel[disc] = 3, (-k, k - 1)
    ids[:, wd - 2:], vel[:, wd - 2:] = 0, (3, 0)
    if not plain:
        if f == 0:
            ids[0, 0:6] = 4
        elif f == 1:
            ids[0, 3:10] = 4
        ids[ht - 2:, 0:4] = 5
        if f % 2:
            ids[ht - 2:, 2:4] = 6
    return ids, vel


def scene(ht, wd, nframes=NFRAMES, edges=EDGES, plain=False, seed=7):
    """dict: labels int32 [nframes,ht,wd] (per-frame permuted ids), truth (the unpermuted ones), perm [nframes,S] (truth id -> label),
    ii, jj int64 [E], target f32 [E,ht,wd,2], valid uint8 [E,ht,wd] (a fixed lattice of zeros), cls int32 [nframes,S]"""
    rng = np.random.RandomState(seed + 131 * ht + wd)
    truth, vels = zip(*(truth_frame(ht, wd, f, plain) for f in range(nframes)))
    truth = np.stack(truth)
    perm = np.zeros((nframes, S), np.int32)
    for f in range(nframes):
        perm[f, 1:] = 1 + rng.permutation(S - 1)
    labels = np.stack([perm[f][truth[f]] for f in range(nframes)]).astype(np.int32)
    ii, jj = np.array([e[0] for e in edges], np.int64), np.array([e[1] for e in edges], np.int64)
    ys, xs = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    target = np.zeros((len(edges), ht, wd, 2), f32)
    for e, (i, j) in enumerate(edges):
        sx = (((xs * 7 + ys * 3 + e) % 5) - 2).astype(f32) * f32(0.11)
        sy = (((xs * 5 + ys * 11 + 2 * e) % 7) - 3).astype(f32) * f32(0.07)
        target[e, ..., 0] = (xs + (j - i) * vels[i][..., 0]).astype(f32) + sx
        target[e, ..., 1] = (ys + (j - i) * vels[i][..., 1]).astype(f32) + sy
    valid = np.ones((len(edges), ht, wd), np.uint8)
    valid[:, (ys * 5 + xs * 3) % 11 == 0] = 0
    class_of_truth = np.array([0, 0, 1, 1, 2, 3, 7, 0], np.int32)             # the second half (6) never matches the whole block (5)
    cls = np.zeros((nframes, S), np.int32)
    for f in range(nframes):
        cls[f][perm[f]] = class_of_truth
    return dict(labels=labels, truth=truth, perm=perm, ii=ii, jj=jj, target=target, valid=valid, cls=cls)


def spread(sc, S_big=160):
    """the scene's labels spread over [0, S_big): label l >= 1 -> 1 + (37 l) mod (S_big - 1) (37 is coprime to 159); cls follows"""
    to = np.zeros(S, np.int32)
    to[1:] = 1 + (37 * np.arange(1, S)) % (S_big - 1)
    cls = np.zeros((sc["cls"].shape[0], S_big), np.int32)
    cls[:, to] = sc["cls"]
    return dict(sc, labels=to[sc["labels"]], cls=cls)


# ------------------------------------------------------------------------------------------------------------- planted cases
def _identity(E, ht, wd):
    ys, xs = np.meshgrid(np.arange(ht), np.arange(wd), indexing="ij")
    return np.tile(np.stack([xs, ys], -1).astype(f32)[None], (E, 1, 1, 1))


def _case(labels, target=None, **kw):
    labels = np.asarray(labels, np.int32)
    nf, ht, wd = labels.shape
    c = dict(labels=labels, ii=np.array([0], np.int64), jj=np.array([1], np.int64), target=_identity(1, ht, wd) if target is None else target,
             S=8, valid=None, cls=None, min_iou=0.25)
    c.update(kw)
    return c


def planted_rounding():
    """4 x 6; frame 0 is all 1, frame 1 carries x + 1 in column x (b tells rx), ty = the pixel's own row.  Twelve pixels carry a target,
    the others NaN.  Row 0: tx = 1.5 (k - 0.5: floor(2.0) = 2, b = 3);  2.5 (k + 0.5: floor(3.0) = 3, b = 4);  0.49999997f (the fp32 sum
    0.49999997 + 0.5 is the tie 1 - 2^-25 and rounds to 1.0: rx = 1, b = 2, where real arithmetic says 0);  -0.5 (floor(0.0) = 0: counted,
    b = 1);  5.5 = wd - 0.5 (floor(6.0) = 6 > 5: dropped);  NaN.  Row 1: +inf, -inf, 1e30, a NaN in ty alone, -0.50000006 (floor of
    -6e-8 is -1: dropped), and ty = 3.5 = ht - 0.5 (dropped).  So four pixels are counted: overlap[1, 3] = [1, 4] = [1, 2] = [1, 1] = 1,
    area_i[1] = 4; area_j[b] = 4 (four rows) for b = 1..6.  a = 1 overlaps four labels with n / d = 1 / (4 + 4 - 1): best_j(1) = 1 by
    the tie rule, best_i(1) = 1, and 1 / 7 < 1 / 4: no match."""
    ht, wd = 4, 6
    labels = np.ones((2, ht, wd), np.int32)
    labels[1] = np.arange(1, wd + 1)[None, :]
    t = np.full((1, ht, wd, 2), np.nan, f32)
    t[0, 0, :, 1], t[0, 1, :, 1] = 0.0, 1.0
    t[0, 0, :, 0] = [1.5, 2.5, f32(0.49999997), -0.5, 5.5, np.nan]
    t[0, 1, :, 0] = [np.inf, -np.inf, 1e30, 2.0, f32(-0.50000006), 2.0]
    t[0, 1, 3, 1], t[0, 1, 5, 1] = np.nan, 3.5
    ov = np.zeros((8, 8), np.int32)
    ov[1, [3, 4, 2, 1]] = 1
    return _case(labels, t), dict(overlap=ov[None], area_i=np.array([[0, 4, 0, 0, 0, 0, 0, 0]]), area_j=np.array([[0, 4, 4, 4, 4, 4, 4, 0]]),
                                  match=np.full((1, 8), -1))


def planted_mask_and_range():
    """4 x 6, identity targets.  Frame 0 is all 1 but (0, 0) = 99, (0, 1) = 8 (= S) and (0, 2) = -5: three labels outside [0, S), read as
    0.  Frame 1 is all 2 but (1, 1) = 1000, read as 0.  valid is zero on row 3.  Counted: 24 - 6 = 18 pixels; a = 0 for three of them
    (overlap[0, 2] = 3), b = 0 for one (overlap[1, 0] = 1), the rest overlap[1, 2] = 18 - 3 - 1 = 14.  area_i = (3, 15), area_j counts the
    WHOLE frame, the masked row included: area_j[2] = 23, area_j[0] = 1.  n / d = 14 / (15 + 23 - 14) = 14 / 24: match[1] = 2."""
    labels = np.ones((2, 4, 6), np.int32)
    labels[0, 0, :3] = [99, 8, -5]
    labels[1] = 2
    labels[1, 1, 1] = 1000
    valid = np.ones((1, 4, 6), np.uint8)
    valid[0, 3] = 0
    ov = np.zeros((8, 8), np.int32)
    ov[0, 2], ov[1, 0], ov[1, 2] = 3, 1, 14
    m, n, d = np.full((1, 8), -1), np.zeros((1, 8), int), np.zeros((1, 8), int)
    m[0, 1], n[0, 1], d[0, 1] = 2, 14, 24
    return _case(labels, valid=valid), dict(overlap=ov[None], area_i=np.array([[3, 15, 0, 0, 0, 0, 0, 0]]), area_j=np.array([[1, 0, 23, 0, 0, 0, 0, 0]]),
                                            match=m, match_n=n, match_d=d)


def planted_ties():
    """2 x 8, identity.  Frame 0: 1 on columns 0..3, 2 on 4..5, 3 on 6..7.  Frame 1: 1 on 0..1, 2 on 2..3 (segment 1 split in halves), 3
    on 4..7 (segments 2 and 3 merged).  a = 1: n = 4 with b = 1 and with b = 2, d = 8 + 4 - 4 = 8 both: the tie goes to the LOWEST b,
    best_j(1) = 1, best_i(1) = 1: match[1] = 1 with 4 / 8.  b = 3: n = 4 from a = 2 and from a = 3, d = 4 + 8 - 4 = 8 both: best_i(3) = 2,
    the lowest a.  match[2] = 3 with 4 / 8; match[3] = -1 (its best_j is 3, whose best_i is 2)."""
    labels = np.zeros((2, 2, 8), np.int32)
    labels[0, :, 0:4], labels[0, :, 4:6], labels[0, :, 6:8] = 1, 2, 3
    labels[1, :, 0:2], labels[1, :, 2:4], labels[1, :, 4:8] = 1, 2, 3
    return _case(labels), dict(match=np.array([[-1, 1, 3, -1, -1, -1, -1, -1]]), match_n=np.array([[0, 4, 4, 0, 0, 0, 0, 0]]),
                               match_d=np.array([[0, 8, 8, 0, 0, 0, 0, 0]]), area_i=np.array([[0, 8, 4, 4, 0, 0, 0, 0]]),
                               area_j=np.array([[0, 4, 4, 8, 0, 0, 0, 0]]))


def planted_not_mutual():
    """1 x 10, identity, min_iou = 0.1.  Frame 0: 1 on columns 0..5, 2 on 6..9.  Frame 1: 0 on 0..3, 1 on 4..9.  a = 1 meets only b = 1:
    n = 2 (columns 4, 5), d = 6 + 6 - 2 = 10, 1 / 5 >= 0.1 - but best_i(1) = 2 (n = 4, d = 4 + 6 - 4 = 6, 2 / 3 > 1 / 5): match[1] = -1
    for want of mutuality alone, match[2] = 1 with 4 / 6."""
    labels = np.zeros((2, 1, 10), np.int32)
    labels[0, 0, 0:6], labels[0, 0, 6:10] = 1, 2
    labels[1, 0, 4:10] = 1
    return _case(labels, min_iou=0.1), dict(match=np.array([[-1, -1, 1, -1, -1, -1, -1, -1]]), match_n=np.array([[0, 0, 4, 0, 0, 0, 0, 0]]),
                                            match_d=np.array([[0, 0, 6, 0, 0, 0, 0, 0]]))


def planted_threshold():
    """1 x 48, identity, min_iou = 0.25.  a = 1 on columns 0..1, b = 1 on 1..3: n = 1, d = 2 + 3 - 1 = 4: exactly 1 / 4, a match.
    a = 2 on columns 8..15, b = 2 on 8..40: n = 8, d = 8 + 33 - 8 = 33: 8 / 33 = 0.2424 < 1 / 4, none."""
    labels = np.zeros((2, 1, 48), np.int32)
    labels[0, 0, 0:2], labels[0, 0, 8:16] = 1, 2
    labels[1, 0, 1:4], labels[1, 0, 8:41] = 1, 2
    return _case(labels), dict(match=np.array([[-1, 1, -1, -1, -1, -1, -1, -1]]), match_n=np.array([[0, 1, 0, 0, 0, 0, 0, 0]]),
                               match_d=np.array([[0, 4, 0, 0, 0, 0, 0, 0]]))


def planted_cls_veto():
    """1 x 8, identity.  Frame 0: 1 everywhere.  Frame 1: 1 on columns 0..5, 2 on 6..7.  Without cls a = 1 takes b = 1 (6 / 8 against
    2 / 8).  cls[0] = (0, 5, ...), cls[1] = (0, 9, 5, ...): the pair (1, 1) is ruled out of BOTH maxima, match[1] = 2 with n = 2,
    d = 8 + 2 - 2 = 8 - exactly 1 / 4."""
    labels = np.ones((2, 1, 8), np.int32)
    labels[1, 0, 6:8] = 2
    cls = np.zeros((2, 8), np.int32)
    cls[0, 1], cls[1, 1], cls[1, 2] = 5, 9, 5
    return _case(labels, cls=cls), dict(match=np.array([[-1, 2, -1, -1, -1, -1, -1, -1]]), match_n=np.array([[0, 2, 0, 0, 0, 0, 0, 0]]),
                                        match_d=np.array([[0, 8, 0, 0, 0, 0, 0, 0]]))


PLANTED = dict(rounding=planted_rounding, mask_and_range=planted_mask_and_range, ties=planted_ties, not_mutual=planted_not_mutual,
               threshold=planted_threshold, cls_veto=planted_cls_veto)


def run(c, **kw):
    """associate on a case or a scene dict"""
    a = dict(S=c.get("S", S), valid=c.get("valid"), cls=c.get("cls"), min_iou=c.get("min_iou", MIN_IOU))
    a.update(kw)
    return associate(c["labels"], c["ii"], c["jj"], c["target"], **a)


def same(a, b, keys=OUTPUTS):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in keys)
