"""Writes tests/golden/feature_transport.npz: inputs and outputs of the REFERENCE's own feature transport, for
tests/test_feature_transport_host.py (reference mode of the contract in include/pvo_hip.h pvo_feature_transport).

    python tests/golden/gen_transport_golden.py <path to the reference checkout>

The reference's methods (flow_transport_feature, flow_transport_feature_with_depth, pose_transport_depth, depth_filter, resize of
VPS_Module/detectron2/modeling/meta_arch/panoptic_fpn.py) are taken out of its source file with `ast` at generation time and executed
against a stub `self`; the file's imports (detectron2) are never executed.  Only the inputs and what the methods returned are stored.
One thread (torch.set_num_threads(1)): the reference's indexed assignment `mask[:, v1, u1] = ...` is then serial, last write wins.

Which source cell won a target cell is read off a second run whose features hold the cell's own index + 1 (exact in fp32).

Cases (keys `<case>/<name>`):
  ident_flow, ident_depth   flow grid == level grid (the resize is the identity), flows on quarter pixels, negative ones included
  planted                   three sources on one target at different depths, two at equal depth
  pose                      pose_transport_depth on a 6 x 20 map (fp64, as the reference computes it)
  resized                   a 30 x 101 flow and depth onto 12 x 39 and 6 x 20 levels, with `skip` masks: the target cells a comparison may
                            leave out (a contender's resized flow, recomputed in fp64, within 2^-10 of an integer; or the two best keys
                            of a cell within 2^-20 relative), at most 1 % of the cells
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

METHODS = ("flow_transport_feature", "flow_transport_feature_with_depth", "pose_transport_depth", "depth_filter", "resize")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "feature_transport.npz")


def reference_self(root, alpha, intr=(1.0, 1.0, 0.0, 0.0)):
    path = os.path.join(root, "VPS_Module", "detectron2", "modeling", "meta_arch", "panoptic_fpn.py")
    tree = ast.parse(open(path).read())
    found = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.ClassDef):
            for fn in node.body:
                if isinstance(fn, ast.FunctionDef) and fn.name in METHODS:
                    found[fn.name] = fn
    assert set(found) == set(METHODS), sorted(set(METHODS) - set(found))
    ns = {"np": np, "torch": torch, "F": F}
    exec(compile(ast.Module(body=list(found.values()), type_ignores=[]), path, "exec"), ns)
    me = types.SimpleNamespace(device=torch.device("cpu"), alpha=alpha, flow_is_npy=True, fx=intr[0], fy=intr[1], cx=intr[2], cy=intr[3])
    for name in METHODS:
        setattr(me, name, types.MethodType(ns[name], me))
    return me


def run_reference(root, ref, cur, flow, depth, alpha):
    """ref, cur: lists of [H,W,C] float32; flow [Hf,Wf,2]; depth [Hd,Wd] or None -> (outs [H,W,2C], srcs [H,W] int32) per level"""
    def once(feats, a):
        me = reference_self(root, a)
        pyr = {str(l): torch.from_numpy(np.stack([r, c]).transpose(0, 3, 1, 2).copy()) for l, (r, c) in enumerate(feats)}
        fl = torch.from_numpy(flow.transpose(2, 0, 1).copy())
        if depth is None:
            res = me.flow_transport_feature(pyr, fl)
        else:
            res = me.flow_transport_feature_with_depth(pyr, fl, torch.from_numpy(depth.copy()))
        return [res[str(l)][0].permute(1, 2, 0).contiguous().numpy() for l in range(len(feats))]

    outs = once(list(zip(ref, cur)), alpha)
    ids = [np.arange(1, r.shape[0] * r.shape[1] + 1, dtype=np.float32).reshape(r.shape[0], r.shape[1], 1) for r in ref]
    won = once([(i, np.zeros_like(i)) for i in ids], 1.0)
    srcs = [np.rint(w[..., 1]).astype(np.int32) - 1 for w in won]
    for o, s, r in zip(outs, srcs, ref):
        assert o.dtype == np.float32 and s.shape == r.shape[:2]
    return outs, srcs


def resize64(A, H, W):
    """the align_corners resize in fp64 (what the reference's F.interpolate computes, without its fp32 rounding)"""
    A = A.astype(np.float64)
    Ha, Wa = A.shape
    py = np.arange(H) * ((Ha - 1) / (H - 1) if H > 1 else 0.0)
    px = np.arange(W) * ((Wa - 1) / (W - 1) if W > 1 else 0.0)
    y0, x0 = np.minimum(py.astype(int), Ha - 1), np.minimum(px.astype(int), Wa - 1)
    y1, x1 = np.minimum(y0 + 1, Ha - 1), np.minimum(x0 + 1, Wa - 1)
    ly, lx = (py - y0)[:, None], (px - x0)[None, :]
    top = (1 - lx) * A[y0][:, x0] + lx * A[y0][:, x1]
    bot = (1 - lx) * A[y1][:, x0] + lx * A[y1][:, x1]
    return (1 - ly) * top + ly * bot


def skip_mask(flow, depth, H, W):
    """target cells a comparison may leave out (module docstring)"""
    fx, fy, d = resize64(flow[..., 0], H, W), resize64(flow[..., 1], H, W), resize64(depth, H, W)
    near = lambda f: np.abs(f - np.rint(f)) < 2.0 ** -10
    unsure = near(fx) | near(fy)
    skip = np.zeros((H, W), bool)
    lands = {}
    for y in range(H):
        for x in range(W):
            cx = {int(np.floor(fx[y, x]))} | ({int(np.rint(fx[y, x])), int(np.rint(fx[y, x])) - 1} if near(fx[y, x]) else set())
            cy = {int(np.floor(fy[y, x]))} | ({int(np.rint(fy[y, x])), int(np.rint(fy[y, x])) - 1} if near(fy[y, x]) else set())
            for qx in cx:
                for qy in cy:
                    tx, ty = x + qx, y + qy
                    if 0 <= tx < W and 0 <= ty < H:
                        if unsure[y, x]:
                            skip[ty, tx] = True
                        else:
                            lands.setdefault((ty, tx), []).append(d[y, x])
    for (ty, tx), keys in lands.items():
        keys = sorted(keys)
        if len(keys) > 1 and keys[1] - keys[0] < 2.0 ** -20 * abs(keys[1]) and keys[1] != keys[0]:
            skip[ty, tx] = True
    return skip


def main(root):
    torch.set_num_threads(1)
    g = np.random.default_rng(20)
    out = {}
    notes = []

    def feats(H, W, C=4):
        return g.standard_normal((H, W, C)).astype(np.float32), g.standard_normal((H, W, C)).astype(np.float32)

    # flow grid == level grid, quarter-pixel flows in [-3, 5]
    H, W = 9, 14
    flow = (g.integers(-12, 21, (H, W, 2)) / 4.0).astype(np.float32)
    flow[0, :4] = [-1.0, 0.75]                     # a negative component of a whole pixel or more: out of the image
    flow[1, :4] = [-0.75, 0.0]                     # in (-1, 0): truncates to zero
    depth = g.uniform(0.5, 8.0, (H, W)).astype(np.float32)
    ref, cur = feats(H, W)
    for name, dep in (("ident_flow", None), ("ident_depth", depth)):
        outs, srcs = run_reference(root, [ref], [cur], flow, dep, 0.5)
        neg = (np.trunc(flow) <= -1).any(-1)
        ok = not np.isin(np.flatnonzero(neg), srcs[0][srcs[0] >= 0]).any()      # no cell with a flow <= -1 is anybody's source
        stay = np.flatnonzero(((flow > -1) & (flow <= 0)).all(-1))
        if dep is None:                                                         # a flow in (-1, 0] stays: its cell is reached by it or a later one
            ok = ok and all((srcs[0].reshape(-1)[s] >= s) for s in stay)
        if not ok:
            notes.append("%s dropped: this numpy casts negative floats to uint16 otherwise" % name)
            continue
        out.update({name + "/flow": flow, name + "/ref": ref, name + "/cur": cur, name + "/out": outs[0], name + "/src": srcs[0],
                    name + "/alpha": np.float32(0.5)})
        if dep is not None:
            out[name + "/depth"] = dep
    empty = np.full((H, W, 2), -1.25, np.float32)
    outs, srcs = run_reference(root, [ref], [cur], empty, None, 1.0)
    assert (srcs[0] == -1).all() and not outs[0][..., 4:].any(), "negative flows must come out empty"
    out.update({"negative/flow": empty, "negative/ref": ref, "negative/cur": cur, "negative/out": outs[0], "negative/src": srcs[0],
                "negative/alpha": np.float32(1.0)})

    # planted collisions on a 6 x 8 level: everything else leaves the image
    H, W = 6, 8
    flow = np.full((H, W, 2), -2.0, np.float32)
    depth = np.ones((H, W), np.float32)
    for (y, x), d in (((1, 1), 1.5), ((2, 3), 3.0), ((0, 2), 2.0)):                 # three on (3, 4): the nearest is not the last
        flow[y, x] = [4 - x, 3 - y]
        depth[y, x] = d
    for (y, x), d in (((0, 5), 2.5), ((1, 6), 2.5)):                                # two on (5, 7) at one depth: the later cell wins
        flow[y, x] = [7 - x, 5 - y]
        depth[y, x] = d
    ref, cur = feats(H, W)
    for name, dep in (("planted", depth), ("planted_flow", None)):
        outs, srcs = run_reference(root, [ref], [cur], flow, dep, 1.0)
        assert srcs[0][3, 4] == (1 * W + 1 if dep is not None else 2 * W + 3) and srcs[0][5, 7] == 1 * W + 6 and (srcs[0] >= 0).sum() == 2
        out.update({name + "/flow": flow, name + "/ref": ref, name + "/cur": cur, name + "/out": outs[0], name + "/src": srcs[0],
                    name + "/alpha": np.float32(1.0)})
        if dep is not None:
            out[name + "/depth"] = dep

    # pose_transport_depth on a 6 x 20 map
    intr = (52.5, 48.25, 9.5, 2.75)
    me = reference_self(root, 1.0, intr)
    depth = g.uniform(1.0, 20.0, (6, 20)).astype(np.float32)

    def pose(seed):
        q = np.random.default_rng(seed)
        w = q.uniform(-0.2, 0.2, 3)
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        th = np.linalg.norm(w)
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, q.uniform(-0.5, 0.5, 3)
        return T

    p0, p1 = pose(1), pose(2)
    moved = me.pose_transport_depth(torch.from_numpy(depth), [p0.reshape(-1).tolist(), p1.reshape(-1).tolist()]).numpy()
    assert moved.dtype == np.float64 and moved.shape == (6, 20)
    rel = p1 @ np.linalg.inv(p0)
    out.update({"pose/depth": depth, "pose/rel_pose": rel[:3].reshape(12), "pose/intrinsics": np.array(intr), "pose/out": moved})

    # one resized case: 30 x 101 onto 12 x 39 and 6 x 20
    Hf, Wf = 30, 101
    shapes = ((12, 39), (6, 20))
    yy, xx = np.mgrid[:Hf, :Wf]
    flow = np.stack([1.3 + 0.011 * xx + 0.7 * np.sin(yy / 5.0), 0.6 + 0.9 * np.cos(xx / 11.0) + 0.02 * yy], -1).astype(np.float32)
    flow += g.uniform(-0.2, 0.2, flow.shape).astype(np.float32)
    flow[:6, :12] = -1.5
    depth = (4.0 + 2.0 * np.sin(xx / 7.0) + g.uniform(0, 1.0, (Hf, Wf))).astype(np.float32)
    pyr = [feats(H, W) for H, W in shapes]
    outs, srcs = run_reference(root, [p[0] for p in pyr], [p[1] for p in pyr], flow, depth, 0.5)
    out.update({"resized/flow": flow, "resized/depth": depth, "resized/alpha": np.float32(0.5)})
    for l, (H, W) in enumerate(shapes):
        skip = skip_mask(flow, depth, H, W)
        assert skip.mean() <= 0.01, ("the inputs must meet the 1 % cap", l, skip.mean())
        assert (srcs[l] >= 0).sum() > H * W // 4
        out.update({"resized/ref%d" % l: pyr[l][0], "resized/cur%d" % l: pyr[l][1], "resized/out%d" % l: outs[l],
                    "resized/src%d" % l: srcs[l], "resized/skip%d" % l: skip})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes;", len(out), "arrays;", "; ".join(notes) or "no case dropped")


if __name__ == "__main__":
    main(sys.argv[1])
