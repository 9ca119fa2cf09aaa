"""Panoptic surface reconstruction: what the label vote and the vertex labels cost on the MI355X, and that the plain calls cost what
they did.

    python tools/tsdf_panoptic_bench.py [--reps 30] [--frames 64] [--dim 256] [--out profiles/r18_tsdf_panoptic.txt]
                                        [--tree DIR --plain_json FILE]  [--parent_json FILE]

tools/tsdf_bench.py's scene and method (64 keyframes in front of a plane with a sphere before it, at 48 x 64 and at 384 x 512, fused
with colours into the 256^3 extent; per call between two device events, median and 10th .. 90th percentile of `reps` repetitions after
5 warm-ups).  Measured, dense and sparse (tools/tsdf_sparse_bench.py's brick volume, allocated once): the plain integrate and mesh
calls, and the panoptic ones with per-frame id maps (the sphere one id, the plane another, from the depth; 48 x 64 maps with label_div
1, and for the 384 x 512 maps the same 48 x 64 ids with label_div 8, as DepthVideo.tsdf(full_res=True, panoptic=True) passes them).
The sha256 of the plain calls' volume and mesh is printed beside the values profiles/r17_tsdf_sparse.txt recorded for the parent
commit's library on this scene; they must be equal.

--tree DIR measures the pvo_amd package of another checkout (a build of the parent commit): only the plain calls, which is all that
checkout has, written to --plain_json.  A later run on this checkout with --parent_json FILE prints those times beside its own: the
new template parameter must cost the plain path nothing, so a difference larger than the two runs' p10 .. p90 spread is a finding.
Needs the GPU: there is no fallback."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tsdf_bench import make_video, measure, stats  # noqa: E402

# profiles/r17_tsdf_sparse.txt: the parent commit's library on this scene (volume = tsdf + wsum + rgb; mesh = counts + verts + normals +
# rgba + faces with capacities 600000 / 1200000)
PARENT_SHA = {(48, 64): ("85bf37690874a1572dddd4a7f5c5afa3d6864823a1899c83eb1ac31bf1afd320",
                         "10bd8a4de0d39caa4ec1bc6f80951b401cb3bd55e505ef00b5c23159aae7f61b"),
              (384, 512): ("1d55852de2f420f3ed7e7601ddf0dab6fdc9da5284dc19938986370a970a48c5",
                           "cfea82a75dea272f7ae4f2db9e359780478a893af01db859e561907e4521d60c")}
ID_SPHERE, ID_PLANE = (1 << 25) + 3, (1 << 24) + 5
VCAP, FCAP = 600000, 1200000


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def mesh_buffers(dev, labels):
    out = {"verts": torch.zeros(VCAP, 3, device=dev), "normals": torch.zeros(VCAP, 3, device=dev),
           "rgba": torch.zeros(VCAP, 4, dtype=torch.uint8, device=dev), "faces": torch.zeros(FCAP, 3, dtype=torch.int32, device=dev),
           "counts": torch.zeros(2, dtype=torch.int32, device=dev)}
    if labels:
        out["vlabel"] = torch.zeros(VCAP, dtype=torch.int32, device=dev)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_tsdf_panoptic.txt"))
    ap.add_argument("--tree", default=ROOT, help="the checkout whose pvo_amd package is measured (another one: plain calls only)")
    ap.add_argument("--plain_json", default=None, help="write the plain calls' times here")
    ap.add_argument("--parent_json", default=None, help="a --plain_json file of the parent commit's build, printed beside this build's")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_panoptic_bench needs the GPU (there is no fallback)")
    sys.path.insert(0, os.path.abspath(args.tree))
    from pvo_amd import droid_backends as db
    from pvo_amd.tsdf_sparse import SparseTSDF
    panoptic = os.path.samefile(args.tree, ROOT)
    parent = json.load(open(args.parent_json)) if args.parent_json else None
    dev = torch.device("cuda:0")
    nf, dim = args.frames, args.dim
    voxel = 2.56 / dim
    trunc, origin = 3.0 * voxel, (-1.28, -1.28, 0.5)
    lines = ["tsdf_panoptic_bench on %s: %d keyframes, the %d^3 extent (voxel %.4f, trunc %.4f), colours on; pvo_amd of %s"
             % (torch.cuda.get_device_name(0), nf, dim, voxel, trunc, "this checkout" if panoptic else "another checkout (plain calls only)"),
             "per call, device events, median [p10 .. p90] of %d repetitions after 5 warm-ups" % args.reps, ""]
    record = {}
    for ht, wd in ((48, 64), (384, 512)):
        poses, disps, intr, images = make_video(nf, ht, wd, dev)
        ix = torch.arange(nf, device=dev)
        div = ht // 48
        labels = torch.where(disps[:, div // 2::div, div // 2::div] > 1.0 / 1.66, ID_SPHERE, ID_PLANE).to(torch.int32).contiguous()
        frames = (poses, disps, intr, ix)
        img = dict(images=images, img_stride=1, img_offset=0)
        # dense
        vol = [torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, 3, device=dev)]
        db.tsdf_integrate(vol[0], vol[1], vol[2], *frames, origin, voxel, trunc, **img)
        out = mesh_buffers(dev, False)
        db.tsdf_mesh_into(vol[0], vol[1], vol[2], origin, voxel, 1.0, out)
        nv, nfaces = out["counts"].tolist()
        got = [sha(vol), sha([out["counts"], out["verts"][:nv], out["normals"][:nv], out["rgba"][:nv], out["faces"][:nfaces]])]
        whole = sha([out[k] for k in ("counts", "verts", "normals", "rgba", "faces")])         # (the zeroed buffers at their capacities)
        if (ht, wd) in PARENT_SHA and whole == PARENT_SHA[(ht, wd)][1]:
            got[1] = whole
        fns = {"dense integrate": lambda: db.tsdf_integrate(vol[0], vol[1], vol[2], *frames, origin, voxel, trunc, **img),
               "dense mesh": lambda: db.tsdf_mesh_into(vol[0], vol[1], vol[2], origin, voxel, 1.0, out)}
        # sparse: allocated once, as tools/tsdf_sparse_bench.py does
        g = -(-dim // 8)
        sp = SparseTSDF(origin, (g, g, g), voxel, trunc, colours=True, device=dev, cap=4096, **({"labels": True} if panoptic else {}))
        bricks = sp.allocate(*frames)
        sout = mesh_buffers(dev, False)
        fns["sparse integrate"] = lambda: db.tsdf_sparse_integrate(sp.volume(), *frames, trunc, **img)
        fns["sparse mesh"] = lambda: db.tsdf_sparse_mesh_into(sp.volume(), 1.0, sout)
        if panoptic:
            label, lconf = torch.zeros(dim, dim, dim, dtype=torch.int32, device=dev), torch.zeros(dim, dim, dim, device=dev)
            pan = dict(label=label, lconf=lconf, labels=labels, label_div=div)
            pout, spout = mesh_buffers(dev, True), mesh_buffers(dev, True)
            fns["dense integrate panoptic"] = lambda: db.tsdf_integrate(vol[0], vol[1], vol[2], *frames, origin, voxel, trunc, **img, **pan)
            fns["dense mesh panoptic"] = lambda: db.tsdf_mesh_into(vol[0], vol[1], vol[2], origin, voxel, 1.0, pout, label=label)
            span = dict(label=sp.label, lconf=sp.lconf, labels=labels, label_div=div)
            fns["sparse integrate panoptic"] = lambda: db.tsdf_sparse_integrate(sp.volume(), *frames, trunc, **img, **span)
            fns["sparse mesh panoptic"] = lambda: db.tsdf_sparse_mesh_into(sp.volume(), 1.0, spout, label=sp.label)
            fns["dense integrate panoptic"]()
            voted, ids = int((label > 0).sum()), sorted(label.unique().tolist())
        t = {k: stats(v) for k, v in measure(fns, args.reps).items()}
        touched = int((vol[1] > 0).sum())
        lines += ["%d x %d maps%s: %d of %d voxels touched; mesh %d vertices, %d faces; %d bricks" % (
            ht, wd, ", ids at %d x %d with label_div %d" % (labels.shape[1], labels.shape[2], div) if panoptic else "", touched, dim ** 3,
            nv, nfaces, bricks)]
        if panoptic:
            lines.append("  %d voxels hold an id after one call (%.1f %% of the touched ones), ids %s" % (voted, 100.0 * voted / touched, ids))
        for kind in ("dense integrate", "dense mesh", "sparse integrate", "sparse mesh"):
            row = "  %-17s plain %9.1f us [%.1f .. %.1f]" % ((kind,) + t[kind])
            if panoptic:
                p = t[kind + " panoptic"]
                row += "   panoptic %9.1f us [%.1f .. %.1f]   panoptic / plain %.3f" % (p + (p[0] / t[kind][0],))
            if parent is not None:
                q = parent["%dx%d" % (ht, wd)][kind]
                spread = max(t[kind][2] - t[kind][1], q[2] - q[1])
                row += "   parent's plain %9.1f us [%.1f .. %.1f]: %+.1f us, %s the larger p10 .. p90 spread (%.1f us)" % (
                    tuple(q) + (t[kind][0] - q[0], "within" if abs(t[kind][0] - q[0]) <= spread else "ABOVE", spread))
            lines.append(row)
        want = PARENT_SHA.get((ht, wd)) if (nf, dim) == (64, 256) else None
        lines += ["  plain volume sha256 %s  %s" % (got[0], "= the parent's" if want and got[0] == want[0] else
                                                   "DIFFERS from the parent's " + want[0] if want else "(no recorded value for this size)"),
                  "  plain mesh   sha256 %s  %s" % (got[1], "= the parent's" if want and got[1] == want[1] else
                                                   "DIFFERS from the parent's " + want[1] if want else "(no recorded value for this size)"), ""]
        record["%dx%d" % (ht, wd)] = {k: list(v) for k, v in t.items() if not k.endswith("panoptic")}
        del poses, disps, images, vol, out, sout, sp, fns
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print("written to", args.out)
    if args.plain_json:
        with open(args.plain_json, "w") as f:
            json.dump(record, f)


if __name__ == "__main__":
    main()
