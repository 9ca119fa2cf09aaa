"""Frame-to-model tracking: the first measurement of pvo_tsdf_track and pvo_tsdf_sparse_track on the MI355X.

    python tools/tsdf_track_bench.py [--reps 20] [--frames 64] [--dim 256] [--parent-lib PATH] [--out profiles/r25_tsdf_track.txt]

tools/tsdf_bench.py's scene - `frames` keyframes in front of a plane with a sphere before it - fused at 48 x 64 into the dim^3 volume
(voxel 2.56 / dim) and into a brick volume over the same extent; then every keyframe tracked against it from its own pose, one slot per
keyframe, with depth maps of 48 x 64 and of 384 x 512.  Per call, between two device events on the stream, median and 10th .. 90th
percentile of `reps` repetitions after 5 warm-ups: one evaluation (iters = 0: view constants, accumulate, solve), a 10-iteration call,
and beside them the depth-only render of the same views and a device-to-device copy of the frames' disps bytes (what reading every
pixel once costs).  (The scene is the timing scene: with one sphere it is rank-deficient for tracking - tests/tsdf_track_reference.py -
which changes no launch.)  With --parent-lib (a libpvo_hip.so built from the parent commit): the plain pvo_tsdf_integrate,
pvo_tsdf_mesh and pvo_tsdf_render calls through both libraries in this process, alternating, with the sha256 of everything they write -
the tracker adds entry points and moves the volume adapters into a header, and must not move these.  No threshold is set: this is
where the numbers are first written down.
Needs the GPU: there is no fallback."""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tsdf_bench import make_video, measure, stats  # noqa: E402
from tsdf_render_bench import copier, plain_calls, sha  # noqa: E402


def plain_render(path, L, vol, origin, voxel, poses, intr, ht, wd, z_far):
    """the depth-only pvo_tsdf_render through the library at `path`, by ctypes alone: (render(), the tensor it writes)"""
    lib = ctypes.CDLL(path)
    for name in ("pvo_tsdf_render_workspace_bytes", "pvo_tsdf_render"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    dev, n = poses.device, poses.shape[0]
    ix = torch.arange(n, device=dev)
    depth = torch.zeros(n, ht, wd, device=dev)
    ws = torch.empty(max(lib.pvo_tsdf_render_workspace_bytes(n), 256), dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    a = L.TsdfRenderArgs()
    a.tsdf, a.wsum = p(vol[0]), p(vol[1])
    a.nz, a.ny, a.nx = vol[0].shape
    a.origin[0], a.origin[1], a.origin[2] = origin
    a.voxel, a.min_weight = voxel, 1.0
    a.poses, a.intrinsics, a.ix, a.N, a.nviews, a.ht, a.wd = p(poses), p(intr), p(ix), n, n, ht, wd
    a.z_near, a.z_far, a.dz = 0.0, z_far, 0.5 * voxel
    a.depth = p(depth)
    keep = (ix, ws, a)

    def render():
        s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if lib.pvo_tsdf_render(ctypes.byref(a), p(ws), ws.numel(), s) != 0:
            raise RuntimeError("plain render failed in " + path)
    return render, depth, keep


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--parent-lib", default=None, help="a libpvo_hip.so built from the parent commit: the plain calls side by side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_tsdf_track.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_track_bench needs the GPU (there is no fallback)")
    from pvo_amd import _lib as L
    from pvo_amd import droid_backends as db
    from pvo_amd.tsdf_sparse import SparseTSDF
    dev = torch.device("cuda:0")
    nf, dim = args.frames, args.dim
    voxel = 2.56 / dim
    trunc, origin = 3.0 * voxel, (-1.28, -1.28, 0.5)
    g = -(-dim // 8)
    lines = ["tsdf_track_bench on %s: %d keyframes, the %d^3 extent (voxel %.4f, trunc %.4f), fused at 48 x 64; one slot per keyframe, from its own pose"
             % (torch.cuda.get_device_name(0), nf, dim, voxel, trunc),
             "per call, device events, median [p10 .. p90] of %d repetitions after 5 warm-ups" % args.reps, ""]
    poses, disps, intr, images = make_video(nf, 48, 64, dev)
    ix = torch.arange(nf, device=dev)
    tsdf, wsum = torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, device=dev)
    db.tsdf_integrate(tsdf, wsum, None, poses, disps, intr, ix, origin, voxel, trunc)
    bricks = SparseTSDF(origin, (g, g, g), voxel, trunc, colours=False, device=dev, cap=4096)
    want = bricks.allocate(poses, disps, intr, ix, margin=2.0)
    bricks.integrate(poses, disps, intr, ix)
    z_far = db._render_range("bench", (dim, dim, dim), origin, voxel, poses, ix, None, 0.0, None)[2]
    lines += ["dense volume: tsdf + wsum = %.1f MB;  brick volume: %d bricks of %d, %.1f MB in use" % (dim ** 3 * 8 / 1e6, want, g ** 3, want * 512 * 8 / 1e6), ""]
    for ht, wd in ((48, 64), (384, 512)):
        vposes, vdisps, vintr, _ = make_video(nf, ht, wd, dev)
        lines += ["%d slots of %d x %d" % (nf, ht, wd)]
        for what, track, render in (
                ("dense", lambda o, it: db.tsdf_track(tsdf, wsum, origin, voxel, vposes, vdisps, vintr, ix, iters=it, out=o),
                 lambda o: db.tsdf_render(tsdf, wsum, None, origin, voxel, vposes, vintr, ix, ht, wd, z_far=z_far, normals=False, out=o)),
                ("bricks", lambda o, it: bricks.track(vposes, vdisps, vintr, ix, iters=it, out=o),
                 lambda o: bricks.render(vposes, vintr, ix, ht, wd, z_far=z_far, normals=False, out=o))):
            outs = {it: {"poses": torch.empty(nf, 7, device=dev), "info": torch.empty(nf, it + 1, 4, device=dev)} for it in (0, 10)}
            depth = {"depth": torch.empty(nf, ht, wd, device=dev)}
            fns = {"eval": lambda: track(outs[0], 0), "ten": lambda: track(outs[10], 10), "render": lambda: render(depth), "copy": copier([vdisps])}
            t = {k: stats(v) for k, v in measure(fns, args.reps).items()}
            info = outs[10]["info"]
            px = nf * ht * wd
            lines += ["  %s: %d of %d pixels contribute at the start; status of the last evaluation: %s"
                      % (what, int(outs[0]["info"][:, 0, 1].sum()), px, sorted(set(info[:, -1, 3].int().tolist()))),
                      "    one evaluation (3 launches)           %10.1f us [%.1f .. %.1f]   %.3g pixels/s" % (t["eval"] + (px / (t["eval"][0] * 1e-6),)),
                      "    10 iterations (23 launches)           %10.1f us [%.1f .. %.1f]   %.1f us per evaluation" % (t["ten"] + (t["ten"][0] / 11.0,)),
                      "    render of the same views, depth alone %10.1f us [%.1f .. %.1f]   render / evaluation = %.1f" % (t["render"] + (t["render"][0] / t["eval"][0],)),
                      "    copy of the frames' disps             %10.1f us [%.1f .. %.1f]   %d bytes: evaluation / copy = %.2f"
                      % (t["copy"] + (4 * px, t["eval"][0] / t["copy"][0]))]
        lines += [""]
        del vdisps
    if args.parent_lib:
        video = (poses, disps, intr, images)
        rgb = torch.zeros(dim, dim, dim, 3, device=dev)
        t2, w2 = torch.zeros_like(tsdf), torch.zeros_like(wsum)
        db.tsdf_integrate(t2, w2, rgb, poses, disps, intr, ix, origin, voxel, trunc, images=images, img_stride=1, img_offset=0)
        m0 = db.tsdf_mesh(t2, w2, rgb, origin, voxel, min_weight=1.0)
        vcap, fcap = m0["verts"].shape[0] + 16, m0["faces"].shape[0] + 16
        del t2, w2, rgb, m0
        runs, renders = {}, {}
        for k, path in (("this", L.LIB_PATH), ("parent", args.parent_lib)):
            runs[k] = plain_calls(path, L, video, dim, origin, voxel, trunc, vcap, fcap)
            renders[k] = plain_render(path, L, (tsdf, wsum), origin, voxel, poses, intr, 48, 64, z_far)
        fns = {}
        for k in runs:                                          # (alternating: measure() walks the dict once per repetition)
            fns[k + " integrate"], fns[k + " mesh"], fns[k + " render"] = runs[k][0], runs[k][1], renders[k][0]
        raw = measure(fns, args.reps)
        t = {k: stats(v) for k, v in raw.items()}
        lines += ["the plain calls (48 x 64 maps into the %d^3 volume; mesh of it; depth render of it), this build and the parent commit's in one "
                  "process, alternating" % dim]
        digests, inside = {}, True
        for k, r in runs.items():
            digests[k] = (sha(*r[2]), sha(*[r[3][n] for n in ("verts", "normals", "rgba", "faces", "counts")]), sha(renders[k][1]))
            lines += ["  %-6s integrate %9.1f us [%.1f .. %.1f] sha256 %s   mesh %8.1f us [%.1f .. %.1f] sha256 %s   render %8.1f us [%.1f .. %.1f] sha256 %s"
                      % ((k,) + t[k + " integrate"] + (digests[k][0],) + t[k + " mesh"] + (digests[k][1],) + t[k + " render"] + (digests[k][2],))]
        for call in ("integrate", "mesh", "render"):
            a, b = t["this " + call], t["parent " + call]
            inside = inside and b[1] <= a[0] <= b[2] and a[1] <= b[0] <= a[2]
        lines += ["  outputs %s; every median inside the other build's p10 .. p90: %s" % ("EQUAL" if digests["this"] == digests["parent"] else "DIFFER", inside), ""]
        if digests["this"] != digests["parent"]:
            print("\n".join(lines))
            raise SystemExit("the plain calls' outputs differ from the parent's")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print("written to", args.out)


if __name__ == "__main__":
    main()
