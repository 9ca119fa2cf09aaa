"""Rendering the fused volume: the first measurement of pvo_tsdf_render and pvo_tsdf_sparse_render on the MI355X.

    python tools/tsdf_render_bench.py [--reps 20] [--frames 64] [--dim 256] [--parent-lib PATH] [--out profiles/r19_tsdf_render.txt]

tools/tsdf_bench.py's scene - `frames` keyframes in front of a plane with a sphere before it - fused at 48 x 64 with colours and
segment ids into the dim^3 volume (voxel 2.56 / dim) and into a brick volume over the same extent, then looked at from the keyframes'
own poses at 48 x 64 and at 384 x 512 (dz = voxel / 2, z_far = the box's far corner): all four outputs, and depth alone.  Per call,
between two device events on the stream, median and 10th .. 90th percentile of `reps` repetitions after 5 warm-ups.  Beside each render:
a device-to-device copy of the volume's bytes plus the outputs' bytes (what touching every voxel and every output once costs - a render
reads only the voxels its rays meet, so it may well be below it) and pvo_tsdf_integrate of the same frames at the same resolution.  From
the `visited` output: the samples the walks examined against the samples of the clipped ranges, and for the brick volume the share of
the dense walk's samples that the jump over bricks that do not exist removed.  Then tools/tsdf_sparse_bench.py's corridor, which only
the brick volume can hold.  With --parent-lib (a libpvo_hip.so built from the parent commit): the plain pvo_tsdf_integrate and
pvo_tsdf_mesh calls through both libraries in this process, alternating, with the sha256 of everything they write - the render adds
entry points and must not move these.  No threshold is set: this is where the numbers are first written down.
Needs the GPU: there is no fallback."""
import argparse
import ctypes
import hashlib
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tsdf_bench import make_video, measure, stats  # noqa: E402
from tsdf_sparse_bench import make_corridor  # noqa: E402

SPHERE_ID, PLANE_ID = 7, 3


def label_maps(disps):
    """int32 ids per pixel: the sphere is everything nearer than 1.68 (its farthest visible point), the plane the rest"""
    return torch.where(disps > 1.0 / 1.68, SPHERE_ID, PLANE_ID).to(torch.int32).contiguous()


def outputs(n, ht, wd, dev, full, visited=False):
    out = {"depth": torch.empty(n, ht, wd, device=dev)}
    if full:
        out.update(normal=torch.empty(n, ht, wd, 3, device=dev), rgba=torch.empty(n, ht, wd, 4, dtype=torch.uint8, device=dev),
                   label=torch.empty(n, ht, wd, dtype=torch.int32, device=dev))
    if visited:
        out["visited"] = torch.empty(n, ht, wd, 2, dtype=torch.int32, device=dev)
    return out


def nbytes(ts):
    return sum(t.numel() * t.element_size() for t in ts if t is not None)


def copier(ts):
    ts = [t for t in ts if t is not None]
    dst = [torch.empty_like(t) for t in ts]

    def run():
        for d, s in zip(dst, ts):
            d.copy_(s)
    return run


def render_block(lines, reps, what, render, volume_tensors, n, ht, wd, dev, integrate):
    """time render(out) with all outputs and with depth alone, a copy of the volume's + outputs' bytes and `integrate`; returns visited sums"""
    vis = outputs(n, ht, wd, dev, True, visited=True)
    render(vis)
    hits = int((vis["depth"] > 0).sum())
    examined, clipped = int(vis["visited"][..., 0].sum()), int(vis["visited"][..., 1].sum())
    full, bare = outputs(n, ht, wd, dev, True), outputs(n, ht, wd, dev, False)
    fns = {"all": lambda: render(full), "depth": lambda: render(bare), "copy": copier(list(volume_tensors) + list(full.values()))}
    if integrate is not None:
        fns["integrate"] = integrate
    t = {k: stats(v) for k, v in measure(fns, reps).items()}
    moved = nbytes(volume_tensors) + nbytes(full.values())
    rays = n * ht * wd
    lines += ["  %s: %d of %d rays hit; %d samples examined of %d in the clipped ranges (%.1f per ray)" % (what, hits, rays, examined, clipped, examined / rays),
              "    render, depth + normal + rgba + label %10.1f us [%.1f .. %.1f]   %.3g rays/s, %.3g samples/s"
              % (t["all"] + (rays / (t["all"][0] * 1e-6), examined / (t["all"][0] * 1e-6))),
              "    render, depth alone                   %10.1f us [%.1f .. %.1f]" % t["depth"],
              "    copy of volume + outputs              %10.1f us [%.1f .. %.1f]   %d bytes read and written: %.0f GB/s;  render / copy = %.2f"
              % (t["copy"] + (moved, 2.0 * moved / (t["copy"][0] * 1e-6) / 1e9, t["all"][0] / t["copy"][0]))]
    if integrate is not None:
        lines += ["    integrate of the same frames          %10.1f us [%.1f .. %.1f]   render / integrate = %.2f"
                  % (t["integrate"] + (t["all"][0] / t["integrate"][0],))]
    return examined, clipped


def sha(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


def plain_calls(path, L, video, dim, origin, voxel, trunc, vcap, fcap):
    """pvo_tsdf_integrate and pvo_tsdf_mesh through the library at `path`, by ctypes alone: (integrate(), mesh(), the tensors they write)"""
    lib = ctypes.CDLL(path)
    for name in ("pvo_tsdf_integrate_workspace_bytes", "pvo_tsdf_mesh_workspace_bytes", "pvo_tsdf_integrate", "pvo_tsdf_mesh"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    poses, disps, intr, images = video
    dev = poses.device
    nf, ht, wd = disps.shape
    ix = torch.arange(nf, device=dev)
    vol = [torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, 3, device=dev)]
    mesh = {"verts": torch.zeros(vcap, 3, device=dev), "normals": torch.zeros(vcap, 3, device=dev), "rgba": torch.zeros(vcap, 4, dtype=torch.uint8, device=dev),
            "faces": torch.zeros(fcap, 3, dtype=torch.int32, device=dev), "counts": torch.zeros(2, dtype=torch.int32, device=dev)}
    ws = torch.empty(max(lib.pvo_tsdf_integrate_workspace_bytes(nf), lib.pvo_tsdf_mesh_workspace_bytes(dim, dim, dim), 256), dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    a = L.TsdfIntegrateArgs()
    a.tsdf, a.wsum, a.rgb, a.nz, a.ny, a.nx = p(vol[0]), p(vol[1]), p(vol[2]), dim, dim, dim
    a.origin[0], a.origin[1], a.origin[2] = origin
    a.voxel, a.trunc, a.z_near, a.w_max = voxel, trunc, 0.0, 0.0
    a.poses, a.disps, a.intrinsics, a.ix, a.N, a.nframes, a.ht, a.wd = p(poses), p(disps), p(intr), p(ix), nf, nf, ht, wd
    a.images, a.IH, a.IW, a.img_stride, a.img_offset = p(images), ht, wd, 1, 0
    m = L.TsdfMeshArgs()
    m.tsdf, m.wsum, m.rgb, m.nz, m.ny, m.nx = p(vol[0]), p(vol[1]), p(vol[2]), dim, dim, dim
    m.origin[0], m.origin[1], m.origin[2] = origin
    m.voxel, m.min_weight, m.vcap, m.fcap = voxel, 1.0, vcap, fcap
    m.verts, m.normals, m.rgba, m.faces, m.counts = p(mesh["verts"]), p(mesh["normals"]), p(mesh["rgba"]), p(mesh["faces"]), p(mesh["counts"])
    keep = (ix, ws, a, m)

    def call(fn, args):
        s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if fn(ctypes.byref(args), p(ws), ws.numel(), s) != 0:
            raise RuntimeError("plain call failed in " + path)

    def integrate():
        for t in vol:                                      # (a fresh volume every time: the same work and the same bytes)
            t.zero_()
        call(lib.pvo_tsdf_integrate, a)
    return integrate, lambda: call(lib.pvo_tsdf_mesh, m), vol, mesh, keep


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--corridor", type=float, default=336.0, help="length of the corridor scene in metres")
    ap.add_argument("--parent-lib", default=None, help="a libpvo_hip.so built from the parent commit: the plain calls side by side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_tsdf_render.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_render_bench needs the GPU (there is no fallback)")
    from pvo_amd import _lib as L
    from pvo_amd import droid_backends as db
    from pvo_amd.tsdf_sparse import SparseTSDF
    dev = torch.device("cuda:0")
    nf, dim = args.frames, args.dim
    voxel = 2.56 / dim
    trunc, origin = 3.0 * voxel, (-1.28, -1.28, 0.5)
    g = -(-dim // 8)
    lines = ["tsdf_render_bench on %s: %d keyframes, the %d^3 extent (voxel %.4f, trunc %.4f), fused at 48 x 64 with colours and ids; rays sampled "
             "every dz = voxel / 2" % (torch.cuda.get_device_name(0), nf, dim, voxel, trunc),
             "per call, device events, median [p10 .. p90] of %d repetitions after 5 warm-ups" % args.reps, ""]
    # the volumes, fused once from the 48 x 64 maps
    poses, disps, intr, images = make_video(nf, 48, 64, dev)
    ix = torch.arange(nf, device=dev)
    labels = label_maps(disps)
    vol = {"tsdf": torch.zeros(dim, dim, dim, device=dev), "wsum": torch.zeros(dim, dim, dim, device=dev), "rgb": torch.zeros(dim, dim, dim, 3, device=dev),
           "label": torch.zeros(dim, dim, dim, dtype=torch.int32, device=dev), "lconf": torch.zeros(dim, dim, dim, device=dev)}
    db.tsdf_integrate(vol["tsdf"], vol["wsum"], vol["rgb"], poses, disps, intr, ix, origin, voxel, trunc, images=images, img_stride=1, img_offset=0,
                      label=vol["label"], lconf=vol["lconf"], labels=labels)
    bricks = SparseTSDF(origin, (g, g, g), voxel, trunc, colours=True, device=dev, cap=4096, labels=True)
    want = bricks.allocate(poses, disps, intr, ix, margin=2.0)
    bricks.integrate(poses, disps, intr, ix, images=images, img_stride=1, img_offset=0, labels=labels)
    z_far = db._render_range("bench", (dim, dim, dim), origin, voxel, poses, ix, None, 0.0, None)[2]
    lines += ["dense volume: %d of %d voxels touched, tsdf + wsum + rgb + label = %.1f MB;  brick volume: %d bricks of %d (%.1f %%), %.1f MB in use"
              % (int((vol["wsum"] > 0).sum()), dim ** 3, dim ** 3 * 24 / 1e6, want, g ** 3, 100.0 * want / g ** 3, want * 512 * 24 / 1e6),
              "z_far = %.3f: at most %d samples per ray before the clip" % (z_far, int(z_far / (0.5 * voxel))), ""]
    dense_t = (vol["tsdf"], vol["wsum"], vol["rgb"], vol["label"])
    pool_t = tuple(t[:want] for t in (bricks.tsdf, bricks.wsum, bricks.rgb, bricks.label)) + (bricks.grid,)
    for ht, wd in ((48, 64), (384, 512)):
        vposes, vdisps, vintr, vimages = make_video(nf, ht, wd, dev)
        scratch = [torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, 3, device=dev)]
        fuse = lambda: db.tsdf_integrate(scratch[0], scratch[1], scratch[2], vposes, vdisps, vintr, ix, origin, voxel, trunc, images=vimages,
                                         img_stride=1, img_offset=0)
        lines += ["%d views of %d x %d" % (nf, ht, wd)]
        ed, _ = render_block(lines, args.reps, "dense", lambda o: db.tsdf_render(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, vposes, vintr, ix, ht, wd,
                                                                                   z_far=z_far, label=vol["label"], out=o),
                             dense_t, nf, ht, wd, dev, fuse)
        es, _ = render_block(lines, args.reps, "bricks", lambda o: bricks.render(vposes, vintr, ix, ht, wd, z_far=z_far, out=o), pool_t, nf, ht, wd, dev, None)
        lines += ["  the jump over bricks that do not exist removed %.1f %% of the samples the dense walk examined" % (100.0 * (1.0 - es / max(ed, 1))), ""]
        del scratch, vdisps, vimages
    # the corridor: only the brick volume can hold it
    step = 3.0
    cf = int(math.ceil(args.corridor / step))
    gz = -(-int(math.ceil((cf * step + 4.0) / voxel)) // 8)
    cposes, cdisps, cintr, cimages = make_corridor(cf, 48, 64, step, dev)
    cix = torch.arange(cf, device=dev)
    cor = SparseTSDF((-1.28, -1.28, -0.5), (gz, g, g), voxel, trunc, colours=True, device=dev, cap=65536, labels=True)
    cwant = cor.allocate(cposes, cdisps, cintr, cix, margin=2.0)
    cor.integrate(cposes, cdisps, cintr, cix, images=cimages, img_stride=1, img_offset=0, labels=label_maps(cdisps))
    lines += ["corridor: %d keyframes %.0f m apart in a world of %d x %d x %d voxels, %d bricks; 48 x 64 views, z_far = 4.5 (the maps reach 4 m)"
              % (cf, step, 8 * g, 8 * g, 8 * gz, cwant)]
    cpool = tuple(t[:cwant] for t in (cor.tsdf, cor.wsum, cor.rgb, cor.label)) + (cor.grid,)
    render_block(lines, args.reps, "bricks", lambda o: cor.render(cposes, cintr, cix, 48, 64, z_far=4.5, out=o), cpool, cf, 48, 64, dev, None)
    lines += [""]
    # the plain calls, this build beside the parent's
    if args.parent_lib:
        video = (poses, disps, intr, images)
        m0 = db.tsdf_mesh(vol["tsdf"], vol["wsum"], vol["rgb"], origin, voxel, min_weight=1.0)
        vcap, fcap = m0["verts"].shape[0] + 16, m0["faces"].shape[0] + 16
        runs = {"this": plain_calls(L.LIB_PATH, L, video, dim, origin, voxel, trunc, vcap, fcap),
                "parent": plain_calls(args.parent_lib, L, video, dim, origin, voxel, trunc, vcap, fcap)}
        fns = {}
        for k, r in runs.items():                              # (alternating: measure() walks the dict once per repetition)
            fns[k + " integrate"], fns[k + " mesh"] = r[0], r[1]
        t = {k: stats(v) for k, v in measure(fns, args.reps).items()}
        lines += ["the plain calls (48 x 64 maps into the %d^3 volume; mesh of it), this build and the parent commit's in one process, alternating" % dim]
        digests = {}
        for k, r in runs.items():
            digests[k] = (sha(*r[2]), sha(*[r[3][n] for n in ("verts", "normals", "rgba", "faces", "counts")]))
            lines += ["  %-6s integrate %10.1f us [%.1f .. %.1f]  sha256 %s   mesh %10.1f us [%.1f .. %.1f]  sha256 %s"
                      % ((k,) + t[k + " integrate"] + (digests[k][0],) + t[k + " mesh"] + (digests[k][1],))]
        lines += ["  outputs %s" % ("EQUAL" if digests["this"] == digests["parent"] else "DIFFER"), ""]
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
