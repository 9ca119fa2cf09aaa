"""Sparse surface reconstruction: the first measurement of the brick volume (pvo_tsdf_sparse_allocate / _integrate / _mesh) beside the
dense volume (pvo_tsdf_integrate / pvo_tsdf_mesh) on the MI355X.

    python tools/tsdf_sparse_bench.py [--reps 30] [--frames 64] [--dim 256] [--out profiles/r17_tsdf_sparse.txt]

tools/tsdf_bench.py's own scene - `frames` keyframes in front of a plane with a sphere before it, at 48 x 64 and at 384 x 512, fused
with colours into the dim^3 extent (voxel 2.56 / dim) and meshed - once into the dense volume and once into a brick volume over the
same extent (margin 2).  Per call, between two device events on the stream, median and 10th .. 90th percentile of `reps` repetitions
after 5 warm-ups, every call on the volume the first pass filled (so allocate finds its bricks held; its marking, counting and scan
are the same work).  Reported: the bricks allocated, the bytes held, and the share of (brick, frame) pairs the cull removes (from the
integrate call's `kept` output).  Then a scene the dense path cannot hold at all: a corridor of 2.56 x 2.56 m cross-section followed
for --corridor metres at the same voxel (its dense volume would have more than 2^31 voxels), 48 x 64 maps, depths beyond 4 m unused.
No threshold is set: this is where the numbers are first written down.  Needs the GPU: there is no fallback."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tsdf_bench import make_video, measure, stats  # noqa: E402


def make_corridor(nf, ht, wd, step, device, half=1.2, reach=4.0, seed=0):
    """cameras on the corridor's axis at z = k * step looking along +z; walls at x = +-half, y = +-half; pixels whose wall point is
    deeper than `reach` carry no depth (disparity 0)"""
    g = torch.Generator().manual_seed(seed)
    fx = fy = 0.8 * wd
    cx, cy = 0.5 * wd - 0.5, 0.5 * ht - 0.5
    yy, xx = torch.meshgrid(torch.arange(ht, dtype=torch.float64), torch.arange(wd, dtype=torch.float64), indexing="ij")
    rx, ry = (xx - cx) / fx, (yy - cy) / fy
    depth = torch.minimum(half / rx.abs().clamp(min=1e-9), half / ry.abs().clamp(min=1e-9))
    disp = torch.where(depth <= reach, 1.0 / depth, torch.zeros_like(depth))
    poses = torch.zeros(nf, 7, dtype=torch.float64)
    poses[:, 6] = 1.0
    poses[:, 2] = -step * torch.arange(nf, dtype=torch.float64)          # world-to-camera: t = -c
    images = torch.randint(0, 256, (nf, 3, ht, wd), generator=g).to(torch.uint8)
    return (poses.float().to(device), disp.float()[None].repeat(nf, 1, 1).contiguous().to(device), torch.tensor([fx, fy, cx, cy]).to(device),
            images.to(device))


def sparse_run(db, SparseTSDF, lines, reps, origin, gdims, voxel, trunc, video, cap):
    poses, disps, intr, images = video
    nf = poses.shape[0]
    dev = poses.device
    ix = torch.arange(nf, device=dev)
    vol = SparseTSDF(origin, gdims, voxel, trunc, colours=True, device=dev, cap=cap)
    want = vol.allocate(poses, disps, intr, ix, margin=2.0)
    kept = torch.zeros(vol.cap, dtype=torch.int32, device=dev)
    fuse = lambda: vol.integrate(poses, disps, intr, ix, images=images, img_stride=1, img_offset=0, kept=kept)
    fuse()
    survivors = int(kept[:want].sum())
    m = vol.mesh(min_weight=1.0)
    nv, nfaces = m["counts"].tolist()
    out = {k: torch.empty_like(v) for k, v in m.items()}
    t = measure({"allocate": lambda: db.tsdf_sparse_allocate(vol.volume(), poses, disps, intr, ix, trunc, margin=2.0), "integrate": fuse,
                 "mesh": lambda: db.tsdf_sparse_mesh_into(vol.volume(), 1.0, out)}, reps)
    ta, ti, tm = stats(t["allocate"]), stats(t["integrate"]), stats(t["mesh"])
    pool_bytes = want * 512 * 20 + want * 12
    grid_bytes = vol.grid.numel() * 4
    lines += ["  sparse: %d bricks of %d allocated (%.1f %% of the voxels), %d of their voxels touched; pool %.1f MB in use (%.1f MB reserved, "
              "cap %d) + grid %.1f MB; mesh %d vertices, %d faces"
              % (want, vol.grid.numel(), 100.0 * want / max(vol.grid.numel(), 1), int((vol.wsum[:want] > 0).sum()), pool_bytes / 1e6,
                 (vol.nbytes() - grid_bytes) / 1e6, vol.cap, grid_bytes / 1e6, nv, nfaces),
              "  cull: %d of %d (brick, frame) pairs survive: %.1f %% removed" % (survivors, want * nf, 100.0 * (1.0 - survivors / max(want * nf, 1))),
              "  sparse allocate  %10.1f us [%.1f .. %.1f]" % ta,
              "  sparse integrate %10.1f us [%.1f .. %.1f]" % ti,
              "  sparse mesh      %10.1f us [%.1f .. %.1f]" % tm,
              "  sparse total     %10.1f us" % (ta[0] + ti[0] + tm[0])]
    return ta[0] + ti[0] + tm[0], ti[0], tm[0]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--corridor", type=float, default=336.0, help="length of the corridor scene in metres")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_tsdf_sparse.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_sparse_bench needs the GPU (there is no fallback)")
    from pvo_amd import droid_backends as db
    from pvo_amd.tsdf_sparse import SparseTSDF
    dev = torch.device("cuda:0")
    nf, dim = args.frames, args.dim
    voxel = 2.56 / dim
    trunc, origin = 3.0 * voxel, (-1.28, -1.28, 0.5)
    g = -(-dim // 8)
    lines = ["tsdf_sparse_bench on %s: %d keyframes, the %d^3 extent (voxel %.4f, trunc %.4f, margin 2), tsdf + wsum + rgb = 20 bytes per voxel"
             % (torch.cuda.get_device_name(0), nf, dim, voxel, trunc),
             "per call, device events, median [p10 .. p90] of %d repetitions after 5 warm-ups" % args.reps, ""]
    for ht, wd in ((48, 64), (384, 512)):
        video = make_video(nf, ht, wd, dev)
        poses, disps, intr, images = video
        ix = torch.arange(nf, device=dev)
        vol = [torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, 3, device=dev)]
        fuse = lambda: db.tsdf_integrate(vol[0], vol[1], vol[2], poses, disps, intr, ix, origin, voxel, trunc, images=images,
                                         img_stride=1, img_offset=0)
        fuse()
        m = db.tsdf_mesh(vol[0], vol[1], vol[2], origin, voxel, min_weight=1.0)
        nv, nfaces = m["counts"].tolist()
        out = {k: torch.empty_like(v) for k, v in m.items()}
        t = measure({"integrate": fuse, "mesh": lambda: db.tsdf_mesh_into(vol[0], vol[1], vol[2], origin, voxel, 1.0, out)}, args.reps)
        ti, tm = stats(t["integrate"]), stats(t["mesh"])
        lines += ["%d x %d maps" % (ht, wd),
                  "  dense: %d of %d voxels touched, volume %.1f MB; mesh %d vertices, %d faces"
                  % (int((vol[1] > 0).sum()), dim ** 3, dim ** 3 * 20 / 1e6, nv, nfaces),
                  "  dense integrate  %10.1f us [%.1f .. %.1f]" % ti,
                  "  dense mesh       %10.1f us [%.1f .. %.1f]" % tm,
                  "  dense total      %10.1f us" % (ti[0] + tm[0])]
        del vol, out, m
        total, si, sm = sparse_run(db, SparseTSDF, lines, args.reps, origin, (g, g, g), voxel, trunc, video, cap=4096)
        lines += ["  dense / sparse: integrate %.2f, mesh %.2f, integrate + mesh against allocate + integrate + mesh %.2f"
                  % (ti[0] / si, tm[0] / sm, (ti[0] + tm[0]) / total), ""]
        del video, poses, disps, images
    # the scene the dense volume cannot hold
    step = 3.0
    cf = int(math.ceil(args.corridor / step))
    gz = -(-int(math.ceil((cf * step + 4.0) / voxel)) // 8)
    voxels = (8 * g) * (8 * g) * (8 * gz)
    lines += ["corridor: %d keyframes %.0f m apart, 48 x 64 maps, a world of %d x %d x %d voxels = %.3g (dense limit 2^31 = %.3g: %s; it would take %.1f GB)"
              % (cf, step, 8 * g, 8 * g, 8 * gz, voxels, 2.0 ** 31, "cannot be held" if voxels >= 2 ** 31 else "could be held", voxels * 20 / 1e9)]
    sparse_run(db, SparseTSDF, lines, args.reps, (-1.28, -1.28, -0.5), (gz, g, g), voxel, trunc, make_corridor(cf, 48, 64, step, dev), cap=65536)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print("written to", args.out)


if __name__ == "__main__":
    main()
