"""Surface reconstruction: the first measurement of pvo_tsdf_integrate and pvo_tsdf_mesh on the MI355X.

    python tools/tsdf_bench.py [--reps 30] [--frames 64] [--dim 256] [--out profiles/r16_tsdf.txt]

A synthetic video - `frames` keyframes on a line, each with a small yaw, in front of a plane with a sphere before it, the inverse depths
from the closed-form ray intersections, random images - at 48 x 64 (the 1/8 maps) and at 384 x 512 (full resolution) is fused into a
dim^3 volume with colours (20 bytes per voxel) and meshed.  Per call, between two device events on the stream, median and 10th .. 90th
percentile of `reps` repetitions after 5 warm-ups: the integration of all frames in one call, the mesh extraction (capacities given, no
synchronisation), and beside them a device-to-device copy of the volume's bytes - what reading and writing the volume once costs,
the floor of the volume stream alone.  The integration's rate is given in voxel-frame pairs per second (frames x voxels / time).  No
threshold is set: this is where the numbers are first written down.  A ratio integrate / copy far above frames / 4 would say that the
per-voxel gathers, not the volume stream, bound the kernel and that per-brick frame lists are the follow-up.
Needs the GPU: there is no fallback."""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANE_N, SPHERE_C, SPHERE_R = (0.15, 0.08, 1.0), (0.1, 0.05, 1.3), 0.35


def make_video(nf, ht, wd, device, seed=0):
    """poses [nf,7] world-to-camera, disps [nf,ht,wd], intr [4], images uint8 [nf,3,ht,wd]"""
    g = torch.Generator().manual_seed(seed)
    n = torch.tensor(PLANE_N, dtype=torch.float64)
    n = n / n.norm()
    pd = 2.0 * n[2]
    sc = torch.tensor(SPHERE_C, dtype=torch.float64)
    fx = fy = 0.8 * wd
    cx, cy = 0.5 * wd - 0.5, 0.5 * ht - 0.5
    yy, xx = torch.meshgrid(torch.arange(ht, dtype=torch.float64), torch.arange(wd, dtype=torch.float64), indexing="ij")
    dc = torch.stack([(xx - cx) / fx, (yy - cy) / fy, torch.ones_like(xx)], -1)
    poses, disps = torch.zeros(nf, 7, dtype=torch.float64), torch.zeros(nf, ht, wd, dtype=torch.float64)
    for k in range(nf):
        c = torch.tensor([1.2 * (k / max(nf - 1, 1) - 0.5), 0.0, 0.0], dtype=torch.float64)
        yaw = -0.2 * float(c[0])
        rcw = torch.tensor([[math.cos(yaw), 0, math.sin(yaw)], [0, 1, 0], [-math.sin(yaw), 0, math.cos(yaw)]], dtype=torch.float64)
        poses[k, :3] = -(rcw.T @ c)
        poses[k, 3:] = torch.tensor([0.0, math.sin(-0.5 * yaw), 0.0, math.cos(-0.5 * yaw)])
        dw = dc @ rcw.T
        s_plane = (pd - n @ c) / (dw @ n)
        oc = c - sc
        qa, qb, qc = (dw * dw).sum(-1), 2.0 * (dw @ oc), oc @ oc - SPHERE_R ** 2
        disc = qb * qb - 4 * qa * qc
        s_sphere = torch.where(disc > 0, (-qb - disc.clamp(min=0).sqrt()) / (2 * qa), torch.full_like(qa, float("inf")))
        disps[k] = 1.0 / torch.minimum(s_plane, s_sphere)
    images = torch.randint(0, 256, (nf, 3, ht, wd), generator=g).to(torch.uint8)
    intr = torch.tensor([fx, fy, cx, cy])
    return poses.float().to(device), disps.float().contiguous().to(device), intr.to(device), images.to(device)


def measure(fns, reps, warm=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in fns}
    for r in range(reps + warm):
        for name, fn in fns.items():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= warm:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: sorted(v) for k, v in times.items()}


def stats(v):
    n = len(v)
    return v[n // 2], v[n // 10], v[(9 * n) // 10]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_tsdf.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_bench needs the GPU (there is no fallback)")
    from pvo_amd import droid_backends as db
    dev = torch.device("cuda:0")
    nf, dim = args.frames, args.dim
    voxel = 2.56 / dim
    trunc, origin = 3.0 * voxel, (-1.28, -1.28, 0.5)
    lines = ["tsdf_bench on %s: %d keyframes into a %d^3 volume (voxel %.4f, trunc %.4f, tsdf + wsum + rgb = 20 bytes per voxel)"
             % (torch.cuda.get_device_name(0), nf, dim, voxel, trunc),
             "per call, device events, median [p10 .. p90] of %d repetitions after 5 warm-ups" % args.reps, ""]
    for ht, wd in ((48, 64), (384, 512)):
        poses, disps, intr, images = make_video(nf, ht, wd, dev)
        ix = torch.arange(nf, device=dev)
        vol = [torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, 3, device=dev)]
        fuse = lambda: db.tsdf_integrate(vol[0], vol[1], vol[2], poses, disps, intr, ix, origin, voxel, trunc, images=images,
                                         img_stride=1, img_offset=0)
        fuse()
        touched = int((vol[1] > 0).sum())
        pairs_fused = float(vol[1].sum())
        m = db.tsdf_mesh(vol[0], vol[1], vol[2], origin, voxel, min_weight=1.0)
        nv, nfaces = m["counts"].tolist()
        out = {k: torch.empty_like(v) for k, v in m.items()}
        copies = [torch.empty_like(t) for t in vol]
        volume_bytes = sum(t.numel() * 4 for t in vol)

        def copy():
            for dst, src in zip(copies, vol):
                dst.copy_(src)

        t = measure({"integrate": fuse, "mesh": lambda: db.tsdf_mesh_into(vol[0], vol[1], vol[2], origin, voxel, 1.0, out), "copy": copy},
                    args.reps)
        ti, tm, tc = stats(t["integrate"]), stats(t["mesh"]), stats(t["copy"])
        pairs = float(nf) * dim ** 3
        lines += ["%d x %d maps: %d of %d voxels touched, %.3g voxel-frame pairs fused of %.3g considered; mesh %d vertices, %d faces"
                  % (ht, wd, touched, dim ** 3, pairs_fused, pairs, nv, nfaces),
                  "  integrate  %10.1f us [%.1f .. %.1f]   %.3g voxel-frame pairs/s" % (ti + (pairs / (ti[0] * 1e-6),)),
                  "  mesh       %10.1f us [%.1f .. %.1f]" % tm,
                  "  copy       %10.1f us [%.1f .. %.1f]   device-to-device, %d bytes read and written: %.0f GB/s"
                  % (tc + (volume_bytes, 2.0 * volume_bytes / (tc[0] * 1e-6) / 1e9)),
                  "  integrate / copy = %.2f   (frames / 4 = %.1f)" % (ti[0] / tc[0], nf / 4.0), ""]
        del poses, disps, images, vol, copies, out, m
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print("written to", args.out)


if __name__ == "__main__":
    main()
