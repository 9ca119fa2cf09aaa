"""Map export: the native call (pvo_map_points) against the composition of the entry points that existed before it - the
reference viewer's formulation (visualization.py:92-107,127-129):

    points = db.iproj(SE3(poses[ix]).inv().data, disps[ix], intrinsics)      count = db.depth_filter(poses, disps, intrinsics, ix, thresh)
    masks  = (count >= 2) & (disps[ix] > .5 * disps[ix].mean(dim=[1,2], keepdim=True))
    pts, clr = points[masks], colours[masks]                                 (two boolean-index gathers; each reads its size back)

    python tools/map_points_bench.py [--reps 30] [--out profiles/r12_map_points.json]

Method: both forms live in ONE process, on the same seeded video (constant-twist poses, a smooth inverse-depth field under 2 %
noise, random images), N = 64 keyframes, at 30 x 101 (the 1/8 maps) and at 240 x 808 (full resolution), and are measured
ALTERNATELY, repetition by repetition, between two device events on the stream after a warm-up; the figure is microseconds per
call, median and 10th .. 90th percentile.  The composition stays on the device (the reference moves everything to the host first; that
copy is not charged to it).  The native call is timed in both of its forms: capacity=None (reads the total back once) and with a
given capacity (no synchronisation).  Before anything is timed the two forms are compared: the same pixels in the same order, points
within 1e-5.  The shader clock (pvo_clock_probe) is noted idle and right after each timed block.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_video(nf, ht, wd, device, seed=0):
    from pvo_amd.geom.se3 import SE3
    g = torch.Generator().manual_seed(seed)
    intr = torch.tensor([wd * 0.625, wd * 0.625, wd / 2.0, ht / 2.0])
    xi = torch.tensor([0.05, 0.0, 0.02, 0.0, 0.01, 0.0])
    poses = torch.stack([SE3.exp(k * xi).data for k in range(nf)], 0).float()
    low = torch.rand(1, 1, 6, 8, generator=g) * 0.8 + 0.2
    field = torch.nn.functional.interpolate(low, size=(ht, wd), mode="bilinear", align_corners=True)[0, 0]
    disps = field[None] * (1.0 + 0.02 * torch.randn(nf, ht, wd, generator=g))
    images = torch.randint(0, 256, (nf, 3, ht, wd), generator=g).to(torch.uint8)
    return poses.to(device), disps.float().contiguous().to(device), intr.to(device), images.to(device)


def composition(db, poses, disps, intr, images, ix, thresh):
    """the reference's lines on the device; colours at the map's own resolution (stride 1, offset 0)"""
    from pvo_amd.geom.se3 import SE3
    p, d = poses.index_select(0, ix), disps.index_select(0, ix)
    points = db.iproj(SE3(p).inv().data.contiguous(), d, intr)
    count = db.depth_filter(poses, disps, intr, ix, thresh)
    masks = (count >= 2) & (d > 0.5 * d.mean(dim=[1, 2], keepdim=True))
    clr = images.index_select(0, ix)[:, [2, 1, 0]].permute(0, 2, 3, 1)
    return points[masks], clr[masks], masks


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
    return {"median_us": v[n // 2], "p10_us": v[n // 10], "p90_us": v[(9 * n) // 10], "reps": n}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--thresh", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_map_points.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("map_points_bench needs the GPU (there is no fallback)")
    from pvo_amd import droid_backends as db
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)

    def clock():
        t = db.clock_probe(side, iters=4000)
        torch.cuda.synchronize()
        return db.clock_ghz(t)

    result = {"device": torch.cuda.get_device_name(0), "frames": args.frames, "thresh": args.thresh, "shader_clock_ghz_idle": clock(),
              "method": "alternating repetitions in one process, device events, medians after warm-up (see the module docstring)",
              "rows": {}}
    for ht, wd in ((30, 101), (240, 808)):
        nf = args.frames
        poses, disps, intr, images = make_video(nf, ht, wd, dev)
        ix = torch.arange(nf, device=dev)
        th = torch.full((nf,), args.thresh, device=dev)
        kw = dict(images=images, img_stride=1, img_offset=0)
        pts, clr, masks = composition(db, poses, disps, intr, images, ix, th)
        got = db.map_points(poses, disps, intr, ix, th, **kw)
        total = int(got["frame_start"][-1])
        # the same pixels (the composition's fp32 mean against the kernel's fp64 one may move a pixel that sits within a rounding of
        # half the mean: counted, and at most one in a million admitted), the same colours, points within 1e-5 where both keep
        HW, src = ht * wd, got["src"].long()
        key_n, key_c = src[:, 0] * HW + src[:, 1], masks.reshape(-1).nonzero()[:, 0]
        keep_n = torch.zeros(nf * HW, dtype=torch.bool, device=dev)
        keep_n[key_n] = True
        mismatches = int((keep_n != masks.reshape(-1)).sum())
        both = keep_n & masks.reshape(-1)
        dense_n, dense_c = torch.zeros(nf * HW, 4, device=dev), torch.zeros(nf * HW, 4, device=dev)
        dense_n[key_n, :3], dense_n[key_n, 3] = got["xyz"], got["rgba"][:, :3].float().sum(1)
        dense_c[key_c, :3], dense_c[key_c, 3] = pts, clr.float().sum(1)
        ordered = bool((key_n[1:] > key_n[:-1]).all())
        if mismatches > 1e-6 * nf * HW or not ordered or not torch.allclose(dense_n[both], dense_c[both], rtol=1e-5, atol=1e-5):
            raise SystemExit("%dx%d: the native call and the composition disagree (%d pixels selected differently)" % (ht, wd, mismatches))
        del dense_n, dense_c, keep_n, both
        cap = total + 1024
        fns = {"composition": lambda: composition(db, poses, disps, intr, images, ix, th),
               "native_capacity_none": lambda: db.map_points(poses, disps, intr, ix, th, **kw),
               "native_capacity_given": lambda: db.map_points(poses, disps, intr, ix, th, capacity=cap, **kw)}
        t = measure(fns, args.reps)
        row = {k: stats(v) for k, v in t.items()}
        row.update(points=total, selection_mismatches=mismatches, candidates=nf * ht * wd, kept_fraction=total / float(nf * ht * wd), shader_clock_ghz_after=clock(),
                   composition_over_native_capacity_none=row["composition"]["median_us"] / row["native_capacity_none"]["median_us"],
                   composition_over_native_capacity_given=row["composition"]["median_us"] / row["native_capacity_given"]["median_us"],
                   workspace_bytes=int(db._lib.load().pvo_map_points_workspace_bytes(nf, ht, wd)),
                   composition_intermediate_bytes=nf * ht * wd * (12 + 4))
        result["rows"]["%dx%d" % (ht, wd)] = row
        print("%4d x %4d: %d of %d pixels kept; composition %.1f us, native %.1f us (capacity=None) / %.1f us (capacity given): %.2fx / %.2fx"
              % (ht, wd, total, nf * ht * wd, row["composition"]["median_us"], row["native_capacity_none"]["median_us"],
                 row["native_capacity_given"]["median_us"], row["composition_over_native_capacity_none"],
                 row["composition_over_native_capacity_given"]))
        del poses, disps, images, pts, clr, masks, got
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written to", args.out)


if __name__ == "__main__":
    main()
