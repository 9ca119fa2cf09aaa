"""What the sensor-depth prior costs inside the native update: the bundle-adjustment stage (the PVO_STAGE_BA probe: HIP events around
the BA of pvo_graph_update) with and without a sensor map on the video.

    python tools/rgbd_ba_bench.py [--reps 40] [--out profiles/r10_rgbd_ba.txt]

Two windows from bench.make_window: S-B (8 keyframes of 48 x 64: the depth phase fused into the Schur kernel) and the frontend window
(26 keyframes of 30 x 101: ba_depth_kernel in front of a dense window's Schur kernel).  Both forms live in ONE process and are measured
ALTERNATELY, update by update (other work shares the machine); the state is restored before every update, so each one solves the same
problem.  The map covers 70 % of the pixels.  The term is two loads and three flops per (pixel, depth frame) beside the ~8 rows per
out-edge the depth phase reads anyway: the expectation is "within noise", the figure is the record.  Needs the GPU."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v):
    v = sorted(v)
    n = len(v)
    return v[n // 2], v[n // 10], v[(9 * n) // 10]


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_rgbd_ba.txt"))
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("rgbd_ba_bench: needs the GPU")
    import bench
    from pvo_amd import droid_backends as db
    from test_chained_updates import structured_operator
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("BA stage of the native update (PVO_STAGE_BA probe) with and without a sensor map; %s; %d updates each, alternating; "
        "microseconds per update, median (p10 .. p90)" % (torch.cuda.get_device_name(0), args.reps))
    for label, kw in (("S-B     8 keyframes  48x64 ", {}),
                      ("window  26 keyframes 30x101", dict(H8=30, W8=101, NKF=26, buffer=32, intr=(60.0, 60.0, 50.5, 15.0)))):
        worlds = {}
        for name in ("plain", "sensor"):
            video, graph = bench.make_window(dev, seed=3, **kw)
            structured_operator(graph.update_op, 0.1)
            if name == "sensor":
                g = torch.Generator().manual_seed(9)
                sens = video.ensure_disps_sens()
                sens[:] = torch.where(torch.rand(sens.shape, generator=g) < 0.7, torch.tensor(1.3), torch.tensor(0.0)).to(dev)
                video.has_sensor_depth = True
            graph.update(None, None, use_inactive=True)            # plans, allocates, warms up
            state = (video.poses.clone(), video.disps.clone(), graph.net.clone(), graph.target_cam.clone(), graph.weight.clone(),
                     graph.raw_mask.clone(), graph.delta_dy.clone(), graph.damping.clone())
            worlds[name] = (video, graph, state, [])
        for r in range(args.reps + 5):
            for name, (video, graph, state, times) in worlds.items():
                video.poses.copy_(state[0]); video.disps.copy_(state[1])
                for dst, src in zip((graph.net, graph.target_cam, graph.weight, graph.raw_mask, graph.delta_dy, graph.damping), state[2:]):
                    dst.copy_(src)
                db.probe_arm("ba", 1)
                graph.update(None, None, use_inactive=True)
                v = db.probe_read(1)
                if r >= 5 and v:
                    times.append(1e3 * v[0])
        a, b = stats(worlds["plain"][3]), stats(worlds["sensor"][3])
        say("%s  E = %3d   without %8.1f (%6.1f .. %6.1f)   with a sensor map %8.1f (%6.1f .. %6.1f)   ratio %.3f"
            % ((label, len(worlds["plain"][1]._ii_h)) + a + b + (b[0] / a[0],)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
