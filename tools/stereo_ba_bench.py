"""What stereo costs: the bundle-adjustment stage of the native update (the PVO_STAGE_BA probe: HIP events around the BA of
pvo_graph_update) with one stereo edge per keyframe against the same window without, and the extra `fnet` pass a keyframe's right
image takes in the motion filter.

    python tools/stereo_ba_bench.py [--reps 40] [--out profiles/r11_stereo.txt]

Two windows from bench.make_window: S-B (8 keyframes of 48 x 64) and the frontend window (26 keyframes of 30 x 101).  Both forms live
in ONE process and are measured ALTERNATELY, update by update (other work shares the machine); the state is restored before every
update, so each one solves the same problem.  A stereo edge is one more edge to the assembly (its workgroups skip the 90-sum
reduce-scatter and store zero coupling rows), one more out-edge to its frame's depth phase and one more row to its Schur block: the
expectation is "the cost of E + NKF edges instead of E", the figure is the record.  The encoder figure is the captured fnet graph of
the motion filter on a 240 x 808 frame, median of `reps` replays between two events.  Needs the GPU."""
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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_stereo.txt"))
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("stereo_ba_bench: needs the GPU")
    import bench
    from pvo_amd import droid_backends as db
    from test_chained_updates import structured_operator
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("BA stage of the native update (PVO_STAGE_BA probe) with and without one stereo edge per keyframe; %s; %d updates each, alternating; "
        "microseconds per update, median (p10 .. p90)" % (torch.cuda.get_device_name(0), args.reps))
    for label, kw in (("S-B     8 keyframes  48x64 ", {}),
                      ("window  26 keyframes 30x101", dict(H8=30, W8=101, NKF=26, buffer=32, intr=(60.0, 60.0, 50.5, 15.0)))):
        worlds = {}
        for name in ("plain", "stereo"):
            video, graph = bench.make_window(dev, seed=3, **kw)
            structured_operator(graph.update_op, 0.1)
            if name == "stereo":
                n = graph.nkf
                g = torch.Generator().manual_seed(17)
                video.ensure_fmaps_right()[:n] = torch.randn(n, video.ht // 8, video.wd // 8, 128, generator=g).half().to(dev)
                graph.add_factors(list(range(n)), list(range(n)))
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
        a, b = stats(worlds["plain"][3]), stats(worlds["stereo"][3])
        say("%s  E = %3d -> %3d   without %8.1f (%6.1f .. %6.1f)   with stereo edges %8.1f (%6.1f .. %6.1f)   ratio %.3f"
            % ((label, len(worlds["plain"][1]._ii_h), len(worlds["stereo"][1]._ii_h)) + a + b + (b[0] / a[0],)))
    # the right image's encoder pass: the motion filter's captured fnet graph on a 240 x 808 frame
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.droid_net import DroidNet
    from pvo_amd.motion_filter import MotionFilter
    torch.manual_seed(0)
    net = DroidNet().to(dev).eval()
    net.update.half(); net.fnet.half(); net.cnet.half()
    video = DepthVideo(image_size=(240, 808), buffer=4, device=dev)
    mf = MotionFilter(net, video, device=dev)
    img = torch.randint(0, 255, (3, 240, 808), dtype=torch.int32, device=dev)
    with torch.no_grad():
        for _ in range(5):
            mf._features_g(img)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = mf._features_g(img).clone()
            e1.record()
            e1.synchronize()
            times.append(1e3 * e0.elapsed_time(e1))
    m = stats(times)
    say("extra fnet pass per keyframe (captured graph + the copy out of its static buffer), 240x808: %8.1f us (%6.1f .. %6.1f); "
        "a non-keyframe's right image is never uploaded or encoded" % m)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
