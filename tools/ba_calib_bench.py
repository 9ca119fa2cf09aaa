"""What the calibrating step costs: one pvo_ba_calib iteration beside ONE plain bundle-adjustment iteration on the same window.

    python tools/ba_calib_bench.py [--reps 40] [--out profiles/r14_ba_calib.txt]

Two windows from bench.make_window after two native updates: S-B (8 keyframes of 48 x 64) and the frontend window (26 keyframes of
30 x 101).  On the window's own BA operands, in ONE process and ALTERNATELY repetition by repetition (other work shares the machine):
  ba 1 it       db.ba(..., iterations=1) on clones of poses / disps - plan + assembly + elimination + solve + back-substitution: the
                yardstick (this code is the parent commit's: the calibration adds entry points and changes none);
  calib 1 it    db.ba_calib(..., iterations=1) on clones of poses / disps / intrinsics: the same plan, assembly and elimination, then the
                border's assembly and elimination, the fp64 inverse of the damped pose system (the uncertainty stage's four launches),
                the bordered solve and the back-substitution;
  calib held    the same with free_mask = 0: the step of `ba 1 it` by the calibrating route.
Device events; median (p10 .. p90) of --reps repetitions in microseconds.  Needs the GPU."""
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


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=40)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_ba_calib.txt"))
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ba_calib_bench: needs the GPU")
    import bench
    from pvo_amd import droid_backends as db
    from test_chained_updates import structured_operator
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("calibrating step (pvo_ba_calib) beside one plain BA iteration on the same window; %s; %d repetitions, alternating; microseconds, "
        "median (p10 .. p90)" % (torch.cuda.get_device_name(0), args.reps))
    for label, kw in (("S-B     8 keyframes  48x64 ", {}),
                      ("window  26 keyframes 30x101", dict(H8=30, W8=101, NKF=26, buffer=32, intr=(60.0, 60.0, 50.5, 15.0)))):
        video, graph = bench.make_window(dev, seed=3, **kw)
        structured_operator(graph.update_op, 0.1)
        for _ in range(2):
            graph.update(None, None, use_inactive=True)
        ht, wd = graph.ht, graph.wd
        t0, t1 = max(1, min(graph._ii_h) + 1), max(max(graph._ii_h), max(graph._jj_h)) + 1
        rows = sorted(set(graph._ii_h) | set(range(t0, t1)))
        eta = (0.2 * graph.damping[torch.tensor(rows, device=dev)] + 1e-7).contiguous()
        target = graph.target_cam.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
        weight = graph.weight.view(-1, ht, wd, 2).permute(0, 3, 1, 2).contiguous()
        ii, jj = graph.ii.contiguous(), graph.jj.contiguous()
        E, P = ii.shape[0], t1 - t0
        poses, disps, intr = video.poses.clone(), video.disps.clone(), video.intrinsics[0].clone()
        status = torch.zeros(4, dtype=torch.int32, device=dev)

        def reset():
            poses.copy_(video.poses)
            disps.copy_(video.disps)
            intr.copy_(video.intrinsics[0])
        runs = {
            "ba 1 it": lambda: db.ba(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, 1, 1e-4, 0.1, False),
            "calib 1 it": lambda: db.ba_calib(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, 1, 1e-4, 0.1, 0.1, 15, status=status),
            "calib held": lambda: db.ba_calib(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, 1, 1e-4, 0.1, 0.1, 0),
        }
        times = {k: [] for k in runs}
        for r in range(args.reps + 5):
            for name, fn in runs.items():
                reset()                                            # (untimed: every iteration starts from the window's state)
                t = timed(fn)
                if r >= 5:
                    times[name].append(t)
        reset()
        dc = runs["calib 1 it"]()[2]
        st = {k: stats(v) for k, v in times.items()}
        say("%s  E = %3d  P = %2d   (step accepted: %s, dc = %s)" % (label, E, P, int(status[0]) == 0, ["%.3g" % v for v in dc.tolist()]))
        for name, s in (("one plain BA iteration (the yardstick)", st["ba 1 it"]), ("one calibrating iteration, all four free", st["calib 1 it"]),
                        ("one calibrating iteration, all four held", st["calib held"])):
            say("    %-42s %8.1f (%7.1f .. %7.1f)" % ((name,) + s))
        say("    calibrating / plain = %.2f" % (st["calib 1 it"][0] / st["ba 1 it"][0]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
