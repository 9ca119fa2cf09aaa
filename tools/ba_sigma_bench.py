"""What the uncertainty stage costs: its five launches beside ONE bundle-adjustment iteration on the same window.

    python tools/ba_sigma_bench.py [--reps 40] [--out profiles/r13_ba_sigma.txt]

Two windows from bench.make_window after two native updates: S-B (8 keyframes of 48 x 64) and the frontend window (26 keyframes of
30 x 101).  On the window's own BA operands, in ONE process and ALTERNATELY repetition by repetition (other work shares the machine):
  ba 1 it     db.ba(..., iterations=1) on clones of poses / disps - plan + assembly + elimination + solve + back-substitution: the
              yardstick;
  local       plan + db.ba_local: what pvo_ba_uncertainty runs in front of the stage (the yardstick's first half);
  the stage   pvo_ba_sigma on what `local` left, between a pair of device events on an otherwise idle stream, called twice: with
              pose_cov only - prepare, factor, invtri and product, the four launches of the fp64 inverse, reported together as
              "system" - and with all outputs; the sigma kernel is the difference of the two, repetition by repetition.
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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_ba_sigma.txt"))
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ba_sigma_bench: needs the GPU")
    import bench
    from pvo_amd import droid_backends as db
    from test_chained_updates import structured_operator
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("uncertainty stage (pvo_ba_sigma) beside one BA iteration on the same window; %s; %d repetitions, alternating; microseconds, "
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
        F, E, P, HW = video.disps.shape[0], ii.shape[0], t1 - t0, ht * wd
        intr = video.intrinsics[0].contiguous()
        ws = db.ba_workspace(E, P, F, HW, dev)
        sysb = torch.zeros((6 * P) ** 2 + 6 * P, dtype=torch.int64, device=dev)
        vc, vp = torch.empty_like(video.disps), torch.empty_like(video.disps)
        poses, disps = video.poses.clone(), video.disps.clone()

        def one_ba():
            poses.copy_(video.poses)
            disps.copy_(video.disps)

        def local():
            db.ba_plan(ii, jj, F, HW, eta.shape[0], t0, t1, ws)
            db.ba_local(video.poses, video.disps, intr, target, weight, eta, ii, jj, t0, t1, False, sysb, ws)
        runs = {
            "ba 1 it": lambda: db.ba(poses, disps, intr, target, weight, eta, ii, jj, t0, t1, 1, 1e-4, 0.1, False),
            "local": local,
            "system": lambda: db.ba_sigma(sysb, ws, ii, jj, video.disps, t0, t1, 1e-4, 0.1),
            "all": lambda: db.ba_sigma(sysb, ws, ii, jj, video.disps, t0, t1, 1e-4, 0.1, vc, vp),
        }
        times = {k: [] for k in runs}
        for r in range(args.reps + 5):
            for name, fn in runs.items():
                if name == "ba 1 it":
                    one_ba()                                       # (untimed: every iteration starts from the window's state)
                elif name != "local":
                    local()                                        # (untimed: the stage reads what plan + local leave)
                t = timed(fn)
                if r >= 5:
                    times[name].append(t)
        st = {k: stats(v) for k, v in times.items()}
        sig = stats([a - b for a, b in zip(times["all"], times["system"])])
        say("%s  E = %3d  P = %2d" % (label, E, P))
        for name, s in (("one BA iteration (the yardstick)", st["ba 1 it"]), ("plan + local (in front of the stage)", st["local"]),
                        ("prepare + factor + invtri + product", st["system"]), ("sigma kernel (all - the four above)", sig),
                        ("the stage: five launches", st["all"])):
            say("    %-40s %8.1f (%7.1f .. %7.1f)" % ((name,) + s))
        say("    stage / one BA iteration = %.2f;  (local + stage) / one BA iteration = %.2f"
            % (st["all"][0] / st["ba 1 it"][0], (st["local"][0] + st["all"][0]) / st["ba 1 it"][0]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
