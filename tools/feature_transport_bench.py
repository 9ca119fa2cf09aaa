"""Feature transport: the first measurement of pvo_feature_transport and of the fusion convolution behind it on the MI355X.

    python tools/feature_transport_bench.py [--reps 40] [--parent-lib PATH] [--out profiles/r31_feature_transport.txt]

The VKITTI pyramid: images of 375 x 1242 padded to 384 x 1248, five levels of 96 x 312, 48 x 156, 24 x 78, 12 x 39 and 6 x 20 cells, C = 256
in fp16, with the current frame's features (out = [cur | transported], 2C wide); the flow and the disparity at the odometry's 1/8
resolution (48 x 156), a smooth flow of a few cells plus noise.  Flow only, and with the disparity as the key (order = -1).  Per call,
between two device events on the stream with the device idle before each, median and 10th .. 90th percentile of `reps` repetitions
after 5 warm-ups, the calls alternating and their order reversed every repetition:

  the call          droid_backends.feature_transport into caller-owned outputs (clear, resolve, gather: three launches)
  copy              device-to-device copies that move the gather's bytes: with cur the gather reads the pyramid twice (cur, and at most
                    every ref row once) and writes it twice - two copies of the pyramid's P bytes into a buffer of 2 P
  the host route    what the call replaces: flow, disparity and the reference frame's features copied to the host, the numpy restatement
                    of the same contract (tests/feature_transport_reference.py), the transported pyramid copied back; `--host-reps` (5)
                    repetitions on a host clock around a device synchronise.  Its src must EQUAL the call's.
  the convolution   droid_backends.conv3x3 (512 -> 256) on each level's [cur | transported], and all five in a row

--parent-lib (a libpvo_hip.so built from the parent commit): FactorGraph.update (pvo_graph_update) on tools/object_motion_bench.py's
window through each library in a child process of its own, `--runs` (5) children per library, alternating parent, this, parent, ...
A build's figure is the median of its runs' medians; the file says WITHIN when this build's figure is no further from the parent's than
the parent's own runs' medians are from one another, else OUTSIDE (and the tool exits non-zero).  No time or ratio is fixed in
advance: the file records what was measured.  Needs the GPU: there is no fallback."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from object_motion_bench import alternating, graph_update_child  # noqa: E402
from tsdf_bench import stats  # noqa: E402

LEVELS = ((96, 312), (48, 156), (24, 78), (12, 39), (6, 20))
HT, WD, C = 48, 156, 256


def make_operands(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(HT, dtype=torch.float32), torch.arange(WD, dtype=torch.float32), indexing="ij")
    flow = torch.stack([2.5 + 1.5 * torch.sin(y / 9.0) + 0.01 * x, -1.0 + 1.2 * torch.cos(x / 17.0)], -1) + 0.3 * torch.randn(HT, WD, 2, generator=g)
    disp = 0.4 + 0.3 * torch.sin(x / 23.0).abs() + 0.1 * torch.rand(HT, WD, generator=g)
    feats = lambda: [torch.randn(1, H, W, C, generator=g).half().to(dev).permute(0, 3, 1, 2) for H, W in LEVELS]
    return flow.contiguous().to(dev), disp.contiguous().to(dev), feats(), feats()


def compare_with_parent(parent, reps, lines, nruns):
    from pvo_amd import _lib as L
    assert not hasattr(ctypes.CDLL(parent), "pvo_feature_transport"), "--parent-lib must be the PARENT commit's library"
    lines += ["FactorGraph.update (pvo_graph_update, 48 edges at 30 x 101) through this build's library and the parent commit's: one child process per",
              "library and run, %d runs each, alternating parent, this, parent, ..." % nruns]
    runs = {"parent": [], "this": []}
    for _ in range(nruns):
        for name, path in (("parent", parent), ("this", L.LIB_PATH)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-lib", path, "--reps", str(reps)],
                               stdout=subprocess.PIPE, text=True, timeout=240, check=True)
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["us"])
    med = {k: [stats(x)[0] for x in v] for k, v in runs.items()}
    spread = max(med["parent"]) - min(med["parent"])
    fig = {k: sorted(v)[len(v) // 2] for k, v in med.items()}
    good = abs(fig["this"] - fig["parent"]) <= spread
    lines += ["    parent %9.1f us (runs' medians %s: the parent against itself moves by %.1f us)" % (fig["parent"], ", ".join("%.1f" % x for x in med["parent"]), spread),
              "    this   %9.1f us (runs' medians %s)" % (fig["this"], ", ".join("%.1f" % x for x in med["this"])),
              "    this / parent = %.4f, %.1f us apart against the parent's own %.1f us: %s"
              % (fig["this"] / fig["parent"], abs(fig["this"] - fig["parent"]), spread, "WITHIN" if good else "OUTSIDE"), ""]
    return good


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5, help="with --parent-lib: child processes per library")
    ap.add_argument("--parent-lib", default=None, help="a libpvo_hip.so built from the parent commit: pvo_graph_update side by side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r31_feature_transport.txt"))
    ap.add_argument("--child-lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("feature_transport_bench needs the GPU (there is no fallback)")
    if args.child_lib:
        return graph_update_child(args.child_lib, args.reps)
    import feature_transport_reference as R
    from pvo_amd import droid_backends as db
    dev = torch.device("cuda:0")
    flow, disp, ref, cur = make_operands(dev)
    scales = [(W / WD, H / HT) for H, W in LEVELS]
    P = sum(H * W for H, W in LEVELS) * C * 2
    outs = [torch.empty(1, H, W, 2 * C, dtype=torch.float16, device=dev).permute(0, 3, 1, 2) for H, W in LEVELS]
    srcs = [torch.empty(H, W, dtype=torch.int32, device=dev) for H, W in LEVELS]
    call = lambda depth: db.feature_transport(ref, cur, flow, scales=scales, depth=depth, order=-1, out=(outs, srcs))
    flat = [torch.cat([t.permute(0, 2, 3, 1).reshape(-1) for t in f]) for f in (ref, cur)]
    dst = torch.empty(2 * P // 2, dtype=torch.float16, device=dev)

    def copy():
        dst[:P // 2].copy_(flat[0])
        dst[P // 2:].copy_(flat[1])

    def host(depth):
        """the route the call replaces, transfers included; returns (seconds, srcs)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f, d = flow.cpu().numpy(), None if depth is None else depth.cpu().numpy()
        feats = [t[0].permute(1, 2, 0).cpu().numpy() for t in ref]
        moved, won = R.transport(feats, None, f, scales=scales, depth=d, order=-1)
        back = [torch.from_numpy(m).to(dev) for m in moved]
        torch.cuda.synchronize()
        return time.perf_counter() - t0, won, back

    lines = ["feature_transport_bench on %s: the VKITTI pyramid, %s, C = %d fp16 with cur (P = %d bytes per frame), flow and disparity %d x %d"
             % (torch.cuda.get_device_name(0), " ".join("%dx%d" % s for s in LEVELS), C, P, HT, WD),
             "per call, device events, device idle before each call, order reversed every repetition; median [p10 .. p90] of %d repetitions after 5 warm-ups" % args.reps, ""]
    ok = True
    for what, depth in (("flow only", None), ("with the disparity as the key (order = -1)", disp)):
        t = {k: stats(v) for k, v in alternating({"call": lambda: call(depth), "copy": copy}, args.reps, warm=5).items()}
        call(depth)
        torch.cuda.synchronize()
        got = [s.cpu().numpy() for s in srcs]
        hs = []
        for _ in range(args.host_reps):
            sec, won, back = host(depth)
            hs.append(sec * 1e6)
        equal = all(np.array_equal(a, b) for a, b in zip(got, won)) and \
            all(torch.equal(o[0, C:].permute(1, 2, 0), b) for o, b in zip(outs, back))
        ok = ok and equal
        h = stats(sorted(hs))
        reached = sum(int((s >= 0).sum()) for s in got)
        lines += ["%s: %d of %d cells reached; src and the transported half equal to the host route's: %s" % (what, reached, sum(H * W for H, W in LEVELS), equal),
                  "    the call (3 launches)                           %8.1f us [%.1f .. %.1f]   %.0f GB/s over the 4 P bytes the gather moves at most"
                  % (t["call"] + (4 * P / t["call"][0] / 1e3,)),
                  "    two copies of P bytes into 2 P (reads 2 P, writes 2 P) %8.1f us [%.1f .. %.1f]   call / copy = %.2f" % (t["copy"] + (t["call"][0] / t["copy"][0],)),
                  "    the host route (transfers + numpy), %d runs      %8.0f us [%.0f .. %.0f]   host / call = %.0f" % ((args.host_reps,) + h + (h[0] / t["call"][0],)), ""]
    # the fusion convolution on the transported pyramid
    w = db.conv3x3_weights(0.02 * torch.randn(C, 2 * C, 3, 3, device=dev), torch.float16)
    bias = torch.zeros(C, device=dev)
    ys = [torch.empty(1, H, W, C, dtype=torch.float16, device=dev).permute(0, 3, 1, 2) for H, W in LEVELS]
    fns = {"%dx%d" % s: (lambda l=l: db.conv3x3(outs[l], w, bias, out=ys[l])) for l, s in enumerate(LEVELS)}
    fns["all five"] = lambda: [db.conv3x3(outs[l], w, bias, out=ys[l]) for l in range(len(LEVELS))]
    fns["transport"] = lambda: call(disp)
    t = {k: stats(v) for k, v in alternating(fns, args.reps, warm=5).items()}
    lines += ["the fusion convolution (pvo_conv3x3, 512 -> 256, fp16) on [cur | transported]:"]
    for l, (H, W) in enumerate(LEVELS):
        k = "%dx%d" % (H, W)
        lines += ["    %-9s %8.1f us [%.1f .. %.1f]   %.1f TFLOP/s" % ((k,) + t[k] + (2.0 * 9 * 2 * C * C * H * W / t[k][0] / 1e6,))]
    lines += ["    all five  %8.1f us [%.1f .. %.1f]" % t["all five"],
              "    the transport beside it (with the disparity) %8.1f us [%.1f .. %.1f]: transport / (transport + convolutions) = %.2f"
              % (t["transport"] + (t["transport"][0] / (t["transport"][0] + t["all five"][0]),)), ""]
    if args.parent_lib:
        ok = compare_with_parent(args.parent_lib, args.reps, lines, args.runs) and ok
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print("written to", args.out)
    if not ok:
        raise SystemExit("the call differs from the host route, or pvo_graph_update is outside the parent's measured spread")


if __name__ == "__main__":
    main()
