"""The per-frame encoders' convolutions: the vendor library (F.conv2d, restricted to kernels that repeat their result, as
BasicEncoder.forward_inference runs it) against the library's own pvo_conv_planes - per layer class of both encoders at the 240 x 808
stream's map sizes, and the whole fnet / cnet, everything replayed as HIP graphs.

    python tools/encoder_conv_bench.py [--replays 60] [--out profiles/r08_encoder_native_conv.txt]

Method: both paths live in ONE process and are measured ALTERNATELY, replay by replay (other work shares the box: a difference between
two separate runs measures that).  A layer is captured as a graph of `--chain` back-to-back calls and a replay is timed with device
events (synchronised after every replay); the figure is microseconds per call.  Median and the 10th .. 90th percentile over the replays
after a warm-up.  "bare" is the convolution alone (what the instance-norm encoder runs in front of pvo_bias_norm_act on both paths);
"layer" is the norm-free encoder's layer - convolution + bias + ReLU: vendor convolution + pvo_bias_norm_act against one
pvo_conv_planes with the epilogue.  The outputs of the two paths are compared before anything is timed.
Needs the GPU: there is no fallback."""
import argparse
import copy
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, ksize, stride, Cin, Cout, H, W of the INPUT, how many such convolutions one encoder has)
LAYER_CLASSES = [("stem 7x7 s2   3->32  @240x808", 7, 2, 3, 32, 240, 808, 1),
                 ("3x3 s1  32->32  @120x404", 3, 1, 32, 32, 120, 404, 4),
                 ("3x3 s2  32->64  @120x404", 3, 2, 32, 64, 120, 404, 1),
                 ("3x3 s1  64->64  @60x202", 3, 1, 64, 64, 60, 202, 3),
                 ("3x3 s2  64->128 @60x202", 3, 2, 64, 128, 60, 202, 1),
                 ("3x3 s1 128->128 @30x101", 3, 1, 128, 128, 30, 101, 3)]


def capture(fn, warm=3):
    for _ in range(warm):                                  # (the vendor library picks its kernels here)
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    g.replay()
    torch.cuda.synchronize()
    return g, out


def measure(graphs, replays, per_replay):
    """graphs: name -> CUDAGraph, replayed in turn; -> name -> sorted list of microseconds per call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in graphs}
    for r in range(replays + 10):
        for name, g in graphs.items():
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            if r >= 10:
                times[name].append(e0.elapsed_time(e1) * 1e3 / per_replay)
    return {k: sorted(v) for k, v in times.items()}


def stats(v):
    n = len(v)
    return v[n // 2], v[n // 10], v[(9 * n) // 10]


def fmt(v):
    return "%8.1f (%6.1f .. %6.1f)" % stats(v)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--replays", type=int, default=60)
    p.add_argument("--chain", type=int, default=8, help="calls of a layer per captured graph")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_encoder_native_conv.txt"))
    p.add_argument("--only", choices=("layers", "encoders"), default=None)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("encoder_conv_bench: needs the GPU")
    from pvo_amd import droid_backends as db
    from pvo_amd.modules.extractor import BasicEncoder
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("encoder convolutions, vendor library against pvo_conv_planes; %s, torch %s; fp16; %d replays, alternating; microseconds, median (p10 .. p90)"
        % (torch.cuda.get_device_name(0), torch.__version__, args.replays))
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True               # as BasicEncoder.forward_inference sets it around its vendor convolutions
    try:
        with torch.no_grad():
            if args.only != "encoders":
                say()
                say("%-32s %28s %28s %7s   %28s %28s %7s" % ("layer class (per call)", "bare: vendor", "bare: native", "ratio", "layer: vendor+act", "layer: native", "ratio"))
                total = {"vendor": 0.0, "native": 0.0}
                for name, k, s, cin, cout, h, w, count in LAYER_CLASSES:
                    g = torch.Generator().manual_seed(cin + cout + h)
                    x = torch.randn(1, cin, h, w, generator=g).half().to(dev)
                    wt = (torch.randn(cout, cin, k, k, generator=g) * (cin * k * k) ** -0.5).half().to(dev)
                    b = torch.randn(cout, generator=g).half().to(dev)
                    pk = db.conv_planes_pack(wt)
                    fns = {"bare vendor": lambda: F.conv2d(x, wt, None, s, k // 2),
                           "bare native": lambda: db.conv_planes(x, pk, stride=s),
                           "layer vendor": lambda: db.bias_norm_act(F.conv2d(x, wt, None, s, k // 2), b, None, norm=False, relu_inner=True),
                           "layer native": lambda: db.conv_planes(x, pk, b, stride=s, relu_inner=True)}
                    d = float((fns["layer vendor"]().float() - fns["layer native"]().float()).abs().max())
                    assert d <= 4e-3 * max(1.0, float(fns["layer vendor"]().float().abs().max())), (name, d)

                    def chain(fn):
                        def run():
                            for _ in range(args.chain):
                                y = fn()
                            return y
                        return run
                    graphs, keep = {}, []
                    for key, fn in fns.items():
                        graphs[key], out = capture(chain(fn))
                        keep.append(out)
                    t = measure(graphs, args.replays, args.chain)
                    say("%-32s %28s %28s %7.2f   %28s %28s %7.2f" % (name, fmt(t["bare vendor"]), fmt(t["bare native"]),
                                                                    stats(t["bare native"])[0] / stats(t["bare vendor"])[0],
                                                                    fmt(t["layer vendor"]), fmt(t["layer native"]),
                                                                    stats(t["layer native"])[0] / stats(t["layer vendor"])[0]))
                    total["vendor"] += count * stats(t["bare vendor"])[0]
                    total["native"] += count * stats(t["bare native"])[0]
                    del graphs, keep
                say("sum over one encoder's 13 convolutions of these classes (bare, medians): vendor %.1f us, native %.1f us" % (total["vendor"], total["native"]))
            if args.only != "layers":
                say()
                say("%-32s %28s %28s %7s %12s" % ("whole encoder, one graph replay", "vendor convolutions", "native convolutions", "ratio", "max |diff|"))
                for label, norm_fn, od in (("fnet (instance norm, 128)", "instance", 128), ("cnet (no norm, 256)", "none", 256)):
                    torch.manual_seed(0)
                    vend = BasicEncoder(output_dim=od, norm_fn=norm_fn).to(dev).eval().half()
                    nat = copy.deepcopy(vend)
                    nat.native_convs = True
                    x = torch.randn(1, 1, 3, 240, 808, generator=torch.Generator().manual_seed(1)).half().to(dev)
                    gv, ov = capture(lambda: vend.forward_inference(x))
                    gn, on = capture(lambda: nat.forward_inference(x))
                    diff = float((ov.float() - on.float()).abs().max()) / float(ov.float().abs().max())
                    t = measure({"vendor": gv, "native": gn}, args.replays, 1)
                    say("%-32s %28s %28s %7.2f %12.2e" % (label, fmt(t["vendor"]), fmt(t["native"]), stats(t["native"])[0] / stats(t["vendor"])[0], diff))
                say("(max |diff|: native against vendor output, relative to the output's largest magnitude)")
    finally:
        torch.backends.cudnn.deterministic = prev
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
