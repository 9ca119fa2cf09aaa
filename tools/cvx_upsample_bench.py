"""Convex 8x upsampling: the library's kernels (pvo_cvx_upsample / pvo_cvx_upsample_vjp) against the PyTorch chain of
pvo_amd.droid_net.cvx_upsample (softmax, unfold, product, sum, permute: the specification, and what DepthVideo.upsample and the
training unroll ran before the kernels existed).

    python tools/cvx_upsample_bench.py [--reps 60] [--out profiles/r09_cvx_upsample.txt]

Method: both forms live in ONE process, work on the same tensors and are measured ALTERNATELY, repetition by repetition (other work
shares the box: a difference between two separate runs measures that).  One repetition is `--chain` back-to-back eager calls between two
device events, synchronised after every repetition; the figure is microseconds per call, median and the 10th .. 90th percentile after a
warm-up.  Eager on both sides: the PyTorch chain's seven launches and the native call's one are issued the way their callers issue them.
Rows:
  S-B      K = 8 frames of 48 x 64, fp16 channels-last mask as the update operator writes it, rows of a 16-frame video updated in place
  window   K = 26 frames of 30 x 101 (the real frontend window), the same
  S-T      B = 6 maps of 25 x 50, planar fp32 mask, forward + backward (one depth map list entry of the training unroll)
The PyTorch chain needs a planar mask; for the two inference rows it is timed both on a planar copy made outside the timed region and
with the layout pass it would need inside it.  Algorithmic bytes are computed from the shapes (mask + data in, 64 D values per pixel
out; backward: mask, data and the output gradient in, both gradients out) and divided by the native time.  The outputs of the two forms
are compared before anything is timed.  Needs the GPU: there is no fallback."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(fns, reps, chain, warm=10):
    """fns: name -> callable, run in turn; -> name -> sorted list of microseconds per call"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in fns}
    for r in range(reps + warm):
        for name, fn in fns.items():
            e0.record()
            for _ in range(chain):
                fn()
            e1.record()
            e1.synchronize()
            if r >= warm:
                times[name].append(e0.elapsed_time(e1) * 1e3 / chain)
    return {k: sorted(v) for k, v in times.items()}


def stats(v):
    n = len(v)
    return v[n // 2], v[n // 10], v[(9 * n) // 10]


def fmt(v):
    return "%8.1f (%6.1f .. %6.1f)" % stats(v)


def forward_bytes(B, H, W, D, mask_elem):
    return B * H * W * (576 * mask_elem + D * 4 + 64 * D * 4)


def backward_bytes(B, H, W, D, elem=4):
    return B * H * W * (2 * 576 * elem + 2 * D * elem + 64 * D * elem)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=60)
    p.add_argument("--chain", type=int, default=8, help="back-to-back calls per timed repetition")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_cvx_upsample.txt"))
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("cvx_upsample_bench: needs the GPU")
    from pvo_amd import droid_backends as db
    from pvo_amd.droid_net import cvx_upsample
    from pvo_amd.geom import upsample_native as un
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    say("convex 8x upsampling, PyTorch chain (droid_net.cvx_upsample) against pvo_cvx_upsample[_vjp]; %s, torch %s; %d repetitions of %d calls, "
        "alternating; microseconds per call, median (p10 .. p90)" % (torch.cuda.get_device_name(0), torch.__version__, args.reps, args.chain))
    say()
    say("%-34s %28s %28s %28s %7s %10s %9s" % ("forward, disps_up[ix] in place", "PyTorch, planar mask given", "PyTorch + layout pass",
                                              "native", "ratio", "MB (alg.)", "GB/s"))
    with torch.no_grad():
        for label, K, H, W, F in (("S-B     K=8  48x64  fp16 cl", 8, 48, 64, 16), ("window  K=26 30x101 fp16 cl", 26, 30, 101, 32)):
            g = torch.Generator().manual_seed(K)
            disps = (torch.rand(F, H, W, generator=g) + 0.2).to(dev)
            up_pt = torch.zeros(F, 8 * H, 8 * W, device=dev)
            up_nat = torch.zeros_like(up_pt)
            ix = torch.arange(F - K, F, device=dev)
            mask_cl = (torch.randn(K, H, W, 576, generator=g) * 4).half().to(dev).permute(0, 3, 1, 2)       # as the operator writes it
            mask_pl = mask_cl.contiguous()

            def pt(mask=mask_pl):
                up_pt[ix] = cvx_upsample(disps[ix].unsqueeze(-1), mask).squeeze(-1)

            def pt_layout():
                pt(mask_cl.contiguous())

            def nat():
                db.cvx_upsample(disps.unsqueeze(-1), mask_cl, out=up_nat.unsqueeze(-1), in_rows=ix, out_rows=ix)
            pt(); nat()
            torch.cuda.synchronize()
            d = float((up_pt - up_nat).abs().max())
            assert d <= 5e-3, (label, d)                       # (the chain computes its softmax in fp16 on an fp16 mask)
            t = measure({"pt": pt, "pt_layout": pt_layout, "nat": nat}, args.reps, args.chain)
            nbytes = forward_bytes(K, H, W, 1, 2)
            say("%-34s %28s %28s %28s %7.2f %10.2f %9.0f" % (label, fmt(t["pt"]), fmt(t["pt_layout"]), fmt(t["nat"]),
                                                           stats(t["nat"])[0] / stats(t["pt"])[0], nbytes / 1e6, nbytes / stats(t["nat"])[0] / 1e3))
    say("(ratio: native over the PyTorch chain on a planar mask, medians; GB/s: algorithmic bytes over the native time)")
    say()
    say("%-34s %28s %28s %7s %10s %9s" % ("S-T  B=6 25x50 planar fp32", "PyTorch", "native", "ratio", "MB (alg.)", "GB/s"))
    B, H, W = 6, 25, 50
    g = torch.Generator().manual_seed(6)
    data = (torch.rand(B, H, W, 1, generator=g) + 0.2).to(dev).requires_grad_()
    mask = (torch.randn(B, 576, H, W, generator=g) * 4).to(dev).requires_grad_()
    gout = torch.randn(B, 8 * H, 8 * W, 1, generator=g).to(dev)

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(data, mask)
        return run

    def fwd_bwd(fn):
        def run():
            data.grad = mask.grad = None
            fn(data, mask).backward(gout)
            return data.grad, mask.grad
        return run
    a, b = fwd_bwd(cvx_upsample)(), fwd_bwd(un.cvx_upsample)()
    for x, y in zip(a, b):
        assert float((x - y).abs().max()) <= 1e-4 * float(x.abs().max()), "the two backward forms disagree"
    t = measure({"pt": fwd(cvx_upsample), "nat": fwd(un.cvx_upsample)}, args.reps, args.chain)
    nb = forward_bytes(B, H, W, 1, 4)
    say("%-34s %28s %28s %7.2f %10.2f %9.0f" % ("forward", fmt(t["pt"]), fmt(t["nat"]), stats(t["nat"])[0] / stats(t["pt"])[0], nb / 1e6,
                                              nb / stats(t["nat"])[0] / 1e3))
    t = measure({"pt": fwd_bwd(cvx_upsample), "nat": fwd_bwd(un.cvx_upsample)}, args.reps, args.chain)
    nb = forward_bytes(B, H, W, 1, 4) + backward_bytes(B, H, W, 1)
    say("%-34s %28s %28s %7.2f %10.2f %9.0f" % ("forward + backward (autograd)", fmt(t["pt"]), fmt(t["nat"]), stats(t["nat"])[0] / stats(t["pt"])[0],
                                              nb / 1e6, nb / stats(t["nat"])[0] / 1e3))
    say("(these calls are tens of microseconds of device work: the eager figures include what the host needs to issue them, on both sides)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
