"""Segment association: the first measurement of pvo_segment_associate on the MI355X.

    python tools/segment_assoc_bench.py [--reps 40] [--parent-lib PATH] [--out profiles/r30_segment_assoc.txt]

tools/object_motion_bench.py's window: 30 x 101 (240 x 808 images), 10 keyframes, the 48 edges |i - j| <= 3, the targets the edges'
reprojections plus 0.1 pixels of noise.  Every keyframe carries the same grid of S - 1 segments (3 x 5, 7 x 9, 3 x 53 for S = 16, 64, 160)
under ids permuted per keyframe; a fourth case, S = 128 with 101 columns ONE pixel wide, is the worst the global form can meet (every
lane of a wave its own pair) and the widest table the LDS form holds.  Per call, between two device events on the stream with the
device idle before each, median and 10th .. 90th percentile of `reps` repetitions after 5 warm-ups, the calls of one S alternating and
their order reversed every repetition (so that no call always follows the same neighbour): the native call (the clear, the counting kernel, the match kernel) with the
counting kernel in the form the library picks (one atomic per wave and distinct pair into global memory) and, up to S = 128, with its
table in LDS (form = 1), a device-to-device copy of the
operands' bytes (labels, target: what reading every operand once costs), and the same three tables written in torch as a user without
the call would write them (round, bounds, a gather, bincount of a S + b; no matching).  The torch tables must EQUAL the call's.
--parent-lib (a libpvo_hip.so built from the parent commit): the calls this change must not have moved - FactorGraph.update
(pvo_graph_update) and pvo_object_motion (16 jobs per edge, iters = 8) on the same window, each through each library in a child process
of its own, `--runs` (5) children per library, alternating parent, this, parent, ...  A build's figure is the median of its runs'
medians; the condition: this build's figure is no further from the parent's than the parent's own runs' medians are from one another
(largest minus smallest).  The file says WITHIN or OUTSIDE, and the tool exits non-zero on OUTSIDE.  No time is fixed in advance: the
file records what was measured.  Needs the GPU: there is no fallback."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from object_motion_bench import HT, NKF, WD, alternating, bound, make_operands  # noqa: E402
from tsdf_bench import stats  # noqa: E402

GRIDS = {16: (3, 5), 64: (7, 9), 160: (3, 53), 128: (1, 127)}


def make_labels(S, dev, seed=0):
    """int32 [NKF,HT,WD]: a grid of S - 1 segments, the ids 1..S-1 permuted per keyframe"""
    rows, cols = GRIDS[S]
    g = torch.Generator().manual_seed(seed + S)
    y, x = torch.meshgrid(torch.arange(HT), torch.arange(WD), indexing="ij")
    block = (y * rows // HT) * cols + x * cols // WD
    return torch.stack([(1 + torch.randperm(S - 1, generator=g))[block] for _ in range(NKF)]).to(torch.int32).to(dev).contiguous()


def torch_tables(labels, ii, jj, target, S):
    """(overlap [E,S,S], area_i [E,S], area_j [E,S]) int64, in plain torch"""
    E, ht, wd = ii.shape[0], labels.shape[1], labels.shape[2]
    t = target.reshape(E, -1, 2)
    rx, ry = torch.floor(t[..., 0] + 0.5), torch.floor(t[..., 1] + 0.5)
    ok = torch.isfinite(t).all(-1) & (rx >= 0) & (rx <= wd - 1) & (ry >= 0) & (ry <= ht - 1)
    at = ry.clamp(0, ht - 1).long() * wd + rx.clamp(0, wd - 1).long()
    a, lj = labels[ii].reshape(E, -1).long(), labels[jj].reshape(E, -1).long()
    b = lj.gather(1, at)
    e = torch.arange(E, device=labels.device)[:, None]
    overlap = torch.bincount(((e * S + a) * S + b)[ok], minlength=E * S * S).reshape(E, S, S)
    return overlap, overlap.sum(2), torch.bincount((e * S + lj).reshape(-1), minlength=E * S).reshape(E, S)


def child(which, path, reps):
    """child process: one untouched call on the window through the library at `path` alone; prints its sorted microseconds as a JSON line"""
    from pvo_amd import _lib as L
    dev = torch.device("cuda:0")
    probe = ctypes.CDLL(path)
    L._lib = bound(path, L, [n for n in L.SIGNATURES if hasattr(probe, n)])          # (the parent's library lacks the new entry points)
    if which == "graph_update":
        import bench
        video, graph = bench.make_window(dev, H8=HT, W8=WD, NKF=NKF, buffer=16)
        if not graph._fused_ok():
            raise SystemExit("the native update path is not active")
        snap = bench.Snapshot(video, graph)

        def run():
            snap.restore()
            graph._ctx_token = None
            graph.update(None, None, use_inactive=True)
    else:
        from pvo_amd import droid_backends as db
        ops = make_operands(dev)
        E = ops["ii"].shape[0]
        job_edge = torch.arange(E, device=dev).repeat_interleave(16).contiguous()
        job_label = (1 + torch.arange(16, device=dev, dtype=torch.int32)).repeat(E).contiguous()
        N = job_edge.shape[0]
        out = {"rel": torch.empty(N, 7, device=dev), "motion": torch.empty(N, 7, device=dev), "info": torch.empty(N, 9, 4, device=dev)}

        def run():
            db.object_motion(ops["poses"], ops["disps"], ops["intrinsics"], ops["labels"], ops["ii"], ops["jj"], ops["target"], job_edge, job_label,
                             iters=8, out=out)
    print(json.dumps({"us": alternating({which: run}, reps)[which]}))


def compare_with_parent(parent, reps, lines, nruns=5):
    from pvo_amd import _lib as L
    assert not hasattr(ctypes.CDLL(parent), "pvo_segment_associate"), "--parent-lib must be the PARENT commit's library"
    lines += ["the untouched calls, this build's library and the parent commit's: one child process per library and run, %d runs each, alternating" % nruns,
              "parent, this, parent, ... (two copies of the library in one process do not time these calls fairly: profiles/r29_object_motion.txt)"]
    ok = True
    for which, what in (("graph_update", "FactorGraph.update (pvo_graph_update), 48 edges at %d x %d" % (HT, WD)),
                        ("object_motion", "pvo_object_motion, 768 jobs, iters = 8")):
        runs = {"parent": [], "this": []}
        for _ in range(nruns):
            for name, path in (("parent", parent), ("this", L.LIB_PATH)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--child-lib", path, "--reps", str(reps)],
                                   stdout=subprocess.PIPE, text=True, timeout=240, check=True)
                runs[name].append(json.loads(r.stdout.strip().splitlines()[-1])["us"])
        t = {k: stats(sorted(sum(v, []))) for k, v in runs.items()}
        med = {k: [stats(x)[0] for x in v] for k, v in runs.items()}
        spread = max(med["parent"]) - min(med["parent"])                       # the parent against itself
        fig = {k: sorted(v)[len(v) // 2] for k, v in med.items()}              # a build's figure: the median of its runs' medians
        good = abs(fig["this"] - fig["parent"]) <= spread
        ok = ok and good
        lines += ["  %s:" % what,
                  "    parent %9.1f us (runs' medians %s: the parent against itself moves by %.1f us; all samples %.1f [%.1f .. %.1f])"
                  % ((fig["parent"], ", ".join("%.1f" % x for x in med["parent"]), spread) + t["parent"]),
                  "    this   %9.1f us (runs' medians %s; all samples %.1f [%.1f .. %.1f])"
                  % ((fig["this"], ", ".join("%.1f" % x for x in med["this"])) + t["this"]),
                  "    this / parent = %.4f, %.1f us apart against the parent's own %.1f us: %s"
                  % (fig["this"] / fig["parent"], abs(fig["this"] - fig["parent"]), spread, "WITHIN" if good else "OUTSIDE")]
    lines += [""]
    return ok


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--runs", type=int, default=5, help="with --parent-lib: child processes per library and call")
    ap.add_argument("--parent-lib", default=None, help="a libpvo_hip.so built from the parent commit: the untouched calls side by side")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_segment_assoc.txt"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-lib", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("segment_assoc_bench needs the GPU (there is no fallback)")
    if args.child:
        return child(args.child, args.child_lib, args.reps)
    from pvo_amd import droid_backends as db
    dev = torch.device("cuda:0")
    ops = make_operands(dev)
    ii, jj, target = ops["ii"], ops["jj"], ops["target"]
    E = ii.shape[0]
    lines = ["segment_assoc_bench on %s: %d keyframes of %d x %d, %d edges; a grid of S - 1 segments per keyframe under ids permuted per keyframe, targets = reprojection + 0.1 px noise"
             % (torch.cuda.get_device_name(0), NKF, HT, WD, E),
             "per call, device events, device idle before each call, order reversed every repetition; median [p10 .. p90] of %d repetitions after 5 warm-ups" % args.reps, ""]
    ok = True
    for S in (16, 64, 160, 128):
        labels = make_labels(S, dev)
        forms = (0, 1) if S <= 128 else (0,)
        outs = [{k: torch.empty((E, S, S) if k == "overlap" else (E, S), dtype=torch.int32, device=dev)
                 for k in ("overlap", "area_i", "area_j", "match", "match_n", "match_d")} for _ in range(2)]
        call = lambda form: db.segment_associate(labels, ii, jj, target, S, out=outs[form], form=form)
        for f in forms:
            call(f)
        want = torch_tables(labels, ii, jj, target, S)
        equal = all(torch.equal(outs[f][k].long(), w) for f in forms for k, w in zip(("overlap", "area_i", "area_j"), want))
        forms_equal = all(torch.equal(outs[0][k], outs[f][k]) for f in forms for k in outs[0])
        ok = ok and equal and forms_equal
        copies = [torch.empty_like(labels), torch.empty_like(target)]
        nbytes = labels.numel() * 4 + target.numel() * 4

        def copy():
            copies[0].copy_(labels)
            copies[1].copy_(target)
        fns = {"native": lambda: call(0), "copy": copy, "torch": lambda: torch_tables(labels, ii, jj, target, S)}
        if 1 in forms:
            fns["lds"] = lambda: call(1)
        t = {k: stats(v) for k, v in alternating(fns, args.reps, warm=5).items()}
        matched = int((outs[0]["match"] >= 0).sum())
        rows, cols = GRIDS[S]
        lines += ["S = %d (a %d x %d grid of segments per keyframe): %d counted pixels, %d of %d segments matched; tables equal to torch's: %s; the forms' bytes equal: %s"
                  % (S, rows, cols, int(outs[0]["overlap"].sum()), matched, E * (S - 1), equal, forms_equal),
                  "    the call (3 launches), as the library picks     %7.1f us [%.1f .. %.1f]" % t["native"]]
        lines += ["    the call, the table in LDS (form = 1)           %7.1f us [%.1f .. %.1f]   LDS / picked = %.2f" % (t["lds"] + (t["lds"][0] / t["native"][0],))
                  if 1 in forms else "    (S > 128: no LDS form)"]
        lines += [
                  "    copy of labels, target                          %7.1f us [%.1f .. %.1f]   %d bytes: call / copy = %.2f"
                  % (t["copy"] + (nbytes, t["native"][0] / t["copy"][0])),
                  "    the three tables in torch (gather, bincount)    %7.1f us [%.1f .. %.1f]   torch / call = %.1f"
                  % (t["torch"] + (t["torch"][0] / t["native"][0],)), ""]
    if args.parent_lib:
        ok = compare_with_parent(args.parent_lib, args.reps, lines, args.runs) and ok
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print("written to", args.out)
    if not ok:
        raise SystemExit("a table differs from torch's, or an untouched call is outside the parent's measured spread")


if __name__ == "__main__":
    main()
