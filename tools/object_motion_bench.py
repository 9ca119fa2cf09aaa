"""Object motion: the first measurement of pvo_object_motion on the MI355X.

    python tools/object_motion_bench.py [--reps 40] [--parent-lib PATH] [--kernel-stats CSV] [--out profiles/r29_object_motion.txt]

The 30 x 101 window (240 x 808 images) with 10 keyframes and the 48 edges |i - j| <= 3; every keyframe carries the same 4 x 4 grid of 16
segments; the targets are the edges' reprojections plus 0.1 pixels of noise, so every job is a well-posed static segment.  1, 4 and 16
jobs per edge (48, 192, 768 jobs).  Per call, between two device events on the stream, median and 10th .. 90th percentile of `reps`
repetitions after 5 warm-ups, the calls of one job count alternating: the native call at iters = 0 (3 launches) and iters = 8 (19), a
device-to-device copy of the operands' bytes (disps, labels, target: what reading every operand once costs), and one evaluation
written in torch as a user without the call would write it (per pixel the job of its label, its A gathered, r and J, the 28 sums by
index_add_ over the jobs).  --kernel-stats: the kernel_stats csv of a separate `rocprofv3 --kernel-trace --stats` run of
tools/object_motion_workload.py; the three kernels' rows are copied into the file.  --parent-lib (a libpvo_hip.so built from the
parent commit): the calls this change must not have moved - the plain pvo_tsdf_track through both libraries in this process, alternating
with the order reversed every repetition and the device idle before each call, and FactorGraph.update's pvo_graph_update on the same
window through each library in a child process of its own, three children each, alternating; the only condition is that each median lies
inside the other build's p10 .. p90 (for the child processes: or that the two builds are no further apart than two runs of one build).  No time is fixed in advance: the file records what was measured.
Needs the GPU: there is no fallback."""
import argparse
import csv
import ctypes
import json
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tsdf_bench import make_video, measure, stats  # noqa: E402

HT, WD, NKF, GRID = 30, 101, 10, 4


def make_operands(dev, seed=0):
    """dict poses, disps, intrinsics, labels, ii, jj, target for the window"""
    from pvo_amd import droid_backends as db
    from pvo_amd.geom.se3 import SE3
    g = torch.Generator().manual_seed(seed)
    xi = torch.tensor([0.05, 0.0, 0.02, 0.0, 0.01, 0.0])
    poses = torch.stack([SE3.exp(k * xi).data for k in range(NKF)]).float().to(dev).contiguous()
    low = torch.rand(1, 1, 6, 8, generator=g) * 0.8 + 0.2
    disp = torch.nn.functional.interpolate(low, size=(HT, WD), mode="bilinear", align_corners=True)[0, 0]
    disps = disp[None].repeat(NKF, 1, 1).to(dev).contiguous()
    intr = torch.tensor([80.0, 80.0, 0.5 * WD - 0.5, 0.5 * HT - 0.5], device=dev)
    pairs = [(i, j) for i in range(NKF) for j in range(NKF) if i != j and abs(i - j) <= 3]
    ii, jj = (torch.tensor([p[k] for p in pairs], device=dev) for k in (0, 1))
    coords, _ = db.reproject(poses, disps, intr[None].repeat(NKF, 1).contiguous(), ii, jj)
    target = (coords + 0.1 * torch.randn(coords.shape, generator=g).to(dev)).contiguous()
    y, x = torch.meshgrid(torch.arange(HT), torch.arange(WD), indexing="ij")
    lab = (1 + (y * GRID // HT) * GRID + x * GRID // WD).to(torch.int32)
    labels = lab[None].repeat(NKF, 1, 1).to(dev).contiguous()
    return dict(poses=poses, disps=disps, intrinsics=intr, labels=labels, ii=ii, jj=jj, target=target)


def torch_evaluation(ops, job_edge, job_label, rel, z_min=0.25):
    """one evaluation in plain torch: (sums [N,28] = H 21, b 6, E; count [N]) at the A of rel [N,7]"""
    E, N = ops["ii"].shape[0], job_edge.shape[0]
    dev = rel.device
    fx, fy, cx, cy = ops["intrinsics"].unbind()
    lab = ops["labels"][ops["ii"]]                                          # [E,ht,wd]
    table = torch.full((E, GRID * GRID + 1), -1, dtype=torch.long, device=dev)
    table[job_edge, job_label.long()] = torch.arange(N, device=dev)
    jid = table.gather(1, lab.reshape(E, -1).long())                        # [E,P] the pixel's job or -1
    on = jid >= 0
    A = rel[jid.clamp(min=0)]                                               # [E,P,7]
    d = ops["disps"][ops["ii"]].reshape(E, -1)
    y, x = torch.meshgrid(torch.arange(HT, device=dev, dtype=torch.float32), torch.arange(WD, device=dev, dtype=torch.float32), indexing="ij")
    z = 1.0 / d
    X = torch.stack([z * ((x.reshape(-1) - cx) / fx), z * ((y.reshape(-1) - cy) / fy), z], -1)
    q, t = A[..., 3:6], A[..., :3]
    uv = 2.0 * torch.cross(q, X, dim=-1)
    Y = X + A[..., 6:7] * uv + torch.cross(q, uv, dim=-1) + t
    tgt = ops["target"].reshape(E, -1, 2)
    on = on & (d > 0) & (Y[..., 2] > z_min) & torch.isfinite(tgt).all(-1)
    iz = 1.0 / Y[..., 2]
    r = torch.stack([fx * Y[..., 0] * iz + cx - tgt[..., 0], fy * Y[..., 1] * iz + cy - tgt[..., 1]], -1)
    ax, ay, zero = fx * iz, fy * iz, torch.zeros_like(iz)
    mx, my = -ax * Y[..., 0] * iz, -ay * Y[..., 1] * iz
    Ju = torch.stack([ax, zero, mx, mx * Y[..., 1], ax * Y[..., 2] - mx * Y[..., 0], -ax * Y[..., 1]], -1)
    Jv = torch.stack([zero, ay, my, my * Y[..., 1] - ay * Y[..., 2], -my * Y[..., 0], ay * Y[..., 0]], -1)
    iu = torch.triu_indices(6, 6, device=dev)
    H = Ju[..., iu[0]] * Ju[..., iu[1]] + Jv[..., iu[0]] * Jv[..., iu[1]]
    b = Ju * r[..., 0:1] + Jv * r[..., 1:2]
    terms = torch.cat([H, b, (r * r).sum(-1, keepdim=True)], -1)
    terms = torch.where(on[..., None], terms, torch.zeros_like(terms)).reshape(-1, 28)
    sums = torch.zeros(N + 1, 28, device=dev).index_add_(0, torch.where(on, jid, torch.full_like(jid, N)).reshape(-1), terms)
    count = torch.zeros(N + 1, device=dev).index_add_(0, torch.where(on, jid, torch.full_like(jid, N)).reshape(-1), torch.ones(E * HT * WD, device=dev))
    return sums[:N], count[:N]


def bound(path, L, names):
    lib = ctypes.CDLL(path)
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return lib


def plain_track(path, L, dev):
    """the plain pvo_tsdf_track (24 slots of 48 x 64 against a 128^3 volume, 4 iterations) through the library at `path`, by ctypes alone"""
    from pvo_amd import droid_backends as db
    lib = bound(path, L, ("pvo_tsdf_track_workspace_bytes", "pvo_tsdf_track"))
    nf, dim = 24, 128
    voxel, origin = 2.56 / dim, (-1.28, -1.28, 0.5)
    poses, disps, intr, _ = make_video(nf, 48, 64, dev)
    ix = torch.arange(nf, device=dev)
    tsdf, wsum = torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, device=dev)
    db.tsdf_integrate(tsdf, wsum, None, poses, disps, intr, ix, origin, voxel, 3.0 * voxel)
    out, info = torch.zeros(nf, 7, device=dev), torch.zeros(nf, 5, 4, device=dev)
    ws = torch.empty(max(lib.pvo_tsdf_track_workspace_bytes(nf, 48, 64), 256), dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    a = L.TsdfTrackArgs()
    a.tsdf, a.wsum = p(tsdf), p(wsum)
    a.nz, a.ny, a.nx = tsdf.shape
    a.origin[0], a.origin[1], a.origin[2] = origin
    a.voxel, a.min_weight = voxel, 1.0
    a.poses, a.disps, a.intrinsics, a.ix = p(poses), p(disps), p(intr), p(ix)
    a.N, a.nframes, a.ht, a.wd, a.iters, a.min_count = nf, nf, 48, 64, 4, 32
    a.band, a.huber, a.lm, a.ep = 0.9, 0.0, 1e-4, 1e-6
    a.poses_out, a.info = p(out), p(info)
    keep = (poses, disps, intr, ix, tsdf, wsum, ws, a)

    def track():
        if lib.pvo_tsdf_track(ctypes.byref(a), p(ws), ws.numel(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) != 0:
            raise RuntimeError("plain tsdf_track failed in " + path)
    return track, (out, info), keep


def alternating(fns, reps, warm=10):
    """name -> sorted microseconds per call.  The order of the calls is reversed every repetition and the whole device is idle before
    each timed call: an update leaves work for the next one on a side stream, which would otherwise be charged to whatever follows it"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {k: [] for k in fns}
    names = list(fns)
    for r in range(reps + warm):
        for name in (names if r % 2 == 0 else names[::-1]):
            torch.cuda.synchronize()
            e0.record()
            fns[name]()
            e1.record()
            e1.synchronize()
            if r >= warm:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: sorted(v) for k, v in times.items()}


def graph_update_child(path, reps):
    """child process: FactorGraph.update (pvo_graph_update) on the window through the library at `path` alone; prints its sorted
    microseconds as one JSON line"""
    from pvo_amd import _lib as L
    import bench
    dev = torch.device("cuda:0")
    probe = ctypes.CDLL(path)
    L._lib = bound(path, L, [n for n in L.SIGNATURES if hasattr(probe, n)])          # (the parent's library lacks the new entry points)
    video, graph = bench.make_window(dev, H8=HT, W8=WD, NKF=NKF, buffer=16)
    if not graph._fused_ok():
        raise SystemExit("the native update path is not active")
    snap = bench.Snapshot(video, graph)

    def run():
        snap.restore()
        graph._ctx_token = None
        graph.update(None, None, use_inactive=True)
    t = alternating({"graph_update": run}, reps)["graph_update"]
    print(json.dumps({"edges": len(graph._ii_h), "us": t}))


def compare_with_parent(parent, reps, dev, lines):
    """pvo_tsdf_track through this build's library and the parent commit's in this process, alternating; FactorGraph.update
    (pvo_graph_update) through each library in a child process of its own, the children alternating (this, parent, this, parent)"""
    from pvo_amd import _lib as L
    probe = ctypes.CDLL(parent)
    assert not hasattr(probe, "pvo_object_motion"), "--parent-lib must be the PARENT commit's library"
    tracks = {"this": plain_track(L.LIB_PATH, L, dev), "parent": plain_track(parent, L, dev)}
    # (a 65 us call: five times the repetitions, or p10 .. p90 of 40 samples is narrower than the drift between two minutes)
    t = {k: stats(v) for k, v in alternating({"this": tracks["this"][0], "parent": tracks["parent"][0]}, 5 * reps).items()}
    same = all(torch.equal(a, b) for a, b in zip(tracks["this"][1], tracks["parent"][1]))
    inside = lambda a, b: b[1] <= a[0] <= b[2] and a[1] <= b[0] <= a[2]
    ok = inside(t["this"], t["parent"])
    lines += ["the untouched calls, this build's library and the parent commit's",
              "  tsdf_track (24 slots of 48 x 64, 4 iterations; one process, %d repetitions, alternating, order reversed every repetition, device idle before each call):" % (5 * reps),
              "    this %9.1f us [%.1f .. %.1f]   parent %9.1f us [%.1f .. %.1f]   each median inside the other's p10 .. p90: %s; outputs %s"
              % (t["this"] + t["parent"] + (ok, "EQUAL" if same else "DIFFER"))]
    runs = {"this": [], "parent": []}
    edges = 0
    for _ in range(3):
        for which, path in (("this", L.LIB_PATH), ("parent", parent)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--graph-update-child", path, "--reps", str(reps)],
                               stdout=subprocess.PIPE, text=True, timeout=240, check=True)
            got = json.loads(r.stdout.strip().splitlines()[-1])
            runs[which].append(got["us"])
            edges = got["edges"]
    g = {k: stats(sorted(sum(v, []))) for k, v in runs.items()}
    # between processes the medians move by more than p10 .. p90 inside one: the spread of a build is also the range of its runs' medians
    med = {k: [stats(x)[0] for x in v] for k, v in runs.items()}
    between = max(max(m) - min(m) for m in med.values())
    ok_g = inside(g["this"], g["parent"]) or abs(g["this"][0] - g["parent"][0]) <= between
    lines += ["  graph_update (FactorGraph.update, %d edges at %d x %d; one child process per library and run, three runs each, alternating this, parent, ... -"
              % (edges, HT, WD),
              "  two copies of the library in ONE process do not measure it: the update overlaps work on the library's own side streams, and the copy loaded",
              "  second ran at 1319 us against 848 us with the same code, presumably for want of a hardware queue):",
              "    this %9.1f us [%.1f .. %.1f] (runs' medians %s)   parent %9.1f us [%.1f .. %.1f] (runs' medians %s)"
              % (g["this"] + (", ".join("%.1f" % x for x in med["this"]),) + g["parent"] + (", ".join("%.1f" % x for x in med["parent"]),)),
              "    this / parent = %.4f; the same build's runs differ by up to %.1f us; each median inside the other's p10 .. p90, or the builds no further apart than that: %s"
              % (g["this"][0] / g["parent"][0], between, ok_g), ""]
    return ok and ok_g and same


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--parent-lib", default=None, help="a libpvo_hip.so built from the parent commit: the untouched calls side by side")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats csv of a rocprofv3 --kernel-trace --stats run of object_motion_workload.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_object_motion.txt"))
    ap.add_argument("--graph-update-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("object_motion_bench needs the GPU (there is no fallback)")
    if args.graph_update_child:
        return graph_update_child(args.graph_update_child, args.reps)
    from pvo_amd import droid_backends as db
    dev = torch.device("cuda:0")
    ops = make_operands(dev)
    E = ops["ii"].shape[0]
    nbytes = sum(ops[k].numel() * ops[k].element_size() for k in ("disps", "labels", "target"))
    lines = ["object_motion_bench on %s: %d keyframes of %d x %d, %d edges, %d segments per keyframe; static segments, targets = reprojection + 0.1 px noise"
             % (torch.cuda.get_device_name(0), NKF, HT, WD, E, GRID * GRID),
             "per call, device events, median [p10 .. p90] of %d repetitions after 5 warm-ups" % args.reps, ""]
    copies = [torch.empty_like(ops[k]) for k in ("disps", "labels", "target")]

    def copy():
        for dst, k in zip(copies, ("disps", "labels", "target")):
            dst.copy_(ops[k])
    for per_edge in (1, 4, 16):
        job_edge = torch.arange(E, device=dev).repeat_interleave(per_edge).contiguous()
        job_label = (1 + torch.arange(per_edge, device=dev, dtype=torch.int32)).repeat(E).contiguous()
        N = job_edge.shape[0]
        call = lambda it, o: db.object_motion(ops["poses"], ops["disps"], ops["intrinsics"], ops["labels"], ops["ii"], ops["jj"], ops["target"],
                                              job_edge, job_label, iters=it, out=o)
        outs = {it: {"rel": torch.empty(N, 7, device=dev), "motion": torch.empty(N, 7, device=dev), "info": torch.empty(N, it + 1, 4, device=dev)}
                for it in (0, 8)}
        call(8, outs[8])
        rel0 = call(0, outs[0])["rel"].clone()
        sums, count = torch_evaluation(ops, job_edge, job_label, rel0)
        agree = float((sums[:, 27] - outs[0]["info"][:, 0, 0]).abs().max() / outs[0]["info"][:, 0, 0].abs().max())
        fns = {"eval": lambda: call(0, outs[0]), "eight": lambda: call(8, outs[8]), "copy": copy,
               "torch": lambda: torch_evaluation(ops, job_edge, job_label, rel0)}
        t = {k: stats(v) for k, v in measure(fns, args.reps).items()}
        info = outs[8]["info"]
        moved = float(info[:, :-1, 2].max(1).values.max())
        lines += ["%d job(s) per edge: %d jobs, %d..%d contributing pixels each; status of the last evaluation %s; largest step %.2e; E falls %.3g -> %.3g"
                  % (per_edge, N, int(info[:, 0, 1].min()), int(info[:, 0, 1].max()), sorted(set(info[:, -1, 3].int().tolist())), moved,
                     float(info[:, 0, 0].sum()), float(info[:, -1, 0].sum())),
                  "    one evaluation, iters = 0 (3 launches)     %10.1f us [%.1f .. %.1f]" % t["eval"],
                  "    iters = 8 (19 launches)                    %10.1f us [%.1f .. %.1f]   %.1f us per evaluation" % (t["eight"] + (t["eight"][0] / 9.0,)),
                  "    copy of disps, labels, target              %10.1f us [%.1f .. %.1f]   %d bytes: evaluation / copy = %.2f"
                  % (t["copy"] + (nbytes, t["eval"][0] / t["copy"][0])),
                  "    one evaluation in torch (index_add_)       %10.1f us [%.1f .. %.1f]   torch / native = %.1f; count equal: %s, E within %.1e (relative)"
                  % (t["torch"] + (t["torch"][0] / t["eval"][0], bool(torch.equal(count, outs[0]["info"][:, 0, 1])), agree)), ""]
    if args.kernel_stats:
        lines += ["per kernel, from a separate rocprofv3 --kernel-trace --stats run of tools/object_motion_workload.py (16 jobs per edge, iters = 8, 20 calls):"]
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                if "motion_" in row.get("Name", ""):
                    name = re.search(r"motion_\w+", row["Name"]).group(0)
                    lines += ["    %-22s calls %6s   average %10.1f ns   min %10s ns   max %10s ns" % (name, row.get("Calls"), float(row.get("AverageNs", 0) or 0),
                                                                                                 row.get("MinNs"), row.get("MaxNs"))]
        lines += [""]
    ok = True
    if args.parent_lib:
        ok = compare_with_parent(args.parent_lib, args.reps, dev, lines)
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print("written to", args.out)
    if not ok:
        raise SystemExit("an untouched call is outside the parent's measured spread, or its outputs differ")


if __name__ == "__main__":
    main()
