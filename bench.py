#!/usr/bin/env python
"""bench.py — VO keyframe updates/sec on the S-B window (BASELINE.json configs[1]).

    python bench.py --gpus N --steps K --warmup W

One STEP = one keyframe update of the frontend on an 8-keyframe window at 512x384 (48x64
maps, 36 edges |i-j|<=3), following droid_frontend.py:36-70 of the reference:
    re-create the newest keyframe's edges  (volume + pyramid build and static GRU terms for 6 edges - on the library's
                                            side stream, beside the rest -, reproject, state rows appended in place)
    frame distances over the window         (proximity search input: the 8 x 8 matrix and one pair, both directions)
    4 graph updates, keyframe-distance test, 2 more graph updates
where one graph update = reproject -> 4-level correlation lookup -> update operator (fp16) ->
mask/weight glue -> dense BA x2 (factor_graph.py:227-307), issued as ONE native call (pvo_graph_update).
Inputs are synthetic (seeded), resident in HBM before the timed region; the update operator has
random-init weights of the reference architecture.  State is restored at the start of every step
so that K steps do identical work (8 device copies inside the timed step that a real run does not have).

N > 1: one process per GPU (torch.distributed, RCCL); every rank tracks its own window
(independent sequences, no data-path collective), value = N*K / max-over-ranks time.

A plain run does what the headline needs and nothing else: set-up, priming, W warm-up steps, the K timed steps, the
JSON line (metric, value, ms_per_step, ...).  --dump-outputs DIR writes what the last timed step computed (step_outputs:
poses, disparities, per-edge state, frame distances) as DIR/<name>.npy; inputs are seeded, so two builds compare file by
file.  Everything below is measured only with --full.

Extra objects on the JSON line with --full: "roofline" for the dominant hand-written HBM-bound kernel (the fused 4-level lookup; its
duration = HIP events around it inside the timed steps minus what an event pair around nothing reads at the same place),
"roofline_wide_conv" (matrix-core roofline of the wide 3x3 convolution, the kernel with the largest share of the step,
with the shader clock the chip sustains under it and inside a step: pvo_clock_probe), "stage_us_in_step", "host",
"workload_S_A" (the reference driver's 30x101 maps), "workload_S_1" (configs[0]: one tools/test_vo2.py clip at 47x156 maps),
"train_step" (configs[4]: one tools/train.py optimizer step at S-T size, bf16 volume), "sequence" (configs[1]'s FULL SEQUENCE: Droid.track
per frame + Droid.terminate on a seeded synthetic 240x808 stream - frames/s, keyframe updates/s, graph updates/s with every stage of the
pipeline in the loop, and the split by component), "edge_sharded" (64-keyframe global
update, edges sharded over the ranks, one integer all-reduce of the pose system's envelope per Gauss-Newton step; at N > 1
with the one-GPU time of the same job and the speed-up against it), "cpu_baseline" (the reference's CPU formulations timed on
this host, rank 0, N=1), "ate_rmse" (synthetic closed loop; ground-truth correspondences stand in for the learned operator -
no weights exist here) and "chained_update_drift" (six native updates against the CPU fp32 chain).  DESIGN.md section 5.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

H8, W8, NKF, RADIUS = 48, 64, 8, 3
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense fp16 / bf16 matrix peak


def s3_segments(H8, W8, frame):
    """S-3: 8 rectangular panoptic instances (ids 1..8; 0 = no segment) on a 2 x 4 grid with a
    background margin; instances 3 and 6 move one pixel per frame"""
    seg = torch.zeros(H8, W8, dtype=torch.int32)
    bh, bw = H8 // 2, W8 // 4
    for n in range(8):
        r, c = divmod(n, 4)
        shift = frame if n + 1 in (3, 6) else 0
        y0, x0 = r * bh + 2, c * bw + 2 + shift
        seg[y0:y0 + bh - 4, max(x0, 0):min(x0 + bw - 4, W8)] = n + 1
    return seg


def make_window(device, seed=0, H8=H8, W8=W8, NKF=NKF, buffer=16, corr_impl="volume", intr=(40.0, 40.0, 32.0, 24.0),
                add_edges=True, max_factors=48, segments=False, thresh=0.8):
    """synthetic keyframe window: S-B by default (8 keyframes, 48x64 maps, edges |i-j| <= 3);
    segments=True: S-3 = S-B + panoptic segments with the vote of factor_graph.py:256-276 switched on"""
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.factor_graph import FactorGraph
    from pvo_amd.geom.se3 import SE3
    from pvo_amd.modules.update import DynamicUpdateModule
    g = torch.Generator().manual_seed(seed)
    video = DepthVideo(image_size=(H8 * 8, W8 * 8), buffer=buffer, device=device, segm_filter=bool(segments), thresh=thresh)
    if segments:
        video.max_segments = 16
    xi = torch.tensor([0.05, 0.0, 0.02, 0.0, 0.01, 0.0])
    low = torch.rand(1, 1, 6, 8, generator=g) * 0.8 + 0.2
    disp_gt = torch.nn.functional.interpolate(low, size=(H8, W8), mode="bilinear", align_corners=True)[0, 0]
    intr = torch.tensor(intr)
    for k in range(NKF):
        video.append(float(k), SE3.exp(max(k - 1, 0) * xi).data.to(device), torch.ones(H8, W8, device=device),
                     intr.to(device), torch.randn(H8, W8, 128, generator=g).half().to(device),
                     torch.tanh(torch.randn(128, H8, W8, generator=g)).half().to(device),
                     torch.relu(torch.randn(128, H8, W8, generator=g)).half().to(device),
                     **(dict(segm=s3_segments(H8, W8, k).to(device)[None]) if segments else {}))
    video.disps[:NKF] = 1.0
    torch.manual_seed(seed)
    update = DynamicUpdateModule().to(device).eval().half()   # fp16 inference weights (the reference runs this module under fp16 autocast)
    graph = FactorGraph(video, update, device=device, max_factors=max_factors, corr_impl=corr_impl)
    graph.nkf = NKF
    if not add_edges:
        return video, graph
    graph.add_neighborhood_factors(0, NKF, r=RADIUS)
    # targets = ground-truth reprojection + noise, so BA has a well-posed problem
    gt_poses = torch.stack([SE3.exp(k * xi).data for k in range(NKF)]).to(device)
    from pvo_amd import droid_backends as db
    c, _ = db.reproject(torch.cat([gt_poses, video.poses[NKF:]]), disp_gt[None].repeat(buffer, 1, 1).to(device).contiguous(),
                        video.intrinsics, graph.ii, graph.jj)
    graph.target_cam = (c + 0.1 * torch.randn(c.shape, generator=g).to(device))[None]
    graph.weight = torch.rand(graph.target_cam.shape, generator=g).to(device)
    return video, graph


class Snapshot:
    """state restored at the start of every step (keeps the K steps identical)"""
    def __init__(self, video, graph):
        self.v, self.g = video, graph
        self.poses, self.disps = video.poses.clone(), video.disps.clone()
        self.net, self.target, self.weight = graph.net.clone(), graph.target_cam.clone(), graph.weight.clone()
        self.raw_mask, self.delta_dy, self.damping = graph.raw_mask.clone(), graph.delta_dy.clone(), graph.damping.clone()

    def restore(self):
        # (the per-edge state - net, targets, weights, masks - is put back by snap_edges_fix AFTER the edge rebuild, in
        # the rebuilt edge order; copying it here as well would only add launches to the timed step)
        torch._foreach_copy_([self.v.poses, self.v.disps, self.g.damping], [self.poses, self.disps, self.damping])


def keyframe_update(video, graph, snap, clock_probe=None):
    """droid_frontend.py:36-70 on a full window (clock_probe: diagnostic hook called after the second graph update)"""
    snap.restore()
    newest = graph.nkf - 1
    pairs = [(i, j) for i, j in zip(graph._ii_h, graph._jj_h) if i == newest or j == newest]
    graph.rm_factors([(i == newest or j == newest) for i, j in zip(graph._ii_h, graph._jj_h)])
    graph.add_factors([p[0] for p in pairs], [p[1] for p in pairs])
    snap_edges_fix(graph, snap)
    d = video.distance(beta=0.3, bidirectional=True)          # NKF x NKF proximity matrix
    for k in range(4):
        graph.update(None, None, use_inactive=True)
        if k == 1 and clock_probe is not None:
            clock_probe()
    dk = video.distance([newest - 2], [newest - 1], beta=0.3, bidirectional=True)
    for _ in range(2):
        graph.update(None, None, use_inactive=True)
    return d, dk


def snap_edges_fix(graph, snap):
    """re-added edges go to the end of the edge list; the restored per-edge state follows the same permutation.  The
    state is copied INTO the graph's tensors (they stay the rows of the graph's own buffers, as in a real run)."""
    names = (("net", "net"), ("target_cam", "target"), ("weight", "weight"), ("raw_mask", "raw_mask"), ("delta_dy", "delta_dy"))
    if not hasattr(snap, "perm"):
        old = snap.edge_list
        snap.perm = torch.tensor([old.index(e) for e in zip(graph._ii_h, graph._jj_h)], device=graph.device)
        snap.permuted = {}
        for gname, sname in names:
            t = torch.empty_like(getattr(graph, gname))
            t.copy_(getattr(snap, sname)[:, snap.perm])
            snap.permuted[gname] = t
    # (one multi-tensor copy: the restore is the benchmark's own work, not the product's - five blits with their gaps before)
    torch._foreach_copy_([getattr(graph, gname) for gname, _ in names], [snap.permuted[gname] for gname, _ in names])


def _host_cpu():
    """(model name, physical cores, logical cpus) of this host"""
    import subprocess
    model, sockets, cps = "unknown", 1, None
    try:
        for line in subprocess.run(["lscpu"], stdout=subprocess.PIPE, text=True, timeout=10).stdout.splitlines():
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "Model name":
                model = v
            elif k == "Socket(s)":
                sockets = int(v)
            elif k == "Core(s) per socket":
                cps = int(v)
    except Exception:
        pass
    logical = os.cpu_count() or 1
    return model, (sockets * cps if cps else logical), logical


def _median_time(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    ts.sort()
    return ts[len(ts) // 2]


def cpu_baseline():
    """The same keyframe update on this host's CPU cores, from the formulations the reference itself would run with its
    CUDA extension disabled (BASELINE.json configs[0]) where it has one:
      volume build   torch.matmul + 3 x avg_pool2d (modules/corr.py:24-38,63-71; pvo_amd.modules.corr.CorrBlock.corr)
      BA             the PyTorch BA (geom/ba.py:31-106; pvo_amd.geom.ba.BA, pinned equal to it), 2 iterations
      update operator the module in fp32 (droid_net.py:256-314)
      lookup         the reference has NO CPU lookup (modules/corr.py:4 imports the CUDA extension unconditionally): the C
                     oracle (a single-threaded port of correlation_kernels.cu:19-70) stands in
    torch threads = physical cores; warm-ups, then the median.  A bounded sample: one graph update's parts, scaled to the
    6 updates + 6 new edges of a keyframe update."""
    import numpy as np
    import torch.nn.functional as F
    from oracle import oracle as O
    from pvo_amd.geom import ba as tba
    from pvo_amd.geom.se3 import SE3
    from pvo_amd.modules.corr import CorrBlock
    from pvo_amd.modules.update import DynamicUpdateModule
    model, cores, logical = _host_cpu()
    torch.set_num_threads(cores)
    g = torch.Generator().manual_seed(0)
    E, HW = 36, H8 * W8
    with torch.no_grad():
        # volume build + pyramid for the 6 edges a keyframe adds (fp32 on the CPU, as configs[0] runs it)
        f1, f2 = torch.randn(1, 6, 128, H8, W8, generator=g), torch.randn(1, 6, 128, H8, W8, generator=g)

        def build():
            c = CorrBlock.corr(f1, f2).reshape(6 * HW, 1, H8, W8)
            pyr = [c]
            for _ in range(3):
                pyr.append(F.avg_pool2d(pyr[-1], 2, stride=2))
            return pyr
        t_build = _median_time(build, 3, 10)
        pyr = [p.view(6, H8, W8, p.shape[-2], p.shape[-1]).numpy() for p in build()]
        # lookup: C oracle, 6 of the 36 edges, scaled
        coords = (np.stack(np.meshgrid(np.arange(W8), np.arange(H8)), -1)[None].astype(np.float32)
                  + np.random.default_rng(0).normal(0, 4, (6, H8, W8, 2)).astype(np.float32))
        t_lookup = _median_time(lambda: O.corr_pyramid_lookup(pyr, coords, 3), 1, 3) * 6
        # update operator, fp32, all 36 edges
        torch.manual_seed(0)
        upd = DynamicUpdateModule().eval()
        a = (torch.randn(1, E, 128, H8, W8, generator=g), torch.randn(1, E, 128, H8, W8, generator=g),
             torch.randn(1, E, 196, H8, W8, generator=g), torch.randn(1, E, 8, H8, W8, generator=g))
        ii = torch.tensor([i for i in range(NKF) for j in range(NKF) if i != j and abs(i - j) <= RADIUS])
        jj = torch.tensor([j for i in range(NKF) for j in range(NKF) if i != j and abs(i - j) <= RADIUS])
        t_upd = _median_time(lambda: upd(*a, ii, None), 1, 3)
        # PyTorch BA, 2 iterations (what FactorGraph.update runs per update), fixedp = 1
        xi = torch.tensor([0.05, 0.0, 0.02, 0.0, 0.01, 0.0])
        poses = SE3(torch.stack([SE3.exp(max(k - 1, 0) * xi).data for k in range(NKF)])[None])
        disps = torch.ones(1, NKF, H8, W8)
        intr = torch.tensor([40.0, 40.0, 32.0, 24.0]).view(1, 1, 4).repeat(1, NKF, 1)
        target = torch.randn(1, E, H8, W8, 2, generator=g) * 2 + torch.stack(torch.meshgrid(
            torch.arange(W8).float(), torch.arange(H8).float(), indexing="xy"), -1)[None, None]
        weight = torch.rand(1, E, H8, W8, 2, generator=g)
        eta = torch.full((1, NKF, H8, W8), 1e-4)

        def ba2():
            p, d = poses, disps
            for _ in range(2):
                p, d = tba.BA(target, weight, eta, p, d, intr, ii, jj, fixedp=1)
        t_ba = _median_time(ba2, 3, 10)
    per_kf = 6 * (t_lookup + t_upd + t_ba) + t_build
    return {"value": 1.0 / per_kf, "unit": "keyframe updates/s", "cores": cores, "kind": "port",
            "host": "%s, %d physical cores / %d logical" % (model, cores, logical),
            "sample": "one graph update's parts, medians after warm-up, scaled to a keyframe update (6 updates + 6 new edges): "
                      "volume build of 6 edges torch.matmul + avg_pool2d fp32 on %d threads %.3fs (median of 10); lookup C oracle "
                      "single thread %.2fs for 36 edges (6 measured, median of 3); update operator torch fp32 on %d threads %.2fs "
                      "(median of 3); PyTorch BA x2 on %d threads %.3fs (median of 10)" % (cores, t_build, t_lookup, cores, t_upd, cores, t_ba),
            "parts_s": {"build_6_edges": t_build, "lookup_36_edges": t_lookup, "update_operator": t_upd, "ba_2_iters": t_ba}}


def synthetic_ate(device, n_frames=120):
    """The ATE half of BASELINE.json's metric, on the only kind of sequence available here (no checkpoint, no dataset): a synthetic
    plane scene at the reference driver's map size (30 x 101 = 240 x 808 / 8) tracked by the REAL DroidFrontend (window of 25 with its
    inactive edges, proximity factors, the keyframe test with its removal branch) and optimised by the REAL DroidBackend (global BA x 2),
    on the HIP kernels, with ground-truth correspondences (+ fixed noise) standing in for the learned operator.  Every third frame of
    the scene barely moves, so the frontend's keyframe test removes it again (droid_frontend.py:54-58).  Sim(3)-aligned translation
    RMSE as test_vo.py:162-163 computes, before and after the global BA.  The same loop against the CPU-oracle path (same keyframe
    decisions, ATE within 1e-3): tests/test_synthetic_vo.py, at 26 frames (the oracle's BA takes ~0.5 s per call at this size)."""
    import numpy as np
    from argparse import Namespace
    from pvo_amd import droid_backends as db
    from pvo_amd.backend import DroidBackend
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.frontend import DroidFrontend
    from pvo_amd.synthetic import OracleFlowOperator, PlaneScene, run_sequence
    from pvo_amd.trajectory import ate_rmse, camera_centres
    scene = PlaneScene(ht=30, wd=101, n_frames=n_frames, seed=0, step=0.06, pattern=(1.0, 1.0, 0.15))
    video = DepthVideo(image_size=(scene.ht * 8, scene.wd * 8), buffer=n_frames + 8, device=device)
    op = OracleFlowOperator(scene, video, lambda p, d, k, i, j: db.reproject(p, d, k, i, j)[0])
    fe = DroidFrontend(op, video, device=device, warmup=8, keyframe_thresh=0.6, frontend_thresh=16.0, frontend_window=25,
                       frontend_radius=2, frontend_nms=1)
    be = DroidBackend(Namespace(update=op), video, Namespace(device=str(device), backend_radius=2, backend_nms=3, backend_thresh=15.0,
                                                             beta=0.3, backend_corr="alt"))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    before, after, frames = run_sequence(scene, video, fe, op, backend=be)
    torch.cuda.synchronize(); el = time.perf_counter() - t0
    gt = camera_centres(scene.poses[frames].numpy())
    length = float(np.abs(np.diff(gt, axis=0)).sum()) if len(frames) > 1 else 0.0
    return {"value": float(ate_rmse(camera_centres(after.numpy()), gt)), "unit": "scene units",
            "ate_rmse_frontend_only": float(ate_rmse(camera_centres(before.numpy()), gt)),
            "trajectory_path_length": float(np.linalg.norm(np.diff(gt, axis=0), axis=1).sum()), "frames": n_frames, "keyframes_kept": len(frames),
            "keyframes_removed_by_the_frontend": int(fe.keyframes_removed), "seconds": el, "finite": bool(torch.isfinite(after).all()),
            "sequence": "synthetic plane scene, 30x101 maps, %d frames (every third barely moves), ground-truth correspondences + 0.05 px noise in "
                        "place of the learned operator; real DroidFrontend (window 25, inactive edges, proximity factors, keyframe removal) + "
                        "DroidBackend (global BA, 7 + 12 steps), HIP BA throughout" % n_frames}


PROBE_EVERY = 5
REMOVAL_RATE = 0.25      # share of the sequence leg's keyframe updates that end in rm_keyframe (seeded schedule)


def timed_steps(video, graph, snap, steps, world, probe_stage="lookup", updates_per_step=6):
    """K keyframe updates bracketed as the driver's contract asks: barrier + synchronize on both sides, max over ranks.
    Returns (elapsed s, host issue time per step, probe readings, what the last step's keyframe_update returned)."""
    from pvo_amd import droid_backends as db
    if probe_stage:
        # HIP events around one kernel, on its stream, in the timed steps: one launch in PROBE_EVERY (co-prime with the updates
        # per step, so every position inside the step is sampled) - the event pair costs the launch stream ~7 us, 2 % of a step
        db.probe_arm(probe_stage, steps * updates_per_step, every=PROBE_EVERY)
    host_issue = []
    last = None
    torch.cuda.synchronize()
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        th = time.perf_counter()
        last = keyframe_update(video, graph, snap)
        host_issue.append(time.perf_counter() - th)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], device=graph.device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    in_step = db.probe_read(steps * updates_per_step) if probe_stage else []
    return elapsed, host_issue, in_step, last


def prime(video, graph, snap, max_blocks=40):
    """untimed priming until the step time has converged (clocks, caches, allocator): blocks of 8 steps until two
    consecutive blocks are within 3 % of the best seen"""
    best, calm, blocks = None, 0, 0
    while calm < 2 and blocks < max_blocks:
        torch.cuda.synchronize(); tb = time.perf_counter()
        for _ in range(8):
            keyframe_update(video, graph, snap)
        torch.cuda.synchronize(); blk = time.perf_counter() - tb
        calm = calm + 1 if (best is not None and blk < 1.03 * best) else 0
        best = blk if best is None else min(best, blk)
        blocks += 1
    return blocks


def scattered_ceiling(device, traffic_bytes, write_bytes, lookup_us):
    """the lookup against the ceiling that actually bounds it: its reads are scattered partial lines (64-byte fetches, counted by
    FETCH_SIZE), which this memory system serves at a REQUEST rate, not at the streaming bandwidth (pvo_mem_probe)"""
    from pvo_amd import droid_backends as db
    g = db.mem_probe_gbps(device)
    if not traffic_bytes:
        return {"probe_gbps": g}
    read = traffic_bytes - write_bytes
    t_us = read / (g["random_64B"] * 1e3) + write_bytes / (g["streaming_128B"] * 1e3)
    return {"probe_gbps": g, "how": "pvo_mem_probe: 1 GiB buffer, 8 independent 16-byte loads in flight per lane, full occupancy; bytes counted as fetched",
            "lookup_read_bytes_64B_fetches": read, "lookup_write_bytes": write_bytes,
            "time_at_ceiling_us": t_us, "frac_of_scattered_ceiling": t_us / lookup_us if lookup_us else None,
            "note": "reads priced at the random-64-byte-line rate (an upper bound on the time: the rate is per line touched, and some of the 64-byte fetches share a line), writes at the streaming rate; `roofline.frac` stays priced on algorithmic bytes against the 8 TB/s peak"}


def lookup_roofline(E, HW, in_step_ms, traffic=None, event_pair_us=None):
    """`achieved` is priced on the kernel's duration = the event reading minus what an event pair around NOTHING reads at the
    same place of the stream (`event_pair_us`, PVO_STAGE_EMPTY, from two extra steps): that is the figure rocprofv3's
    per-kernel average agrees with (profiles/); both readings are in the object.  Without the calibration (None): the raw one."""
    in_us = sorted(1e3 * v for v in in_step_ms)
    raw = sum(in_us) / max(len(in_us), 1)
    us = raw - event_pair_us if event_pair_us is not None and raw > event_pair_us else raw
    alg = E * HW * (4 * 64 * 2 + 8 + 128 * 2)      # taps + coords + (encoded) output, fp16
    ach = alg / (us * 1e-6) / 1e9 if us > 0 else 0.0
    return {"kernel": "corr_lookup_r3_kernel<half, tiled, enc> (4-level lookup + 196->128 encoder layer, 8x8-tiled resident volumes)",
            "bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
            "traffic": traffic, "algorithmic_bytes_per_launch": alg, "avg_launch_us": us, "launches_timed": len(in_us),
            "avg_event_reading_us": raw, "event_pair_around_nothing_us": event_pair_us,
            "timing": "HIP events around the kernel on its launch stream, inside the timed steps (every %dth launch), minus the reading of an event pair around nothing at the same place" % PROBE_EVERY,
            "in_step_us_min_median_max": [in_us[0], in_us[len(in_us) // 2], in_us[-1]] if in_us else None}


def workload_sa(device, steps):
    """S-A: the map shape of the reference's own driver - test_vo.py resizes VKITTI2 frames to 240 x 808, i.e.
    30 x 101 maps (evaluation_scripts/test_vo.py:19,64) - with a 10-keyframe window and the frontend's 48-edge budget
    (|i-j| <= 3: 48 edges).  Same step as S-B; reported next to it, not as `value`."""
    video, graph = make_window(device, seed=1, H8=30, W8=101, NKF=10, intr=(90.0, 90.0, 50.5, 15.0))
    if not graph._fused_ok():
        return {"error": "native update path not active at 30x101"}
    snap = Snapshot(video, graph)
    snap.edge_list = list(zip(graph._ii_h, graph._jj_h))
    prime(video, graph, snap, max_blocks=6)
    elapsed, host_issue, in_step, _ = timed_steps(video, graph, snap, steps, 1)
    E = len(graph._ii_h)
    return {"workload": "S-A: 30x101 maps (test_vo.py's 240x808 input), 10 keyframes, E=%d, itrs=2, synthetic" % E,
            "value": steps / elapsed, "unit": "keyframe updates/s", "ms_per_step": elapsed / steps * 1e3, "steps": steps,
            "graph_updates_per_s": steps * 6 / elapsed, "roofline": lookup_roofline(E, 30 * 101, in_step)}


def workload_s1(device, reps=3):
    """BASELINE.json configs[0] (S-1) on the GPU: one clip of tools/test_vo2.py - 2 frames at 376x1248 (47x156 maps), 2 edges,
    DroidNet.forward with num_steps=15, fixedp=2 (volume build + 15 four-level lookups on the HIP kernels, fp32; a
    depth-only BA), random-init weights.  Wall time per clip, first clip excluded."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import test_vo2 as T
    from pvo_amd.droid_net import DroidNet
    from pvo_amd.synthetic import TrainClips
    torch.manual_seed(0)
    net = DroidNet().to(device).eval()
    clips = TrainClips(2, (376, 1248), length=reps + 1, seed=5, step=0.03)
    ts = []
    for k in range(reps + 1):
        images, poses, disps, intr, gt_masks, gt_vals, _ = [x[None].to(device) for x in clips[k]]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = T.estimate_clip(net, images, poses, intr, gt_vals, num_steps=15)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    # the lookup alone at this map size, in the reference's volume layout (fp32, what DroidNet.forward correlates in)
    from pvo_amd import droid_backends as db
    pyr = [torch.randn(2, 47, 156, 47 >> l, 156 >> l, device=device) for l in range(4)]
    c = (torch.stack(torch.meshgrid(torch.arange(156.0), torch.arange(47.0), indexing="xy"), -1)[None].repeat(2, 1, 1, 1).to(device)
         + 4 * torch.randn(2, 47, 156, 2, device=device)).contiguous()
    for _ in range(3):
        db.corr_pyramid_lookup(pyr, c, 3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        db.corr_pyramid_lookup(pyr, c, 3)
    e1.record(); torch.cuda.synchronize()
    lk_us = e0.elapsed_time(e1) / 20 * 1e3
    lk_bytes = 2 * 47 * 156 * (4 * 64 * 4 + 8 + 196 * 4)
    ms = 1e3 * sorted(ts[1:])[len(ts[1:]) // 2]
    return {"workload": "S-1: BASELINE.json configs[0] on the GPU (tools/test_vo2.py clip: 2 frames 376x1248 -> 47x156 maps, 2 edges, "
                        "num_steps=15, fixedp=2, fp32, random-init weights)", "ms_per_clip": ms, "clips_per_s": 1e3 / ms,
            "lookup_fp32_us": lk_us, "lookup_fp32_gbps": lk_bytes / (lk_us * 1e-6) / 1e9,
            "final_depth_change_mean": float((out["disps"] - 1.0).abs().mean())}


def train_step_leg(device, reps=3):
    """BASELINE.json configs[4] (S-T) at N = 1: one optimizer step of tools/train.py - 6 frames at 200x400 (25x50 maps), the
    20-edge co-visibility graph, 15 unrolled updates, semi-supervised objective, bf16 correlation volume (HIP lookup
    forward + backward), fp32 operator and BA, Adam.  Median wall time of `reps` steps after one warm-up step, and the
    lookup-backward kernel alone at this size."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import train as T
    from pvo_amd import droid_backends as db
    from pvo_amd.droid_net import DroidNet
    from pvo_amd.geom import losses as L
    from pvo_amd.geom.graph_utils import build_frame_graph
    from pvo_amd.geom.se3 import SE3
    from pvo_amd.synthetic import TrainClips
    args = T.parse_args(["--device", "cuda"])
    torch.manual_seed(0)
    net = DroidNet().to(device).train()
    opt = torch.optim.Adam(net.parameters(), lr=args.lr, weight_decay=1e-5)
    ssim = L.SSIM().to(device)
    clips = TrainClips(6, (200, 400), length=reps + 1)
    ts, loss = [], None
    for k in range(reps + 1):
        images, poses, disps, intr, gt_masks, gt_vals, segments = [x[None].to(device) for x in clips[k]]
        graph = build_frame_graph(poses, disps, intr, num=20, need_inv=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad()
        Ps = SE3(poses)
        Gs = SE3.IdentityLike(Ps)
        Gs.data[:, 0] = Ps.data[:, 0]; Gs.data[:, 1:] = Ps.data[:, [1]]
        out = net(Gs, images, torch.ones_like(disps[:, :, 3::8, 3::8]), intr / 8.0, graph, num_steps=15, fixedp=2, ret_flow=True,
                  downsample=True, segments=segments, corr_dtype=torch.bfloat16)
        loss, _ = T.objective(args, L, out, (images, Ps, disps, intr, gt_masks, gt_vals), graph, ssim, 0)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), args.clip)
        opt.step()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    E = sum(len(v) for v in graph.values())
    vol = torch.empty(E, 25, 50, 25, 50, dtype=torch.bfloat16, device=device)
    c = (torch.stack(torch.meshgrid(torch.arange(50.0), torch.arange(25.0), indexing="xy"), 0)[None].repeat(E, 1, 1, 1).to(device)
         + 3 * torch.randn(E, 2, 25, 50, device=device)).contiguous()
    gr = torch.randn(E, 7, 7, 25, 50, device=device).to(torch.bfloat16)
    for _ in range(3):
        db.corr_index_backward(vol, c, gr, 3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        db.corr_index_backward(vol, c, gr, 3)
    e1.record(); torch.cuda.synchronize()
    bw_us = e0.elapsed_time(e1) / 20 * 1e3
    ms = 1e3 * sorted(ts[1:])[len(ts[1:]) // 2]
    return {"workload": "S-T: BASELINE.json configs[4] at N=1 (tools/train.py step: 6 frames 200x400 -> 25x50 maps, %d edges, 15 unrolled "
                        "updates, semisup objective, bf16 volume + HIP lookup fwd/bwd, fp32 operator / BA, Adam), random-init weights" % E,
            "ms_per_step": ms, "steps_per_s": 1e3 / ms, "loss": float(loss.detach()),
            "lookup_backward_level0_us": bw_us, "lookup_backward_level0_gbps": vol.numel() * 2 / (bw_us * 1e-6) / 1e9,
            "data_parallel": "DDP over RCCL, one clip per rank (tools/train.py --gpus 0,1,2,3); gradient all-reduce 17.3 MB per step"}


def chained_drift_leg(device):
    """six chained native graph updates on S-B against the CPU fp32 chain (oracle lookup -> fp32 operator -> oracle BA,
    oracle/chain.py): the drift of poses / depths / flow targets, and the CPU chain's time (the CPU port of the whole update)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import chain
    from test_chained_updates import structured_operator
    video, graph = make_window(device, seed=0)
    structured_operator(graph.update_op, 0.1)
    ov, cg = chain.cpu_twin(video, graph, graph.nkf)
    t_cpu = 0.0
    for _ in range(6):
        graph.update(None, None, use_inactive=True)
        t0 = time.perf_counter()
        cg.update(None, None, use_inactive=True)
        t_cpu += time.perf_counter() - t0
    torch.cuda.synchronize()
    n = graph.nkf
    return {"updates": 6, "operator": "random init, last layer of the two flow heads x 0.1 (sub-pixel revisions)",
            "pose_max_abs": float((video.poses[:n].cpu() - ov.poses[:n]).abs().max()),
            "disp_mean_abs": float((video.disps[:n].cpu() - ov.disps[:n]).abs().mean()),
            "flow_epe_mean_px": float((graph.target_cam.cpu() - cg.target_cam).norm(dim=-1).mean()),
            "reference": "CPU fp32 chain: C-oracle lookup of an fp32 volume -> fp32 update operator (PyTorch) -> C-oracle BA",
            "cpu_chain_s_per_update": t_cpu / 6}


def lookup_traffic():
    """HBM bytes per launch of the fused lookup from the committed PMC profile - only if that profile was taken on THIS source
    of the kernel (it records the sha256 of corr_lookup.hip); otherwise None: a counter value is not carried over a code change"""
    import hashlib
    sha = hashlib.sha256(open(os.path.join(ROOT, "pvo_amd", "csrc", "corr_lookup.hip"), "rb").read()).hexdigest()
    for name in ("r06_lookup_pmc.json", "r05_lookup_pmc.json", "r04_lookup_pmc.json", "r03_lookup_pmc.json", "r02_lookup_pmc.json"):
        path = os.path.join(ROOT, "profiles", name)
        if not os.path.exists(path):
            continue
        j = json.load(open(path))
        if j.get("kernel_source_sha256") in (None, sha):
            return j.get("fused_encoder", j).get("hbm_bytes_per_launch"), {"file": "profiles/" + name, "kernel_source_sha256": j.get("kernel_source_sha256"),
                                                                            "matches_this_source": j.get("kernel_source_sha256") == sha}
    return None, None


def measure_lookup_traffic(timeout_s=150):
    """HBM bytes per launch of the fused lookup MEASURED IN THIS RUN: two rocprofv3 passes (--pmc FETCH_SIZE, --pmc WRITE_SIZE; kernel trace
    only, as /opt/skills/guides/MI355X_MICROARCH.md prescribes) over tools/pmc_lookup.py in child processes - the S-B lookup with the
    Infinity Cache evicted between launches, and a 512 MiB copy whose known traffic calibrates both counters (on gfx950 FETCH_SIZE
    reports half the bytes of 16-byte-per-lane reads).  Returns (bytes per launch, details) or (None, why)."""
    import csv, glob, shutil, subprocess, tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, {"error": "rocprofv3 not found"}
    med = lambda v: sorted(v)[len(v) // 2]
    raw = {}
    tmp = tempfile.mkdtemp(prefix="pvo_pmc_", dir="/tmp")
    try:
        for C in ("FETCH_SIZE", "WRITE_SIZE"):
            d = os.path.join(tmp, C)
            r = subprocess.run([exe, "--pmc", C, "--kernel-trace", "-f", "csv", "-d", d, "--", sys.executable, os.path.join(ROOT, "tools", "pmc_lookup.py")],
                               cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=timeout_s)
            files = glob.glob(os.path.join(d, "*", "*counter_collection.csv"))
            if r.returncode != 0 or not files:
                return None, {"error": "rocprofv3 --pmc %s failed (rc %d)" % (C, r.returncode), "tail": r.stdout[-300:]}
            for row in csv.DictReader(open(files[0])):
                if row.get("Counter_Name") != C:
                    continue
                k = row["Kernel_Name"]
                name = "lookup_enc" if "corr_lookup_r3_enc_kernel" in k else ("copy" if ("copy" in k.lower() or "CatArrayBatchedCopy" in k) else None)
                if name == "copy" and float(row["Counter_Value"]) < 1e5:
                    name = None
                if name:
                    raw.setdefault(name, {}).setdefault(C, []).append(float(row["Counter_Value"]))
    except Exception as e:                                          # noqa: BLE001 (timeout, missing tool, unreadable output)
        return None, {"error": repr(e)}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    try:
        cf, cw = med(raw["copy"]["FETCH_SIZE"]), med(raw["copy"]["WRITE_SIZE"])
        f, w = med(raw["lookup_enc"]["FETCH_SIZE"]), med(raw["lookup_enc"]["WRITE_SIZE"])
    except KeyError as e:
        return None, {"error": "counter rows missing: %r" % (e,), "kernels_seen": sorted(raw)}
    fcorr, wcorr = 512 * 1024 / cf, 512 * 1024 / cw                 # counters in KB; the calibration copy moved 512 MiB each way
    rd, wr = f * 1024 * fcorr, w * 1024 * wcorr
    return rd + wr, {"measured_in_this_run": True, "how": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes, kernel trace only) over tools/pmc_lookup.py; "
                     "median of %d launches, Infinity Cache evicted before each; corrected by the 512 MiB calibration copy of the same passes" % len(raw["lookup_enc"]["FETCH_SIZE"]),
                     "hbm_read_bytes_per_launch": rd, "hbm_write_bytes_per_launch": wr, "fetch_correction": fcorr, "write_correction": wcorr,
                     "read_requests_64B_per_launch": rd / 64.0, "write_requests_64B_per_launch": wr / 64.0,
                     "FETCH_SIZE_raw_KB": f, "WRITE_SIZE_raw_KB": w}


def edge_sharded_leg(device, rank, world, steps=3):
    """BASELINE.json configs[3] / north star "partition the factor graph across GPUs with RCCL all-reduce of the pose-block
    Hessian": a 64-keyframe global update (droid_backend.py:25-41 -> FactorGraph.update_lowmem) whose edges are sharded BY
    SOURCE KEYFRAME over the ranks (pvo_amd/parallel.py).  Per Gauss-Newton step ONE collective: all-reduce (integer sum)
    of the ENVELOPE of the reduced pose system; lookup, update operator, damping and depth updates are rank-local.  Strong
    scaling: the same graph at every N - and, at N > 1, every rank first runs the WHOLE graph alone on its GPU, so that the
    line carries the speed-up against one GPU measured in the same job (`speedup_vs_one_gpu`, global update and BA only).
    Reports global updates/s, the BA-only time, the all-reduce latency and a bitwise cross-rank check of the poses."""
    import torch.distributed as dist
    from pvo_amd.parallel import ShardedBA, shard_edges
    nkf, H, W = 64, H8, W8
    corr_impl = os.environ.get("PVO_BENCH_GLOBAL_CORR", "volume")      # "alt": the reference's alt-corr path
    ii = [i for i in range(nkf) for j in range(nkf) if i != j and abs(i - j) <= RADIUS]
    jj = [j for i in range(nkf) for j in range(nkf) if i != j and abs(i - j) <= RADIUS]

    def sync(collective):
        torch.cuda.synchronize()
        if collective and world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def run(ii_l, jj_l, collective):
        """the global update over the given edges; collective=False: this process alone (no group communication)"""
        video, graph = make_window(device, seed=7, NKF=nkf, buffer=80, corr_impl=corr_impl, add_edges=False, max_factors=-1)
        video.counter = nkf
        graph.add_factors(ii_l, jj_l)
        g = torch.Generator().manual_seed(3)
        # (per-edge noise drawn for the WHOLE graph and indexed by edge, so that shards and the whole graph see the same values)
        noise = 0.5 * torch.randn(len(ii), H, W, 2, generator=g)
        wts = torch.rand(len(ii), H, W, 2, generator=g)
        pos = {e: k for k, e in enumerate(zip(ii, jj))}
        sel = torch.tensor([pos[e] for e in zip(graph._ii_h, graph._jj_h)])
        graph.target_cam = graph.target_cam + noise[sel].to(device)[None]
        graph.weight = wts[sel].to(device)[None].contiguous()
        sharded = ShardedBA(structure=(ii, jj), communicate=collective)
        poses0, disps0 = video.poses.clone(), video.disps.clone()
        net0, tgt0, w0 = graph.net.clone(), graph.target_cam.clone(), graph.weight.clone()

        def reset():
            video.poses.copy_(poses0); video.disps.copy_(disps0)
            graph.net, graph.target_cam, graph.weight = net0.clone(), tgt0.clone(), w0.clone()
            graph.raw_mask.zero_(); graph.delta_dy.zero_()
        graph.update_lowmem(steps=1, sharded=sharded)                 # warm-up
        reset(); sync(collective)
        t0 = time.perf_counter()
        graph.update_lowmem(steps=steps, sharded=sharded)
        sync(collective)
        el = time.perf_counter() - t0
        poses_after = video.poses.clone()
        # BA only: the same sharded BA on the final state, 10 calls of 2 Gauss-Newton steps
        src = sorted(set(graph._ii_h))
        rows = sorted(set(range(1, nkf)) | set(src))
        eta = torch.full((len(rows), H, W), 1e-4, device=device)
        target = graph.target_cam.view(-1, H, W, 2).permute(0, 3, 1, 2).contiguous()
        weight = graph.weight.view(-1, H, W, 2).permute(0, 3, 1, 2).contiguous()
        bi, bj = graph.ii.contiguous(), graph.jj.contiguous()
        ba = lambda: sharded.ba(video.poses, video.disps, video.intrinsics[0], target, weight, eta, bi, bj, 1, nkf, itrs=2,
                                lm=1e-5, ep=1e-2, plan_key=("bench", rank, collective))
        ba(); sync(collective)
        t0 = time.perf_counter()
        for _ in range(10):
            ba()
        sync(collective)
        ba_ms = (time.perf_counter() - t0) / 10 * 1e3
        msg_bytes = sharded.last_message_bytes
        # the part of those two steps that SHARDS (assembly + Schur elimination of this rank's edges: pvo_ba_local) timed alone; the
        # rest - envelope, conversion, the pose solve, back-substitution of the pose update - every rank repeats
        local_ms = None
        if world == 1 or not collective:
            from pvo_amd import droid_backends as db
            sysb, wsb = sharded._sys, sharded._ws[1]
            pi, pj = sharded._plan_edges

            def loc():
                db.ba_local(video.poses, video.disps, video.intrinsics[0], target, weight, eta, pi, pj, 1, nkf, False, sysb, wsb)      # (clears sys itself)
            loc(); sync(False)
            t0 = time.perf_counter()
            for _ in range(20):
                loc()
            sync(False)
            local_ms = 2.0 * (time.perf_counter() - t0) / 20 * 1e3
            sysb.zero_()
        del graph, video
        torch.cuda.empty_cache()
        return el, ba_ms, poses_after, msg_bytes, local_ms

    whole = None
    if world > 1:
        # every rank alone on the whole graph (identical work on every GPU): the one-GPU reference of this job
        whole = run(ii, jj, False)
    ii_l, jj_l, _ = shard_edges(ii, jj, world, rank)
    if not ii_l:
        raise RuntimeError("rank %d owns no edges" % rank)
    el, ba_ms, poses_after, msg_bytes, local_ms = run(ii_l, jj_l, True)
    # the collective alone: the envelope message, 50 all-reduces
    P = nkf - 1
    dense_bytes = 8 * ((6 * P) ** 2 + 6 * P)
    ar_us = None
    one_rank = None
    if world == 1 and os.environ.get("PVO_BENCH_RCCL_ONE_RANK", "1") == "1":
        # No second GPU here: the collective of the edge-sharded BA still runs through RCCL on a ONE-rank group - the int64
        # envelope message, on the BA's stream, between pvo_ba_local and pvo_ba_finish (ShardedBA.collective_at_one) - so that the
        # path the 8-GPU run takes is executed (ordering, dtype, message size) and its latency floor is on record.
        try:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29577")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)
            try:
                video, graph = make_window(device, seed=7, NKF=nkf, buffer=80, corr_impl=corr_impl, add_edges=False, max_factors=-1)
                video.counter = nkf
                graph.add_factors(ii, jj)
                H_, W_ = graph.ht, graph.wd
                g = torch.Generator().manual_seed(3)
                target = (graph.target_cam + 0.5 * torch.randn(len(ii), H_, W_, 2, generator=g).to(device)[None]).view(-1, H_, W_, 2).permute(0, 3, 1, 2).contiguous()
                weight = torch.rand(len(ii), H_, W_, 2, generator=g).to(device).permute(0, 3, 1, 2).contiguous()
                eta = torch.full((nkf, H_, W_), 1e-4, device=device)
                bi, bj = graph.ii.contiguous(), graph.jj.contiguous()
                res = {}
                for name, on in (("plain", False), ("rccl", True)):
                    sb = ShardedBA(structure=(ii, jj))
                    sb.always_pack, sb.collective_at_one = True, on
                    p_, d_ = video.poses.clone(), video.disps.clone()
                    run_ba = lambda: sb.ba(p_, d_, video.intrinsics[0], target, weight, eta, bi, bj, 1, nkf, itrs=2, lm=1e-5, ep=1e-2, plan_key=("one", name))
                    run_ba(); torch.cuda.synchronize()
                    p_.copy_(video.poses); d_.copy_(video.disps)
                    run_ba(); torch.cuda.synchronize()
                    first = p_.clone()
                    t0 = time.perf_counter()
                    for _ in range(10):
                        run_ba()
                    torch.cuda.synchronize()
                    res[name] = ((time.perf_counter() - t0) / 10 * 1e3, first, sb.last_message_bytes)
                msg = torch.zeros(max(res["rccl"][2] // 8, 1), dtype=torch.int64, device=device)
                for _ in range(5):
                    dist.all_reduce(msg)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(50):
                    dist.all_reduce(msg)
                torch.cuda.synchronize()
                one_rank = {"backend": dist.get_backend(), "world_size": 1, "allreduce_us": (time.perf_counter() - t0) / 50 * 1e6,
                            "allreduce_bytes": int(res["rccl"][2]), "ba_2_steps_ms_with_the_collective": res["rccl"][0],
                            "ba_2_steps_ms_packed_message_no_collective": res["plain"][0],
                            "message_packing": "library (pvo_ba_pack -> all-reduce -> pvo_ba_finish_packed): no torch launch in between",
                            "poses_bitwise_equal_with_and_without_the_collective": bool(torch.equal(res["rccl"][1], res["plain"][1]))}
                del graph, video
                torch.cuda.empty_cache()
            finally:
                dist.destroy_process_group()
        except Exception as e:                                       # noqa: BLE001
            one_rank = {"error": repr(e)}
    if world > 1:
        msg = torch.zeros(max(msg_bytes // 8, 1), dtype=torch.int64, device=device)
        for _ in range(5):
            dist.all_reduce(msg)
        sync(True)
        t0 = time.perf_counter()
        for _ in range(50):
            dist.all_reduce(msg)
        torch.cuda.synchronize()
        ar_us = (time.perf_counter() - t0) / 50 * 1e6
    # every rank must hold bit-identical poses - and, the pose system being an integer sum, the poses of the whole graph on one GPU
    same, same_as_whole = True, None
    if world > 1:
        ref = poses_after.clone()
        dist.broadcast(ref, 0)
        flag = torch.tensor([1 if torch.equal(ref, poses_after) else 0, 1 if torch.equal(whole[2], poses_after) else 0], device=device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        same, same_as_whole = bool(flag[0].item()), bool(flag[1].item())
    out = {"workload": "S-20: 64 keyframes, 48x64 maps, %d edges (|i-j| <= 3) sharded by source keyframe, global update "
                       "(%s + update operator + BA x2), strong scaling"
                       % (len(ii), "resident volume pool, one native call per step" if corr_impl == "volume" else "alt-corr lookup, 8-frame operator chunks"),
           "correlation": corr_impl,
           "global_updates_per_s": steps / el, "ms_per_global_update": el / steps * 1e3, "edges_this_rank": len(ii_l),
           "ba_2_steps_ms": ba_ms, "allreduce_us": ar_us, "allreduce_bytes": int(msg_bytes) if world > 1 else None,
           "allreduce_bytes_dense": dense_bytes, "allreduce_message": "envelope blocks of the lower triangle + rhs, int64 fixed point",
           "backend": dist.get_backend() if world > 1 else None, "world_size": world, "poses_bitwise_equal_across_ranks": same}
    one_ba, one_local = (ba_ms, local_ms) if world == 1 else (whole[1], whole[4])
    if one_local is not None and one_ba > 0:
        rep = max(one_ba - one_local, 0.0)
        out["ba_only_ceiling"] = {
            "one_gpu_ba_2_steps_ms": one_ba, "sharded_part_ms": one_local, "replicated_part_ms": rep,
            "speedup_bound_at_n_gpus": {str(n): one_ba / (one_local / n + rep) for n in (2, 4, 8)},
            "note": "BA alone CANNOT reach north_star's >= 6x at 8 GPUs with a replicated pose solve: assembly + Schur elimination shard by "
                    "edge (sharded_part), the envelope / conversion / pose solve / retraction run on every rank (replicated_part), and each "
                    "step adds one latency-bound all-reduce that this bound leaves out.  The >= 6x figure to read is "
                    "speedup_vs_one_gpu.global_update (lookup + operator + BA), measured at N > 1 in the same job"}
    if one_rank is not None:
        out["rccl_one_rank"] = one_rank
    if world > 1:
        tt = torch.tensor([el, ba_ms, whole[0], whole[1]], device=device, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        el, ba_ms, w_el, w_ba = [float(x) for x in tt.tolist()]
        out["global_updates_per_s"] = steps / el; out["ms_per_global_update"] = el / steps * 1e3
        out["ba_2_steps_ms"] = ba_ms
        out["one_gpu_same_job"] = {"ms_per_global_update": w_el / steps * 1e3, "ba_2_steps_ms": w_ba}
        out["speedup_vs_one_gpu"] = {"global_update": w_el / el, "ba_only": w_ba / ba_ms, "n_gpus": world}
        out["poses_bitwise_equal_to_one_gpu"] = same_as_whole
    return out


_REAL_STDOUT = None


class _Split:
    """wall-clock split of a run by component: every wrapped call is bracketed by device synchronisations (the instrumented
    pass is therefore slower than the plain one - it apportions the time, the plain pass gives the rate)"""
    def __init__(self):
        self.t, self.n, self.stack = {}, {}, []

    def wrap(self, obj, name, key):
        fn = getattr(obj, name)
        split = self

        def timed(*a, **kw):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            split.stack.append(0.0)
            try:
                return fn(*a, **kw)
            finally:
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                inner = split.stack.pop()
                split.t[key] = split.t.get(key, 0.0) + dt - inner            # exclusive time: nested wrapped calls are subtracted
                split.n[key] = split.n.get(key, 0) + 1
                if split.stack:
                    split.stack[-1] += dt
        setattr(obj, name, timed)


def _sequence_pass(device, n_frames, filter_thresh, keyframe_thresh, split=None, record=None, terminate=True, seed=0, removal_rate=0.0, pipelined=False):
    """tools/test_vo.py's loop (evaluation_scripts/test_vo.py:88-108) on the synthetic stream: Droid.track per frame, then
    terminate (backend x2 + trajectory filler)"""
    from pvo_amd.droid import Droid, default_args
    from pvo_amd.synthetic import drifting_texture_stream
    torch.manual_seed(seed)
    args = default_args(device=str(device), image_size=[240, 808], buffer=max(64, n_frames + 40), segm_filter=True, thresh=0.8,
                        filter_thresh=filter_thresh, keyframe_thresh=keyframe_thresh, pipelined=pipelined)
    droid = Droid(args)
    fe, mf = droid.frontend, droid.filterx
    counts = {"keyframe_updates": 0, "keyframes_removed": 0, "graph_updates": 0}
    upd, rmk = fe._update_begin, fe.graph.rm_keyframe      # (_update_begin: the first half of a keyframe update, in either order of the tracker)

    def _upd():
        counts["keyframe_updates"] += 1
        return upd()

    def _rmk(ix):
        counts["keyframes_removed"] += 1
        return rmk(ix)
    fe._update_begin, fe.graph.rm_keyframe = _upd, _rmk
    if removal_rate > 0:
        # the frontend's keyframe test compares distances between poses a RANDOM network produced (chaotic): its branch is driven by a
        # seeded schedule instead - decision k is fixed for the k-th keyframe update of every pass (DroidFrontend.keyframe_decision);
        # the distance is still computed and read back
        import random
        rng = random.Random(1234 + seed)
        sched = [rng.random() < removal_rate for _ in range(4 * n_frames + 64)]
        fe.keyframe_decision = lambda k, dist: sched[k]
    gupd = fe.graph.update

    windows = []

    def _gupd(*a, **kw):
        counts["graph_updates"] += 1
        r = gupd(*a, **kw)
        st = fe.graph._cache.get("fused")
        if st is not None and counts["graph_updates"] == 600 and os.environ.get("PVO_BENCH_DUMP_BA"):      # (tools/ba_kernel_timeline.py BA_DUMP=...)
            v = fe.graph.video
            torch.save({k: (x.detach().cpu() if torch.is_tensor(x) else x) for k, x in dict(
                poses=v.poses, disps=v.disps, intr=v.intrinsics[0], target=st["target_ba"], weight=st["weight_ba"], ii=st["ii_ba"], jj=st["jj_ba"],
                t0=st["key"][1], t1=st["key"][2], rows=st["frames"], damping=fe.graph.damping).items()}, os.environ["PVO_BENCH_DUMP_BA"])
        if st is not None and counts["graph_updates"] % 50 == 0:          # what a BA of this run looks like (host lists only)
            g = fe.graph
            m_l = [(i >= st["key"][1] - 3) and (j >= st["key"][1] - 3) for i, j in zip(g._ii_inac_h, g._jj_inac_h)]
            src = list(g._ii_h) + [i for i, k in zip(g._ii_inac_h, m_l) if k]
            deg = {}
            for i in src:
                deg[i] = deg.get(i, 0) + 1
            windows.append({"poses": st["key"][2] - st["key"][1], "active_edges": len(g._ii_h), "inactive_edges_in_ba": st["n_in"],
                            "max_out_degree": max(deg.values()), "depth_frames": len(deg)})
        return r
    fe.graph.update = _gupd
    from pvo_amd.factor_graph import FactorGraph as _FG
    backend_graphs = []
    lowmem = _FG.update_lowmem

    def _lowmem(graph, *a, **kw):
        backend_graphs.append({"edges": len(graph._ii_h), "keyframes": int(graph.video.counter), "correlation": graph.corr_impl})
        return lowmem(graph, *a, **kw)
    _FG.update_lowmem = _lowmem
    if record is not None:                       # calibration pass: the two quantities the thresholds are compared with
        op, dist = mf.update, droid.video.distance

        def _op(*a, **kw):
            out = op(*a, **kw)
            record["motion"].append(float(out[1][..., 0:2].float().norm(dim=-1).mean()))
            return out

        def _dist(ii=None, jj=None, **kw):
            d = dist(ii, jj, **kw)
            if ii is not None and len(ii) == 1:
                record["keyframe_distance"].append(float(d.reshape(-1)[0]))
            return d
        mf.update, droid.video.distance = _op, _dist
    if split is not None:
        # (the graphed calls, not the modules: a device synchronisation inside a captured region is illegal)
        split.wrap(mf, "_features_g", "encoders (fnet, cnet)"); split.wrap(mf, "_context_g", "encoders (fnet, cnet)")
        split.wrap(mf, "track", "motion filter (volume + lookup + operator + test)")
        split.wrap(fe.graph, "add_proximity_factors", "edge bookkeeping + proximity (distance matrix, add / rm factors, volume build)")
        split.wrap(fe.graph, "rm_factors", "edge bookkeeping + proximity (distance matrix, add / rm factors, volume build)")
        split.wrap(fe.graph, "rm_keyframe", "edge bookkeeping + proximity (distance matrix, add / rm factors, volume build)")
        split.wrap(fe.graph, "update", "frontend graph updates")
        split.wrap(fe, "_initialize", "frontend initialisation (12-keyframe bootstrap)")
        split.wrap(fe, "_update", "frontend other (keyframe test .item(), pose / depth seed)")
        split.wrap(droid, "backend", "backend (global BA x2)")
        split.wrap(droid, "traj_filler", "trajectory filler")
    frames = list(drifting_texture_stream(n_frames, seed=seed))
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for t, image, intr, segm in frames:
        droid.track(t, image, intrinsics=intr, segments=segm)
    droid.flush()                              # (pipelined: the last keyframe update's second half)
    torch.cuda.synchronize(); t_track = time.perf_counter() - t0
    out = dict(counts, ba_windows_sampled=windows, frames=n_frames, keyframes=int(droid.video.counter), track_s=t_track,
               edges_at_end=len(fe.graph._ii_h), finite=bool(torch.isfinite(droid.video.poses[:droid.video.counter]).all()))
    try:
        if terminate:
            # where the HOST spends terminate (no synchronisation added: a call's time is what it blocks the host for - allocation of the
            # global graph's volume pool, read-backs - the device work it queued may finish later, inside a later entry)
            host = {}

            def _timed(obj, name, label):
                f = getattr(obj, name)

                def g(*a, **kw):
                    t = time.perf_counter()
                    try:
                        return f(*a, **kw)
                    finally:
                        host[label] = host.get(label, 0.0) + time.perf_counter() - t
                setattr(obj, name, g)
            if split is None:
                _timed(droid.backend, "_connect_all", "backend: connect (proximity edges, volume pool)")
                _timed(droid, "_release_cached_memory", "release cached memory")
                _timed(droid, "traj_filler", "trajectory filler")
                _timed(_FG, "update_lowmem", "backend: graph updates (host side)")
            t0 = time.perf_counter()
            traj = droid.terminate(iter(frames), need_inv=True)
            host["all, to the last read-back"] = time.perf_counter() - t0
            torch.cuda.synchronize(); out["terminate_s"] = time.perf_counter() - t0
            out["terminate_host_s"] = {k: round(v, 4) for k, v in host.items()}
            out["trajectory_rows"] = int(traj.shape[0]); out["finite"] = out["finite"] and bool((traj == traj).all())
            out["trajectory"] = traj
            out["backend_graphs"] = backend_graphs
    finally:
        _FG.update_lowmem = lowmem
    del droid      # (the allocator keeps its blocks: the next pass's volume pools come out of the cache, as a second sequence in one process would)
    return out


def sequence_leg(device, n_frames=160, instrumented=True, cprofile=None, reps=3, order="both"):
    """The run the metric is named after (BASELINE.json configs[1] "full sequence"; evaluation_scripts/test_vo.py:88-164): a seeded
    synthetic 240 x 808 stream with panoptic segments through Droid.track per frame and Droid.terminate (backend x2 + filler), random-
    init weights.  No checkpoint exists here, so a random network decides which frames become keyframes.  To keep the run REPRODUCIBLE
    the stream is built so that the decision is not a coin toss: every fourth frame drifts 1 pixel, the others 9, and the one-step flow
    magnitudes of the two kinds form two tight clusters (0.2005 +- 0.0008 / 0.2045 +- 0.0006 with the seeded weights) - the motion
    filter's threshold is put half way between them on a 48-frame warm-up pass, so a quarter of the frames is dropped by the filter and
    three quarters become keyframes.  The frontend's keyframe test compares distances of poses a random network produced (0.04 .. 3,
    chaotic): its outcome follows a SEEDED schedule instead (REMOVAL_RATE of the keyframe updates end in rm_keyframe + the counter /
    t1 roll-back, droid_frontend.py:54-58; the others get their 4 + 2 graph updates) - the distance is still computed and read back.  Three
    passes: warm-up + calibration, plain (the rates), instrumented (the split; device synchronisations around every component)."""
    rec = {"motion": [], "keyframe_distance": []}
    _sequence_pass(device, min(n_frames, 48), 0.0, 0.0, record=rec, terminate=True)
    mo = sorted(rec["motion"])
    low, high = mo[:max(len(mo) // 5, 1)], mo[len(mo) // 2:]
    f_th, k_th = 0.5 * (sum(low) / len(low) + sum(high) / len(high)), 0.0
    if cprofile:
        import cProfile, io, pstats
        pr = cProfile.Profile()
        pr.enable()
    plain = _sequence_pass(device, n_frames, f_th, k_th, removal_rate=REMOVAL_RATE, pipelined=(order == "pipelined"))   # (order != "both": profiling runs, one order only)
    if cprofile:
        pr.disable()
        buf = io.StringIO()
        pstats.Stats(pr, stream=buf).sort_stats("cumulative").print_stats(70)
        pstats.Stats(pr, stream=buf).sort_stats("tottime").print_stats(45)
        for fn in ("as_tensor", "'to' of", "'item' of", "'cpu' of", "'tolist' of"):
            pstats.Stats(pr, stream=buf).sort_stats("tottime").print_callers(fn)
        with open(cprofile, "w") as f:
            f.write(buf.getvalue())
    # the same sequence through the PIPELINED tracker (Droid(args.pipelined=True): the second half of a keyframe update runs inside the
    # next track() call, behind the next frame's encoder launch): same operations in the same dependency order - the trajectory must be
    # bit-identical to the plain pass's.  The two orders alternate, three passes each: the boxes' hosts are shared, a pass half of
    # whose time is host work moves by 20 % when a neighbour is busy (seen: 95 and 120 frames/s minutes apart on one box) - the MEDIAN
    # pass of each order is reported, every sample listed.
    import numpy as np
    pipe = _sequence_pass(device, n_frames, f_th, k_th, removal_rate=REMOVAL_RATE, pipelined=True) if order == "both" else plain
    same = bool(plain.get("trajectory") is not None and pipe.get("trajectory") is not None and
                np.array_equal(plain["trajectory"], pipe["trajectory"]))
    plains, pipes = [plain], [pipe]
    for _ in range(reps - 1 if order == "both" else 0):
        plains.append(_sequence_pass(device, n_frames, f_th, k_th, removal_rate=REMOVAL_RATE))
        pipes.append(_sequence_pass(device, n_frames, f_th, k_th, removal_rate=REMOVAL_RATE, pipelined=True))
        same = same and np.array_equal(plains[0]["trajectory"], plains[-1]["trajectory"]) and np.array_equal(plains[0]["trajectory"], pipes[-1]["trajectory"])
    e2e = lambda p: p["track_s"] + p.get("terminate_s", 0.0)
    samples = {"frames_per_s": [round(p["frames"] / p["track_s"], 2) for p in plains],
               "frames_per_s_end_to_end": [round(p["frames"] / e2e(p), 2) for p in plains],
               "terminate_s": [round(p.get("terminate_s", 0.0), 3) for p in plains],
               "pipelined_frames_per_s": [round(p["frames"] / p["track_s"], 2) for p in pipes],
               "pipelined_frames_per_s_end_to_end": [round(p["frames"] / e2e(p), 2) for p in pipes],
               "order": "plain, pipelined, plain, pipelined, plain, pipelined"}
    plain = sorted(plains, key=e2e)[len(plains) // 2]
    pipe = sorted(pipes, key=e2e)[len(pipes) // 2]
    sp = _Split()
    inst = _sequence_pass(device, n_frames, f_th, k_th, split=sp, removal_rate=REMOVAL_RATE) if instrumented else {"track_s": float("nan")}
    total = sum(sp.t.values())
    return {"workload": "synthetic 240x808 stream (30x101 maps), %d frames, panoptic segments (segm_filter), random-init weights; "
                        "tools/test_vo.py's loop: Droid.track per frame, terminate = backend(7) + backend(12) + trajectory filler" % n_frames,
            "calibration": {"motion_first_32": [round(x, 4) for x in rec["motion"][:32]], "keyframe_distance": [round(x, 4) for x in rec["keyframe_distance"][:24]]},
            "thresholds": {"filter_thresh": f_th, "keyframe_thresh": k_th,
                           "how": "filter: half way between the two clusters of one-step flow magnitudes on a 48-frame warm-up pass (1-pixel and 9-pixel frames); keyframe test: seeded schedule, see keyframe_removal"},
            "frames_per_s": plain["frames"] / plain["track_s"],
            "frames_per_s_end_to_end": plain["frames"] / (plain["track_s"] + plain.get("terminate_s", 0.0)),
            "keyframe_removal": {"rate_scheduled": REMOVAL_RATE, "removed": plain["keyframes_removed"], "keyframe_updates": plain["keyframe_updates"],
                                 "how": "seeded decision per keyframe update through DroidFrontend.keyframe_decision (the distance is still computed and read back): rm_keyframe + the counter / t1 roll-back of droid_frontend.py:54-58 are in the timed loop"},
            "keyframe_updates_per_s": plain["keyframe_updates"] / plain["track_s"],
            "pipelined": {"what": "Droid(args.pipelined=True), same stream and schedule: frame t + 1's graph is launched before the second half of "
                                  "keyframe t's frontend update; results lag by half an update between calls (flush() at the end is in the time)",
                          "frames_per_s": pipe["frames"] / pipe["track_s"],
                          "frames_per_s_end_to_end": pipe["frames"] / (pipe["track_s"] + pipe.get("terminate_s", 0.0)),
                          "keyframe_updates_per_s": pipe["keyframe_updates"] / pipe["track_s"],
                          "keyframe_updates": pipe["keyframe_updates"], "keyframes_removed": pipe["keyframes_removed"],
                          "terminate_s": pipe.get("terminate_s"), "trajectories_identical_in_all_six_passes": bool(same)},
            "samples": samples,
            "graph_updates_per_s": plain["graph_updates"] / plain["track_s"],
            "ms_per_keyframe_update_all_in": 1e3 * plain["track_s"] / max(plain["keyframe_updates"], 1),
            "ba_windows_sampled": plain.get("ba_windows_sampled"), "terminate_s": plain.get("terminate_s"), "terminate_host_s": plain.get("terminate_host_s"), "backend_graphs": plain.get("backend_graphs"), "counts": {k: plain[k] for k in ("frames", "keyframes", "keyframe_updates", "keyframes_removed", "graph_updates", "edges_at_end", "trajectory_rows")},
            "finite": plain["finite"],
            "split_instrumented_pass": {"note": "exclusive wall time per component with a device synchronisation on both sides of every call (this pass: %.2f s of tracking against %.2f s plain)" % (inst["track_s"], plain["track_s"]),
                                        "seconds": {k: round(v, 4) for k, v in sorted(sp.t.items(), key=lambda kv: -kv[1])},
                                        "calls": sp.n, "share": {k: round(v / total, 3) for k, v in sorted(sp.t.items(), key=lambda kv: -kv[1])} if total else None}}


def _own_stdout():
    """Everything that any library writes to file descriptor 1 during the run goes to stderr instead (RCCL prints a five-line version
    banner to stdout when a process group comes up, from C, flushed at exit - i.e. AFTER the result line); the ONE JSON line of the
    contract is written to the original descriptor by emit()."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def emit(obj):
    line = (json.dumps(obj) + "\n").encode()
    sys.stdout.flush()
    os.write(_REAL_STDOUT if _REAL_STDOUT is not None else 1, line)


DUMP_LIMIT_BYTES = 64 << 20
NET_SAMPLE = 1 << 20        # hidden-state values kept by --dump-outputs (the whole state: 36 x 128 x 48 x 64 = 14.2 M)


def step_outputs(video, graph, last):
    """What a caller of the keyframe update receives from the last timed step, as float32 / float64 numpy arrays: the window's
    poses and disparities after the bundle adjustments, the per-edge state the next update starts from (edge list, targets,
    confidence weights, raw mask, dynamic-flow term; the hidden state as a fixed seeded sample of NET_SAMPLE values in logical
    [edge, channel, row, column] order), the per-frame damping, and the two frame-distance results."""
    def f(t):
        a = t.detach().cpu().numpy()
        return a if a.dtype.name in ("float32", "float64") else a.astype("float32")
    n = graph.nkf
    d, dk = last
    net = graph.net.reshape(-1)
    pick = torch.randint(net.numel(), (min(NET_SAMPLE, net.numel()),), generator=torch.Generator().manual_seed(0))
    return {"poses": f(video.poses[:n]), "disps": f(video.disps[:n]), "damping": f(graph.damping[:n]),
            "edges": f(torch.stack([graph.ii, graph.jj])), "target": f(graph.target_cam), "weight": f(graph.weight),
            "raw_mask": f(graph.raw_mask), "delta_dy": f(graph.delta_dy), "net_sample": f(net[pick.to(net.device)]),
            "distance_matrix": f(d), "distance_pair": f(dk)}


def write_outputs(dirname, arrays):
    """arrays -> dirname/<name>.npy (refuses more than DUMP_LIMIT_BYTES in all)"""
    import numpy as np
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise ValueError("outputs of %d bytes exceed the %d-byte dump limit" % (total, DUMP_LIMIT_BYTES))
    for name, a in arrays.items():
        if a.dtype.name not in ("float32", "float64"):
            raise ValueError("%s: dtype %s, the dump holds float32 / float64 only" % (name, a.dtype))
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def self_launch(n):
    """run this script as n ranks of one node and return the launcher's exit status"""
    import socket
    import subprocess
    with socket.socket() as sk:                      # a free port for the rendezvous
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # (dmabuf IPC: RCCL between processes needs it on these hosts)
    if env.get("PVO_BENCH_BACKEND", "nccl") == "nccl" and torch.cuda.device_count() < n:
        sys.stderr.write("bench.py --gpus %d: this node shows %d GPU(s); RCCL needs one device per rank "
                         "(PVO_BENCH_BACKEND=gloo runs the ranks as a dry run on the devices there are)\n" % (n, torch.cuda.device_count()))
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=120, help="timed keyframe updates (default 120: a timed region of ~0.5 s; the driver passes its own)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--full", action="store_true", help="after the headline steps, also measure everything else the line can carry: "
                    "four more blocks of K steps, per-stage and per-kernel (roofline) figures, the S-A / S-1 / training / full-sequence / "
                    "edge-sharded legs, the CPU baseline, the synthetic ATE and the CPU-chain drift.  Without it a run sets up, primes, "
                    "warms up, times the K steps and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed (step_outputs) as "
                    "DIR/<name>.npy, float32 / float64, at most 64 MB; inputs are seeded, so two builds can be compared file by file")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline, the synthetic ATE and the drift leg")
    ap.add_argument("--no-pmc", action="store_true", help="with --full: do not measure roofline.traffic in this run (two rocprofv3 --pmc "
                    "child passes, ~1 min); the committed profile of the same kernel source is reported instead")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the S-A, S-1, training, sequence and edge-sharded legs")
    ap.add_argument("--sequence-reps", type=int, default=3, help="passes per order of the full-sequence leg (the median pass is reported)")
    ap.add_argument("--sequence-order", choices=("both", "plain", "pipelined"), default="both",
                    help="profiling runs: trace one order of the tracker only (with --sequence-reps 1: calibration pass + one pass)")
    ap.add_argument("--sequence-only", action="store_true", help="run only the full-sequence leg (Droid.track / terminate on the synthetic "
                    "240x808 stream) and print its object: the command tools/sequence_timeline.sh profiles")
    ap.add_argument("--sequence-frames", type=int, default=160)
    ap.add_argument("--sequence-plain", action="store_true", help="with --sequence-only: skip the instrumented pass (profiler runs)")
    ap.add_argument("--sequence-cprofile", default=None, help="with --sequence-only: host profile (cProfile) of the plain pass -> this file")
    ap.add_argument("--steps-only", action="store_true", help="priming, warm-up and the timed steps ONLY (for profilers: no stage probes, no "
                    "isolated kernel loops, no measurement kernels); prints a reduced line")
    args = ap.parse_args()
    # (behind the parser: --help and argument errors keep the real stdout.  Descriptor 1 is NOT handed back afterwards: RCCL's
    # banner sits in a C stdio buffer that is flushed at exit, and must not land behind the result line)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` by itself: re-launch as N ranks, one per GPU, through torch.distributed.run (static rendezvous on
        # 127.0.0.1 - the container's host name may not resolve); rank 0 of the children prints the ONE line, this process only
        # forwards their output and exit status (non-zero if any rank failed).
        raise SystemExit(self_launch(args.gpus))
    _own_stdout()
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("bench.py --gpus %d inside a job of WORLD_SIZE=%d" % (args.gpus, world))
    local = local % max(torch.cuda.device_count(), 1)      # (a 2-process dry run on a 1-GPU box shares device 0)
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        import torch.distributed as dist
        torch.set_num_threads(max(1, (os.cpu_count() or 8) // world))      # N host processes share the cores
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("PVO_BENCH_BACKEND", "nccl")              # "nccl" is RCCL on ROCm; "gloo" for the dry run above
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)

    from pvo_amd import _lib
    from pvo_amd import droid_backends as db
    _lib.load()                                         # fail loudly if the HIP library is missing
    if args.sequence_only:
        emit({"sequence": sequence_leg(device, args.sequence_frames, instrumented=not args.sequence_plain, cprofile=args.sequence_cprofile,
                                       reps=args.sequence_reps, order=args.sequence_order)})
        return
    video, graph = make_window(device, seed=rank)
    if not graph._fused_ok():
        raise SystemExit("the native update path is not active")
    snap = Snapshot(video, graph)
    snap.edge_list = list(zip(graph._ii_h, graph._jj_h))

    # Untimed priming until the step time has converged (no library needs a solver search any more: every kernel of the
    # step is in libpvo_hip), then W warm-up steps, then exactly K timed steps.
    blocks = prime(video, graph, snap)
    for _ in range(args.warmup):
        keyframe_update(video, graph, snap)
    updates_per_step = 6
    # (the lookup's in-step event pairs feed only the --full roofline: a plain run times its steps without them)
    probe = "lookup" if args.full or args.steps_only else None
    elapsed, host_issue, in_step_lookup, last = timed_steps(video, graph, snap, args.steps, world, probe_stage=probe)
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, step_outputs(video, graph, last))

    if args.steps_only:
        if rank == 0:
            emit(({"metric": "VO keyframe updates/sec (steps only: profiler run)", "value": world * args.steps / elapsed,
                              "unit": "keyframe updates/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                              "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
                              "note": "bench.py --steps-only: the timed loop of the default run and nothing behind it"}))
        return
    if rank == 0:
        hi = sorted(host_issue)
        out = {
            "metric": "VO keyframe updates/sec (8-keyframe window, 512x384, 36 edges; 6 graph updates + edge rebuild per keyframe)",
            "value": world * args.steps / elapsed, "unit": "keyframe updates/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f16 (volume, lookup, update operator) / f32 (BA assembly) / f64 (pose solve)",
            "data": "synthetic",
            "config": {"workload": "S-B: BASELINE.json configs[1] window (8 keyframes, 48x64 maps, E=36, itrs=2), synthetic",
                       "edges": len(graph._ii_h), "graph_updates_per_step": updates_per_step, "parallelism": "independent window per GPU",
                       "update_path": "pvo_graph_update: one native call per graph update, no MIOpen / hipBLASLt"},
            "graph_updates_per_s": world * args.steps * updates_per_step / elapsed,
            "host": {"issue_ms_per_step_median": 1e3 * hi[len(hi) // 2], "issue_ms_per_step_max": 1e3 * hi[-1],
                     "priming_blocks_of_8_steps": blocks},
        }
    if not args.full:
        if rank == 0:
            emit(out)
        if world > 1:
            dist.destroy_process_group()
        return

    # --full: the same K steps four more times (each bracketed like the first): `value` is the FIRST block, as the contract
    # defines it; the five block times say whether a 3 % move between two runs is the code or the box
    block_ms = [elapsed / args.steps * 1e3]
    for _ in range(4):
        el_b, _, _, _ = timed_steps(video, graph, snap, args.steps, world, probe_stage=None)
        block_ms.append(el_b / args.steps * 1e3)
    # per-stage durations inside the step, from a few extra untimed steps (one probe at a time)
    stage_us = {}
    for stage in ("gates", "candidate", "ba", "update", "empty"):
        db.probe_arm(stage, 2 * updates_per_step)
        for _ in range(2):
            keyframe_update(video, graph, snap)
        v = db.probe_read(2 * updates_per_step)
        stage_us[stage] = 1e3 * sum(v) / max(len(v), 1)

    # the dominant HBM-bound kernel on the bench's own inputs, as the step launches it (lookup fused with the first
    # encoder layer).  COLD: the 0.9 GB volume pool never fits the 256 MB Infinity Cache inside a step, but identical
    # back-to-back launches would be served from it, so the cache is evicted (by a 600 MB read) before every timed launch
    # and each launch gets its own pair of HIP events on the launch stream.
    coords1, _ = video.reproject(graph.ii, graph.jj)
    pw = graph.update_op.packed_weights(torch.float16)
    c1 = coords1[0].contiguous()
    launch = lambda: db.corr_lookup_encode_tiled(graph.corr.levels, c1, pw.tensors["enc0_w"], pw.tensors["enc0_b"],
                                                 slots=graph.corr.slots_tensor())
    flush = torch.zeros(150 * 1024 * 1024, dtype=torch.float32, device=device)      # 600 MB
    for _ in range(3):
        launch()
    cold = []
    for _ in range(20):
        flush.max()             # a 600 MB READ evicts the cache with clean lines (a fill would leave dirty lines to write back)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); launch(); e1.record()
        cold.append((e0, e1))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(50):
        launch()
    ev1.record()
    torch.cuda.synchronize()
    lookup_cold_us = sum(a.elapsed_time(b) for a, b in cold) / len(cold) * 1e3
    lookup_b2b_us = ev0.elapsed_time(ev1) / 50 * 1e3
    del flush

    # the kernel with the largest share of the step's GPU time: the wide 3x3 convolution, here as the ConvGRU gate launch
    # (320 -> 256 channels + sigmoid epilogue) at the step's own shape, back to back (its inputs are cache-warm in the step too)
    Eg = len(graph._ii_h)
    gn = torch.tanh(torch.randn(Eg, H8, W8, 128, device=device)).half().permute(0, 3, 1, 2)
    gc = torch.relu(torch.randn(Eg, H8, W8, 192, device=device)).half().permute(0, 3, 1, 2)
    gw = (torch.randn(9, 256, 320, device=device) * 0.02).half()
    gg = torch.randn(Eg, 384, device=device)
    gp = torch.randn(Eg, H8, W8, 256, device=device).half().permute(0, 3, 1, 2)
    # ... and the clock the chip holds meanwhile: MI355X trades clock for power, and this kernel is power-limited - one probe
    # wave (pvo_clock_probe) on a second stream reads shader cycles against the 100 MHz counter while the launches run;
    # the same launches on zero-filled operands (no switching in the multipliers) show what the instruction stream
    # itself sustains
    side = torch.cuda.Stream(device=device)

    def gates_run(n, zero):
        a = [torch.zeros_like(t) if zero else t for t in (gn, gc, gw, gg, gp)]
        for _ in range(3):
            db.gru_conv_gates(*a)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        clk = None
        for i in range(n):
            db.gru_conv_gates(*a)
            if i == 4:
                side.wait_stream(torch.cuda.current_stream())          # (starts beside the fifth launch, not before the first)
                clk = db.clock_probe(side, iters=4000)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3, db.clock_ghz(clk)
    torch.cuda.synchronize()
    idle_clk = db.clock_probe(side, iters=4000)
    torch.cuda.synchronize()
    idle_ghz = db.clock_ghz(idle_clk)
    gates_us, gates_ghz = gates_run(20, False)
    gates_zero_us, gates_zero_ghz = gates_run(20, True)

    # what the vendor's GEMM sustains on this box under the same conditions (random fp16 operands, back to back, the clock the
    # chip holds meanwhile): the gate convolution's own implicit-GEMM shape [E*H*W, 9*320] x [9*320, 256] - with none of the
    # convolution's halo handling, segment gathers or GRU epilogue - and a large square one (the guide's 1.25 PFLOP/s figure)
    def gemm_run(M, K, N, n=20):
        A = torch.randn(M, K, device=device).half()
        Bm = torch.randn(K, N, device=device).half()
        for _ in range(3):
            torch.matmul(A, Bm)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        clk = None
        for i in range(n):
            torch.matmul(A, Bm)
            if i == 4:
                side.wait_stream(torch.cuda.current_stream())
                clk = db.clock_probe(side, iters=4000)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / n * 1e3
        return {"shape": [M, K, N], "us": us, "tflops": 2.0 * M * K * N / (us * 1e-6) / 1e12, "frac": 2.0 * M * K * N / (us * 1e-6) / 1e12 / MFMA_PEAK_TFLOPS,
                "shader_clock_ghz": db.clock_ghz(clk)}
    try:
        vendor_gemm = {"same_shape_as_the_gate_convolution": gemm_run(Eg * H8 * W8, 9 * 320, 256), "square_8192": gemm_run(8192, 8192, 8192, n=10),
                       "library": "hipBLASLt / rocBLAS through torch.matmul, fp16, random operands, back to back"}
    except Exception as e:
        vendor_gemm = {"error": repr(e)}
    gates_flop = 2.0 * Eg * H8 * W8 * 9 * 320 * 256
    # the clock inside a full step (probe beside the third graph update of an extra, untimed step)
    step_clk = []
    for _ in range(2):
        keyframe_update(video, graph, snap, clock_probe=lambda: step_clk.append(db.clock_probe(side, iters=4000)))
    torch.cuda.synchronize()
    step_ghz = sum(db.clock_ghz(c) for c in step_clk) / max(len(step_clk), 1)
    del gn, gc, gw, gg, gp

    if rank == 0:
        E, HW = len(graph._ii_h), H8 * W8
        traffic, traffic_src = (None, None)
        if world == 1 and not args.no_pmc:
            torch.cuda.empty_cache()
            traffic, traffic_src = measure_lookup_traffic()
        if traffic is None:                                         # (no profiler here: the committed, sha-guarded profile of the same source)
            why = traffic_src
            traffic, traffic_src = lookup_traffic()
            if traffic_src is not None and why is not None:
                traffic_src = dict(traffic_src, in_run_measurement=why)
        try:
            scat = scattered_ceiling(device, traffic, E * HW * 128 * 2, 1e3 * sum(in_step_lookup) / max(len(in_step_lookup), 1))
        except Exception as e:
            scat = {"error": repr(e)}
        out.update({
            "step_ms_blocks": {"blocks_of_steps": args.steps, "ms_per_step": block_ms, "median": sorted(block_ms)[len(block_ms) // 2],
                               "min": min(block_ms), "max": max(block_ms), "spread_pct": 100.0 * (max(block_ms) - min(block_ms)) / min(block_ms),
                               "note": "five consecutive blocks of K steps, each barrier + synchronize bracketed; `value` is the first"},
            "roofline": dict(lookup_roofline(E, HW, in_step_lookup, traffic, stage_us.pop("empty", None)), isolated_cold_us=lookup_cold_us,
                             isolated_cold="Infinity Cache evicted by a 600 MB read before each of 20 launches",
                             warm_back_to_back_us=lookup_b2b_us, traffic_source=traffic_src, scattered_lines=scat),
            "roofline_wide_conv": {
                "kernel": "conv3x3_big_kernel<half> as pvo_gru_conv_gates (3x3 convolution 320 -> 256 on v_mfma_f32_32x32x16_f16 + sigmoid gates)",
                "bound": "mfma", "achieved": gates_flop / (stage_us["gates"] * 1e-6) / 1e12, "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": gates_flop / (stage_us["gates"] * 1e-6) / 1e12 / MFMA_PEAK_TFLOPS, "flop_per_launch": gates_flop,
                "avg_launch_us": stage_us["gates"], "launches_timed": 2 * updates_per_step,
                "timing": "HIP events around the kernel on its launch stream, inside two extra (untimed) steps of the same loop",
                "isolated_back_to_back_us": gates_us, "isolated_frac": gates_flop / (gates_us * 1e-6) / 1e12 / MFMA_PEAK_TFLOPS,
                "shader_clock_ghz": {"idle": idle_ghz, "under_this_kernel_random_operands": gates_ghz,
                                     "under_this_kernel_zero_operands": gates_zero_ghz, "inside_a_step": step_ghz,
                                     "how": "pvo_clock_probe: one wave on a second stream, s_memtime cycles / s_memrealtime"},
                "zero_operands_us": gates_zero_us, "zero_operands_frac": gates_flop / (gates_zero_us * 1e-6) / 1e12 / MFMA_PEAK_TFLOPS,
                "frac_of_peak_at_sustained_clock": gates_flop / (gates_us * 1e-6) / 1e12 / (MFMA_PEAK_TFLOPS * gates_ghz / 2.4),
                "note": "power-limited: on random operands the chip drops from 2.4 GHz to the clock above, and the dense peak scales with it",
                "vendor_gemm": vendor_gemm,
                "share_of_update_time": stage_us["gates"] / stage_us["update"] if stage_us["update"] else None},
            "stage_us_in_step": dict(stage_us, lookup=1e3 * sum(in_step_lookup) / max(len(in_step_lookup), 1)),
        })
    # second workload and the edge-sharded mode: reported beside the headline, never part of `value`
    extra = {}
    if not args.no_extras:
        if world == 1:
            for key, leg in (("workload_S_A", lambda: workload_sa(device, max(10, min(args.steps // 2, 30)))), ("workload_S_1", lambda: workload_s1(device)),
                             ("train_step", lambda: train_step_leg(device)),
                             ("sequence", lambda: sequence_leg(device, args.sequence_frames))):
                try:
                    extra[key] = leg()
                except Exception as e:      # a failure here must not cost the headline line
                    extra[key] = {"error": repr(e)}
                torch.cuda.empty_cache()
        try:
            extra["edge_sharded"] = edge_sharded_leg(device, rank, world)
        except Exception as e:
            extra["edge_sharded"] = {"error": repr(e)}
    if rank == 0:
        out.update(extra)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
            out["ate_rmse"] = synthetic_ate(device)
            try:
                out["chained_update_drift"] = chained_drift_leg(device)
            except Exception as e:
                out["chained_update_drift"] = {"error": repr(e)}
        emit(out)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
