"""Where one S-T training step goes (BASELINE.json configs[4] at N = 1: tools/train.py's step, 6 frames 200x400, 20 edges, 15
unrolled updates, bf16 volume, fp32 operator / BA, Adam).   On the GPU box:

    cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats -f csv -d /tmp/ts -- python $GRAFT_REPO_ROOT/tools/prof_train_step.py
    python $GRAFT_REPO_ROOT/tools/prof_train_step.py --summarise /tmp/ts  > gpurun_out/r04_train_step_stats.txt

Without rocprofv3 it prints the step's wall time and the host-side time of its phases (forward / loss / backward / optimizer),
each closed by a device synchronisation.  `--native_ba True` runs the unrolled BA steps in libpvo_hip (pvo_amd.geom.ba_native),
`--native_ba both` alternates the two forms step by step in one process (the same clips for both); PVO_TRAIN_REPS measured steps
(default 3) follow PVO_TRAIN_WARMUP warm-up steps (default 1) per form.  `--native_upsample True | both` does the same for the depth maps'
convex upsampling (pvo_amd.geom.upsample_native); with both switches on `both` the four combinations alternate."""
import csv, glob, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))

if "--summarise" in sys.argv:
    d = sys.argv[sys.argv.index("--summarise") + 1]
    rows = list(csv.DictReader(open(glob.glob(os.path.join(d, "*", "*kernel_stats.csv"))[0])))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    groups = {}
    def group(n):
        if "corr_lookup" in n or "corr_build" in n or "altcorr" in n: return "pvo: correlation (lookup fwd / bwd, volume build)"
        if "ba_train_" in n: return "pvo: training BA (ba_train_*, native_ba)"
        if "se3_" in n: return "pvo: SE3 kernels (forward)"
        if "(anonymous namespace)" in n and "at::" not in n: return "pvo: other HIP kernels"
        if "Cijk_" in n or "gemm" in n.lower() or "ck::" in n or "igemm" in n or "MIOpen" in n or "miopen" in n or "conv" in n.lower(): return "PyTorch: convolutions / GEMMs (MIOpen, hipBLASLt, CK)"
        if "elementwise" in n or "vectorized" in n or "reduce" in n or "index" in n or "gather" in n or "scatter" in n or "cat" in n.lower() or "copy" in n.lower() or "fill" in n.lower(): return "PyTorch: element-wise / reductions / indexing / copies"
        return "other"
    for r in rows:
        g = groups.setdefault(group(r["Name"]), [0, 0.0]); g[0] += int(r["Calls"]); g[1] += float(r["TotalDurationNs"])
    print("kernel time of the profiled steps: %.1f ms in %d launches" % (tot / 1e6, sum(int(r["Calls"]) for r in rows)))
    for k, (c, t) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
        print("  %-70s %8d launches %9.1f ms  %5.1f %%" % (k, c, t / 1e6, 100 * t / tot))
    print("\ntop 25 kernels:")
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:25]:
        print("  %8s x %9.1f us = %8.1f ms  %s" % (r["Calls"], float(r["AverageNs"]) / 1e3, float(r["TotalDurationNs"]) / 1e6, r["Name"][:150]))
    # the native BA's own launches (native_ba=True): its ba_train_* kernels, and of the projective-transform kernels - which the
    # rest of the step launches too - the ones the BA issues: proj_fwd right before ba_train_assemble, proj_vjp right after
    # ba_train_vjp_assemble (one stream: dispatch order = start-time order)
    traces = glob.glob(os.path.join(d, "*", "*kernel_trace.csv"))
    disp = sorted(csv.DictReader(open(traces[0])), key=lambda r: int(r["Start_Timestamp"])) if traces else []
    names = [r["Kernel_Name"] for r in disp]
    own = {}
    for k, r in enumerate(disp):
        n, key = names[k], None
        if "ba_train_" in n:
            key = "ba_train_" + n.split("ba_train_", 1)[1].split("<")[0]
        elif "proj_fwd_kernel" in n and k + 1 < len(disp) and "ba_train_assemble" in names[k + 1]:
            key = "proj_fwd_kernel (the BA's)"
        elif "proj_vjp_kernel" in n and k > 0 and "ba_train_vjp_assemble" in names[k - 1]:
            key = "proj_vjp_kernel (the BA's)"
        elif "proj_fwd_kernel" in n or "proj_vjp_kernel" in n:
            key = ("proj_fwd_kernel" if "proj_fwd_kernel" in n else "proj_vjp_kernel") + " (other projections)"
        if key:
            e = own.setdefault(key, [0, 0.0]); e[0] += 1; e[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    if own:
        print("\nthe native BA's launches and the other projections (per-dispatch trace):")
        for k, (c, t) in sorted(own.items(), key=lambda kv: -kv[1][1]):
            print("  %8d x %9.2f us = %8.3f ms  %s" % (c, t / c / 1e3, t / 1e6, k))
    sys.exit(0)

import torch
import train as T
from pvo_amd.droid_net import DroidNet
from pvo_amd.geom import losses as L
from pvo_amd.geom.graph_utils import build_frame_graph
from pvo_amd.geom.se3 import SE3
from pvo_amd.synthetic import TrainClips

device = torch.device("cuda:0")
args = T.parse_args(["--device", "cuda"])
native = sys.argv[sys.argv.index("--native_ba") + 1] if "--native_ba" in sys.argv else "False"
ups = sys.argv[sys.argv.index("--native_upsample") + 1] if "--native_upsample" in sys.argv else "False"
_sel = {"true": [True], "false": [False], "both": [False, True]}
forms = [(b, u) for b in _sel[native.lower()] for u in _sel[ups.lower()]]          # (native_ba, native_upsample), alternating step by step
torch.manual_seed(0)
net = DroidNet().to(device).train()
opt = torch.optim.Adam(net.parameters(), lr=args.lr, weight_decay=1e-5)
ssim = L.SSIM().to(device)
reps = int(os.environ.get("PVO_TRAIN_REPS", "3"))
warm = int(os.environ.get("PVO_TRAIN_WARMUP", "1"))
clips = TrainClips(6, (200, 400), length=reps + warm)
ph = {form: {"forward": [], "loss": [], "backward": [], "optimizer": [], "step": []} for form in forms}
def lap(t0):
    torch.cuda.synchronize(); return time.perf_counter() - t0
for k in range(reps + warm):
    images, poses, disps, intr, gt_masks, gt_vals, segments = [x[None].to(device) for x in clips[k]]
    graph = build_frame_graph(poses, disps, intr, num=20, need_inv=False)
    for form in forms:
        torch.cuda.synchronize()
        opt.zero_grad()
        Ps = SE3(poses); Gs = SE3.IdentityLike(Ps)
        Gs.data[:, 0] = Ps.data[:, 0]; Gs.data[:, 1:] = Ps.data[:, [1]]
        t0 = time.perf_counter()
        out = net(Gs, images, torch.ones_like(disps[:, :, 3::8, 3::8]), intr / 8.0, graph, num_steps=15, fixedp=2, ret_flow=True,
                  downsample=True, segments=segments, corr_dtype=torch.bfloat16, native_ba=form[0], native_upsample=form[1])
        f = lap(t0); t0 = time.perf_counter()
        loss, _ = T.objective(args, L, out, (images, Ps, disps, intr, gt_masks, gt_vals), graph, ssim, 0)
        l = lap(t0); t0 = time.perf_counter()
        loss.backward()
        b = lap(t0); t0 = time.perf_counter()
        torch.nn.utils.clip_grad_norm_(net.parameters(), args.clip); opt.step()
        o = lap(t0)
        if k >= warm:
            for name, v in (("forward", f), ("loss", l), ("backward", b), ("optimizer", o), ("step", f + l + b + o)):
                ph[form][name].append(v)
import statistics
for form in forms:
    print("S-T training step, native_ba=%s native_upsample=%s (median [min, max] of %d after %d warm-up): " % (form[0], form[1], reps, warm) +
          ", ".join("%s %.1f [%.1f, %.1f] ms" % (k, statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3) for k, v in ph[form].items()))
