"""The live volume: the first measurement of pvo_tsdf_reintegrate / pvo_tsdf_sparse_reintegrate and of LiveMap.update on the MI355X.

    python tools/tsdf_reintegrate_bench.py [--reps 30] [--frames 64] [--dim 256] [--parent-lib <the parent commit's libpvo_hip.so>]
                                           [--out profiles/r27_tsdf_reintegrate.txt]

tools/tsdf_bench.py's scene (64 keyframes at 48 x 64 in front of a plane with a sphere, random images) fused into a dim^3 volume with
colours, and into a brick volume over the same world.  8 of the 64 keyframes are then moved by a voxel, and per call - between two
device events, median and 10th .. 90th percentile of `reps` repetitions after 5 warm-ups - are measured:
  (a) one fused re-integration: the 8 removed as they were and added as they are, one pass over the volume
  (b) the same as two calls, remove-only then add-only: two passes
  (c) fusing all 64 from scratch (pvo_tsdf_integrate), what a stale volume costs to rebuild
  (d) a device-to-device copy of the volume's bytes: what reading and writing the volume once costs
  (e) LiveMap.update end to end (wall clock around a synchronised call: map_points, the weights, drift, the read-back, the native call,
      the snapshots) with 8 keyframes moved, at 64 and at 512 fused keyframes
Every repetition moves the 8 keyframes the other way, so the volume stays the scene's.  No time is fixed in advance: this is where the
numbers are first written down.
--parent-lib: the kernels this round must not have changed - pvo_tsdf_integrate, pvo_tsdf_sparse_integrate, pvo_tsdf_mesh and
pvo_tsdf_render - through both libraries, alternated in one process: medians with p10 .. p90 and the sha256 of everything they write.
The hashes must be EQUAL and each median must lie inside the other build's p10 .. p90; the tool says so and exits with 1 otherwise.
Needs the GPU: there is no fallback."""
import argparse
import ctypes
import hashlib
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tsdf_bench import make_video, measure, stats  # noqa: E402


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is not None:
            h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def moved(poses, which, voxel):
    out = poses.clone()
    out[which, 0] += voxel
    return out


def wall(fn, reps, warm=5):
    """sorted wall-clock microseconds of fn(rep), the device idle before and after"""
    times = []
    for r in range(reps + warm):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(r)
        torch.cuda.synchronize()
        if r >= warm:
            times.append((time.perf_counter() - t0) * 1e6)
    return sorted(times)


def live_map_figures(nf, dim, voxel, origin, dev, reps):
    from pvo_amd.depth_video import DepthVideo
    from pvo_amd.live_map import LiveMap
    ht, wd = 48, 64
    poses, disps, intr, images = make_video(nf, ht, wd, dev)
    video = DepthVideo((8 * ht, 8 * wd), nf + 8, dev, store_images=True)
    video.poses[:nf], video.disps[:nf], video.intrinsics[:nf] = poses, disps, intr
    video.tstamp[:nf] = torch.arange(nf, device=dev, dtype=torch.float32)
    video.images[:nf, :, 3::8, 3::8] = images
    video.counter = nf
    lm = LiveMap(video, voxel, origin, (dim, dim, dim), thresh=0.1, lag=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    first = lm.update()
    torch.cuda.synchronize()
    t_first = (time.perf_counter() - t0) * 1e6
    which = torch.arange(nf // 16, nf, nf // 8, device=dev)[:8]
    counts = []

    def step(r):
        video.poses[which, 0] += voxel if r % 2 == 0 else -voxel
        counts.append(lm.update())
    t = wall(step, reps)
    idle = wall(lambda r: lm.update(), reps)
    refreshed = sorted(c[1] for c in counts)
    return first, t_first, stats(t), stats(idle), (refreshed[0], refreshed[len(refreshed) // 2], refreshed[-1])


def compare_with_parent(path, args, lines):
    """pvo_tsdf_integrate / _sparse_integrate / _mesh / _render through this build and the parent's, alternated; returns True if the
    hashes are equal and each median lies inside the other's p10 .. p90"""
    from pvo_amd import _lib, droid_backends as db
    from pvo_amd.tsdf_sparse import SparseTSDF
    this = _lib.load()
    parent = ctypes.CDLL(os.path.abspath(path))
    for name, (res, argtypes) in _lib.SIGNATURES.items():
        if hasattr(parent, name):
            fn = getattr(parent, name)
            fn.restype, fn.argtypes = res, argtypes
    assert not hasattr(parent, "pvo_tsdf_reintegrate"), "--parent-lib must be the PARENT commit's library"
    libs = {"this": this, "parent": parent}
    dev = torch.device("cuda:0")
    nf, dim = args.frames, args.dim
    voxel = 2.56 / dim
    trunc, origin = 3.0 * voxel, (-1.28, -1.28, 0.5)
    ht, wd = 48, 64
    poses, disps, intr, images = make_video(nf, ht, wd, dev)
    ix = torch.arange(nf, device=dev)
    vol = [torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, 3, device=dev)]
    bricks = SparseTSDF(origin, (dim // 8,) * 3, voxel, trunc, colours=True, device=dev, cap=4096)
    bricks.allocate(poses, disps, intr, ix)
    views = torch.arange(0, nf, max(nf // 16, 1), device=dev)
    mesh_out = None

    def on(lib, fn):
        def run():
            _lib._lib = libs[lib]
            try:
                return fn()
            finally:
                _lib._lib = this
        return run

    def integrate():
        db.tsdf_integrate(vol[0], vol[1], vol[2], poses, disps, intr, ix, origin, voxel, trunc, images=images, img_stride=1, img_offset=0)

    def sparse_integrate():
        bricks.integrate(poses, disps, intr, ix, images=images, img_stride=1, img_offset=0)

    def mesh():
        db.tsdf_mesh_into(vol[0], vol[1], vol[2], origin, voxel, 1.0, mesh_out)

    render_out = {}

    def render():
        render_out.update(db.tsdf_render(vol[0], vol[1], vol[2], origin, voxel, poses, intr, views, ht, wd))

    def zero():
        for t in vol + [bricks.tsdf, bricks.wsum, bricks.rgb]:
            t.zero_()

    hashes = {}
    for lib in libs:                                                    # one clean run each for the bytes
        zero()
        on(lib, integrate)()
        on(lib, sparse_integrate)()
        m = on(lib, lambda: db.tsdf_mesh(vol[0], vol[1], vol[2], origin, voxel, min_weight=1.0))()
        mesh_out = {k: torch.zeros_like(v) for k, v in m.items()}
        on(lib, mesh)()
        on(lib, render)()
        torch.cuda.synchronize()
        hashes[lib] = {"integrate": sha(*vol), "sparse_integrate": sha(bricks.tsdf, bricks.wsum, bricks.rgb, bricks.coord, bricks.grid),
                       "mesh": sha(*[mesh_out[k] for k in sorted(mesh_out)]), "render": sha(*[render_out[k] for k in sorted(render_out)])}
    # which build goes first changes with every repetition: the second call of a pair finds the first one's lines in the caches, and a
    # fixed order would put that on one build's account
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ops = (("integrate", integrate), ("sparse_integrate", sparse_integrate), ("mesh", mesh), ("render", render))
    t = {(name, lib): [] for name, _ in ops for lib in libs}
    for r in range(2 * args.reps + 6):
        for name, fn in ops:
            for lib in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
                run = on(lib, fn)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                if r >= 6:
                    t[(name, lib)].append(e0.elapsed_time(e1) * 1e3)
    t = {k: sorted(v) for k, v in t.items()}
    ok = True
    lines += ["", "kernels this round must not have changed, this build against %s, alternated in one process:" % path]
    for name in ("integrate", "sparse_integrate", "mesh", "render"):
        a, b = stats(t[(name, "this")]), stats(t[(name, "parent")])
        same = hashes["this"][name] == hashes["parent"][name]
        inside = b[1] <= a[0] <= b[2] and a[1] <= b[0] <= a[2]
        ok = ok and same and inside
        lines.append("  %-17s this %9.1f us [%.1f .. %.1f]   parent %9.1f us [%.1f .. %.1f]   sha256 %s / %s: %s; medians inside the other's p10 .. p90: %s"
                     % ((name,) + a + b + (hashes["this"][name], hashes["parent"][name], "EQUAL" if same else "DIFFERENT", "yes" if inside else "NO")))
    return ok


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_tsdf_reintegrate.txt"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_reintegrate_bench needs the GPU (there is no fallback)")
    from pvo_amd import droid_backends as db
    from pvo_amd.tsdf_sparse import SparseTSDF
    dev = torch.device("cuda:0")
    nf, dim = args.frames, args.dim
    voxel = 2.56 / dim
    trunc, origin = 3.0 * voxel, (-1.28, -1.28, 0.5)
    ht, wd = 48, 64
    poses, disps, intr, images = make_video(nf, ht, wd, dev)
    every = torch.arange(nf, device=dev)
    which = torch.arange(nf // 16, nf, nf // 8, device=dev)[:8]
    poses2 = moved(poses, which, voxel)
    vol = [torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, device=dev), torch.zeros(dim, dim, dim, 3, device=dev)]
    scratch = [torch.zeros_like(t) for t in vol]
    copies = [torch.empty_like(t) for t in vol]
    volume_bytes = sum(t.numel() * 4 for t in vol)
    kw = dict(images=images, img_stride=1, img_offset=0)
    db.tsdf_integrate(vol[0], vol[1], vol[2], poses, disps, intr, every, origin, voxel, trunc, **kw)
    sets = {False: (poses, disps, which, None), True: (poses2, disps, which, None)}
    state = {"dense": False, "two": False, "bricks": False}

    def fused():
        s = state["dense"]
        db.tsdf_reintegrate(vol[0], vol[1], vol[2], origin, voxel, trunc, intr, remove=sets[s], add=sets[not s], **kw)
        state["dense"] = not s

    def two_calls():
        s = state["dense"]
        db.tsdf_reintegrate(vol[0], vol[1], vol[2], origin, voxel, trunc, intr, remove=sets[s], **kw)
        db.tsdf_reintegrate(vol[0], vol[1], vol[2], origin, voxel, trunc, intr, add=sets[not s], **kw)
        state["dense"] = not s

    def from_scratch():
        db.tsdf_integrate(scratch[0], scratch[1], scratch[2], poses, disps, intr, every, origin, voxel, trunc, **kw)

    def copy():
        for dst, src in zip(copies, vol):
            dst.copy_(src)

    bricks = SparseTSDF(origin, (dim // 8,) * 3, voxel, trunc, colours=True, device=dev, cap=4096)
    bricks.allocate(poses, disps, intr, every)
    bricks.allocate(poses2, disps, intr, every)
    bricks.integrate(poses, disps, intr, every, **kw)
    pool = bricks.volume()
    kept = torch.zeros(bricks.cap, dtype=torch.int32, device=dev)

    def brick_fused():
        s = state["bricks"]
        db.tsdf_sparse_reintegrate(pool, trunc, intr, remove=sets[s], add=sets[not s], kept=kept, **kw)
        state["bricks"] = not s

    def brick_scratch():
        db.tsdf_sparse_integrate(pool, poses, disps, intr, every, trunc, **kw)

    t = measure({"fused": fused, "two": two_calls, "scratch": from_scratch, "copy": copy, "brick_fused": brick_fused}, args.reps)
    nb = bricks.bricks
    survivors = float(kept[:nb].float().mean())
    tb = measure({"brick_scratch": brick_scratch}, args.reps)
    ta, tt, tc, td, tf, ts = [stats(t[k]) for k in ("fused", "two", "scratch", "copy", "brick_fused")] + [stats(tb["brick_scratch"])]
    lines = ["tsdf_reintegrate_bench on %s: %d keyframes at %d x %d, a %d^3 volume (voxel %.4f, trunc %.4f, 20 bytes per voxel) and %d bricks "
             "of 8^3; 8 keyframes moved by a voxel" % (torch.cuda.get_device_name(0), nf, ht, wd, dim, voxel, trunc, nb),
             "per call, device events, median [p10 .. p90] of %d repetitions after 5 warm-ups" % args.reps, "",
             "dense",
             "  (a) reintegrate, 8 out + 8 in, one call   %10.1f us [%.1f .. %.1f]" % ta,
             "  (b) remove-only, then add-only            %10.1f us [%.1f .. %.1f]   (b) / (a) = %.2f" % (tt + (tt[0] / ta[0],)),
             "  (c) integrate all %d from scratch          %10.1f us [%.1f .. %.1f]   (c) / (a) = %.2f" % ((nf,) + tc + (tc[0] / ta[0],)),
             "  (d) copy of the volume's bytes            %10.1f us [%.1f .. %.1f]   %d bytes read and written: %.0f GB/s; (a) / (d) = %.2f"
             % (td + (volume_bytes, 2.0 * volume_bytes / (td[0] * 1e-6) / 1e9, ta[0] / td[0])),
             "bricks",
             "  (a) sparse reintegrate, 8 out + 8 in      %10.1f us [%.1f .. %.1f]   survivors of 16 slots per brick: %.2f" % (tf + (survivors,)),
             "  (c) sparse integrate all %d                %10.1f us [%.1f .. %.1f]   (c) / (a) = %.2f" % ((nf,) + ts + (ts[0] / tf[0],)), ""]
    del vol, scratch, copies, bricks, pool
    torch.cuda.empty_cache()
    lines.append("(e) LiveMap.update end to end (wall clock, synchronised): map_points + weights + drift + one read-back + re-integration + snapshots")
    for n in (nf, 8 * nf):
        first, t_first, moved_t, idle_t, refreshed = live_map_figures(n, dim, voxel, origin, dev, args.reps)
        lines += ["  %4d fused keyframes: first update %s in %.0f us; 8 moved by a voxel %10.1f us [%.1f .. %.1f], keyframes refreshed per update "
                  "min %d median %d max %d; nothing moved %10.1f us [%.1f .. %.1f]"
                  % ((n, first, t_first) + moved_t + refreshed + idle_t)]
    ok = True
    if args.parent_lib:
        ok = compare_with_parent(args.parent_lib, args, lines)
        lines.append("unchanged kernels: %s" % ("hashes EQUAL, medians inside each other's spread" if ok else "SEE ABOVE - a hash differs or a median lies outside"))
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print("written to", args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
