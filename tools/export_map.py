"""Run the VO system over an image sequence like tools/test_vo.py (same arguments and data layout) and export the dense map.

    python tools/export_map.py --datapath <.../SceneXX> --weights <checkpoint.pth> --map out.ply [--full_res] [--filter_thresh_map 0.005]
                               [--reconstruction_path DIR] [--uncertainty [--max_rel_sigma X]]
                               [--mesh out.ply --voxel V [--trunc T] [--sigma_weight] [--sparse] [--panoptic [--track_ids] [--instances_dir DIR]]
                                [--render_dir DIR]]
                               [--live_map out.ply --voxel V --origin X Y Z --dims NZ NY NX [--sparse]]

--map writes the filtered point cloud of all keyframes after the global bundle adjustment (Droid.get_map: points confirmed by two
neighbouring keyframes, pvo_map_points) as a binary little-endian PLY: x y z float, red green blue uchar, int label (the per-frame
dense panoptic label, with --segm_filter True).  --full_res tracks with the convex upsampling and exports every pixel of the
full-resolution depth maps instead of the 1/8 lattice.  --reconstruction_path DIR also writes upstream DROID-SLAM's
tstamps / disps / poses / intrinsics / images .npy files.  --uncertainty tracks with args.uncertainty (every keyframe's inverse-depth
variances from the frontend's bundle adjustment, estimated after the keyframe's last local update - the global bundle adjustment
does not refresh them) and adds `property float sigma` to the PLY; --max_rel_sigma X also leaves out the cells whose relative
standard deviation sigma / disp exceeds X.  --mesh also fuses the same pixels into a TSDF volume of --voxel sized cells (truncation
--trunc, default three voxels) and writes its surface-nets mesh (Droid.get_mesh: pvo_tsdf_integrate / pvo_tsdf_mesh) as a binary PLY
with vertex normals, colours and triangle faces; --sigma_weight (with --uncertainty) weights every pixel by its inverse-depth
variance instead of counting all alike; --sparse fuses into a brick volume over the map's full extent (pvo_tsdf_sparse_*) where the
dense volume is clipped to what fits; --panoptic keeps the frames' panoptic ids as given (args.store_segment_ids), fuses them into the
volume by a weighted vote (pvo_tsdf_integrate_panoptic) and adds `property int label` to the mesh's vertices, and --instances_dir DIR
also writes one mesh per id, DIR/segment_<id>.ply; --track_ids (with --panoptic) tracks with args.segment_tracks - the keyframes' segments
associated along the graph's flow (pvo_segment_associate) - and fuses the ledger's track ids in place of the ids as given, for ids that
a per-image panoptic network numbers anew in every frame.  --render_dir DIR (with --mesh) also looks at the fused volume from every keyframe
(Droid.get_renders: pvo_tsdf_render / pvo_tsdf_sparse_render, at the resolution the volume was fused from) and writes per keyframe k
DIR/depth_%06d.npy (f32 [ht,wd], 0 = no surface), normal_%06d.npy (f32 [ht,wd,3]), rgba_%06d.npy (uint8 [ht,wd,4]) and, with
--panoptic, label_%06d.npy (int32 [ht,wd]: ids that are consistent across keyframes); it prints how each keyframe's own depth
agrees with the fused surface (DepthVideo.model_residual).  Without --mesh the output is what it was without the option, and without
--sparse / --panoptic / --render_dir the mesh is.  --live_map also keeps a TSDF volume current WHILE tracking (args.live_map:
pvo_amd.live_map.LiveMap over the world box --origin / --dims of --voxel sized cells, pvo_tsdf_reintegrate; with --sparse a brick
volume), writes its mesh, and prints how many keyframe refreshes it took and how the live volume compares with one fused from scratch
after the global bundle adjustment.  Without --live_map the output is what it was.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_vo  # noqa: E402  (tools/test_vo.py: the driver this one extends)


def parse_args(argv=None):
    import argparse
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--map", required=True, help="output .ply")
    p.add_argument("--full_res", action="store_true")
    p.add_argument("--filter_thresh_map", "--map_filter_thresh", type=float, default=0.005,
                   help="the depth filter's threshold (the reference viewer's filter_thresh; test_vo.py's --filter_thresh is the motion filter's)")
    p.add_argument("--reconstruction_path", default=None)
    p.add_argument("--uncertainty", action="store_true", help="estimate depth variances while tracking and write a sigma column")
    p.add_argument("--max_rel_sigma", type=float, default=None, help="with --uncertainty: drop cells with sigma / disp above this")
    p.add_argument("--mesh", default=None, help="also write the fused surface's triangle mesh to this .ply (needs --voxel)")
    p.add_argument("--voxel", type=float, default=None, help="with --mesh: the TSDF volume's voxel size, in the units of the poses")
    p.add_argument("--trunc", type=float, default=None, help="with --mesh: the truncation distance (default: 3 voxels)")
    p.add_argument("--sigma_weight", action="store_true", help="with --mesh and --uncertainty: weight pixels by their variance")
    p.add_argument("--sparse", action="store_true", help="with --mesh: a brick volume over the map's full extent")
    p.add_argument("--panoptic", action="store_true", help="with --mesh: fuse the frames' panoptic ids, write a label per vertex")
    p.add_argument("--track_ids", action="store_true", help="with --panoptic: fuse track ids associated across keyframes, not the ids as given")
    p.add_argument("--instances_dir", default=None, help="with --panoptic: also one segment_<id>.ply per id into this folder")
    p.add_argument("--render_dir", default=None, help="with --mesh: also depth / normal / rgba (/ label) images of the fused volume per keyframe")
    p.add_argument("--live_map", default=None, help="also keep a live TSDF volume while tracking and write its mesh to this .ply")
    p.add_argument("--origin", type=float, nargs=3, default=None, help="with --live_map: the centre of voxel (0,0,0), x y z")
    p.add_argument("--dims", type=int, nargs=3, default=None, help="with --live_map: the volume's size in voxels, nz ny nx")
    own, rest = p.parse_known_args(argv)
    args = test_vo.parse_args(rest)
    for k, v in vars(own).items():
        setattr(args, k, v)
    if args.max_rel_sigma is not None and not args.uncertainty:
        p.error("--max_rel_sigma needs --uncertainty")
    if args.mesh is not None and not (args.voxel is not None and args.voxel > 0):
        p.error("--mesh needs --voxel V with V > 0")
    if args.sigma_weight and not (args.mesh is not None and args.uncertainty):
        p.error("--sigma_weight needs --mesh and --uncertainty")
    if args.sparse and args.mesh is None and args.live_map is None:
        p.error("--sparse needs --mesh")
    if args.live_map is not None and not (args.voxel is not None and args.voxel > 0 and args.origin is not None and args.dims is not None):
        p.error("--live_map needs --voxel V with V > 0, --origin X Y Z and --dims NZ NY NX: the world box of a running session")
    if args.panoptic and args.mesh is None:
        p.error("--panoptic needs --mesh")
    if args.track_ids and not args.panoptic:
        p.error("--track_ids needs --panoptic")
    if args.instances_dir is not None and not args.panoptic:
        p.error("--instances_dir needs --panoptic")
    if args.render_dir is not None and args.mesh is None:
        p.error("--render_dir needs --mesh")
    return args


def write_mesh(droid, args):
    """the --mesh output of a tracked sequence; returns the line that says what was written"""
    from pvo_amd.handoff import split_mesh_by_label, write_ply_mesh
    kw = {"sparse": True} if args.sparse else {}
    if args.panoptic:
        kw["panoptic"] = True
    if getattr(args, "track_ids", False):
        kw["track_ids"] = True
    render_dir = getattr(args, "render_dir", None)
    if render_dir is not None and not args.sparse:
        kw["keep_rgb"] = True                                # (the dense colour volume, for the renders; the mesh is the same)
    g = droid.get_mesh(voxel=args.voxel, trunc=args.trunc, thresh=args.filter_thresh_map, full_res=args.full_res,
                       use_sigma=args.sigma_weight, max_rel_sigma=args.max_rel_sigma, **kw)
    nv, nf = write_ply_mesh(args.mesh, g["verts"], g["faces"], g["rgba"], g["normals"], **({"label": g["vlabel"]} if args.panoptic else {}))
    what = ("%d bricks of 8^3" % g["volume"].bricks) if args.sparse else ("a %s volume" % "x".join(str(d) for d in g["tsdf"].shape))
    line = "mesh: %d vertices, %d triangles from %s of %g-sized voxels written to %s" % (nv, nf, what, args.voxel, args.mesh)
    if args.panoptic:
        ids = sorted(set(g["vlabel"].unique().tolist()))
        line += "; %d segments" % len(ids)
        if args.instances_dir is not None:
            parts = split_mesh_by_label(g["verts"], g["faces"], g["vlabel"])
            for i in ids:                                    # (an id that owns no face: its vertices alone)
                v, f = parts.get(i, (g["verts"][g["vlabel"] == i], g["faces"][:0]))
                write_ply_mesh(os.path.join(args.instances_dir, "segment_%d.ply" % i), v, f)
            line += ", one mesh each written to %s" % args.instances_dir
    if render_dir is not None:
        line += "\n" + write_renders(droid, args, g)
    return line


def write_renders(droid, args, volume):
    """the --render_dir output: the volume of write_mesh seen from every keyframe; returns the line that says what was written"""
    import numpy as np
    os.makedirs(args.render_dir, exist_ok=True)
    r = droid.get_renders(volume, full_res=args.full_res)
    names = ["depth", "normal", "rgba"] + (["label"] if args.panoptic else [])
    host = {k: r[k].cpu().numpy() for k in names}
    n = host["depth"].shape[0]
    for k in range(n):
        for name in names:
            np.save(os.path.join(args.render_dir, "%s_%06d.npy" % (name, k)), host[name][k])
    res = droid.video.model_residual(volume, full_res=args.full_res)
    med, p90, share = [res[k].cpu().numpy() for k in ("median", "p90", "share")]
    seen = np.isfinite(med)
    worst = (float(np.median(med[seen])), float(med[seen].max()), float(np.median(p90[seen])), float(p90[seen].max())) if seen.any() else (float("nan"),) * 4
    return ("renders: %s of %d keyframes at %d x %d written to %s; model residual |1/disp - depth| / depth per keyframe: median %.4f "
            "(worst keyframe %.4f), 90th percentile %.4f (worst %.4f), over %.1f %% of the pixels"
            % (" / ".join(names), n, host["depth"].shape[1], host["depth"].shape[2], args.render_dir, worst[0], worst[1], worst[2], worst[3],
               100.0 * float(share.mean()) if n else 0.0))


def write_live_map(droid, args):
    """the --live_map output: the live volume's mesh, and the volume against one fused from scratch now; returns the lines"""
    from pvo_amd.handoff import write_ply_mesh
    lm = droid.live_map
    g = droid.get_live_map()
    nv, nf = write_ply_mesh(args.live_map, g["verts"], g["faces"], g["rgba"], g["normals"])
    line = ("live map: %d vertices, %d triangles written to %s; %d keyframes fused, %d keyframe refreshes while tracking"
            % (nv, nf, args.live_map, len(lm.fused), lm.refreshed_total))
    dims = lm.sparse.to_dense()["tsdf"].shape if lm.sparse is not None else lm.tsdf.shape
    ref = droid.get_mesh(voxel=args.voxel, trunc=args.trunc, thresh=args.filter_thresh_map, origin=args.origin, dims=tuple(dims))
    live = lm.sparse.to_dense() if lm.sparse is not None else {"tsdf": lm.tsdf, "wsum": lm.wsum}
    both = (live["wsum"] >= lm.min_weight) & (ref["wsum"] >= lm.min_weight)
    only = int(((live["wsum"] >= lm.min_weight) ^ (ref["wsum"] >= lm.min_weight)).sum())
    d = (live["tsdf"] - ref["tsdf"])[both].abs()
    line += ("\nlive volume against one fused from scratch after terminate: %d voxels usable in both, %d in only one; |tsdf difference| "
             "mean %.5f max %.4f; from-scratch mesh %d vertices"
             % (int(both.sum()), only, float(d.mean()) if d.numel() else 0.0, float(d.max()) if d.numel() else 0.0, ref["verts"].shape[0]))
    return line


def main(argv=None):
    from pvo_amd.droid import Droid
    from pvo_amd.handoff import save_reconstruction, write_kitti_trajectory, write_ply
    args = parse_args(argv)
    args.half_update = True
    args.store_images = True
    args.store_segment_ids = bool(args.panoptic)
    if args.track_ids:
        args.segment_tracks = True
    args.upsample = bool(args.full_res)
    if args.datapath.endswith("20"):
        args.thresh = 0.9
    if args.live_map is not None:
        args.live_map_path, args.live_map = args.live_map, dict(voxel=args.voxel, trunc=args.trunc, origin=args.origin, dims=args.dims,
                                                                sparse=args.sparse, thresh=args.filter_thresh_map)
    droid = Droid(args)
    with_segm = args.segm_filter or args.panoptic                      # (--panoptic reads the ids whether or not they filter the graph)
    for t, image, intr, segm in test_vo.image_stream(args.datapath, args.image_size, "val", with_segm):
        droid.track(t, image, intrinsics=intr, segments=segm)
    print("video frames:", droid.video.counter)
    traj = droid.terminate(test_vo.image_stream(args.datapath, args.image_size, "val", with_segm), need_inv=True)
    out_dir = os.path.join(args.out, os.path.basename(args.datapath.rstrip("/")), test_vo.SPLIT["val"])
    write_kitti_trajectory(os.path.join(out_dir, "pvo_traj.txt"), traj)
    kw = {"max_rel_sigma": args.max_rel_sigma if args.max_rel_sigma is not None else float("inf")} if args.uncertainty else {}
    m = droid.get_map(thresh=args.filter_thresh_map, full_res=args.full_res, **kw)
    n = write_ply(args.map, m["xyz"], m["rgba"], m.get("label") if args.segm_filter else None, **({"sigma": m["sigma"]} if args.uncertainty else {}))
    print("map: %d points of %d keyframes written to %s" % (n, droid.video.counter, args.map))
    if args.mesh is not None:
        print(write_mesh(droid, args))
    if getattr(args, "live_map_path", None) is not None:
        args.live_map = args.live_map_path
        print(write_live_map(droid, args))
    if args.reconstruction_path:
        for p in save_reconstruction(args.reconstruction_path, droid.video):
            print("wrote", p)


if __name__ == "__main__":
    main()
