"""tools/test_vo.py with sensor depth (RGB-D): every frame's depth map goes to Droid.track, each keyframe's measurements become a prior
of the bundle adjustment and the trajectory is metric (pvo_amd/droid.py `args.rgbd`, include/pvo_hip.h pvo_ba_depth_prior).

    python tools/vo_rgbd.py --datapath <sequence> --depth_dir <folder> [every other argument of tools/test_vo.py] [--no_rgbd]

--depth_dir: one depth .npy per frame (metres, [H0,W0], in the images' sorted order; <= 0 or non-finite = no measurement), resized and
cropped like the image, nearest neighbour.  The driver itself stays the reference's (tools/test_vo.py is not edited): this entry point
parses its two arguments, hands the rest to test_vo.parse_args and runs test_vo's loop with the depth image added to track().  The ATE
is printed after Sim(3) alignment, as test_vo.py does, and beside it the estimated path length over the true one - the scale, which
sensor depth fixes at 1.  `--no_rgbd` runs the monocular path through the same code for an A/B."""
import argparse
import glob
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vo  # noqa: E402


def load_depth(path, image_size=(240, 808)):
    """a frame's depth .npy [H0,W0] -> [H,W] float32 at the tracker's image size: nearest-neighbour resize, cropped like the image"""
    d = torch.as_tensor(np.load(path).astype(np.float32))[None, None]
    h1, w1 = int(image_size[0]), int(image_size[1])
    return F.interpolate(d, size=(h1, w1), mode="nearest")[0, 0, :h1 - h1 % 8, :w1 - w1 % 8].contiguous()


def parse_args(argv=None):
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--depth_dir", default=None, help="folder with one depth .npy per frame (metres), in the images' order")
    p.add_argument("--rgbd", dest="rgbd", action="store_true", default=True, help="use the sensor depth (default here)")
    p.add_argument("--no_rgbd", dest="rgbd", action="store_false", help="ignore the depth: the monocular run")
    own, rest = p.parse_known_args(argv)
    args = test_vo.parse_args(rest)
    args.rgbd, args.depth_dir = own.rgbd, own.depth_dir
    return args


def main(argv=None):
    from pvo_amd.droid import Droid
    from pvo_amd.handoff import write_kitti_trajectory
    from pvo_amd.trajectory import ate_rmse
    args = parse_args(argv)
    args.half_update = True
    if args.datapath.endswith("20"):
        args.thresh = 0.9                                             # test_vo.py:94-95
    depths = sorted(glob.glob(os.path.join(args.depth_dir, "*.npy"))) if args.rgbd and args.depth_dir else []
    if args.rgbd and not depths:
        raise SystemExit("vo_rgbd: --depth_dir with one depth .npy per frame is needed (or --no_rgbd)")
    droid = Droid(args)
    for t, image, intr, segm in test_vo.image_stream(args.datapath, args.image_size, "val", args.segm_filter):
        depth = load_depth(depths[t], args.image_size) if t < len(depths) else None
        droid.track(t, image, depth=depth, intrinsics=intr, segments=segm)
    print("video frames:", droid.video.counter, "(sensor depth)" if droid.video.has_sensor_depth else "(monocular)")
    traj = droid.terminate(test_vo.image_stream(args.datapath, args.image_size, "val", args.segm_filter), need_inv=True)
    out_dir = os.path.join(args.out, os.path.basename(args.datapath.rstrip("/")), test_vo.SPLIT["val"])
    est_file = os.path.join(out_dir, "pvo_traj_rgbd.txt" if args.rgbd else "pvo_traj.txt")
    write_kitti_trajectory(est_file, traj)
    print("trajectory written to", est_file)
    gt_file = os.path.join(args.datapath, test_vo.SPLIT["val"], "extrinsic.txt")
    if os.path.exists(gt_file):
        gt = test_vo.read_vkitti2_poses(gt_file)[:, :3, 3]
        n = min(len(gt), len(traj))
        print("ATE-RMSE (Sim(3)-aligned, translation): %.4f m over %d poses" % (ate_rmse(traj[:n, :3], gt[:n]), n))
        length = lambda p: float(np.linalg.norm(np.diff(p, axis=0), axis=1).sum())
        print("path length: estimated %.3f m, true %.3f m (scale %.4f)" % (length(traj[:n, :3]), length(gt[:n]), length(traj[:n, :3]) / length(gt[:n])))


if __name__ == "__main__":
    main()
