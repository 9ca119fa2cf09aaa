"""tools/test_vo.py with a right view (stereo): every frame's right image goes to Droid.track, each keyframe gets a stereo edge - the
fixed left -> right transform of a rectified rig - and the trajectory is metric in the units of the baseline (pvo_amd/droid.py
`args.stereo`, include/pvo_hip.h pvo_ba_stereo).

    python tools/vo_stereo.py --datapath <sequence> --right_dir <folder> --baseline <metres> [every other argument of tools/test_vo.py] [--no_stereo]

--right_dir: one right image per frame (.jpg / .png, in the left images' sorted order; VKITTI2: <scene>/<variation>/frames/rgb/Camera_1),
read, resized and cropped exactly like the left ones.  --baseline: the rig's baseline in the units the trajectory is wanted in
(VKITTI2 and KITTI: 0.532725 / 0.54 m); the default 0.1 is upstream DROID-SLAM's constant.  The driver itself stays the reference's
(tools/test_vo.py is not edited): this entry point parses its own arguments, hands the rest to test_vo.parse_args and runs test_vo's
loop with the right image added to track().  The ATE is printed after Sim(3) alignment, as test_vo.py does, and beside it the
estimated path length over the true one - the scale, which the baseline fixes at 1.  `--no_stereo` runs the monocular path through
the same code for an A/B."""
import argparse
import glob
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_vo  # noqa: E402


def load_image(path, image_size=(240, 808)):
    """an image file -> [3,H,W] int BGR at the tracker's image size: test_vo.image_stream's own steps (bilinear resize, crop to a
    multiple of 8, channel flip, int32)"""
    from PIL import Image
    h1, w1 = int(image_size[0]), int(image_size[1])
    rgb = np.asarray(Image.open(path).convert("RGB").resize((w1, h1), Image.BILINEAR))
    rgb = rgb[:h1 - h1 % 8, :w1 - w1 % 8]
    return torch.as_tensor(rgb[..., ::-1].copy()).int().permute(2, 0, 1)


def right_images(right_dir):
    return sorted(glob.glob(os.path.join(right_dir, "*.jpg")) + glob.glob(os.path.join(right_dir, "*.png")))


def parse_args(argv=None):
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--right_dir", default=None, help="folder with one right image per frame, in the left images' order")
    p.add_argument("--baseline", type=float, default=0.1, help="the rig's baseline, in the units the trajectory is wanted in")
    p.add_argument("--stereo", dest="stereo", action="store_true", default=True, help="use the right view (default here)")
    p.add_argument("--no_stereo", dest="stereo", action="store_false", help="ignore the right view: the monocular run")
    own, rest = p.parse_known_args(argv)
    args = test_vo.parse_args(rest)
    args.stereo, args.stereo_baseline, args.right_dir = own.stereo, own.baseline, own.right_dir
    return args


def track_pairs(droid, args):
    """test_vo's loop: left frame t of the sequence with the t-th right image"""
    rights = right_images(args.right_dir) if args.stereo and args.right_dir else []
    if args.stereo and not rights:
        raise SystemExit("vo_stereo: --right_dir with one right image per frame is needed (or --no_stereo)")
    for t, image, intr, segm in test_vo.image_stream(args.datapath, args.image_size, "val", args.segm_filter):
        right = load_image(rights[t], args.image_size) if t < len(rights) else None
        droid.track(t, image, intrinsics=intr, segments=segm, right=right)


def main(argv=None):
    from pvo_amd.droid import Droid
    from pvo_amd.handoff import write_kitti_trajectory
    from pvo_amd.trajectory import ate_rmse
    args = parse_args(argv)
    args.half_update = True
    if args.datapath.endswith("20"):
        args.thresh = 0.9                                             # test_vo.py:94-95
    droid = Droid(args)
    track_pairs(droid, args)
    print("video frames:", droid.video.counter, "(stereo, baseline %g)" % droid.video.stereo_baseline if droid.video.has_stereo else "(monocular)")
    traj = droid.terminate(test_vo.image_stream(args.datapath, args.image_size, "val", args.segm_filter), need_inv=True)
    out_dir = os.path.join(args.out, os.path.basename(args.datapath.rstrip("/")), test_vo.SPLIT["val"])
    est_file = os.path.join(out_dir, "pvo_traj_stereo.txt" if args.stereo else "pvo_traj.txt")
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
