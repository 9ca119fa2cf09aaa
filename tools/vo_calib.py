"""tools/test_vo.py's driver for a sequence WITHOUT a trusted calibration: the same arguments, plus online intrinsics calibration.

    python tools/vo_calib.py --datapath <.../SceneXX> --weights <checkpoint.pth> --opt_intr [--focal_only] [--init_focal_scale 1.1]

  --opt_intr            after initialisation and after every kept keyframe's last frontend update, two more steps of the window's
                        bundle adjustment run with (fx, fy, cx, cy) as unknowns shared by all frames (Droid args.opt_intr)
  --focal_only          only fx, fy are free (args.opt_intr_free = "focal")
  --init_focal_scale S  the file's fx, fy times S before tracking: a wrong calibration to start from

Prints the initial and the final intrinsics (image resolution) beside the ATE."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def scaled_stream(stream, scale):
    """the stream of tools/test_vo.py with fx, fy times `scale`"""
    for t, image, intr, segm in stream:
        intr = intr.clone()
        intr[0:2] *= scale
        yield t, image, intr, segm


def parse_args(argv=None):
    import test_vo
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--opt_intr", action="store_true")
    p.add_argument("--focal_only", action="store_true")
    p.add_argument("--init_focal_scale", type=float, default=1.0)
    own, rest = p.parse_known_args(argv)
    if not (own.init_focal_scale > 0):
        raise SystemExit("--init_focal_scale must be positive")
    args = test_vo.parse_args(rest)
    args.opt_intr, args.opt_intr_free, args.init_focal_scale = own.opt_intr, ("focal" if own.focal_only else "all"), own.init_focal_scale
    return args


def main(argv=None):
    import test_vo
    from pvo_amd.droid import Droid
    from pvo_amd.handoff import write_kitti_trajectory
    from pvo_amd.trajectory import ate_rmse
    args = parse_args(argv)
    args.half_update = True
    if args.datapath.endswith("20"):
        args.thresh = 0.9
    stream = lambda: scaled_stream(test_vo.image_stream(args.datapath, args.image_size, "val", args.segm_filter), args.init_focal_scale)
    droid = Droid(args)
    first = None
    for t, image, intr, segm in stream():
        if first is None:
            first = intr.clone()
        droid.track(t, image, intrinsics=intr, segments=segm)
    print("video frames:", droid.video.counter)
    traj = droid.terminate(stream(), need_inv=True)
    fmt = lambda v: "fx %.3f fy %.3f cx %.3f cy %.3f" % tuple(float(x) for x in v)
    print("intrinsics, initial (file x %.3f on the focal lengths): %s" % (args.init_focal_scale, fmt(first)))
    print("intrinsics, final (%s):  %s" % ("opt_intr, %s free" % args.opt_intr_free if args.opt_intr else "not optimised", fmt(droid.get_intrinsics())))
    out_dir = os.path.join(args.out, os.path.basename(args.datapath.rstrip("/")), test_vo.SPLIT["val"])
    est_file = os.path.join(out_dir, "pvo_traj.txt")
    write_kitti_trajectory(est_file, traj)
    print("trajectory written to", est_file)
    gt_file = os.path.join(args.datapath, test_vo.SPLIT["val"], "extrinsic.txt")
    if os.path.exists(gt_file):
        gt = test_vo.read_vkitti2_poses(gt_file)[:, :3, 3]
        n = min(len(gt), len(traj))
        print("ATE-RMSE (Sim(3)-aligned, translation): %.4f m over %d poses" % (ate_rmse(traj[:n, :3], gt[:n]), n))


if __name__ == "__main__":
    main()
