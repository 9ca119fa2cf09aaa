"""Per-instance object tracks of a sequence: evaluation_scripts/test_vo.py's driver (tools/test_vo.py) with args.object_motion on.

    python tools/object_tracks.py --datapath DIR [--weights FILE] [--tracks object_tracks.npz] [--min-pixels 64] [--dynamic-share S]
                                  [--huber H] [tools/test_vo.py's other options]

After every keyframe's last frontend update the rigid motion of every panoptic segment between consecutive keyframes is solved from the
graph's full flow (pvo_object_motion) and kept per (tstamp_i, tstamp_j, label).  Written as ONE .npz: label int32 [M], tstamp_i,
tstamp_j f32 [M], motion f32 [M,7] (world frame, (t, q)), centroid f32 [M,3] (world, time i), count, status int32 [M]; printed per label:
the path length of the centroid carried through its motions.  Whether the network's dynamic flow is accurate enough for these motions to
be useful is not measured here.  Needs the GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def rotate(q, v):
    """v rotated by the quaternion (x, y, z, w)"""
    u = 2.0 * np.cross(q[:3], v)
    return v + q[3] * u + np.cross(q[:3], u)


def save_tracks(path, tracks):
    """tracks: Droid.get_object_tracks().  Returns {label: path length}"""
    rows = [t for label in sorted(tracks) for t in tracks[label]]
    np.savez(path, label=np.array([t["label"] for t in rows], np.int32), tstamp_i=np.array([t["tstamp_i"] for t in rows], np.float32),
             tstamp_j=np.array([t["tstamp_j"] for t in rows], np.float32),
             motion=np.array([t["motion"] for t in rows], np.float32).reshape(-1, 7), centroid=np.array([t["centroid"] for t in rows], np.float32).reshape(-1, 3),
             count=np.array([t["count"] for t in rows], np.int32), status=np.array([t["status"] for t in rows], np.int32))
    length = {}
    for label in sorted(tracks):
        solved = [t for t in tracks[label] if t["status"] == 0]
        length[label] = float(sum(np.linalg.norm(rotate(t["motion"][3:].astype(np.float64), t["centroid"].astype(np.float64))
                                                 + t["motion"][:3] - t["centroid"]) for t in solved))
        print("label %6d: %3d pairs (%d solved), centroid path %.4f" % (label, len(tracks[label]), len(solved), length[label]))
    return length


def main(argv=None):
    import argparse
    import test_vo
    from pvo_amd.droid import Droid
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--tracks", default="object_tracks.npz")
    ap.add_argument("--min-pixels", type=int, default=64)
    ap.add_argument("--dynamic-share", type=float, default=None)
    ap.add_argument("--huber", type=float, default=0.0)
    own, rest = ap.parse_known_args(argv)
    args = test_vo.parse_args(rest)
    args.half_update = True
    args.segm_filter = True                                           # (the stream hands the panoptic ids over only with the filter on)
    args.store_segment_ids = True                                     # (the ids as given: the same instance keeps its label across frames)
    args.object_motion = dict(min_pixels=own.min_pixels, dynamic_share=own.dynamic_share, huber=own.huber)
    if args.datapath.endswith("20"):
        args.thresh = 0.9
    droid = Droid(args)
    for t, image, intr, segm in test_vo.image_stream(args.datapath, args.image_size, "val", True):
        droid.track(t, image, intrinsics=intr, segments=segm)
    print("video frames:", droid.video.counter)
    save_tracks(own.tracks, droid.get_object_tracks())
    print("written to", own.tracks)


if __name__ == "__main__":
    main()
