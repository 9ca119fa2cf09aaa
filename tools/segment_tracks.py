"""Temporally consistent panoptic ids of a sequence: evaluation_scripts/test_vo.py's driver (tools/test_vo.py) with args.segment_tracks on.

    python tools/segment_tracks.py --datapath DIR [--weights FILE] [--tracks segment_tracks.npz] [--min-iou 0.25] [--cls-div N]
                                   [tools/test_vo.py's other options]

After every keyframe's last frontend update the keyframes' segments are associated along the graph's full flow (pvo_segment_associate)
and every (keyframe stamp, raw id) gets a track id that stays the same across keyframes.  Written as ONE .npz: the table tstamp f32 [M],
raw_id int32 [M], track int32 [M] in time order, and per track (track_id int32 [T], ascending) its keyframe stamps and pixel counts as
rows of track_start int32 [T + 1] into track_tstamp f32 [K] and track_pixels int32 [K] (pixels at 1/8 resolution).  --cls-div N: ids coded
category * N + instance match only inside their category.  Whether the network's flow carries real objects onto themselves well enough
is not measured here.  Needs the GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def save_tracks(path, table, track_map, tstamps):
    """table: Droid.get_segment_tracks(); track_map int [n,h,w] (SegmentTracks.track_map) and the n keyframes' stamps.  Returns
    {track id: [(tstamp, pixels), ...]}"""
    track_map, tstamps = np.asarray(track_map), [float(t) for t in tstamps]
    per = {}
    for k, t in enumerate(tstamps):
        ids, count = np.unique(track_map[k], return_counts=True)
        for i, c in zip(ids.tolist(), count.tolist()):
            if i > 0:
                per.setdefault(i, []).append((t, c))
    for t, _, track in table:                                                 # (a track whose keyframes are all beyond the map: no rows)
        per.setdefault(int(track), [])
    order = sorted(per)
    start = np.cumsum([0] + [len(per[i]) for i in order]).astype(np.int32)
    np.savez(path, tstamp=np.array([r[0] for r in table], np.float32), raw_id=np.array([r[1] for r in table], np.int32),
             track=np.array([r[2] for r in table], np.int32), track_id=np.array(order, np.int32), track_start=start,
             track_tstamp=np.array([t for i in order for t, _ in per[i]], np.float32),
             track_pixels=np.array([c for i in order for _, c in per[i]], np.int32))
    for i in order:
        print("track %6d: %3d keyframes, %d pixels" % (i, len(per[i]), sum(c for _, c in per[i])))
    return per


def main(argv=None):
    import argparse
    import test_vo
    from pvo_amd.droid import Droid
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--tracks", default="segment_tracks.npz")
    ap.add_argument("--min-iou", type=float, default=0.25)
    ap.add_argument("--cls-div", type=int, default=None)
    own, rest = ap.parse_known_args(argv)
    args = test_vo.parse_args(rest)
    args.half_update = True
    args.segm_filter = True                                           # (the stream hands the panoptic ids over only with the filter on)
    args.store_segment_ids = True
    args.segment_tracks = dict(min_iou=own.min_iou, cls_div=own.cls_div)
    if args.datapath.endswith("20"):
        args.thresh = 0.9
    droid = Droid(args)
    for t, image, intr, segm in test_vo.image_stream(args.datapath, args.image_size, "val", True):
        droid.track(t, image, intrinsics=intr, segments=segm)
    print("video frames:", droid.video.counter)
    n = droid.video.counter
    save_tracks(own.tracks, droid.get_segment_tracks(), droid.segment_tracks.track_map().cpu().numpy(), droid.video.tstamp[:n].tolist())
    print("written to", own.tracks)


if __name__ == "__main__":
    main()
