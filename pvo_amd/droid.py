"""Droid - the VO system object: motion filter -> frontend (local BA) -> backend (global BA) -> trajectory filler.

Counterpart of the reference's Droid (VO_Module/droid_slam/droid.py:19-124): same constructor argument object
(the fields of evaluation_scripts/test_vo.py:58-83), `track`, `terminate`, `get_traj`, `get_depth`, `get_flow`.
There is no visualiser process and no shared-memory video: one process owns one GPU.  With `args.weights = None`
the network keeps its seeded default initialisation (this image has no checkpoints).
"""
from argparse import Namespace
from collections import OrderedDict

import torch

from .backend import DroidBackend
from .depth_video import DepthVideo
from .droid_net import DroidNet, upsample_inter
from .frontend import DroidFrontend
from .geom.se3 import SE3
from .motion_filter import MotionFilter
from .trajectory_filler import PoseTrajectoryFiller


def default_args(**over):
    """the defaults of evaluation_scripts/test_vo.py:58-83"""
    a = dict(device="cuda:0", weights=None, buffer=1024, image_size=[240, 808], disable_vis=True, use_aff_bri=False,
             beta=0.6, filter_thresh=1.75, warmup=12, keyframe_thresh=2.25, frontend_thresh=12.0, frontend_window=25,
             frontend_radius=2, frontend_nms=1, backend_thresh=15.0, backend_radius=2, backend_nms=3,
             segm_filter=False, thresh=0.8, half_update=True, pipelined=False, rgbd=False, stereo=False, stereo_baseline=0.1,
             store_images=False, uncertainty=False, opt_intr=False, opt_intr_free="all", store_segment_ids=False, live_map=None,
             object_motion=None, segment_tracks=None)
    # uncertainty: after every keyframe's last frontend update, estimate the window's inverse-depth variances and pose covariance from
    # the bundle adjustment's normal equations (DepthVideo.uncertainty; get_uncertainty(), get_map(max_rel_sigma=...)).  Read only: the
    # trajectory and the depths are bit for bit those of a run without it.  A window of more than 64 poses (frontend_window above 64) is
    # not estimated: its keyframes keep +inf.  False (default): nothing is allocated, no launch is added.
    # opt_intr: online intrinsics calibration for a video without (or with a wrong) calibration - after initialisation and after every
    # kept keyframe's last frontend update the window's bundle adjustment runs two more steps with (fx, fy, cx, cy) as unknowns shared by
    # all frames (opt_intr_free = "all") or the focal lengths only ("focal"); DepthVideo.ba_calib, get_intrinsics().  Windows of more than
    # 64 poses are not calibrated.  Not with rgbd / stereo.  False (default): no launch is added, every result is what it was.
    # rgbd: use the `depth` image of track() - each keyframe's sensor depth becomes a prior of the bundle adjustment, the trajectory
    # and the map are metric (DepthVideo, include/pvo_hip.h pvo_ba_depth_prior).  False (default): `depth` is IGNORED, nothing is
    # allocated for it and every result is what a monocular run computes.
    # stereo: use the `right` image of track() - each keyframe's right view gives the graph a stereo edge (i, i) with the fixed baseline
    # stereo_baseline (in the units the trajectory is wanted in: metres give a metric trajectory; 0.1 is upstream's constant).  False
    # (default): `right` is IGNORED, nothing is allocated for it and every result is what a monocular run computes.
    # store_images: keep every keyframe's image on the device (DepthVideo.images, uint8 [buffer,3,H,W]) so that get_map() can colour
    # its points.  False (default): nothing is allocated, no result changes, and get_map() returns points without colours.
    # store_segment_ids: keep every keyframe's panoptic ids AS GIVEN (DepthVideo.segms_raw, int32 [buffer,H/8,W/8]; `segms` relabels each
    # frame on its own) so that get_mesh(panoptic=True) can fuse them across frames.  False (default): nothing is allocated or changed.
    # live_map: a dict of pvo_amd.live_map.LiveMap's keyword arguments (voxel, origin, dims at least) - a TSDF volume kept current WHILE
    # tracking: track() fuses the keyframes that have left the frontend's window and re-fuses the ones whose pose or depth moved,
    # terminate() brings it up to the last keyframe after the global bundle adjustment; get_live_map().  Not with pipelined.  None
    # (default): nothing is imported, allocated or launched.
    # object_motion: True, or a dict of pvo_amd.object_motion.ObjectTracks' keyword arguments (min_pixels, dynamic_share, iters, huber, ...) -
    # after every keyframe's last frontend update the rigid motion of every segment between consecutive keyframes is solved from the
    # graph's full flow (pvo_object_motion) and kept per (tstamp_i, tstamp_j, label); get_object_tracks().  Read only: the trajectory
    # and the depths are bit for bit those of a run without it.  None (default): nothing is imported, allocated or launched.
    # segment_tracks: True, or a dict of pvo_amd.segment_tracks.SegmentTracks' keyword arguments (min_iou, cls_div); needs store_segment_ids -
    # after every keyframe's last frontend update the keyframes' segments are associated along the graph's full flow
    # (pvo_segment_associate) and every (tstamp, raw id) gets a track id that stays the same across keyframes; get_segment_tracks(),
    # get_mesh(panoptic=True, track_ids=True), get_object_tracks(by_track=True).  Read only: the trajectory and the depths are bit for
    # bit those of a run without it.  None (default): nothing is imported, allocated or launched.
    a.update(over)
    return Namespace(**a)


class Droid:
    def __init__(self, args):
        self.args = args
        if getattr(args, "opt_intr", False) and (getattr(args, "rgbd", False) or getattr(args, "stereo", False)):
            raise ValueError("args.opt_intr together with args.rgbd or args.stereo is not supported: the calibrating bundle adjustment has "
                             "neither the sensor-depth prior nor stereo edges")
        if getattr(args, "opt_intr_free", "all") not in ("all", "focal"):
            raise ValueError("args.opt_intr_free must be 'all' or 'focal', got %r" % (args.opt_intr_free,))
        if getattr(args, "live_map", None) is not None and getattr(args, "pipelined", False):
            raise ValueError("args.live_map together with args.pipelined is not supported: between two pipelined track() calls a keyframe "
                             "update is half done, and the live map would fuse it as it stands")
        if getattr(args, "segment_tracks", None) and not getattr(args, "store_segment_ids", False):
            raise ValueError("args.segment_tracks needs the raw segment ids: set args.store_segment_ids = True")
        self.load_weights(args.weights, args.use_aff_bri)
        self.video = DepthVideo(args.image_size, args.buffer, args.device, args.segm_filter, args.thresh,
                                store_images=bool(getattr(args, "store_images", False)),
                                store_segment_ids=bool(getattr(args, "store_segment_ids", False)))
        self.filterx = MotionFilter(self.net, self.video, thresh=args.filter_thresh, device=args.device)
        self.filterx.overlap_upload = bool(getattr(args, "pipelined", False))
        self.filterx.use_depth = bool(getattr(args, "rgbd", False))
        self.filterx.use_stereo = bool(getattr(args, "stereo", False))
        self.video.stereo_baseline = float(getattr(args, "stereo_baseline", 0.1))
        self.frontend = DroidFrontend(self.net.update, self.video, args.device, warmup=args.warmup, beta=args.beta,
                                      frontend_nms=args.frontend_nms, keyframe_thresh=args.keyframe_thresh,
                                      frontend_window=args.frontend_window, frontend_thresh=args.frontend_thresh,
                                      frontend_radius=args.frontend_radius, upsample=bool(getattr(args, "upsample", False)),
                                      uncertainty=bool(getattr(args, "uncertainty", False)),
                                      opt_intr=bool(getattr(args, "opt_intr", False)),
                                      opt_intr_free=getattr(args, "opt_intr_free", "all"))
        self.filterx.before_context = self.frontend.keyframe_ahead
        self.backend = DroidBackend(self.net, self.video, args)
        self.traj_filler = PoseTrajectoryFiller(self.net, self.video, args.device)
        self.live_map = None
        if getattr(args, "live_map", None) is not None:
            from .live_map import LiveMap
            kw = dict(args.live_map)
            kw.setdefault("lag", args.frontend_window)
            self.live_map = LiveMap(self.video, **kw)

        om = getattr(args, "object_motion", None)
        if om:
            from .object_motion import ObjectTracks
            self.frontend.object_tracks = ObjectTracks(self.video, **(dict(om) if isinstance(om, dict) else {}))

        self.segment_tracks = None
        st = getattr(args, "segment_tracks", None)
        if st:
            from .segment_tracks import SegmentTracks
            self.segment_tracks = self.frontend.segment_tracks = SegmentTracks(self.video, **(dict(st) if isinstance(st, dict) else {}))

    def load_weights(self, weights, use_aff_bri=False):
        """droid.py:55-62; DataParallel's "module." prefix is stripped"""
        self.net = DroidNet(use_aff_bri)
        if weights is not None:
            sd = torch.load(weights, map_location=self.args.device)
            self.net.load_state_dict(OrderedDict((k.replace("module.", ""), v) for k, v in sd.items()))
        self.net.to(self.args.device).eval()
        if getattr(self.args, "half_update", True) and torch.device(self.args.device).type == "cuda":
            self.net.update.half()          # the fused 16-bit operator path
            if getattr(self.args, "half_encoders", True):
                # the encoders run under fp16 autocast (motion_filter.py:50): every convolution, norm and add is an fp16 operation
                # either way, but fp32 parameters are cast again in EVERY forward - 33 tiny kernels of ~120 per frame.  Cast once.
                self.net.fnet.half(); self.net.cnet.half()
        if getattr(self.args, "native_encoders", False):
            # the encoders' 3 x 3 / 7 x 7 convolutions on the library's own deterministic kernel instead of the vendor library (opt-in)
            self.net.fnet.native_convs = self.net.cnet.native_convs = True

    def track(self, tstamp, image, depth=None, intrinsics=None, segments=None, right=None):
        """one frame (droid.py:64-75).  right [3,H,W]: the right view of a rectified stereo pair, prepared like `image`; used only
        with args.stereo and ignored otherwise.  depth [H,W] (host or device, resized and cropped like the image; <= 0 / non-finite = no
        measurement) is used only with args.rgbd, on every frame that brings one, and ignored otherwise.  args.pipelined (default False: the reference's order, the video is final for this frame when
        the call returns): the frame's graph is launched FIRST, then the second half of the previous keyframe's frontend update (its
        keyframe test was left in flight when the previous call returned), then the motion test is read and this frame's frontend
        work is issued up to ITS keyframe test.  Same operations on the same data in the same dependency order - poses, depths and the
        trajectory are bit-identical (tests/test_vo_system.py) - but the device has work queued while the host waits for a scalar
        or books edges.  The video then lags by half a keyframe update between calls: `flush()` (called by terminate / get_*)
        completes it."""
        with torch.no_grad():
            if not getattr(self.args, "pipelined", False):
                self.filterx.track(tstamp, image, depth, intrinsics, segments, right=right)
                self.frontend()
                if self.live_map is not None:
                    self.live_map.update()
                return
            self.filterx.begin(tstamp, image, depth, intrinsics, segments, right=right)
            self.frontend.finish()
            self.filterx.finish()
            self.frontend.begin()

    def flush(self):
        """complete a keyframe update a pipelined track() left half done"""
        fe = getattr(self, "frontend", None)
        if fe is not None:
            with torch.no_grad():
                fe.finish()

    def terminate(self, stream=None, need_inv=True):
        """two global BA passes, then fill in every frame's pose; returns [num_frames, 7] (t, q) (droid.py:77-98)"""
        self.flush()
        self.filterx.before_context = None          # (a bound method of the frontend: it would keep the frontend's volumes alive)
        del self.frontend
        self._release_cached_memory()
        self.backend(7)
        self._release_cached_memory()
        self.backend(12)
        if self.live_map is not None:
            self.live_map.update(upto=self.video.counter, force=False)
        traj = self.traj_filler(stream)
        return (traj.inv() if need_inv else traj).data.cpu().numpy()

    def _release_cached_memory(self):
        """droid.py:84,88 empty the allocator's cache before each global BA - on the 11-24 GB GPUs the reference runs on the
        frontend's volumes have to go first.  On MI355X that is 50 ms of hipFree per call (and the backend then allocates again)
        for nothing while HBM is mostly free: only done when less than a quarter of the device memory is available."""
        if torch.device(self.args.device).type != "cuda":
            return
        free, total = torch.cuda.mem_get_info(torch.device(self.args.device))
        if free < 0.25 * total:
            torch.cuda.empty_cache()

    def get_traj(self):
        self.flush()
        return SE3(self.video.poses[:self.video.counter]).data.cpu().numpy()

    def get_depth(self, convex=False):
        """inverse depth of the keyframes at image resolution [counter, H, W]: bilinear enlargement of the 1/8-resolution maps, or -
        convex=True, tracking with args.upsample - the convex upsampling the network was trained to produce (video.disps_up)"""
        self.flush()
        if convex:
            if not getattr(self.args, "upsample", False) or self.video.disps_up is None:
                raise RuntimeError("get_depth(convex=True) needs tracking with args.upsample = True (video.disps_up is not maintained)")
            return self.video.disps_up[:self.video.counter]
        d = self.video.disps[:self.video.counter]
        return upsample_inter(d[None, ..., None]).squeeze(4).squeeze(0)

    def get_intrinsics(self):
        """(fx, fy, cx, cy) at image resolution: 8 x the vector the video stores - the calibrated one after tracking with
        args.opt_intr = True, else the first keyframe's"""
        self.flush()
        return 8.0 * self.video.intrinsics[0]

    def get_uncertainty(self):
        """(sigma_disp = sqrt(var_cond + var_pose), var_cond, var_pose [counter, H/8, W/8], poses_cov [counter, 6, 6] fp64) of the
        keyframes, from tracking with args.uncertainty = True; +inf where a keyframe was never estimated"""
        self.flush()
        v, n = self.video, self.video.counter
        if not getattr(self.args, "uncertainty", False) or v.disps_var_cond is None:
            raise RuntimeError("get_uncertainty() needs tracking with args.uncertainty = True (the variances are not maintained)")
        return v.sigma_disp()[:n], v.disps_var_cond[:n], v.disps_var_pose[:n], v.poses_cov[:n]

    def get_map(self, **kw):
        """the dense map of the keyframes: DepthVideo.map_points(ix=None, thresh=0.005, full_res=False, dirty_only=False, reject=None,
        max_rel_sigma=None) - a dict of xyz [n,3], rgba [n,4] (colours with args.store_images, else 0; a = votes), label [n], src [n,2],
        frame_start, and with max_rel_sigma (args.uncertainty) sigma [n]"""
        self.flush()
        return self.video.map_points(**kw)

    def get_mesh(self, **kw):
        """the fused surface of the keyframes: DepthVideo.tsdf(voxel, trunc=None, ix=None, thresh=0.005, full_res=False, reject=None,
        use_sigma=False, origin=None, dims=None, min_weight=1.0, w_max=0) - a dict of the mesh verts [V,3], normals [V,3], rgba [V,4],
        faces [F,3] and the volume tsdf, wsum [nz,ny,nx], origin, voxel.  sparse=True (with margin=2): a brick volume in place of the dense
        one, returned as `volume` (DepthVideo.tsdf).  panoptic=True (args.store_segment_ids): the keyframes' segment ids fused into the volume
        as well - vlabel [V], one id per vertex, and the volumes label, lconf.  A one-off fusion of the video as it stands: a volume
        that follows the keyframes while they move is args.live_map / get_live_map().  track_ids=True (with panoptic=True, needs
        args.segment_tracks): the ledger's track ids are fused in place of the ids as given (SegmentTracks.track_map), so that an
        object numbered anew in every keyframe still gets one label."""
        self.flush()
        if kw.pop("track_ids", False):
            if self.segment_tracks is None:
                raise RuntimeError("get_mesh(track_ids=True) needs args.segment_tracks (True, or a dict of SegmentTracks' arguments)")
            kw["labels"] = self.segment_tracks.track_map(self.video)
        return self.video.tsdf(**kw)

    def get_object_tracks(self, by_track=False):
        """{label: [entry, ...]} in time order, an entry per pair of consecutive keyframes on which the segment had enough pixels: dict
        tstamp_i, tstamp_j, label, motion [7] (the segment's rigid motion in the world frame between the two keyframes, the identity
        for a static one), centroid [3] (its points' mean in the world at time i), count, status (0 = solved), E.  Needs
        args.object_motion.  by_track=True (needs args.segment_tracks too): keyed by the track id of (tstamp_i, label) in place of the
        label, each entry with its `track`; entries whose segment has no track are left out."""
        if self.frontend.object_tracks is None:
            raise RuntimeError("get_object_tracks() needs args.object_motion (True, or a dict of ObjectTracks' arguments)")
        self.flush()
        tracks = self.frontend.object_tracks.tracks()
        if not by_track:
            return tracks
        if self.segment_tracks is None:
            raise RuntimeError("get_object_tracks(by_track=True) needs args.segment_tracks (True, or a dict of SegmentTracks' arguments)")
        out = {}
        for entry in sorted((e for es in tracks.values() for e in es), key=lambda e: (e["tstamp_i"], e["tstamp_j"], e["label"])):
            track = self.segment_tracks.entries.get((entry["tstamp_i"], entry["label"]))
            if track is not None:
                out.setdefault(track, []).append(dict(entry, track=track))
        return out

    def get_segment_tracks(self):
        """[(tstamp, raw id, track id), ...] in time order: the track id of every segment of every keyframe, the same for the same object
        across keyframes as far as the flow carried it onto itself (pvo_amd.segment_tracks.SegmentTracks).  Needs args.segment_tracks."""
        if self.segment_tracks is None:
            raise RuntimeError("get_segment_tracks() needs args.segment_tracks (True, or a dict of SegmentTracks' arguments)")
        self.flush()
        return self.segment_tracks.table()

    def get_live_map(self):
        """the volume args.live_map keeps current and its mesh as it stands: LiveMap.as_volume() (tsdf, wsum, rgb with images, origin,
        voxel; or volume = the SparseTSDF) plus verts, normals, rgba, faces.  Fused up to the keyframes that have left the frontend's
        window, after terminate() up to the last one."""
        if self.live_map is None:
            raise RuntimeError("get_live_map() needs args.live_map (a dict of LiveMap's arguments: voxel, origin, dims, ...)")
        out = self.live_map.as_volume()
        out.update(self.live_map.mesh())
        return out

    def get_renders(self, volume, **kw):
        """the fused volume seen from the keyframes (or from explicit poses): DepthVideo.tsdf_render(volume, ix=None, poses=None,
        full_res=False, dz=None, z_near=0.0, z_far=None, min_weight=1.0, normals=True) on the dict get_mesh returned - a dict of depth
        [n,ht,wd], normal [n,ht,wd,3], rgba [n,ht,wd,4] and, for a panoptic volume, label [n,ht,wd]"""
        self.flush()
        return self.video.tsdf_render(volume, **kw)

    # refine_to_model's Huber threshold, in truncations.  A keyframe's residuals against the volume it was fused into are heavy-tailed:
    # at the true pose of the analytic test scene their median is 0.006 while 14 % exceed 0.1 (beside a silhouette the views that see
    # past it average free space into the surface's voxels).  The quadratic loss follows that tail to a pose where the keyframe's median
    # model_residual is 2.4 times the other keyframes'; five times the inliers' median holds it at 1.35.
    REFINE_HUBER = 0.03

    def refine_to_model(self, volume, ix=None, apply=False, **kw):
        """frame-to-model tracking of the keyframes ix (default: all) against the fused volume get_mesh returned:
        DepthVideo.tsdf_track(volume, ix, **kw) from each keyframe's own depth and pose, with huber = REFINE_HUBER unless given (kw:
        weight, full_res, iters, band, huber, lm, ep, min_count, min_weight; not disps / poses: the residuals below are the stored
        keyframes').  apply=True writes the refined poses of the slots whose last status is 0 into video.poses (one small
        read-back) and needs ix, without repeats: which keyframes to overwrite is the caller's decision - a keyframe that already
        agrees with the volume gains nothing from it.  Otherwise the video is not touched.  Returns a dict: ix, poses [N,7], info
        [N,iters+1,4] and DepthVideo.model_residual of those keyframes `before` and `after` (after: at the refined poses, whether
        applied or not)."""
        for k in ("disps", "poses"):
            if k in kw:
                raise ValueError("refine_to_model tracks the stored keyframes from their own depths and poses: no %s= (DepthVideo.tsdf_track takes it)" % k)
        if apply:
            if ix is None:
                raise ValueError("refine_to_model(apply=True) needs ix: the keyframes whose poses to overwrite")
            ids = torch.as_tensor(ix, dtype=torch.long).reshape(-1)
            if ids.unique().numel() != ids.numel():
                raise ValueError("refine_to_model(apply=True): ix names a keyframe twice")
        kw.setdefault("huber", self.REFINE_HUBER)
        self.flush()
        v = self.video
        n = v.counter
        full_res = bool(kw.get("full_res", False))
        before = v.model_residual(volume, ix=ix, full_res=full_res)
        out = v.tsdf_track(volume, ix=ix, **kw)
        sel = out["ix"]
        inside = (sel >= 0) & (sel < n)
        rows = sel.clamp(0, max(n - 1, 0))
        good = inside & (out["info"][:, -1, 3] == 0)
        poses = torch.where(good[:, None], out["poses"], v.poses[:n][rows])
        depth = v.tsdf_render(volume, poses=poses, full_res=full_res, normals=False)["depth"]
        med, p90, share = v.depth_residual((v.disps_up if full_res else v.disps)[:n][rows], depth)
        after = {"ix": sel, "median": med, "p90": p90, "share": share}
        if apply:
            v.poses[rows[good]] = out["poses"][good]
        return {"ix": sel, "poses": out["poses"], "info": out["info"], "before": before, "after": after}

    def get_flow(self):
        self.flush()
        return upsample_inter(self.video.full_flow[:self.video.counter][None] * 8)
