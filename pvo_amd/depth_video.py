"""DepthVideo — keyframe state buffers and the native calls made on them.

Counterpart of the reference's DepthVideo (VO_Module/droid_slam/depth_video.py:13-214):
same attribute names and shapes (poses [buf,7], disps [buf,H/8,W/8], intrinsics [buf,4],
fmaps/nets/inps fp16, segms int32), same `reproject` / `distance` / `ba` methods.
Differences: one process per GPU, so the counter is a plain int and there is no lock;
feature maps are kept channels-last ([buf,H/8,W/8,128]) because that is the layout both
the matrix-core volume build and AltCorr read; `reproject` is one HIP kernel instead of the
lietorch broadcast chain.

RGB-D (upstream DROID-SLAM's `disps_sens`; the reference stripped it): `append(..., depth=...)` / `video[k] = (..., depth)` store a
keyframe's measured inverse depth at 1/8 resolution, 0 = no measurement, in `disps_sens` (allocated on first use), and from then on
`ba()` and the factor graph's native update carry the sensor-depth prior of the bundle adjustment (include/pvo_hip.h,
pvo_ba_depth_prior).  `has_sensor_depth` is the host-side flag everything asks; a video that never saw a depth image allocates
nothing and computes exactly what it computed before.

Stereo: `append(..., right_fmap=...)` stores the feature map of a keyframe's RIGHT view in `fmaps_right` (allocated on first use).  On
such a video (`has_stereo`: a right view was seen and `stereo_baseline` > 0) an edge (i, i) is a stereo edge - the fixed left -> right
transform of a rectified rig, u_right = u - fx b d - in `reproject`, `reproject_into`, `ba` and the factor graph's native update
(include/pvo_hip.h, pvo_ba_stereo); the factor graph correlates it against the right map.  Every keyframe of a stereo video is expected
to bring its right view (one that does not gets a zero map).  A video that never saw a right view allocates nothing and computes
exactly what it computed before, (i, i) edges included.

Uncertainty: `uncertainty(...)`, beside `ba(...)` and on its operands, writes every optimised keyframe's inverse-depth variances -
`disps_var_cond` (given the poses) and `disps_var_pose` (what pose uncertainty adds) - and the diagonal 6 x 6 blocks of the window's
pose covariance `poses_cov` (include/pvo_hip.h, pvo_ba_uncertainty).  The three buffers are allocated on first use
(`ensure_uncertainty`, +inf = never estimated) and travel with their keyframe; a video that never asks allocates nothing.
`map_points(max_rel_sigma=...)` filters the map by them and returns each point's sigma.

Calibration: `ba_calib(...)`, on `ba(...)`'s operands, is the depth BA with the four intrinsics as unknowns shared by all frames
(include/pvo_hip.h, pvo_ba_calib).  It runs on `intrinsics[0]`; once a step has been ACCEPTED - decided on the device, without a host
synchronisation: row 0 moved - the result is copied into every row IN PLACE (captured graphs and the native update hold the buffer's
pointer) and the device flag `calibrated_dev` is set: from then on `append` and `video[k] = ...` keep the calibrated vector instead of
the caller's, whose stale guess `reproject` would otherwise read per frame.  While every step was rejected the rows and the flag stay
as they were and the caller's vectors are still written.  `calibrated` is the host-side "ba_calib has run": a video that never
calibrates launches nothing more and behaves as before.

Surface: `tsdf(voxel, ...)` fuses the pixels `map_points` would keep into a truncated signed distance volume, weighted by
`fusion_weights` (the per-cell sigma as a weight, not a threshold), and returns its surface-nets mesh (include/pvo_hip.h,
pvo_tsdf_integrate / pvo_tsdf_mesh).  Read only: the video is unchanged.
"""
import math

import torch

from . import droid_backends as db


class StaticTermPool:
    """The ConvGRU's static-input terms conv(W[:, inp], inp), one row per KEYFRAME: P_zr [buffer,256,h,w], P_q [buffer,128,h,w],
    channels-last ([buffer,h,w,C] in memory), in the update operator's 16-bit type.

    The terms are a function of a keyframe's context features `inps[f]` and the packed weights only, so every factor graph on a video
    shares one pool (`DepthVideo.static_pool`) and an edge reads the row of its source frame (pvo_graph_update_rows' static_rows).
    A row is valid while the stamp it was computed at is still the frame's `DepthVideo` stamp: `ensure(frames)` computes the rows
    that are not, contiguous runs of frames in one pvo_conv3x3 call per term, written straight into the pool.  `computed` counts
    the frames convolved so far."""

    def __init__(self, video, weights, dtype):
        n, h8, w8 = video.inps.shape[0], video.ht // 8, video.wd // 8
        self.video, self.weights, self.serial, self.dtype = video, weights, weights.serial, dtype
        self.P_zr = torch.empty(n, h8, w8, 256, dtype=dtype, device=video.device).permute(0, 3, 1, 2)
        self.P_q = torch.empty(n, h8, w8, 128, dtype=dtype, device=video.device).permute(0, 3, 1, 2)
        self.row_stamp = [-1] * n        # the frame's stamp its row was computed at (-1: never)
        self.epoch = video._inps_epoch
        self.computed = 0
        self.ready, self.ready_serial = None, 0      # event behind the latest computation / copy, and how many there have been

    def valid(self, f):
        v = self.video
        v._inps_foreign_check()
        return self.epoch == v._inps_epoch and self.row_stamp[f] == v._inp_stamp[f]

    def _mark(self):
        if self.video.device.type == "cuda":
            self.ready = torch.cuda.Event()
            self.ready.record(torch.cuda.current_stream(self.video.device))
        self.ready_serial += 1

    def _compute(self, a, b):
        """rows [a, b) from the frames' slab of `inps` (contiguous channels-last images), one call per term"""
        x = self.video.inps[a:b]
        if x.dtype != self.dtype:
            x = x.to(self.dtype).contiguous(memory_format=torch.channels_last)
        db.conv3x3(x, self.weights.tensors["zr_inp_w"], out=self.P_zr[a:b])
        db.conv3x3(x, self.weights.tensors["q_inp_w"], out=self.P_q[a:b])

    def ensure(self, frames):
        """rows of `frames` (host ints) valid on the current stream; returns the number of frames computed"""
        v = self.video
        v._inps_foreign_check()
        if self.epoch != v._inps_epoch:
            self.row_stamp = [-1] * len(self.row_stamp)
            self.epoch = v._inps_epoch
        need = sorted({int(f) for f in frames if self.row_stamp[int(f)] != v._inp_stamp[int(f)]})
        k = 0
        while k < len(need):
            a = b = need[k]
            while k + 1 < len(need) and need[k + 1] == b + 1:
                k += 1; b += 1
            k += 1
            self._compute(a, b + 1)
            for f in range(a, b + 1):
                self.row_stamp[f] = v._inp_stamp[f]
        if need:
            self.computed += len(need)
            self._mark()
        return len(need)

    def shift(self, ix, stamp):
        """rm_keyframe: row ix + 1 moves to ix with its validity (`stamp`: frame ix's new stamp)"""
        self.P_zr[ix] = self.P_zr[ix + 1].clone()
        self.P_q[ix] = self.P_q[ix + 1].clone()
        ok = self.epoch == self.video._inps_epoch and self.row_stamp[ix + 1] == self.video._inp_stamp[ix + 1]
        self.row_stamp[ix] = stamp if ok else -1
        self._mark()


class DepthVideo:
    def __init__(self, image_size=(480, 640), buffer=1024, device="cuda:0", segm_filter=False, thresh=0.8,
                 store_images=False, store_segment_ids=False):
        self.counter = 0
        self.ht, self.wd = ht, wd = int(image_size[0]), int(image_size[1])
        self.device = torch.device(device)
        h8, w8 = ht // 8, wd // 8
        kw = dict(device=self.device)
        self.tstamp = torch.zeros(buffer, dtype=torch.float, **kw)
        self.images = torch.zeros(buffer, 3, ht, wd, dtype=torch.uint8, **kw) if store_images else None
        self.dirty = torch.zeros(buffer, dtype=torch.bool, **kw)
        self.poses = torch.zeros(buffer, 7, dtype=torch.float, **kw)
        self.poses[:, 6] = 1.0                                   # identity (depth_video.py:49-50)
        self.disps = torch.ones(buffer, h8, w8, dtype=torch.float, **kw)
        self.disps_up = None
        self.disps_sens = None             # RGB-D: measured inverse depth per keyframe [buffer,H/8,W/8], 0 = none (ensure_disps_sens)
        self.has_sensor_depth = False      # host-side: some keyframe brought a depth image
        self.sensor_alpha = 0.05           # weight of the sensor-depth prior (upstream's alpha)
        # uncertainty (ensure_uncertainty): inverse-depth variance given the poses / added by the poses [buffer,H/8,W/8], +inf = never
        # estimated, and the diagonal blocks of the window's pose covariance [buffer,6,6] fp64
        self.disps_var_cond = self.disps_var_pose = self.poses_cov = None
        self.intrinsics = torch.zeros(buffer, 4, dtype=torch.float, **kw)
        self.calibrated = False            # host side: ba_calib has run on this video (calibrated_dev says whether a step was accepted)
        self.calibrated_dev = None         # device bool [1]: a calibrating step was accepted - every row holds the calibrated vector and keeps it
        self.fmaps = torch.zeros(buffer, h8, w8, 128, dtype=torch.half, **kw)      # channels-last
        self.fmaps_right = None            # stereo: the right views' feature maps [buffer,H/8,W/8,128] channels-last (ensure_fmaps_right)
        self.stereo_baseline = 0.1         # the rig's baseline in the units of the poses' translations (upstream's constant)
        # [buffer,128,h,w] as the reference has them, stored channels-last: an edge's rows are gathered straight into the
        # layout the update operator reads (factor_graph.py add_factors)
        self.nets = torch.zeros(buffer, h8, w8, 128, dtype=torch.half, **kw).permute(0, 3, 1, 2)
        self.inps = torch.zeros(buffer, h8, w8, 128, dtype=torch.half, **kw).permute(0, 3, 1, 2)
        # who wrote `inps` last, for the per-keyframe static GRU terms (StaticTermPool): a stamp per frame, bumped where THIS class
        # writes the frame; `inps._version` as of our last write - if it moved otherwise somebody wrote the buffer directly, and
        # every frame's terms are invalid (a new epoch)
        self._inp_stamp = [0] * buffer
        self._inp_clock = 0
        self._inps_epoch = 0
        self._inps_seen = self.inps._version
        self._static = None
        self.segms = torch.zeros(buffer, 1, h8, w8, dtype=torch.int, **kw)
        # the frames' panoptic ids as given (segms relabels every frame on its own): what tsdf(panoptic=True) fuses; <= 0 = no segment
        self.segms_raw = torch.zeros(buffer, h8, w8, dtype=torch.int32, **kw) if store_segment_ids else None
        self.full_flow = torch.ones(buffer, h8, w8, 2, dtype=torch.float, **kw)
        self.segm_filter, self.thresh = segm_filter, thresh
        self.max_segments = 1024
        self._segments_seen = 1            # the largest number of dense labels any stored frame has had (segments_bound)
        # feature maps of EVERY tracked frame by time stamp (keyframe or not): the motion filter computes them anyway, the
        # trajectory filler needs them again at the end (trajectory_filler.py:32-38 re-encodes every image).  0.78 MB per
        # 240 x 808 frame: a 10 000-frame sequence is 7.8 GB of the 288 GB - kept resident instead of recomputed, up to this budget
        # Every entry carries a fingerprint of the frame it was computed from (`frame_fingerprint`), which the filler checks: a
        # terminate() stream that reuses time stamps with other images (another stride, resize, sequence) is re-encoded, as the
        # reference always does.  The budget is a tenth of the device memory (at most 32 GiB); entries are released as the filler
        # consumes them and the rest when it is done (`forget_features`).
        self.frame_fmaps = {}
        self.frame_fmaps_budget = 32 << 30
        if torch.device(device).type == "cuda" and torch.cuda.is_available():
            self.frame_fmaps_budget = min(self.frame_fmaps_budget, torch.cuda.mem_get_info(torch.device(device))[1] // 10)
        self._frame_fmaps_bytes = 0

    # ------------------------------------------------------------------ bookkeeping
    def _inps_foreign_check(self):
        """a write to `inps` that did not go through this class (torch's version counter moved): every frame's static terms are invalid"""
        if self.inps._version != self._inps_seen:
            self._inps_epoch += 1
            self._inps_seen = self.inps._version

    def _write_inps(self, index, value):
        """inps[index] = value, stamped: the frames written get a new stamp (an index that is not an int: all of them)"""
        self._inps_foreign_check()
        self.inps[index] = value
        self._inps_seen = self.inps._version
        self._inp_clock += 1
        if isinstance(index, int):
            self._inp_stamp[index] = self._inp_clock
        else:
            self._inp_stamp = [self._inp_clock] * len(self._inp_stamp)

    def shift_inps(self, ix):
        """rm_keyframe's frame shift of `inps` (row ix + 1 to ix), and of the static-term pool's rows with it"""
        self._write_inps(ix, self.inps[ix + 1].clone())
        if self._static is not None:
            self._static.shift(ix, self._inp_stamp[ix])

    def static_pool(self, weights, dtype):
        """the per-keyframe static GRU terms of this video for the packed weights `weights` (a PackedWeights) in `dtype`, allocated on
        first use: 768 bytes per pixel and frame.  Other weights or another dtype start a new pool (every row invalid)."""
        st = self._static
        if st is None or st.serial != weights.serial or st.dtype != dtype:
            st = self._static = StaticTermPool(self, weights, dtype)
        return st

    def _fmap_cl(self, f, channels_last):
        """feature map -> the stored channels-last layout.  The layout is taken from the shape wherever that is
        unambiguous ([..,128,h,w] vs [..,h,w,128] with h,w of THIS video); for maps that are 128 wide or high pass
        channels_last explicitly (MotionFilter / the trajectory filler produce the reference's [128,h,w])."""
        h8, w8 = self.ht // 8, self.wd // 8
        if channels_last is None:
            is_cl = tuple(f.shape[-3:]) == (h8, w8, 128)
            is_cf = tuple(f.shape[-3:]) == (128, h8, w8)
            if is_cl == is_cf:
                if is_cl:
                    raise ValueError("feature map layout is ambiguous for a %dx%d map: pass channels_last=True/False" % (h8, w8))
                raise ValueError("feature map of shape %s fits neither [128,%d,%d] nor [%d,%d,128]" % (tuple(f.shape), h8, w8, h8, w8))
            channels_last = is_cl
        return f if channels_last else f.movedim(-3, -1)

    def _dense_segments(self, segm):
        """panoptic ids -> dense per-frame labels in [0, max_segments) with 0 kept as 'no segment'.  The reference keys the
        vote by lay * 1e6 + id (factor_graph.py:259), i.e. by the raw id; raw ids (R + 256 G + 65536 B, category * 1000 +
        instance, ...) do not fit a histogram, and only the grouping inside one frame matters to the vote."""
        if isinstance(segm, torch.Tensor) and not segm.is_cuda and self.device.type == "cuda" and segm.numel() <= (1 << 16):
            # a frame's ids arrive on the host (test_vo.py hands over numpy / CPU tensors) and are a few thousand integers: relabelled
            # THERE and sent up through the pinned staging ring.  On the device torch.unique is ~15 launches and reads its result's size
            # back - with the blocking upload in front of it 0.9 ms per keyframe of waiting for whatever the stream still held (1.3 ms
            # in the pipelined tracker: the previous keyframe's graph updates).
            import numpy as np
            seg_h = segm.numpy().astype(np.int64, copy=False)
            u_h, inv_h = np.unique(seg_h, return_inverse=True)
            shift = 1 if u_h.size and int(u_h[0]) != 0 else 0
            n = int(u_h.size) + shift
            if n > self.max_segments:
                raise ValueError("frame has %d panoptic segments, more than max_segments = %d" % (n, self.max_segments))
            self._segments_seen = max(self._segments_seen, n)
            lab = torch.from_numpy((inv_h.reshape(seg_h.shape) + shift).astype(np.int32))
            return db.to_device_async(lab, torch.int32, self.device)
        seg = torch.as_tensor(segm, device=self.device).to(torch.int64)
        u, inv = torch.unique(seg, return_inverse=True)
        if u.numel() and int(u[0]) != 0:
            inv = inv + 1
        n = int(u.numel()) + (1 if u.numel() and int(u[0]) != 0 else 0)
        if n > self.max_segments:
            raise ValueError("frame has %d panoptic segments, more than max_segments = %d" % (n, self.max_segments))
        self._segments_seen = max(self._segments_seen, n)
        return inv.to(torch.int32).reshape(seg.shape)

    def _raw_segments(self, segm, shape):
        """a frame's (or several frames') panoptic ids unmodified, as int32 of `shape` on the device; ids outside int32 are an error"""
        seg = torch.as_tensor(segm)
        if seg.is_floating_point() or seg.dtype == torch.bool:
            raise ValueError("panoptic ids must be integers, got %s" % seg.dtype)
        if seg.numel() and seg.dtype not in (torch.int32, torch.int16, torch.int8, torch.uint8):
            lo, hi = int(seg.min()), int(seg.max())
            if lo < -(1 << 31) or hi > (1 << 31) - 1:
                raise ValueError("panoptic ids in [%d, %d] do not fit int32 (store_segment_ids)" % (lo, hi))
        return seg.to(device=self.device, dtype=torch.int32).reshape(shape)

    @staticmethod
    def frame_fingerprint(image):
        """what identifies a frame for the feature cache: its shape, dtype and the sum of a ~100-pixel lattice of its values, taken
        where the frame lies (a few hundred elements: no OpenMP team is woken on the host, no kernel worth naming on the device)"""
        if not isinstance(image, torch.Tensor):
            return None
        h, w = image.shape[-2], image.shape[-1]
        sample = image[..., h // 11::max(1, h // 7), w // 13::max(1, w // 11)]
        return (tuple(image.shape), str(image.dtype), float(sample.double().sum()))

    def remember_features(self, tstamp, fmap, image=None):
        """keep a tracked frame's feature map [..,128,h,w] (a copy) for the trajectory filler; `image`: the frame it came from"""
        n = fmap.numel() * fmap.element_size()
        if self.frame_fmaps_budget <= 0 or self._frame_fmaps_bytes + n > self.frame_fmaps_budget:
            return
        old = self.frame_fmaps.pop(float(tstamp), None)
        if old is not None:
            self._frame_fmaps_bytes -= old[0].numel() * old[0].element_size()
        self.frame_fmaps[float(tstamp)] = (fmap.detach().clone(), self.frame_fingerprint(image) if image is not None else None)
        self._frame_fmaps_bytes += n

    def recall_features(self, tstamp, image=None):
        """the kept feature map of the frame tracked under `tstamp` if `image` is that frame (same fingerprint), else None.  The
        entry is released either way: a frame's pose is filled once."""
        hit = self.frame_fmaps.pop(float(tstamp), None)
        if hit is None:
            return None
        fmap, fp = hit
        self._frame_fmaps_bytes -= fmap.numel() * fmap.element_size()
        if fp is None or image is None or fp != self.frame_fingerprint(image):
            return None
        return fmap

    def forget_features(self):
        self.frame_fmaps.clear()
        self._frame_fmaps_bytes = 0

    def segments_bound(self):
        """the histogram width the panoptic vote needs: a power of two above every dense label stored so far (at least 16, at most
        max_segments) - a frame has tens of segments, and a 1024-wide table per edge is filled and cleared in every update"""
        b = 16
        while b < self._segments_seen:
            b *= 2
        return max(1, min(self.max_segments, b))

    @property
    def has_stereo(self):
        """host-side: some keyframe brought a right view and the baseline is positive - edges (i, i) are stereo edges"""
        return self.fmaps_right is not None and self.stereo_baseline > 0

    def rig_baseline(self):
        """the baseline the native calls get: stereo_baseline on a stereo video, else 0 (no stereo edges)"""
        return float(self.stereo_baseline) if self.has_stereo else 0.0

    def ensure_fmaps_right(self):
        """the right views' feature maps [buffer, H/8, W/8, 128] fp16 channels-last, allocated on first use"""
        if self.fmaps_right is None:
            self.fmaps_right = torch.zeros_like(self.fmaps)
        return self.fmaps_right

    def ensure_disps_sens(self):
        """the sensor inverse depths [buffer, H/8, W/8], allocated (zero = no measurement) on first use"""
        if self.disps_sens is None:
            self.disps_sens = torch.zeros_like(self.disps)
        return self.disps_sens

    def ensure_uncertainty(self):
        """the variance maps [buffer, H/8, W/8] (+inf: never estimated) and the pose covariance blocks [buffer, 6, 6] fp64 (+inf on
        the diagonals), allocated on first use -> (disps_var_cond, disps_var_pose, poses_cov)"""
        if self.disps_var_cond is None:
            self.disps_var_cond = torch.full_like(self.disps, float("inf"))
            self.disps_var_pose = torch.full_like(self.disps, float("inf"))
            self.poses_cov = torch.zeros(self.disps.shape[0], 6, 6, dtype=torch.float64, device=self.device)
            self.poses_cov.diagonal(dim1=1, dim2=2).fill_(float("inf"))
        return self.disps_var_cond, self.disps_var_pose, self.poses_cov

    def reset_uncertainty(self, index):
        """keyframe(s) `index` got a new depth map: what was estimated for the old one no longer holds"""
        if self.disps_var_cond is not None:
            self.disps_var_cond[index] = float("inf")
            self.disps_var_pose[index] = float("inf")
            self.poses_cov[index] = torch.diag(torch.full((6,), float("inf"), dtype=torch.float64, device=self.device))

    @staticmethod
    def sense_depth_host(depth):
        """a host depth image [H,W] -> its inverse depth on the 1/8 lattice [H/8,W/8] fp32: 1 / depth[3::8, 3::8] where that is
        finite and > 0, else 0 (upstream DROID-SLAM's ingest; pvo_depth_sense is the same on the device)"""
        d = torch.as_tensor(depth)
        h8, w8 = d.shape[-2] // 8, d.shape[-1] // 8
        d = d[..., 3::8, 3::8][..., :h8, :w8].to(torch.float32)
        ok = torch.isfinite(d) & (d > 0)
        return torch.where(ok, 1.0 / torch.where(ok, d, torch.ones_like(d)), torch.zeros_like(d))

    def set_depth(self, k, depth):
        """keyframe k's sensor map from a depth image [H,W] at image resolution (None: no measurement for this keyframe)"""
        if depth is None:
            if self.disps_sens is not None:
                self.disps_sens[k].zero_()
            return
        sens = self.ensure_disps_sens()
        depth = torch.as_tensor(depth)
        if depth.dim() == 3 and depth.shape[0] == 1:
            depth = depth[0]
        if tuple(depth.shape) != (self.ht, self.wd):
            raise ValueError("depth image of shape %s for a %dx%d video" % (tuple(depth.shape), self.ht, self.wd))
        if depth.is_cuda:
            if depth.dtype not in (torch.float32, torch.float16):
                depth = depth.float()
            db.depth_sense(depth.contiguous(), sens[k])
        else:
            # a host image: sampled THERE (1/64 of its pixels) and sent up through the pinned staging ring - no blocking transfer
            sens[k] = db.to_device_async(self.sense_depth_host(depth), torch.float32, self.device)
        self.has_sensor_depth = True

    def append(self, tstamp, pose, disp, intrinsics, fmap, net, inp, segm=None, image=None, channels_last=None, depth=None,
               right_fmap=None):
        """store one keyframe; fmap may be [128,h,w] (reference layout) or [h,w,128] (see _fmap_cl).  depth: the frame's sensor
        depth image [H,W] (RGB-D, see set_depth); None leaves the video as it is - nothing is allocated for it.  right_fmap: the
        feature map of the frame's right view (stereo), in fmap's layouts; None likewise allocates nothing."""
        k = self.counter
        if right_fmap is not None:
            self.ensure_fmaps_right()[k] = self._fmap_cl(right_fmap, channels_last)
        elif self.fmaps_right is not None:
            self.fmaps_right[k].zero_()        # (a stale row, as rm_keyframe leaves one)
        if depth is not None or self.disps_sens is not None:
            self.set_depth(k, depth)
        self.reset_uncertainty(slice(k, k + 1))
        # (a Python number goes in with fill_ on a slice - a kernel argument.  `buf[k] = number` builds a host tensor and copies it with a
        # BLOCKING transfer queued behind everything on the stream: measured 1.3 ms per keyframe in the pipelined tracker)
        if isinstance(tstamp, torch.Tensor):
            self.tstamp[k] = tstamp
        else:
            self.tstamp[k:k + 1].fill_(float(tstamp))
        if pose is not None:
            self.poses[k] = pose
        if disp is not None:
            if isinstance(disp, torch.Tensor):
                self.disps[k] = disp
            else:
                self.disps[k:k + 1].fill_(float(disp))
        self.intrinsics[k] = self._kept_intrinsics(intrinsics)
        self.fmaps[k] = self._fmap_cl(fmap, channels_last)
        self.nets[k] = net
        self._write_inps(k, inp)
        if segm is not None:
            self.segms[k] = self._dense_segments(segm).reshape(self.segms[k].shape)
            if self.segms_raw is not None:
                self.segms_raw[k] = self._raw_segments(segm, self.segms_raw[k].shape)
        if image is not None and self.images is not None:
            self.images[k] = image
        self.counter = k + 1

    def __setitem__(self, index, item):
        """video[index] = (tstamp, image, pose, disp, intrinsics[, fmap[, net[, inp[, segm[, depth]]]]]) with None = keep
        (depth_video.py:64-101).  The counter grows to cover an int index; fmap may be NCHW or channels-last.  depth (an int
        index only): the keyframe's sensor depth image [H,W], as upstream DROID-SLAM's extra item."""
        if len(item) > 9 and item[9] is not None:
            if not isinstance(index, int):
                raise ValueError("a depth image is set for one keyframe at a time")
            self.set_depth(index, item[9])
        if isinstance(index, int) and index >= self.counter:
            self.counter = index + 1
        self.tstamp[index] = torch.as_tensor(item[0], dtype=torch.float, device=self.device)
        if item[1] is not None and self.images is not None:
            self.images[index] = item[1].to(self.images.dtype)
        for buf, val in ((self.poses, item[2]), (self.disps, item[3]), (self.intrinsics, item[4])):
            if val is not None:
                buf[index] = self._kept_intrinsics(val) if buf is self.intrinsics else val
        if item[3] is not None:
            self.reset_uncertainty(slice(index, index + 1) if isinstance(index, int) else index)
        if len(item) > 5 and item[5] is not None:
            self.fmaps[index] = self._fmap_cl(item[5], None)
        if len(item) > 6:
            self.nets[index] = item[6]
        if len(item) > 7:
            self._write_inps(index, item[7])
        if self.segm_filter and len(item) > 8 and item[8] is not None:
            if self.segms_raw is not None:
                self.segms_raw[index] = self._raw_segments(item[8], self.segms_raw[index].shape)
            seg = torch.as_tensor(item[8], device=self.device)
            if isinstance(index, int) or seg.dim() <= 3:
                self.segms[index] = self._dense_segments(seg).reshape(self.segms[index].shape)
            else:                                           # several frames at once: labels are per frame
                self.segms[index] = torch.stack([self._dense_segments(x) for x in seg]).reshape(self.segms[index].shape)

    def _kept_intrinsics(self, value):
        """what `append` / `video[k] = ...` store for a caller's intrinsics: the caller's, or - on a video whose calibration was
        accepted (the device flag; no host synchronisation) - the calibrated vector"""
        if not self.calibrated:
            return value
        value = torch.as_tensor(value, dtype=torch.float, device=self.device)
        return torch.where(self.calibrated_dev, self.intrinsics[0], value)

    def __getitem__(self, index):
        """(pose, disp, intrinsics, fmap, net, inp) of a keyframe; negative ints count from the end (:103-121)"""
        if isinstance(index, int) and index < 0:
            index = self.counter + index
        return (self.poses[index], self.disps[index], self.intrinsics[index], self.fmaps[index], self.nets[index],
                self.inps[index])

    def normalize(self):
        """rescale so the mean inverse depth of the stored keyframes is 1 (depth_video.py:145-152)"""
        n = self.counter
        s = self.disps[:n].mean()
        self.disps[:n] /= s
        self.poses[:n, :3] *= s
        self.dirty[:n] = True

    def ensure_disps_up(self):
        """the full-resolution inverse depths [buffer, H, W], allocated on first use (most runs never ask for them)"""
        if self.disps_up is None:
            self.disps_up = torch.zeros(self.disps.shape[0], self.ht, self.wd, dtype=torch.float, device=self.device)
        return self.disps_up

    def upsample(self, ix, mask):
        """convex 8x upsampling of the inverse depth of keyframes ix (depth_video.py:139-143): disps_up[ix] from disps[ix] and the
        logits mask [len(ix), 576, h, w] (planar, or channels-last as the native update operator writes them).  On the device one
        native kernel reads rows ix of disps and writes rows ix of disps_up in place (ix: a tensor or a host sequence, each frame
        once); on the host the PyTorch formulation."""
        up = self.ensure_disps_up()
        if self.device.type == "cuda":
            if isinstance(ix, torch.Tensor):
                ix = ix.to(device=self.device, dtype=torch.long).reshape(-1).contiguous()
            if mask.dim() == 5 and mask.shape[0] == 1:
                mask = mask[0]
            db.cvx_upsample(self.disps.unsqueeze(-1), mask, out=up.unsqueeze(-1), in_rows=ix, out_rows=ix)
            return
        from .droid_net import cvx_upsample
        ix = torch.as_tensor(ix, dtype=torch.long, device=self.device)
        mask = mask.reshape(-1, 576, self.ht // 8, self.wd // 8).float().contiguous()
        up[ix] = cvx_upsample(self.disps[ix].unsqueeze(-1), mask).squeeze(-1)

    @staticmethod
    def format_indicies(ii, jj, device):
        if not isinstance(ii, torch.Tensor):
            ii = torch.as_tensor(ii)
        if not isinstance(jj, torch.Tensor):
            jj = torch.as_tensor(jj)
        return (ii.to(device=device, dtype=torch.long).reshape(-1).contiguous(),
                jj.to(device=device, dtype=torch.long).reshape(-1).contiguous())

    # ------------------------------------------------------------------ native calls
    def reproject(self, ii, jj):
        """project points ii -> jj (depth_video.py:154-163): coords [1,E,h,w,2], valid [1,E,h,w,1]"""
        ii, jj = self.format_indicies(ii, jj, self.device)
        coords, valid = db.reproject(self.poses, self.disps, self.intrinsics, ii, jj, **self._rig_kw("baseline"))
        return coords[None], valid[None]

    def reproject_into(self, ii, jj, coords_out):
        """reproject(ii, jj)[0][0] written into coords_out [E,h,w,2] (device tensors only)"""
        ii, jj = self.format_indicies(ii, jj, self.device)
        db.reproject(self.poses, self.disps, self.intrinsics, ii, jj, out=coords_out, **self._rig_kw("baseline"))

    def _rig_kw(self, name):
        """{name: baseline} on a stereo video, {} otherwise: the native call is then exactly the one a monocular video makes"""
        return {name: float(self.stereo_baseline)} if self.has_stereo else {}

    def distance(self, ii=None, jj=None, beta=0.3, bidirectional=True):
        """frame distance metric (depth_video.py:165-195)"""
        return_matrix = ii is None
        if return_matrix:
            N = self.counter
            grid = self.__dict__.get("_grid")
            if grid is None or grid[0] != N:                       # (the N x N index grid: uploaded once per window size)
                gi, gj = torch.meshgrid(torch.arange(N), torch.arange(N), indexing="ij")
                both = db.to_device_async(torch.cat([gi.reshape(-1), gj.reshape(-1)]), torch.long, self.device)
                grid = self.__dict__["_grid"] = (N, both[:N * N], both[N * N:])
            ii, jj = grid[1], grid[2]
        if not (isinstance(ii, torch.Tensor) and ii.is_cuda):      # host index lists: staged through the pinned ring, no stream drain
            ii_h = torch.as_tensor(ii, dtype=torch.long).reshape(-1)
            jj_h = torch.as_tensor(jj, dtype=torch.long).reshape(-1)
            both = db.to_device_async(torch.cat([ii_h, jj_h]), torch.long, self.device)
            ii, jj = both[:ii_h.numel()], both[ii_h.numel():]
        ii, jj = self.format_indicies(ii, jj, self.device)
        if bidirectional and self.poses.is_cuda:
            # both directions and their mean in one launch, bit-identical to the two calls below (which remain the host /
            # test formulation: the reference's call sequence is pinned on them)
            d = db.frame_distance_bidirectional(self.poses, self.disps, self.intrinsics[0], ii, jj, beta)
        elif bidirectional:
            poses = self.poses[:self.counter]              # (the reference clones them, depth_video.py:183; the kernel only reads)
            d1 = db.frame_distance(poses, self.disps, self.intrinsics[0], ii, jj, beta)
            d2 = db.frame_distance(poses, self.disps, self.intrinsics[0], jj, ii, beta)
            d = 0.5 * (d1 + d2)
        else:
            d = db.frame_distance(self.poses, self.disps, self.intrinsics[0], ii, jj, beta)
        return d.reshape(N, N) if return_matrix else d

    def sigma_disp(self):
        """sqrt(var_cond + var_pose) [buffer, H/8, W/8]: the standard deviation of the inverse depths (+inf where never estimated)"""
        if self.disps_var_cond is None:
            raise RuntimeError("no uncertainty has been estimated on this video (DepthVideo.uncertainty / args.uncertainty = True)")
        return torch.sqrt(self.disps_var_cond + self.disps_var_pose)

    @staticmethod
    def rel_sigma_reject(sigma, disps, max_rel_sigma, reject=None):
        """the map export's reject mask [.., H/8, W/8] (bool) of a bound on the RELATIVE standard deviation: sigma / disp >
        max_rel_sigma (relative depth error = relative inverse-depth error to first order; a never-estimated +inf cell is rejected),
        OR a caller's own mask ([buffer, H/8, W/8] or [buffer, 1, H/8, W/8], nonzero = reject)"""
        m = ~(sigma <= float(max_rel_sigma) * disps)              # (NaN and +inf reject)
        if reject is not None:
            r = reject if reject.dim() == m.dim() else reject.reshape(m.shape)
            m = m | (r != 0)
        return m

    def map_points(self, ix=None, thresh=0.005, full_res=False, dirty_only=False, reject=None, max_rel_sigma=None):
        """the dense map of keyframes ix (default: all stored ones) as db.map_points returns it - the reference's viewer loop
        (visualization.py:76-134) without the viewer: points confirmed by two neighbouring keyframes within `thresh` (the viewer's
        filter_thresh) and nearer than twice the frame's mean depth, with colours when the video stores images (`store_images`; RGB
        zero otherwise) and the per-frame dense labels of `segms`.  full_res: from disps_up (tracking with args.upsample) with
        8 * intrinsics, colours at every pixel and labels at (y // 8, x // 8); otherwise from the 1/8 maps with the colours of
        [3::8, 3::8].  dirty_only: export where(dirty[:counter]) and clear those flags (the viewer's semantics).  reject: bool / uint8
        [buffer, H/8, W/8] or [buffer, 1, H/8, W/8]; nonzero cells are left out (dynamic objects, "thing" classes).
        max_rel_sigma (needs the variances of `uncertainty`): cells whose relative standard deviation sigma / disp exceeds it are
        left out as well - at 1/8 resolution, for full_res through the same (y // 8, x // 8) rule as the labels - and the result gains
        `sigma` [n], each point's standard deviation of the inverse depth (of its 1/8 cell)."""
        n = self.counter
        if dirty_only:
            if ix is not None:
                raise ValueError("dirty_only exports the dirty keyframes: no ix")
            ix = torch.where(self.dirty[:n])[0]
            self.dirty[ix] = False
        elif ix is None:
            ix = torch.arange(n, device=self.device)
        ix = torch.as_tensor(ix, dtype=torch.long, device=self.device).reshape(-1).contiguous()
        th = torch.full((ix.shape[0],), float(thresh), dtype=torch.float, device=self.device)
        if full_res:
            if self.disps_up is None:
                raise RuntimeError("map_points(full_res=True) needs the full-resolution depths of tracking with args.upsample = True "
                                   "(video.disps_up is not maintained)")
            disps, intr, stride, offset, div = self.disps_up, 8.0 * self.intrinsics[0], 1, 0, 8
        else:
            disps, intr, stride, offset, div = self.disps, self.intrinsics[0], 8, 3, 1
        sigma = None
        if max_rel_sigma is not None:
            sigma = self.sigma_disp()
            reject = self.rel_sigma_reject(sigma, self.disps, max_rel_sigma, reject).to(torch.uint8)
        out = db.map_points(self.poses, disps, intr.contiguous(), ix, th, images=self.images, img_stride=stride, img_offset=offset,
                            labels=self.segms, label_div=div, reject=reject)
        if sigma is not None:
            out["sigma"] = self.gather_sigma(sigma, out["src"], self.wd // 8, div)
        return out

    @staticmethod
    def gather_sigma(sigma, src, w8, div):
        """per map point the sigma of its 1/8 cell: src [n,2] = (keyframe, pixel index in the map the points were taken from -
        the 1/8 map, or for div = 8 the full-resolution one)"""
        frame, pix = src[:, 0].long(), src[:, 1].long()
        wd = w8 * div
        y, x = torch.div(pix, wd, rounding_mode="floor") // div, (pix % wd) // div
        return sigma[frame, y, x]

    @staticmethod
    def fusion_weights(keep, disps, sigma=None, rel0=0.05):
        """the TSDF fusion's per-pixel weights (f32, the shape of keep): `keep` itself, or with sigma - the standard deviation of the
        inverse depths, shaped like disps - keep / (1 + (sigma / (rel0 * disps))^2): a pixel whose relative standard deviation is rel0
        counts half, a confident one fully.  A non-finite sigma (a never-estimated cell) gives 0.  Works on CPU tensors."""
        w = keep.to(torch.float32)
        if sigma is None:
            return w
        w = w / (1.0 + (sigma / (float(rel0) * disps)) ** 2)
        return torch.where(torch.isfinite(sigma) & torch.isfinite(w), w, torch.zeros_like(w))

    @staticmethod
    def tsdf_bounds(xyz, voxel, trunc):
        """a volume around the points xyz [n,3]: per axis the 1st and 99th percentile - s[floor(0.01 (m-1))] and s[ceil(0.99 (m-1))] of
        the sorted values s of the strided subsample xyz[::ceil(n / 2^20)] (m points) - widened by trunc on both sides.  Returns
        (origin [x,y,z] as floats, (nz,ny,nx)) with dim = ceil((hi - lo + 2 trunc) / voxel) + 1.  Works on CPU tensors."""
        n = int(xyz.shape[0])
        if n == 0:
            raise ValueError("tsdf_bounds: no points")
        sub = xyz[::max(1, -(-n // (1 << 20)))].to(torch.float64)
        m = sub.shape[0]
        s = torch.sort(sub, dim=0).values
        lo, hi = s[int(math.floor(0.01 * (m - 1)))], s[int(math.ceil(0.99 * (m - 1)))]
        origin = [float(v) - float(trunc) for v in lo]
        dims = [int(math.ceil((float(h) - float(l) + 2.0 * float(trunc)) / float(voxel))) + 1 for l, h in zip(lo, hi)]
        return origin, (dims[2], dims[1], dims[0])

    @staticmethod
    def tsdf_sparse_bounds(xyz, voxel, trunc):
        """the brick world around the points xyz [n,3]: tsdf_bounds with the 0.1st and 99.9th percentile - the map's full extent but for
        stray points - and every axis rounded up to whole 8-voxel bricks.  Returns (origin [x,y,z] as floats, (gz,gy,gx) bricks); a
        ValueError where that is over the brick grid's limit (2^21 voxels per axis, fewer than 2^31 bricks).  Works on CPU tensors."""
        from .tsdf_sparse import AXIS_LIMIT, BRICK, GRID_LIMIT
        n = int(xyz.shape[0])
        if n == 0:
            raise ValueError("tsdf_sparse_bounds: no points")
        sub = xyz[::max(1, -(-n // (1 << 20)))].to(torch.float64)
        m = sub.shape[0]
        s = torch.sort(sub, dim=0).values
        lo, hi = s[int(math.floor(0.001 * (m - 1)))], s[int(math.ceil(0.999 * (m - 1)))]
        origin = [float(v) - float(trunc) for v in lo]
        dims = [int(math.ceil((float(h) - float(l) + 2.0 * float(trunc)) / float(voxel))) + 1 for l, h in zip(lo, hi)]
        g = [-(-d // BRICK) for d in dims]
        if max(g) > AXIS_LIMIT or g[0] * g[1] * g[2] >= GRID_LIMIT:
            raise ValueError("tsdf_sparse_bounds: %d x %d x %d voxels of %g are over the brick grid's limit (2^21 voxels per axis, fewer "
                             "than 2^31 bricks of 8^3): use a larger voxel" % (dims[0], dims[1], dims[2], float(voxel)))
        return origin, (g[2], g[1], g[0])

    def tsdf(self, voxel, trunc=None, ix=None, thresh=0.005, full_res=False, reject=None, use_sigma=False, origin=None, dims=None,
             min_weight=1.0, w_max=0, max_rel_sigma=None, rel0=0.05, sparse=False, margin=2, panoptic=False, keep_rgb=False,
             labels=None):
        """the fused surface of keyframes ix (default: all stored ones; a one-off fusion of the video as it stands - a volume that
        follows keyframes which move later is pvo_amd.live_map.LiveMap): a TSDF volume of `voxel`-sized cells, truncation `trunc` (default 3 voxels), integrated natively
        (pvo_tsdf_integrate) from exactly the pixels map_points(ix, thresh, full_res, reject, max_rel_sigma) keeps, and its surface-nets
        mesh (pvo_tsdf_mesh).  use_sigma (needs the variances of `uncertainty`): pixels are weighted by fusion_weights(keep, disps,
        sigma, rel0), sigma at the 1/8 cell for full_res.  origin [x,y,z] / dims (nz,ny,nx): the volume; default tsdf_bounds of the map's
        points.  Returns a dict: verts, normals, rgba, faces (the mesh; min_weight = the least wsum of a usable voxel), tsdf, wsum
        (the volume), origin, voxel.
        sparse=True: the same pixels and weights into a brick volume (pvo_amd.tsdf_sparse.SparseTSDF: bricks allocated within `margin`
        voxels of the samples along every kept pixel's ray, pvo_tsdf_sparse_allocate / _integrate / _mesh) - for maps a dense volume
        cannot hold.  The world defaults to tsdf_sparse_bounds of the map's points; given dims are rounded up to bricks.  Returns the
        mesh, origin, voxel and `volume`, the SparseTSDF, in place of tsdf / wsum.
        panoptic=True (a video made with store_segment_ids, ValueError otherwise): the frames' raw segment ids segms_raw[:n] are fused
        by a weighted vote per voxel (pvo_tsdf_integrate_panoptic; ids <= 0 = no segment) and every vertex gets the id of its cell's
        nearest labelled corner: the dict gains vlabel int32 [V] and the volumes label, lconf (sparse: the SparseTSDF holds them).
        labels (with panoptic=True): an int32 [counter,h/8,w/8] label tensor fused in place of segms_raw[:n] - e.g.
        pvo_amd.segment_tracks.SegmentTracks.track_map(), ids that stay the same across keyframes; then store_segment_ids is not needed.
        keep_rgb=True (dense, a video with images): the dict also keeps the colour volume rgb [nz,ny,nx,3], so that tsdf_render
        can colour its images (the SparseTSDF holds its own)."""
        trunc = 3.0 * float(voxel) if trunc is None else float(trunc)
        n = self.counter
        if panoptic and labels is None and self.segms_raw is None:
            raise ValueError("tsdf(panoptic=True) needs the raw segment ids: make the video with store_segment_ids=True")
        if labels is not None:
            if not panoptic:
                raise ValueError("tsdf(labels=...) goes with panoptic=True")
            if not torch.is_tensor(labels) or labels.dtype != torch.int32 or tuple(labels.shape) != tuple(self.disps[:n].shape):
                raise ValueError("tsdf(labels=...) must be an int32 tensor of shape %s" % (list(self.disps[:n].shape),))
            labels = labels.to(self.device).contiguous()
        else:
            labels = self.segms_raw[:n] if panoptic else None
        m = self.map_points(ix=ix, thresh=thresh, full_res=full_res, reject=reject, max_rel_sigma=max_rel_sigma)
        if full_res:
            disps, intr, stride, offset, div = self.disps_up[:n], 8.0 * self.intrinsics[0], 1, 0, 8
        else:
            disps, intr, stride, offset, div = self.disps[:n], self.intrinsics[0], 8, 3, 1
        ix = torch.arange(n, device=self.device) if ix is None else torch.as_tensor(ix, dtype=torch.long, device=self.device).reshape(-1)
        ix = ix[(ix >= 0) & (ix < n)].contiguous()
        keep = torch.zeros(disps.shape, dtype=torch.bool, device=self.device)
        src = m["src"].long()
        keep.view(n, -1)[src[:, 0], src[:, 1]] = True
        sigma = None
        if use_sigma:
            sigma = self.sigma_disp()[:n]
            if div > 1:
                sigma = sigma.repeat_interleave(div, 1).repeat_interleave(div, 2)
        weight = self.fusion_weights(keep, disps, sigma, rel0).contiguous()
        if sparse:
            from .tsdf_sparse import BRICK, SparseTSDF
            if origin is None or dims is None:
                origin, gdims = self.tsdf_sparse_bounds(m["xyz"], voxel, trunc)
            else:
                gdims = [-(-int(v) // BRICK) for v in dims]
            vol = SparseTSDF(origin, gdims, voxel, trunc, colours=self.images is not None, device=self.device, labels=panoptic)
            frames = (self.poses[:n], disps.contiguous(), intr.contiguous(), ix)
            vol.allocate(*frames, weight=weight, margin=margin)
            vol.integrate(*frames, weight=weight, images=self.images, img_stride=stride, img_offset=offset, w_max=w_max, labels=labels,
                          label_div=div)
            out = vol.mesh(min_weight=min_weight)
            out.pop("counts")
            out.update(volume=vol, origin=[float(v) for v in origin], voxel=float(voxel))
            return out
        if origin is None or dims is None:
            origin, dims = self.tsdf_bounds(m["xyz"], voxel, trunc)
        nz, ny, nx = [int(v) for v in dims]
        vol = torch.zeros(nz, ny, nx, dtype=torch.float32, device=self.device)
        wsum = torch.zeros_like(vol)
        rgb = torch.zeros(nz, ny, nx, 3, dtype=torch.float32, device=self.device) if self.images is not None else None
        label = torch.zeros(nz, ny, nx, dtype=torch.int32, device=self.device) if panoptic else None
        lconf = torch.zeros_like(vol) if panoptic else None
        db.tsdf_integrate(vol, wsum, rgb, self.poses[:n], disps.contiguous(), intr.contiguous(), ix, origin, voxel, trunc, weight=weight,
                          images=self.images, img_stride=stride, img_offset=offset, w_max=w_max, label=label, lconf=lconf, labels=labels,
                          label_div=div)
        out = db.tsdf_mesh(vol, wsum, rgb, origin, voxel, min_weight=min_weight, label=label)
        out.pop("counts")
        out.update(tsdf=vol, wsum=wsum, origin=[float(v) for v in origin], voxel=float(voxel))
        if keep_rgb and rgb is not None:
            out.update(rgb=rgb)
        if panoptic:
            out.update(label=label, lconf=lconf)
        return out

    def tsdf_render(self, volume, ix=None, poses=None, full_res=False, **kw):
        """the fused volume seen from cameras (pvo_tsdf_render / pvo_tsdf_sparse_render): `volume` is the dict `tsdf` returns - dense
        (tsdf, wsum, origin, voxel, with images rgb, with panoptic=True label) or with volume = the SparseTSDF.  Views: the stored
        keyframes ix (default: all) with the video's intrinsics at 1/8 resolution, or with full_res at image resolution (8 * intrinsics);
        or explicit poses [n,7] (world-to-camera), all of them rendered.  Returns a dict: depth [n,ht,wd], normal [n,ht,wd,3], rgba
        [n,ht,wd,4] and, for a panoptic volume, label [n,ht,wd].  kw: dz, z_near, z_far, min_weight, normals, out of
        droid_backends.tsdf_render."""
        if poses is None:
            n = self.counter
            ix = torch.arange(n, device=self.device) if ix is None else torch.as_tensor(ix, dtype=torch.long, device=self.device).reshape(-1)
            poses, ix = self.poses[:n], ix.contiguous()
        else:
            if ix is not None:
                raise ValueError("tsdf_render: explicit poses are all rendered, in their order: no ix")
            poses = torch.as_tensor(poses, dtype=torch.float32, device=self.device).reshape(-1, 7).contiguous()
            ix = torch.arange(poses.shape[0], device=self.device)
        scale = 8 if full_res else 1
        intr = (float(scale) * self.intrinsics[0]).contiguous()
        ht, wd = scale * (self.ht // 8), scale * (self.wd // 8)
        if "volume" in volume:
            return volume["volume"].render(poses, intr, ix, ht, wd, **kw)
        return db.tsdf_render(volume["tsdf"], volume["wsum"], volume.get("rgb"), volume["origin"], volume["voxel"], poses, intr, ix, ht, wd,
                              label=volume.get("label"), **kw)

    @staticmethod
    def depth_residual(disps, depth):
        """per frame of disps / depth [n,ht,wd] (a keyframe's own inverse depths and the model's rendered depth, 0 = no surface): the
        median and the 90th percentile of |1/disps - depth| / depth over the pixels where both exist (disps finite and > 0, depth > 0),
        and the share of pixels that do; NaN for a frame without such a pixel.  Returns three [n] float64 tensors.  Works on CPU tensors."""
        n = disps.shape[0]
        med, p90, share = [torch.full((n,), float("nan"), dtype=torch.float64, device=disps.device) for _ in range(3)]
        for k in range(n):
            d, z = disps[k].reshape(-1).double(), depth[k].reshape(-1).double()
            both = torch.isfinite(d) & (d > 0) & (z > 0)
            share[k] = both.double().mean() if both.numel() else 0.0
            if both.any():
                rel = (1.0 / d[both] - z[both]).abs() / z[both]
                q = torch.quantile(rel, torch.tensor([0.5, 0.9], dtype=torch.float64, device=rel.device))
                med[k], p90[k] = q[0], q[1]
        return med, p90, share

    def model_residual(self, volume, ix=None, full_res=False):
        """how well each keyframe's own depth agrees with the fused surface: the volume rendered at the keyframes ix (tsdf_render) against
        1/disps (disps_up with full_res) - a dict of ix and, per keyframe, median, p90 (of |1/disps - depth| / depth where both exist)
        and share (of pixels where both exist)"""
        r = self.tsdf_render(volume, ix=ix, full_res=full_res, normals=False)
        n = self.counter
        ix = torch.arange(n, device=self.device) if ix is None else torch.as_tensor(ix, dtype=torch.long, device=self.device).reshape(-1)
        own = (self.disps_up if full_res else self.disps)[ix.clamp(0, max(n - 1, 0))]
        med, p90, share = self.depth_residual(own, r["depth"])
        return {"ix": ix, "median": med, "p90": p90, "share": share}

    def tsdf_track(self, volume, ix=None, poses=None, disps=None, weight=None, full_res=False, **kw):
        """frame-to-model tracking (pvo_tsdf_track / pvo_tsdf_sparse_track): camera poses refined so that the frames' own depths lie on
        the fused surface.  `volume` is the dict `tsdf` returns (dense, or with volume = the SparseTSDF).  By default slot s tracks
        the stored keyframe ix[s] (default: all) from its own depth (disps, or disps_up with full_res) starting at its own pose.
        disps= [nframes,ht,wd]: any inverse-depth maps in place of the stored ones (for example disps_sens for RGB-D), at the 1/8
        resolution or with full_res at image resolution, ix then indexing them (default: all).  poses= [N,7]: explicit starts, ONE PER
        SLOT (several slots may track one frame from different starts).  weight like disps or None.  kw: iters, band, huber, lm, ep,
        min_count, min_weight, system, residual, jac, out of droid_backends.tsdf_track.  Returns its dict with ix added.  The video
        is never written."""
        n = self.counter
        if disps is None:
            disps = (self.disps_up if full_res else self.disps)[:n]
        disps = torch.as_tensor(disps, dtype=torch.float32, device=self.device).contiguous()
        nf = disps.shape[0]
        ix = torch.arange(nf, device=self.device) if ix is None else torch.as_tensor(ix, dtype=torch.long, device=self.device).reshape(-1)
        ix = ix.contiguous()
        if poses is None:
            if nf > n:
                raise ValueError("tsdf_track: %d depth maps but %d stored keyframes: pass poses, one start per slot" % (nf, n))
            poses = self.poses[:n][ix.clamp(0, max(n - 1, 0))]
        poses = torch.as_tensor(poses, dtype=torch.float32, device=self.device).reshape(-1, 7).contiguous()
        if poses.shape[0] != ix.shape[0]:
            raise ValueError("tsdf_track: %d starts for %d slots" % (poses.shape[0], ix.shape[0]))
        if weight is not None:
            weight = torch.as_tensor(weight, dtype=torch.float32, device=self.device).contiguous()
        intr = (float(8 if full_res else 1) * self.intrinsics[0]).contiguous()
        if "volume" in volume:
            out = volume["volume"].track(poses, disps, intr, ix, weight=weight, **kw)
        else:
            out = db.tsdf_track(volume["tsdf"], volume["wsum"], volume["origin"], volume["voxel"], poses, disps, intr, ix, weight=weight, **kw)
        out = dict(out)
        out["ix"] = ix
        return out

    def ba(self, target, weight, eta, ii, jj, t0=1, t1=None, itrs=2, lm=1e-4, ep=0.1, motion_only=False,
           t1_hint=None):
        """dense bundle adjustment (depth_video.py:197-214); in place on poses / disps"""
        if t1 is None:
            t1 = t1_hint if t1_hint is not None else int(max(ii.max().item(), jj.max().item())) + 1
        if eta is None and not motion_only:
            k = torch.unique(torch.cat([ii, jj], 0)).shape[0]
            eta = 1e-7 * torch.ones([k, self.ht // 8, self.wd // 8], device=self.device)
        # (RGB-D: the sensor-depth prior, once a keyframe has brought a depth image)
        kw = {"disps_sens": self.disps_sens, "alpha": self.sensor_alpha} if self.has_sensor_depth and not motion_only else {}
        kw.update(self._rig_kw("stereo_baseline"))      # (stereo: edges (i, i) under the rig's fixed transform)
        db.ba(self.poses, self.disps, self.intrinsics[0], target, weight, eta, ii, jj, t0, t1, itrs, lm, ep,
              motion_only, **kw)
        self.disps.clamp_(min=0.001)

    def ba_calib(self, target, weight, eta, ii, jj, t0=1, t1=None, itrs=2, lm=1e-4, ep=0.1, ep_c=0.1, free="all"):
        """online intrinsics calibration: `itrs` steps of the depth BA `ba(target, weight, eta, ii, jj, t0, t1, lm=lm, ep=ep)` with
        (fx, fy, cx, cy) free (free="all") or the focal lengths only ("focal"), damped by ep_c (pvo_ba_calib).  In place on poses, disps
        and - through row 0, then copied to every row once a step was accepted - intrinsics; a step the library rejects changes nothing.  Returns
        [dx, dz, dc, status] of the last step (device tensors; status[0] = 1: a step was rejected).  No host synchronisation.
        Not with the sensor-depth prior or stereo edges: the calibrating step has neither."""
        if self.has_sensor_depth or self._rig_kw("stereo_baseline"):
            raise NotImplementedError("DepthVideo.ba_calib: calibration together with the sensor-depth prior or stereo edges is not supported")
        if free not in ("all", "focal"):
            raise ValueError("free must be 'all' or 'focal', got %r" % (free,))
        if t1 is None:
            t1 = int(max(ii.max().item(), jj.max().item())) + 1
        status = torch.zeros(4, dtype=torch.int32, device=self.device)
        before = self.intrinsics[0].clone()
        out = db.ba_calib(self.poses, self.disps, self.intrinsics[0], target, weight, eta, ii, jj, t0, t1, itrs, lm, ep, ep_c,
                          db.BA_CALIB_FREE[free], status=status)
        self.disps.clamp_(min=0.001)
        # accepted = row 0 moved (status[0] says "some step was rejected", which an earlier accepted step of the same call survives).
        # In place and on the device: the same storage; every row the calibrated vector, or every row what it was
        moved = (self.intrinsics[0] != before).any().reshape(1)
        if self.intrinsics.shape[0] > 1:
            rest = self.intrinsics[1:]
            rest.copy_(torch.where(moved, self.intrinsics[0:1].expand_as(rest), rest))
        self.calibrated_dev = moved if self.calibrated_dev is None else (self.calibrated_dev | moved)
        self.calibrated = True
        return out + [status]

    def uncertainty(self, target, weight, eta, ii, jj, t0=1, t1=None, lm=1e-4, ep=0.1):
        """depth and pose uncertainty of the depth-BA step `ba(target, weight, eta, ii, jj, t0, t1, lm=lm, ep=ep)` would take from the
        present state, read only (pvo_ba_uncertainty): writes disps_var_cond / disps_var_pose on the optimised keyframes'
        rows and the diagonal blocks of the pose covariance into poses_cov[t0:t1]; returns the whole covariance [P,6,P,6] fp64.
        Honours the sensor-depth prior and the rig's baseline exactly as `ba` does."""
        if t1 is None:
            t1 = int(max(ii.max().item(), jj.max().item())) + 1
        vc, vp, pc = self.ensure_uncertainty()
        kw = {"disps_sens": self.disps_sens, "alpha": self.sensor_alpha} if self.has_sensor_depth else {}
        kw.update(self._rig_kw("stereo_baseline"))
        cov = db.ba_uncertainty(self.poses, self.disps, self.intrinsics[0], target, weight, eta, ii, jj, t0, t1, lm, ep,
                                var_cond=vc, var_pose=vp, **kw)
        if t1 > t0:
            pc[t0:t1] = torch.diagonal(cov, dim1=0, dim2=2).permute(2, 0, 1)
        return cov
