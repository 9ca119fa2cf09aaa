"""A TSDF map that exists while the camera moves: LiveMap fuses keyframes as they leave the frontend's window and, whenever a fused
keyframe's pose or depth has moved by more than a tolerance (the frontend's window moves them a little, the backend's global bundle
adjustment a lot), takes its OLD observation out of the running average and puts the new one in - one native pass over the volume
(include/pvo_hip.h pvo_tsdf_reintegrate / pvo_tsdf_sparse_reintegrate; BundleFusion's re-integration).  The ledger is what makes that
possible: per keyframe slot a snapshot of the pose, the depths and the weights it was fused with.

What LiveMap does not do: panoptic votes (a running majority cannot be inverted), full-resolution (disps_up) maps, freeing bricks a
removal emptied, the pipelined tracker, and exactness once a weight cap has been hit (it fuses without one).  A brick allocated for a
keyframe's new pose holds only what was fused after it existed.  The colours of a DROPPED slot are removed with the slot's present
picture (its successor's): approximate there; tsdf and wsum are not affected.  Its defaults tol, w_floor and lag rest on nothing
measured on real sequences."""
import torch

from . import droid_backends as db

# Not measured on real sequences, any of them: a quarter of a voxel is where a moved observation starts to blur a surface that is a
# voxel thick; 2^-10 is far above the ulps a removal leaves of weights of order 1 and far below any weight that counts (it must stay
# below min_weight); the lag is the frontend's window, inside which a keyframe can still be REMOVED, which shifts the slots behind it.
DEFAULT_TOL = 0.25
DEFAULT_W_FLOOR = 2.0 ** -10
DEFAULT_LAG = 25


def backproject(poses, disps, intrinsics):
    """world points [n,ht,wd,3] of every pixel of the frames: poses [n,7] world-to-camera (t, q as stored), disps [n,ht,wd],
    intrinsics [4].  Plain torch, fp32; a pixel without a positive finite inverse depth gives non-finite values."""
    n, ht, wd = disps.shape
    fx, fy, cx, cy = [intrinsics[k] for k in range(4)]
    y, x = torch.meshgrid(torch.arange(ht, device=disps.device, dtype=disps.dtype), torch.arange(wd, device=disps.device, dtype=disps.dtype),
                          indexing="ij")
    z = 1.0 / disps
    Xc = torch.stack([(x - cx) / fx * z, (y - cy) / fy * z, z], -1) - poses[:, None, None, :3]
    qx, qy, qz, qw = [poses[:, k, None, None] for k in (3, 4, 5, 6)]
    # R(q)^T applied: the rows of R as the contract writes it
    r = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
         [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
         [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]]
    return torch.stack([r[0][e] * Xc[..., 0] + r[1][e] * Xc[..., 1] + r[2][e] * Xc[..., 2] for e in range(3)], -1)


class LiveMap:
    def __init__(self, video, voxel, origin, dims, trunc=None, sparse=False, margin=2, thresh=0.005, use_sigma=False, rel0=0.05, reject=None,
                 min_weight=1.0, w_floor=DEFAULT_W_FLOOR, tol=DEFAULT_TOL, lag=None):
        """a volume of `voxel`-sized cells over the world box origin [x,y,z] / dims (nz,ny,nx) - required: the box of a running session
        is the caller's knowledge - fused from the 1/8-resolution maps of `video` (a DepthVideo).  trunc defaults to 3 voxels.  sparse:
        a brick volume (SparseTSDF, dims rounded up to bricks, bricks within `margin` voxels of the surfaces) in place of the dense
        tsdf / wsum / rgb (rgb when the video stores images).  thresh, reject, use_sigma, rel0: the pixels and weights of
        DepthVideo.tsdf - fusion_weights(keep, disps, sigma, rel0) with keep from map_points(ix=...)["src"].  tol (voxels): a fused
        keyframe is refreshed when its drift exceeds it; lag: the youngest `lag` keyframes are not fused yet (default DEFAULT_LAG, the
        frontend's window); w_floor: pvo_tsdf_reintegrate's, below min_weight.  See the module's note on these defaults."""
        if not float(w_floor) < float(min_weight):
            raise ValueError("LiveMap: w_floor = %g must stay below min_weight = %g - a voxel kept alive by less weight than a usable "
                             "voxel needs could never be emptied" % (float(w_floor), float(min_weight)))
        self.video = video
        self.voxel, self.origin = float(voxel), [float(v) for v in origin]
        self.trunc = 3.0 * self.voxel if trunc is None else float(trunc)
        self.thresh, self.use_sigma, self.rel0, self.reject = thresh, bool(use_sigma), float(rel0), reject
        self.min_weight, self.w_floor, self.tol = float(min_weight), float(w_floor), float(tol)
        self.lag = DEFAULT_LAG if lag is None else int(lag)
        self.margin = float(margin)
        dev = video.device
        nz, ny, nx = [int(v) for v in dims]
        self.sparse = None
        self.tsdf = self.wsum = self.rgb = None
        if sparse:
            from .tsdf_sparse import BRICK, SparseTSDF
            self.sparse = SparseTSDF(self.origin, [-(-v // BRICK) for v in (nz, ny, nx)], self.voxel, self.trunc,
                                     colours=video.images is not None, device=dev)
        else:
            self.tsdf = torch.zeros(nz, ny, nx, dtype=torch.float32, device=dev)
            self.wsum = torch.zeros_like(self.tsdf)
            self.rgb = torch.zeros(nz, ny, nx, 3, dtype=torch.float32, device=dev) if video.images is not None else None
        # the ledger: what each keyframe slot was fused with, and (host) which slots are fused, with their time stamps
        self.poses_fused = torch.zeros_like(video.poses)
        self.disps_fused = torch.zeros_like(video.disps)
        self.weight_fused = torch.zeros_like(video.disps)
        self.weight_now = torch.zeros_like(video.disps)
        self.fused = {}
        self.refreshed_total = 0

    # ---------------------------------------------------------------------------------------------------- the present state
    def weights(self, upto):
        """the fusion weights [upto,ht,wd] the keyframes [0, upto) have NOW: DepthVideo.tsdf's"""
        v = self.video
        disps = v.disps[:upto]
        m = v.map_points(ix=torch.arange(upto, device=v.device), thresh=self.thresh, reject=self.reject)
        keep = torch.zeros(disps.shape, dtype=torch.bool, device=v.device)
        src = m["src"].long()
        keep.view(upto, -1)[src[:, 0], src[:, 1]] = True
        sigma = v.sigma_disp()[:upto] if self.use_sigma else None
        return v.fusion_weights(keep, disps, sigma, self.rel0).contiguous()

    def drift(self, ix, weight=None):
        """per keyframe of ix (fused ones): how far its fused observation has moved, in voxels - the RMS 3-D distance between each
        pixel's point back-projected from the snapshot and from the video's current pose and depth; a pixel kept (weight > 0) in only
        one of the two counts as trunc, one kept in neither does not count; 0 without a counted pixel.  weight [>= max(ix)+1,ht,wd]: the
        current weights if the caller has them (update does), else computed.  Plain torch on [n,ht,wd]; returns a device tensor [n]."""
        v = self.video
        ix = torch.as_tensor(ix, dtype=torch.long, device=v.device).reshape(-1)
        if ix.numel() == 0:
            return torch.zeros(0, dtype=torch.float32, device=v.device)
        if weight is None:
            weight = self.weights(int(ix.max()) + 1)
        intr = v.intrinsics[0]
        was, now = self.weight_fused[ix] > 0, weight[ix] > 0
        a = backproject(self.poses_fused[ix], self.disps_fused[ix], intr)
        b = backproject(v.poses[ix], v.disps[ix], intr)
        both = was & now
        d2 = torch.where(both, ((a - b) ** 2).sum(-1), torch.zeros_like(a[..., 0]))
        d2 = torch.where(was ^ now, torch.full_like(d2, self.trunc ** 2), d2)
        d2 = torch.where(torch.isfinite(d2), d2, torch.full_like(d2, self.trunc ** 2))
        count = (was | now).flatten(1).sum(1).clamp(min=1)
        return torch.sqrt(d2.flatten(1).sum(1) / count) / self.voxel

    # ---------------------------------------------------------------------------------------------------- the update
    def _reintegrate(self, remove, add):
        v = self.video
        intr = v.intrinsics[0].contiguous()
        if self.sparse is not None:
            self.sparse.reintegrate(intr, remove=remove, add=add, images=v.images, img_stride=8, img_offset=3, w_floor=self.w_floor,
                                    margin=self.margin)
        else:
            db.tsdf_reintegrate(self.tsdf, self.wsum, self.rgb, self.origin, self.voxel, self.trunc, intr, remove=remove, add=add,
                                images=v.images if self.rgb is not None else None, img_stride=8, img_offset=3, w_floor=self.w_floor)

    def update(self, upto=None, force=False):
        """bring the volume up to the video: the candidates are the keyframes [0, upto) (default video.counter - lag).  Candidates not
        yet fused are added; fused ones whose drift exceeds tol (all of them with force) are removed as their snapshot holds them and
        added as they are now; a fused slot whose time stamp no longer matches (its keyframe was removed from the window and the slots
        behind it shifted) is removed and then treated as new.  One native re-integration, then the snapshots are refreshed.
        Returns (added, refreshed, dropped).  Costs ONE small device-to-host read per call: the slots' time stamps and drifts."""
        v = self.video
        n = int(v.counter)
        upto = max(0, min(n, n - self.lag if upto is None else int(upto)))
        known = sorted(self.fused)
        m = max([upto] + [k + 1 for k in known])
        if m == 0:
            return 0, 0, 0
        weight = None
        if upto > 0:
            weight = self.weights(upto)
            self.weight_now[:upto] = weight
        cand = [k for k in known if k < upto]
        drift = self.drift(cand, self.weight_now) if cand else torch.zeros(0, device=v.device)
        host = torch.cat([v.tstamp[:m].double(), drift.double()]).tolist()          # the one read-back
        stamp, drift = host[:m], dict(zip(cand, host[m:]))
        dropped = [k for k in known if k >= n or stamp[k] != self.fused[k]]      # (a slot at or past the counter holds no keyframe)
        refresh = [k for k in cand if k not in dropped and (force or drift[k] > self.tol)]
        new = [k for k in range(upto) if k not in self.fused]
        out = sorted(refresh + dropped)
        into = sorted(new + refresh + [k for k in dropped if k < upto])
        if out or into:
            dev = v.device
            remove = (self.poses_fused, self.disps_fused, torch.tensor(out, dtype=torch.long, device=dev), self.weight_fused) if out else None
            add = (v.poses, v.disps, torch.tensor(into, dtype=torch.long, device=dev), self.weight_now) if into else None
            self._reintegrate(remove, add)
        for k in dropped:
            del self.fused[k]
        if into:
            sel = torch.tensor(into, dtype=torch.long, device=v.device)
            self.poses_fused[sel], self.disps_fused[sel], self.weight_fused[sel] = v.poses[sel], v.disps[sel], self.weight_now[sel]
            for k in into:
                self.fused[k] = stamp[k]
        self.refreshed_total += len(refresh)
        return len(new), len(refresh), len(dropped)

    # ---------------------------------------------------------------------------------------------------- the volume's users
    def as_volume(self):
        """the dict DepthVideo.tsdf returns, without the mesh: tsdf_render, model_residual, tsdf_track and refine_to_model take it"""
        if self.sparse is not None:
            return {"volume": self.sparse, "origin": list(self.origin), "voxel": self.voxel}
        out = {"tsdf": self.tsdf, "wsum": self.wsum, "origin": list(self.origin), "voxel": self.voxel}
        if self.rgb is not None:
            out["rgb"] = self.rgb
        return out

    def mesh(self):
        """the surface-nets mesh of the volume as it stands: verts, normals, rgba, faces"""
        if self.sparse is not None:
            out = self.sparse.mesh(min_weight=self.min_weight)
        else:
            out = db.tsdf_mesh(self.tsdf, self.wsum, self.rgb, self.origin, self.voxel, min_weight=self.min_weight)
        out.pop("counts")
        return out

    def render(self, **kw):
        """DepthVideo.tsdf_render of the live volume"""
        kw.setdefault("min_weight", self.min_weight)
        return self.video.tsdf_render(self.as_volume(), **kw)

    def track(self, **kw):
        """DepthVideo.tsdf_track against the live volume"""
        return self.video.tsdf_track(self.as_volume(), **kw)
