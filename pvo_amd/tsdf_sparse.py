"""The brick volume of the sparse surface reconstruction (include/pvo_hip.h, "Sparse surface reconstruction"): SparseTSDF owns the
indirection grid and the pool of 8 x 8 x 8 bricks, grows the pool when an allocation overflows it, and forwards to the native calls
(droid_backends.tsdf_sparse_allocate / _integrate / _mesh).  A brick holds the frames integrated since it was allocated, so the
intended use is: allocate for all keyframes, then integrate, then mesh."""
import torch

from . import droid_backends as db

BRICK = 8
GRID_LIMIT = 1 << 31            # gz * gy * gx must stay below it
AXIS_LIMIT = (1 << 21) // BRICK  # bricks per axis: voxel indices stay exact in fp32


class SparseTSDF:
    def __init__(self, origin, grid_dims, voxel, trunc, colours=True, device="cuda", cap=1024, labels=False):
        """a world of grid_dims = (gz,gy,gx) bricks whose voxel (0,0,0) has its centre at origin [x,y,z]; cap: the pool's first size;
        labels: also own the two pools of the segment-id vote (label int32, lconf f32)"""
        gz, gy, gx = [int(v) for v in grid_dims]
        if min(gz, gy, gx) < 0 or max(gz, gy, gx) > AXIS_LIMIT or gz * gy * gx >= GRID_LIMIT:
            raise ValueError("SparseTSDF: a grid of %d x %d x %d bricks is over the limit (each axis <= %d bricks, fewer than 2^31 in all); "
                             "use a larger voxel or a smaller extent" % (gz, gy, gx, AXIS_LIMIT))
        self.origin, self.voxel, self.trunc = [float(v) for v in origin], float(voxel), float(trunc)
        self.device = torch.device(device)
        self.grid = torch.full((gz, gy, gx), -1, dtype=torch.int32, device=self.device)
        self.counts = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.colours = bool(colours)
        self.labels = bool(labels)
        self.tsdf = self.wsum = self.rgb = self.coord = self.label = self.lconf = None
        self._resize(max(int(cap), 1))

    @property
    def cap(self):
        return self.tsdf.shape[0]

    @property
    def bricks(self):
        """the number of bricks in use (reads the device)"""
        return min(int(self.counts[0]), self.cap)

    def _resize(self, cap):
        """a zeroed pool of cap bricks with the old pool's contents copied in"""
        B = BRICK
        new = {"tsdf": torch.zeros(cap, B, B, B, dtype=torch.float32, device=self.device),
               "wsum": torch.zeros(cap, B, B, B, dtype=torch.float32, device=self.device),
               "rgb": torch.zeros(cap, B, B, B, 3, dtype=torch.float32, device=self.device) if self.colours else None,
               "coord": torch.zeros(cap, 3, dtype=torch.int32, device=self.device),
               "label": torch.zeros(cap, B, B, B, dtype=torch.int32, device=self.device) if self.labels else None,
               "lconf": torch.zeros(cap, B, B, B, dtype=torch.float32, device=self.device) if self.labels else None}
        for k, t in new.items():
            old = getattr(self, k)
            if old is not None and t is not None:
                t[:old.shape[0]] = old
            setattr(self, k, t)

    def volume(self):
        """the dict the native calls take"""
        return {"grid": self.grid, "coord": self.coord, "counts": self.counts, "tsdf": self.tsdf, "wsum": self.wsum, "rgb": self.rgb,
                "origin": self.origin, "voxel": self.voxel}

    def allocate(self, poses, disps, intrinsics, ix, weight=None, z_near=0.0, margin=2.0):
        """bricks near the surfaces keyframes ix see.  Reads counts ONCE (the call's one synchronisation); if the volume wants more
        bricks than the pool has, the pool is doubled (until it fits) by copy and the call repeated, which finishes the job.
        Returns the number of bricks in use."""
        args = (poses, disps, intrinsics, ix, self.trunc)
        db.tsdf_sparse_allocate(self.volume(), *args, weight=weight, z_near=z_near, margin=margin)
        want = int(self.counts[0])
        if want > self.cap:
            cap = self.cap
            while cap < want:
                cap *= 2
            self._resize(cap)
            db.tsdf_sparse_allocate(self.volume(), *args, weight=weight, z_near=z_near, margin=margin)
        return want

    def integrate(self, poses, disps, intrinsics, ix, weight=None, images=None, img_stride=8, img_offset=3, z_near=0.0, w_max=0.0, kept=None,
                  labels=None, label_div=1):
        """keyframes ix, in that order, into the bricks in use (no synchronisation); kept int32 [cap] or None: survivors of the cull;
        labels int32 [nframes,LH,LW] (a volume made with labels=True): the frames' segment ids into the label pools as well"""
        if labels is not None and not self.labels:
            raise ValueError("SparseTSDF.integrate: labels need a volume made with labels=True")
        pan = dict(label=self.label, lconf=self.lconf, labels=labels, label_div=label_div) if labels is not None else {}
        db.tsdf_sparse_integrate(self.volume(), poses, disps, intrinsics, ix, self.trunc, weight=weight,
                                 images=images if self.colours else None, img_stride=img_stride, img_offset=img_offset, z_near=z_near,
                                 w_max=w_max, kept=kept, **pan)

    def reintegrate(self, intrinsics, remove=None, add=None, images=None, img_stride=8, img_offset=3, z_near=0.0, w_max=0.0,
                    w_floor=2.0 ** -10, margin=2.0, kept=None):
        """keyframes taken out as they were fused (remove) and put in as they are now (add), each (poses, disps, ix, weight or None) or
        None, in one pass over the bricks (droid_backends.tsdf_sparse_reintegrate).  Bricks for `add` are allocated first - the one
        synchronisation, and the pool grows as in allocate; bricks a removal empties stay allocated.  The segment-id vote cannot be
        inverted (a Boyer-Moore majority keeps no history): a volume made with labels=True is refused."""
        if self.labels:
            raise ValueError("SparseTSDF.reintegrate: a volume made with labels=True cannot be re-integrated - the per-voxel label vote "
                             "is a running majority and cannot be inverted; keep the labels in a volume fused after tracking")
        if add is not None and add[2].numel():
            self.allocate(add[0], add[1], intrinsics, add[2], weight=add[3], z_near=z_near, margin=margin)
        db.tsdf_sparse_reintegrate(self.volume(), self.trunc, intrinsics, remove=remove, add=add, images=images if self.colours else None,
                                   img_stride=img_stride, img_offset=img_offset, z_near=z_near, w_max=w_max, w_floor=w_floor, kept=kept)

    def mesh(self, min_weight=1.0, vcap=None, fcap=None):
        """the mesh dict of droid_backends.tsdf_sparse_mesh; with labels=True it has vlabel"""
        return db.tsdf_sparse_mesh(self.volume(), min_weight=min_weight, vcap=vcap, fcap=fcap, label=self.label)

    def render(self, poses, intrinsics, ix, ht, wd, dz=None, z_near=0.0, z_far=None, min_weight=1.0, normals=True, out=None):
        """the volume seen from the views ix of poses: the dict of droid_backends.tsdf_sparse_render (depth, normal, rgba; with
        labels=True label as well)"""
        return db.tsdf_sparse_render(self.volume(), poses, intrinsics, ix, ht, wd, dz=dz, z_near=z_near, z_far=z_far,
                                     min_weight=min_weight, label=self.label, normals=normals, out=out)

    def track(self, poses, disps, intrinsics, ix, weight=None, **kw):
        """frame-to-model tracking against the bricks: the dict of droid_backends.tsdf_sparse_track (poses, info, and on request
        system, residual, jac); kw as there"""
        return db.tsdf_sparse_track(self.volume(), poses, disps, intrinsics, ix, weight=weight, **kw)

    def nbytes(self):
        """device bytes held: the grid and the pool"""
        return sum(t.numel() * t.element_size() for t in (self.grid, self.coord, self.counts, self.tsdf, self.wsum, self.rgb, self.label, self.lconf)
                   if t is not None)

    def to_dense(self):
        """the bricks in use scattered into a dense [8gz,8gy,8gx] volume (zero elsewhere): dict tsdf, wsum, rgb (or None), with labels=True
        label and lconf, and allocated bool [gz,gy,gx].  For tests and small volumes."""
        B = BRICK
        gz, gy, gx = self.grid.shape
        n = self.bricks
        c = self.coord[:n].long()
        out = {"allocated": self.grid >= 0}
        for k, t in (("tsdf", self.tsdf), ("wsum", self.wsum), ("rgb", self.rgb), ("label", self.label), ("lconf", self.lconf)):
            if t is None and k in ("label", "lconf"):
                continue
            if t is None:
                out[k] = None
                continue
            tail = tuple(t.shape[4:])
            dense = torch.zeros((gz, gy, gx, B, B, B) + tail, dtype=t.dtype, device=t.device)
            dense[c[:, 0], c[:, 1], c[:, 2]] = t[:n]
            perm = (0, 3, 1, 4, 2, 5) + tuple(range(6, 6 + len(tail)))
            out[k] = dense.permute(*perm).reshape((B * gz, B * gy, B * gx) + tail).contiguous()
        return out
