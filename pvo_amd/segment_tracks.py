"""Temporally consistent panoptic ids: segments associated across keyframes along the factor graph's full flow - the host layer over
droid_backends.segment_associate (include/pvo_hip.h pvo_segment_associate).  Plain torch; everything but the native call itself runs on
CPU tensors too.

    dense_labels(raw)                           per-frame dense labels, and the raw id behind each, from the ids as given
    graph_segment_associate(graph, ...)         operands from a graph (object motion's: coords0 + full_flow), the native call
    SegmentTracks(video)                        an opt-in ledger (args.segment_tracks): (tstamp, raw id) -> track id, kept by the frontend;
                                                Droid.get_segment_tracks(), track_map() for DepthVideo.tsdf(panoptic=True, labels=...)

A per-image panoptic network numbers its segments anew in every frame; the ledger gives the same object the same track id in every
keyframe as long as the flow carries it onto itself.  Whether the network's flow on real video does is not measured here (no weights, no
dataset): the call is held to an analytic scene (tests/segment_assoc_reference.py)."""
from fractions import Fraction

import torch


def dense_labels(raw):
    """raw int [n,h,w] (DepthVideo.segms_raw[:n]: panoptic ids as given) -> (dense int32 [n,h,w], ids int32 [n,S], count int64 [n]).
    Raw ids <= 0 map to dense 0 (no segment); a frame's other raw ids map, in ascending order, to 1, 2, ..., count[f];
    ids[f, dense] is the raw id (0 where there is none) and S = 1 + the largest count.  Built from one torch.unique over (frame, id).
    Synchronises (the number of distinct ids is data: the mask, torch.unique and S, a shape, each read a size back): an export step,
    not for a captured region."""
    n, h, w = raw.shape
    dev = raw.device
    r = raw.long()
    pos = r > 0
    dense = torch.zeros(n, h, w, dtype=torch.int32, device=dev)
    if n == 0 or not bool(pos.any()):
        return dense, torch.zeros(n, 1, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.long, device=dev)
    span = 1 << 31
    frame = torch.arange(n, device=dev)[:, None, None].expand(n, h, w)
    u, inv = torch.unique(frame[pos] * span + r[pos], return_inverse=True)          # sorted: ascending (frame, raw id)
    uf, uid = u // span, u % span
    count = torch.bincount(uf, minlength=n)
    rank = torch.arange(u.numel(), device=dev) - (torch.cumsum(count, 0) - count)[uf] + 1
    S = 1 + int(count.max())
    dense[pos] = rank[inv].to(torch.int32)
    ids = torch.zeros(n, S, dtype=torch.int32, device=dev)
    ids[uf, rank] = uid.to(torch.int32)
    return dense, ids, count


def _native(ops, **kw):
    from . import droid_backends as db
    return db.segment_associate(ops["labels"], ops["ii"], ops["jj"], ops["target"], ops["S"], valid=ops["valid"], cls=ops["cls"], **kw)


def graph_segment_associate(graph, edges=None, min_iou=0.25, valid=None, cls_div=None, native=_native):
    """the segments of the graph's keyframes associated along its edges (edges: a list / tensor of edge indices, default all) from the
    full flow of the last update: the operands are object motion's (pvo_amd.object_motion.graph_operands: target = coords0 + full_flow,
    ii, jj), the labels dense_labels of video.segms_raw (a video made with store_segment_ids; video.segms follows a removed keyframe
    only with segm_filter on).  valid: uint8 / bool [E,ht,wd] for the edges given, or None.  cls_div: segments whose raw id // cls_div
    differs never match (ids coded category * cls_div + instance).  Returns droid_backends.segment_associate's dict plus ids [n,S] (the
    raw id behind each dense label), ii, jj (of those edges).  Synchronises (dense_labels)."""
    from .object_motion import graph_operands
    raw = getattr(graph.video, "segms_raw", None)
    if raw is None:
        raise ValueError("segment association needs the raw segment ids: make the video with store_segment_ids=True")
    ops = graph_operands(graph)
    ii, jj, target = ops["ii"], ops["jj"], ops["target"]
    dev = ii.device
    if edges is not None:
        edges = torch.as_tensor(edges, dtype=torch.long, device=dev).reshape(-1)
        ii, jj, target = ii[edges].contiguous(), jj[edges].contiguous(), target[edges].contiguous()
    hosts = list(getattr(graph, "_ii_h", ())) + list(getattr(graph, "_jj_h", ()))
    n = (max(hosts) + 1) if hosts else (int(torch.maximum(ii.max(), jj.max())) + 1 if ii.numel() else 0)
    dense, ids, _ = dense_labels(raw[:n])
    if valid is not None:
        valid = valid.to(device=dev, dtype=torch.uint8).contiguous()
    cls = None if cls_div is None else torch.div(ids, int(cls_div), rounding_mode="floor").to(torch.int32).contiguous()
    out = dict(native(dict(labels=dense.contiguous(), ii=ii, jj=jj, target=target, S=int(ids.shape[1]), valid=valid, cls=cls), min_iou=min_iou))
    out.update(ids=ids, ii=ii, jj=jj)
    return out


class SegmentTracks:
    """An opt-in ledger of track ids (Droid's args.segment_tracks: True, or a dict of min_iou, cls_div): (tstamp, raw id) -> track id >= 1.
    The frontend calls observe(graph) after a keyframe's updates.  The graph's edges with ii < jj are associated
    (graph_segment_associate) and walked in ascending (jj, ii):
      - a keyframe that has no earlier keyframe to lean on gives its segments fresh ids, in ascending raw id;
      - a segment b of keyframe j without a track takes the track of a segment a matched to it (match[e, a] = b on an edge i -> j).  Among
        several the largest IoU n / d wins, compared exactly; ties go to the larger i, then to the lower a.  A track is held by at most
        one segment of a keyframe: claims are served in that order, the larger IoU keeps the track, and the loser goes on to its next
        candidate, if it has one;
      - a segment left without gets a fresh id;
      - a segment that has a track keeps it - the first assignment sticks, so a map's labels do not flicker between updates.
    remove(tstamp) drops a keyframe's entries when the frontend removes that keyframe.  Reads the graph and the video, writes neither.
    Synchronises (dense_labels and the copy to the host): not for a captured region, and off by default."""

    def __init__(self, video=None, min_iou=0.25, cls_div=None, solve=graph_segment_associate):
        self.video, self.min_iou, self.cls_div, self._solve = video, float(min_iou), cls_div, solve
        self.entries = {}                                  # (tstamp, raw id) -> track id
        self.next_id = 1
        self.observations = 0
        self.last = None                                   # the outputs of the last association (tests compare them with a direct call)

    def _fresh(self):
        self.next_id += 1
        return self.next_id - 1

    def observe(self, graph):
        ii_h, jj_h = list(graph._ii_h), list(graph._jj_h)
        edges = sorted((e for e in range(len(ii_h)) if ii_h[e] < jj_h[e]), key=lambda e: (jj_h[e], ii_h[e]))
        if not edges:
            return 0
        out = self._solve(graph, edges=edges, min_iou=self.min_iou, cls_div=self.cls_div)
        self.observations += 1
        self.last = out
        match, mn, md, ids = (out[k].detach().cpu().tolist() for k in ("match", "match_n", "match_d", "ids"))
        src, dst = out["ii"].tolist(), out["jj"].tolist()
        tstamp = graph.video.tstamp[:len(ids)].tolist()
        new = 0
        for f in sorted(set(src) | set(dst)):
            segs = [(s, rid) for s, rid in enumerate(ids[f]) if s >= 1 and rid > 0]
            open_ = {s for s, rid in segs if (tstamp[f], rid) not in self.entries}
            held = {self.entries[(tstamp[f], rid)] for s, rid in segs if s not in open_}
            claims = []
            for e, (i, j) in enumerate(zip(src, dst)):
                if j != f:
                    continue
                for a, b in enumerate(match[e]):
                    track = self.entries.get((tstamp[i], ids[i][a])) if b in open_ else None
                    if track is not None:
                        claims.append((-Fraction(mn[e][a], md[e][a]), -i, a, b, track))
            for _, _, _, b, track in sorted(claims):
                if b in open_ and track not in held:
                    self.entries[(tstamp[f], ids[f][b])] = track
                    open_.discard(b)
                    held.add(track)
            for s in sorted(open_):                                           # (dense labels ascend with the raw ids)
                self.entries[(tstamp[f], ids[f][s])] = self._fresh()
            new += len(segs)
        return new

    def remove(self, tstamp):
        """the frontend removed the keyframe stamped `tstamp`: its entries go"""
        t = float(tstamp)
        for key in [k for k in self.entries if k[0] == t]:
            del self.entries[key]

    def track_map(self, video=None):
        """int32 [counter,h/8,w/8]: every keyframe pixel's track id, 0 where its segment has none (or it has no segment) - the label
        tensor for DepthVideo.tsdf(panoptic=True, labels=...).  A table gather over dense_labels(video.segms_raw); synchronises."""
        video = self.video if video is None else video
        n = video.counter
        if n == 0:
            return torch.zeros((0,) + tuple(video.segms_raw.shape[1:]), dtype=torch.int32, device=video.segms_raw.device)
        dense, ids, _ = dense_labels(video.segms_raw[:n])
        tstamp = video.tstamp[:n].tolist()
        table = [[self.entries.get((tstamp[f], rid), 0) if rid > 0 else 0 for rid in row] for f, row in enumerate(ids.cpu().tolist())]
        table = torch.tensor(table, dtype=torch.int32, device=dense.device).reshape(n, -1)
        return torch.gather(table, 1, dense.reshape(n, -1).long()).reshape(dense.shape).contiguous()

    def table(self):
        """[(tstamp, raw id, track id), ...] in time order"""
        return [(k[0], k[1], self.entries[k]) for k in sorted(self.entries)]

    def tracks(self):
        """{track id: [(tstamp, raw id), ...]} in time order"""
        out = {}
        for t, rid, track in self.table():
            out.setdefault(track, []).append((t, rid))
        return out
