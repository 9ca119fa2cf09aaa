"""Per-instance rigid object motion from the factor graph's full flow: the host layer over droid_backends.object_motion
(include/pvo_hip.h pvo_object_motion).  Plain torch; everything but the native call itself runs on CPU tensors too.

    edge_jobs(labels, ii, jj, min_pixels)       the job list: one job per (edge, label of frame ii[e]) with enough pixels
    graph_object_motion(graph, ...)             FactorGraph.object_motion: operands from a graph, jobs, the native call
    ObjectTracks(video)                         an opt-in ledger (args.object_motion): the latest motion per (tstamp_i, tstamp_j, label)
                                                between consecutive keyframes, kept by the frontend; Droid.get_object_tracks()

Whether the network's dynamic flow on real video is accurate enough for these motions to be useful is not measured here (no weights,
no dataset): the call is held to an analytic scene (tests/object_motion_reference.py)."""
import torch


def edge_jobs(labels, ii, jj, min_pixels, member=None, skip=(0,)):
    """one job per (edge e, label l of frame ii[e]) with at least `min_pixels` member pixels, ascending in (edge, label).
    labels int [nframes,ht,wd]; ii, jj int64 [E] (jj is not read: membership is frame ii[e]'s); member: optional bool [E,ht,wd], only
    these pixels count; skip: labels that never become a job (0: no segment).  Returns (job_edge int64 [N], job_label int32 [N], pixels
    int64 [N]) on labels' device.  Synchronises once (the number of jobs is data): an export step, not for a captured region."""
    dev = labels.device
    E = int(ii.shape[0])
    empty = (torch.zeros(0, dtype=torch.long, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.long, device=dev))
    if E == 0 or labels.numel() == 0:
        return empty
    lab = labels[ii.to(dev).long()].reshape(E, -1).long()                 # [E,P]
    keep = torch.ones_like(lab, dtype=torch.bool)
    if member is not None:
        keep &= member.reshape(E, -1).to(dev)
    for s in skip:
        keep &= lab != int(s)
    edge = torch.arange(E, device=dev)[:, None].expand_as(lab)[keep]
    lab = lab[keep]
    if lab.numel() == 0:
        return empty
    lo = lab.min()
    span = lab.max() - lo + 1
    key, count = torch.unique(edge * span + (lab - lo), return_counts=True)          # sorted: ascending (edge, label)
    ok = count >= int(min_pixels)
    key, count = key[ok], count[ok]
    return key // span, (key % span + lo).to(torch.int32), count


def graph_operands(graph):
    """the native call's operands from a FactorGraph as it stands after an update: dict poses, disps, intrinsics, labels, ii, jj, target
    (= coords0 + full_flow, [E,ht,wd,2]).  labels: video.segms_raw when the video stores the ids as given, else video.segms[:, 0]."""
    v = graph.video
    raw = getattr(v, "segms_raw", None)
    labels = raw if raw is not None else v.segms[:, 0]
    E = int(graph.ii.shape[0])
    target = (graph.coords0 + graph.full_flow).reshape(E, graph.ht, graph.wd, 2).float().contiguous()
    return dict(poses=v.poses, disps=v.disps, intrinsics=v.intrinsics[0].contiguous(), labels=labels.to(torch.int32).contiguous(),
                ii=graph.ii.contiguous(), jj=graph.jj.contiguous(), target=target)


def _native(ops, job_edge, job_label, **kw):
    from . import droid_backends as db
    return db.object_motion(ops["poses"], ops["disps"], ops["intrinsics"], ops["labels"], ops["ii"], ops["jj"], ops["target"],
                            job_edge, job_label, **kw)


def graph_object_motion(graph, edges=None, min_pixels=64, dynamic_share=None, native=_native, **kw):
    """FactorGraph.object_motion: the rigid motion of every segment on the graph's edges (edges: a list / tensor of edge indices, default
    all) from the full flow of the last update.  Jobs from edge_jobs (labels <= 0 are no segment and never a job); with dynamic_share
    only segments of which at least that share of pixels is dynamic - a pixel is dynamic where sigmoid(raw_mask) < dy_thresh in either
    channel - become jobs.  kw: weight, start, iters, z_min, huber, lm, ep, min_count, system, centroid, residual, jac of
    droid_backends.object_motion.  Returns its dict plus job_edge, job_label (into the edges given), ii, jj (of those edges).
    Synchronises once (edge_jobs)."""
    ops = graph_operands(graph)
    dev = ops["ii"].device
    if edges is not None:
        edges = torch.as_tensor(edges, dtype=torch.long, device=dev).reshape(-1)
        ops["ii"], ops["jj"], ops["target"] = ops["ii"][edges].contiguous(), ops["jj"][edges].contiguous(), ops["target"][edges].contiguous()
    E = int(ops["ii"].shape[0])
    lab_e = ops["labels"][ops["ii"]] if E else ops["labels"][:0]
    positive = lab_e > 0
    if dynamic_share is None:
        job_edge, job_label, _ = edge_jobs(ops["labels"], ops["ii"], ops["jj"], min_pixels, member=positive, skip=())
    else:
        raw = graph.raw_mask.reshape(-1, graph.ht, graph.wd, graph.raw_mask.shape[-1])
        raw = raw if edges is None else raw[edges]
        dynamic = (torch.sigmoid(raw) < graph.dy_thresh).any(-1)
        je, jl, total = edge_jobs(ops["labels"], ops["ii"], ops["jj"], min_pixels, member=positive, skip=())
        de, dl, moving = edge_jobs(ops["labels"], ops["ii"], ops["jj"], 1, member=positive & dynamic, skip=())
        span = int(max(int(jl.max()) if jl.numel() else 0, int(dl.max()) if dl.numel() else 0)) + 1
        share = torch.zeros(je.shape[0], dtype=torch.float64, device=dev)
        if je.numel() and de.numel():
            a, b = je * span + jl.long(), de * span + dl.long()
            pos = torch.searchsorted(a, b).clamp(max=a.numel() - 1)
            hit = a[pos] == b
            share[pos[hit]] = moving[hit].double()
        keep = share / total.clamp(min=1).double() >= float(dynamic_share)
        job_edge, job_label = je[keep], jl[keep]
    out = dict(native(ops, job_edge.contiguous(), job_label.contiguous(), **kw))
    out.update(job_edge=job_edge, job_label=job_label, ii=ops["ii"], jj=ops["jj"])
    return out


class ObjectTracks:
    """An opt-in ledger of object motions (Droid's args.object_motion: True, or a dict of graph_object_motion's keyword arguments).  The
    frontend calls observe(graph) after a keyframe's updates; the graph's edges (k, k + 1) between consecutive keyframes are solved and
    the latest estimate per (tstamp_i, tstamp_j, label) kept: motion [7] (world frame), centroid [3] (world, time i), count, status, E.
    A later estimate of the same key replaces the earlier one; remove(tstamp) drops a keyframe's entries when the frontend removes that
    keyframe.  Reads the graph and the video, writes neither.  Synchronises (the job list and the copy to the host): not for a
    captured region, and off by default."""

    def __init__(self, video=None, min_pixels=64, dynamic_share=None, solve=graph_object_motion, **kw):
        self.video, self.min_pixels, self.dynamic_share, self.kw, self._solve = video, int(min_pixels), dynamic_share, dict(kw), solve
        self.entries = {}                                  # (tstamp_i, tstamp_j, label) -> dict
        self.observations = 0
        self.last = None                                   # the operands and outputs of the last solve (tests compare them with a direct call)

    @staticmethod
    def consecutive(ii, jj):
        """indices of the edges (k, k + 1) in host lists ii, jj, one per pair (the first)"""
        seen, out = set(), []
        for e, (i, j) in enumerate(zip(ii, jj)):
            if j == i + 1 and i not in seen:
                seen.add(i)
                out.append(e)
        return out

    def observe(self, graph):
        edges = self.consecutive(graph._ii_h, graph._jj_h)
        if not edges:
            return 0
        out = self._solve(graph, edges=edges, min_pixels=self.min_pixels, dynamic_share=self.dynamic_share, centroid=True, **self.kw)
        self.observations += 1
        self.last = out
        tstamp = graph.video.tstamp
        ti, tj = tstamp[out["ii"]].tolist(), tstamp[out["jj"]].tolist()
        host = {k: out[k].detach().cpu() for k in ("motion", "centroid", "info", "job_edge", "job_label")}
        for n, (e, lab) in enumerate(zip(host["job_edge"].tolist(), host["job_label"].tolist())):
            E, count, _, status = host["info"][n, -1].tolist()
            self.entries[(ti[e], tj[e], int(lab))] = dict(tstamp_i=ti[e], tstamp_j=tj[e], label=int(lab), motion=host["motion"][n].numpy().copy(),
                                                          centroid=host["centroid"][n].numpy().copy(), count=int(count), status=int(status), E=E)
        return len(host["job_edge"])

    def remove(self, tstamp):
        """the frontend removed the keyframe stamped `tstamp`: its entries go"""
        t = float(tstamp)
        for key in [k for k in self.entries if k[0] == t or k[1] == t]:
            del self.entries[key]

    def tracks(self):
        """{label: [entry, ...]} in time order (tstamp_i, then tstamp_j)"""
        out = {}
        for key in sorted(self.entries):
            out.setdefault(key[2], []).append(self.entries[key])
        return out
