"""Host side of tests/test_ba_shard_invariance_gpu.py: the launch-rule predicates of tests/ba_reference.py on the windows that claim a
form, the host-side solve-form rule (pvo_ba_solve_kind: no GPU), and the wrapper - ShardedBA must hand ba_finish, on both dense-message
paths, inputs of the solve-form rule that are equal on every rank.  No GPU is needed."""
import threading

import pytest
import torch

import ba_reference as B
import rgbd_reference as R
from pvo_amd.parallel import ShardedBA


@pytest.mark.parametrize("graph", sorted(B.LAUNCH_FORMS))
def test_every_window_reaches_the_form_it_claims(graph):
    s = B.regime_window("control", **B.GRAPHS[graph])
    paths = B.frame_paths(s)
    kinds = sorted({p for p, _, _ in paths.values()})
    print("%s: %s, frames by path %s, rows %d .. %d" % (graph, B.launch_form(s), {k: sum(p == k for p, _, _ in paths.values()) for k in kinds},
                                                         min(B.frame_rows(s).values()), max(B.frame_rows(s).values())))
    assert B.launch_form(s) == B.LAUNCH_FORMS[graph] and B.LAUNCH_FORMS[graph] in B.FORM_NAMES
    assert len({pix for _, pix, _ in paths.values()}) == 1
    form = B.LAUNCH_FORMS[graph]
    assert B.schur_chunk(s) == {"chunk512": 512, "chunk1024": 1024}.get(form, 256)
    if form.startswith("window"):
        assert "staged" in kinds and ("stream" in kinds) == (form == "window_mixed") and ("lds" in kinds) == (form == "window_direct")
        assert all(n == 1 for p, _, n in paths.values() if p == "staged")
    else:
        assert "staged" not in kinds and "lds" not in kinds
    if form in ("chunk512", "chunk1024"):
        assert {"pass", "stream"} <= set(kinds)                                # both templates over the chunk: schur_pass and schur_rowpass


def test_the_form_names_cover_the_launch_rule():
    assert {B.LAUNCH_FORMS[g] for g, _, _ in B.LAUNCHES} | {"fused256"} == set(B.FORM_NAMES)
    assert B.n_add(4) == 66 + 6 + 4 + 2 and B.n_add(4, 512) == 130 + 12 and B.n_add(10, 1024) == 258 + 18 + 10 + 2


def test_the_solve_form_reads_the_free_poses_and_the_whole_graphs_edge_count():
    from pvo_amd import droid_backends as db
    assert db.ba_solve_kind(0, 10) == "status"
    assert db.ba_solve_kind(29, 10 ** 6) == "dense" and db.ba_solve_kind(30, 240) == "envelope" and db.ba_solve_kind(30, 241) == "blocks"
    assert db.ba_solve_kind(39, 438) == "blocks" and db.ba_solve_kind(39, 312) == "envelope"
    assert db.ba_solve_kind(39, 438, packed=True) == "envelope"                # a packed message never takes the edge-count form


class _Exchange:
    """an in-process all-reduce between the threads that stand for ranks"""

    def __init__(self, n):
        self.n, self.bar, self.slots = n, threading.Barrier(n), [None] * n

    def allreduce(self, rank, t):
        self.slots[rank] = t.clone()
        self.bar.wait()
        total = sum(self.slots[1:], self.slots[0].clone())
        self.bar.wait()
        t.copy_(total)


class _Recorder:
    """stands where the HIP library stands (fixed-point system, no native packing): records what ba_finish is given"""
    BA_SYS_DTYPE = torch.int64

    def __init__(self):
        self.finishes = []

    def ba_workspace(self, E, P, F, HW, device):
        return {}

    def ba_plan(self, ii, jj, F, HW, K_eta, t0, t1, ws):
        pass

    def ba_local(self, poses, disps, intr, targets, weights, eta, ii, jj, t0, t1, motion_only, sys_buf, ws, sys_is_zero=False):
        sys_buf[-6 * (t1 - t0):].add_(int(ii.shape[0]))                        # (the right-hand side: part of every message form)

    def ba_finish(self, poses, disps, sys_buf, ii, jj, t0, t1, lm, ep, motion_only, ws, packed=None, graph_edges=None):
        # what solve_form reads (ba.hip): P, the edge count - the stated whole graph's, else this call's own - and whether the message is packed
        self.finishes.append((t1 - t0, int(ii.shape[0]) if graph_edges is None else int(graph_edges), packed is not None, sys_buf.clone()))
        sys_buf.zero_()
        return torch.zeros(t1 - t0, 6), None


class _Rank(ShardedBA):
    def __init__(self, rank, exchange, **kw):
        super().__init__(**kw)
        self.rank, self.exchange = rank, exchange

    def _world(self):
        return self.exchange.n

    def _allreduce(self, t):
        self.exchange.allreduce(self.rank, t)


@pytest.mark.parametrize("path", ["structure_none", "torch_pack"])
def test_sharded_ba_gives_the_solve_form_rule_the_same_inputs_on_every_rank(path):
    """two unequal shards of the blocked39 graph (438 edges, 39 free poses) on the dense-message paths: no structure (the dense system is
    all-reduced) and torch_pack (the index message is copied back into the dense buffer)"""
    from pvo_amd import droid_backends as db
    F, t0, t1, ht, wd = 40, 1, 40, 2, 3
    ii, jj = (torch.as_tensor(v) for v in R.radius_graph(F, 6))
    frames = sorted(set(ii.tolist()))
    first = set(frames[:(3 * len(frames)) // 4])
    own = torch.tensor([0 if int(f) in first else 1 for f in ii])
    E, P = int(ii.shape[0]), t1 - t0
    counts = [int((own == r).sum()) for r in range(2)]
    assert E == 438 and counts[0] > 8 * P >= counts[1]
    ex = _Exchange(2)
    structure = None if path == "structure_none" else (ii.tolist(), jj.tolist())
    recs, errors = [_Recorder(), _Recorder()], []

    def rank(r):
        try:
            m = own == r
            sb = _Rank(r, ex, backend=recs[r], structure=structure)
            sb.torch_pack = path == "torch_pack"
            n = counts[r]
            sb.ba(torch.zeros(F, 7), torch.ones(F, ht, wd), torch.ones(4), torch.zeros(n, 2, ht, wd), torch.ones(n, 2, ht, wd),
                  torch.ones(P + 1, ht, wd), ii[m].contiguous(), jj[m].contiguous(), t0, t1, itrs=2)
        except Exception as e:                                                 # (a failed rank must not leave the other at the barrier)
            errors.append(e)
            ex.bar.abort()

    threads = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(60)
    assert not errors, errors
    assert len(recs[0].finishes) == len(recs[1].finishes) == 2
    for a, b in zip(recs[0].finishes, recs[1].finishes):
        assert a[:3] == b[:3] == (P, E, False)                                 # every value the rule reads, equal across the ranks
        assert torch.equal(a[3], b[3]) and int(a[3].max()) == E                # ... on the same summed system
        assert db.ba_solve_kind(a[0], a[1], a[2]) == db.ba_solve_kind(b[0], b[1], b[2]) == "blocks"
    assert db.ba_solve_kind(P, counts[0]) != db.ba_solve_kind(P, counts[1])    # what the ranks' own counts would have chosen
