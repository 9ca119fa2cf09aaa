"""Shard invariance of the dense bundle adjustment at the WORDS of `sys` (include/pvo_hip.h, pvo_ba_local: "identical for any partition
of the edges by source frame over ranks"), under every form of the launch rule, and the two rules that used to read rank-local
quantities (schur_stage_slot in ba_workspace.h, solve_form in ba.hip):

  staging      whether a dense window's frame adds its chunk sums in fp64 and rounds once was decided by the NUMBER of depth frames of
               the call (`Kgrid <= P + 8`, from K_eta).  front10 - 30 depth frames on the whole graph, 25 or fewer on a balanced shard, P + 8 = 28 -
               ran unstaged as a whole and staged in shards, and a broadcast eta flipped the same switch: different words.  Now the
               frame's identity decides (schur_stage_slot);
  solve form   the 48 x 48 block solve was picked by this call's edge count: of two unequal shards of blocked39 (438 edges, 8 P = 312)
               one took it and the other the envelope solve, on the same summed system.  Now the whole graph's count decides, which a
               shard states (pvo_ba_finish_graph); pvo_ba_solve_kind reports the choice.

The sharded tests of tests/test_sharded_ba.py compare poses; a pose rarely shows a last-place difference of the fp64 system, the int64
words always do.  Shards are run by hand - ba_plan / ba_local per shard, the integer sum, ba_finish per replica - as an all-reduce
would; tests/test_ba_shard_invariance_host.py holds the wrapper (ShardedBA) to passing the rules rank-invariant inputs."""
import numpy as np
import pytest
import torch

import ba_reference as B
from pvo_amd.parallel import local_eta_rows, partition_by_source

pytestmark = pytest.mark.gpu

GRAPHS = ("win29", "front10", "mixed26", "c512", "tiny", "blocked39")
LM, EP = B.DAMPINGS["local"]


def owners(s, sharding):
    """rank of every edge, two ranks, whole source frames: `balanced` is partition_by_source's, `unequal` gives rank 0 the first three
    quarters of the source frames"""
    ii = s["ii"].tolist()
    if sharding == "balanced":
        return partition_by_source(ii, 2)[0]
    frames = sorted(set(ii))
    first = set(frames[:(3 * len(frames)) // 4])
    return [0 if f in first else 1 for f in ii]


def _local(db, s, cuda, keep, eta=None, pad=0):
    """ba_plan + ba_local on the edges `keep` (a bool tensor; None: the whole graph) from the window's own poses and depths
    -> dict(sys, ws, ii, jj, poses, disps, rows).  pad: frames appended to the pose and depth buffers behind the window (a video
    buffer longer than the graph, as the tracker's is)"""
    d = lambda t: t.to(cuda).contiguous()
    if pad:
        s = dict(s, poses=torch.cat([s["poses"], s["poses"][-1:].repeat(pad, 1)]), disps=torch.cat([s["disps"], s["disps"][-1:].repeat(pad, 1, 1)]))
    F, ht, wd = s["disps"].shape
    P, HW = s["t1"] - s["t0"], ht * wd
    m = torch.ones(s["ii"].shape[0], dtype=torch.bool) if keep is None else keep
    ii, jj = s["ii"][m], s["jj"][m]
    rows = local_eta_rows(s["ii"].tolist(), ii.tolist(), s["t0"], s["t1"])
    r = dict(ii=d(ii), jj=d(jj), poses=d(s["poses"].clone()), disps=d(s["disps"].clone()), rows=rows,
             eta=d(s["eta"][rows]) if eta is None else d(eta), target=d(s["target"][m]), weight=d(s["weight"][m]))
    r["ws"] = db.ba_workspace(int(ii.shape[0]), P, F, HW, cuda)
    r["sys"] = torch.zeros((6 * P) ** 2 + 6 * P, dtype=torch.int64, device=cuda)
    db.ba_plan(r["ii"], r["jj"], F, HW, r["eta"].shape[0], s["t0"], s["t1"], r["ws"])
    db.ba_local(r["poses"], r["disps"], d(s["intr"]), r["target"], r["weight"], r["eta"], r["ii"], r["jj"], s["t0"], s["t1"], False, r["sys"], r["ws"])
    return r


def _finish(db, s, r, words, graph_edges=None):
    st = torch.full((4,), -1, dtype=torch.int32, device=words.device)
    dx, _ = db.ba_finish(r["poses"], r["disps"], words.clone(), r["ii"], r["jj"], s["t0"], s["t1"], LM, EP, False, r["ws"], status=st,
                         graph_edges=graph_edges)
    assert int(st[0]) == 0
    return dx


@pytest.mark.parametrize("sharding", ["balanced", "unequal"])
@pytest.mark.parametrize("graph", GRAPHS)
def test_the_words_of_sys_and_the_step_do_not_depend_on_the_partition(cuda, graph, sharding):
    from pvo_amd import droid_backends as db
    s, _ = B.window_of(graph, "control")
    assert B.launch_form(s) == B.LAUNCH_FORMS[graph]
    P, E = s["t1"] - s["t0"], s["ii"].shape[0]
    own = torch.tensor(owners(s, sharding))
    whole = _local(db, s, cuda, None)
    shards = [_local(db, s, cuda, own == r) for r in range(2)]
    E0, E1 = (int(sh["ii"].shape[0]) for sh in shards)
    assert E0 > 0 and E1 > 0 and E0 + E1 == E and (sharding == "balanced" or E0 > 2 * E1)
    if graph == "front10":
        # what the old rule read: the whole graph has more depth frames than staging slots, every shard has fewer
        assert len(whole["rows"]) > P + B.STAGE_FRONT >= min(len(sh["rows"]) for sh in shards)
    total = shards[0]["sys"] + shards[1]["sys"]                                # what the all-reduce produces
    diff = int((whole["sys"] != total).sum())
    print("%s %s [%s]: E %d = %d + %d, depth frames %d | %d + %d; words that differ: %d of %d" % (
        graph, sharding, B.LAUNCH_FORMS[graph], E, E0, E1, len(whole["rows"]), len(shards[0]["rows"]), len(shards[1]["rows"]), diff, total.numel()))
    assert bool(whole["sys"].any()) and diff == 0 and torch.equal(whole["sys"], total)
    # the solve form: by P and the whole graph's edge count, which every shard states - the same on both ranks and on the whole graph
    dxs = [_finish(db, s, sh, total, graph_edges=E) for sh in shards]
    dxw = _finish(db, s, whole, whole["sys"])
    assert torch.equal(dxs[0], dxs[1]) and torch.equal(shards[0]["poses"], shards[1]["poses"])      # replicas, bit for bit
    assert torch.equal(dxs[0], dxw) and torch.equal(shards[0]["poses"], whole["poses"])             # ... and the whole graph's
    assert float(dxw.abs().max()) > 1e-4
    d0 = s["disps"].to(cuda)
    merged = d0 + sum(sh["disps"] - d0 for sh in shards)
    assert float((merged - whole["disps"]).abs().max()) < 2e-6 and float((whole["disps"] - d0).abs().max()) > 1e-3


def test_a_broadcast_eta_and_full_rows_of_the_same_constant_give_the_same_words(cuda):
    """K_eta = 1 makes the grid as tall as the host's bound on the depth frames - min(nframes, P + E): in a buffer ten frames longer
    than the graph, 41 rows where the full eta has 31 - taller than P + 8 = 37, which used to switch staging off for the whole launch"""
    from pvo_amd import droid_backends as db
    s, _ = B.window_of("win29", "control")
    assert B.launch_form(s) == "window_staged"
    K, (F, ht, wd), P, pad = s["eta"].shape[0], s["disps"].shape, s["t1"] - s["t0"], 10
    assert min(F + pad, P + s["ii"].shape[0]) > P + B.STAGE_FRONT >= K
    full = _local(db, s, cuda, None, eta=torch.full((K, ht, wd), 0.0078125), pad=pad)
    one = _local(db, s, cuda, None, eta=torch.full((1, ht, wd), 0.0078125), pad=pad)
    diff = int((full["sys"] != one["sys"]).sum())
    print("win29, eta one broadcast row against %d full rows: words that differ: %d" % (K, diff))
    assert bool(full["sys"].any()) and diff == 0


def test_unequal_shards_of_a_dense_graph_factorise_the_summed_system_with_one_form(cuda):
    """blocked39: E = 438 > 8 P = 312 picks the 48 x 48 blocks.  Rank 0 of the unequal sharding holds more than 312 edges and rank 1
    fewer: by their OWN counts - the rule until now - they chose differently.  With the dense (unpacked) message both state the whole
    graph's count and take the whole graph's form"""
    from pvo_amd import droid_backends as db
    s, _ = B.window_of("blocked39", "control")
    P, E = s["t1"] - s["t0"], s["ii"].shape[0]
    own = torch.tensor(owners(s, "unequal"))
    E0, E1 = int((own == 0).sum()), int((own == 1).sum())
    assert E == 438 and P == 39 and E0 > 8 * P >= E1
    assert db.ba_solve_kind(P, E0) == "blocks" and db.ba_solve_kind(P, E1) == "envelope"      # what each rank's own count selects
    assert db.ba_solve_kind(P, E) == "blocks" and db.ba_solve_kind(P, E, packed=True) == "envelope"
    shards = [_local(db, s, cuda, own == r) for r in range(2)]
    whole = _local(db, s, cuda, None)
    total = shards[0]["sys"] + shards[1]["sys"]
    assert torch.equal(total, whole["sys"])
    dxs = [_finish(db, s, sh, total, graph_edges=E) for sh in shards]
    dxw = _finish(db, s, whole, whole["sys"])
    assert torch.equal(dxs[0], dxs[1]) and torch.equal(dxs[0], dxw)
    # the envelope solve on the same words - what rank 1 alone would have run - agrees to fp64 rounding only, within the case's bound
    c = B.case("blocked39", "control", "local")
    other = _local(db, s, cuda, own == 1)
    dxe = _finish(db, s, other, total)                                         # (no graph_edges: this call's own 8 P >= E1)
    ok, sh = B.share("dx", dxe.cpu().numpy().astype(np.float64), c)
    print("blocked39 unequal: E %d = %d + %d; blocks against envelope on the same words: max |ddx| %.3e, envelope's share of the bound %.3f"
          % (E, E0, E1, float((dxe - dxw).abs().max()), sh))
    assert ok
