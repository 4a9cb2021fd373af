"""The all-to-all sharded store (csrc/dist.hip; dist.sharded_step, ShardedPipeline, rsag_step) bit
for bit, in worker-rank order, on every lane layout its owner kernels can take.

Every comparison in this file is np.array_equal on uint32 views (or == on integers and doubles);
the only tolerance is metric_exact.logloss_sum's own bound on the loss, as in
tests/test_gpu_split_exact.py.  The yardstick is oracle/dist_oracle.py (ShardedOracle, AggOracle,
StaleOracle), which applies a key's records in rank order, on the batches of tests/dist_ref.py:
every owner holds keys pushed by every subset of the workers, the merged runs put equal keys of
two ranks across merge-tile boundaries, worker 0 holds keys of 129 and 1025 occurrences, and
tests/test_dist_ref.py shows on the CPU that applying the records in another order changes bits
on every owner (push_agg=sum: only through keys that three or more workers push).

Per step and worker: the predictions, AUC * n, the loss (within its bound), nrows.  After the last
step: EVERY key of the union of all batches on its owner — the state (w, sqrt_g, z, fea_cnt) and
V | Vaux as Store.entry returns them — and every server's seed, n_keys, new_w and V-row count.

The owner kernels' lanes (vec_group, dist.hip:580-585, restated here; every case asserts the G it
names) and the worker's (launch_fwd_records, launch_bwd_positions: lanes_for(d, records_vec(d)),
fm.hip:679-696 and :792-802, with BwdArgs::cpl == 0) are derived, not read from the device, so a
changed rule needs its row here changed with it.  V_dim 260 is a multiple of 4 but not of the 8
coordinates a float4 lane would hold above 256: the worker takes the scalar lanes there (before this
file existed it took float4 lanes, read the record's {w, live} as coordinates 260..263 and wrote
XV*p over the row's p, so every gradient was zero and the model never moved).

rsag_step: LoopbackComm.reduce_scatter_sum adds whole buffers in rank order starting from worker
0's, a worker that lacks a key contributing a zero row; x + 0.0 == x for every x but -0.0.  The
zero-sign note of the issue was NOT needed: the rsag cases below compare every bit like the
others."""
import time

import numpy as np
import pytest
import torch

from tests import dist_ref as X
from tests import metric_exact as M
from tests.test_gpu_backward_paths import _entry_eq
from tests.test_gpu_split_exact import _bits, _first_diff, _lanes_for

pytestmark = pytest.mark.gpu

T, V = X.T, X.V


@pytest.fixture(scope="module")
def H():
    from difacto_amd import hotpath
    return hotpath


@pytest.fixture(scope="module")
def DI():
    from difacto_amd import dist
    return dist


def _worker_lanes(d):
    """launch_fwd_records / launch_bwd_positions: float4 lanes when V_dim is a multiple of the
    lane's CPL (records_vec, fm.hip:792-802), else the scalar set"""
    g, c, vec = _lanes_for(d)
    return _lanes_for(d, vec=False) if vec and d % c else (g, c, vec)


def _vec_group(d):
    """vec_group (dist.hip:580-585): lanes per key of the owner's _vec kernels, 0: the scalar ones"""
    if d <= 0 or d % 4:
        return 0
    g = 1
    while g < d // 4 and g < 64:
        g <<= 1
    return g


# V_dim, owner lanes G, float4 chunks per record nc, the worker's (G, CPL, float4)
LANES = [
    (0, 0, 0, (1, 1, False)),
    (5, 0, 0, (8, 1, False)),        # scalar k_fm_fwd / k_fm_bwd over unaligned records
    (4, 1, 1, (1, 4, True)),
    (8, 2, 2, (2, 4, True)),
    (16, 4, 4, (4, 4, True)),
    (32, 8, 8, (8, 4, True)),
    (64, 16, 16, (16, 4, True)),
    (128, 32, 32, (32, 4, True)),
    (256, 64, 64, (64, 4, True)),
    (260, 64, 65, (64, 8, False)),   # nc > G: the second-chunk branch c != l of the _vec kernels
]


def test_lane_table_covers_every_group():
    for d, G, nc, wk in LANES:
        assert _vec_group(d) == G and (d // 4 if G else 0) == nc and _worker_lanes(d) == wk, d
    assert {G for _, G, _, _ in LANES} == {0, 1, 2, 4, 8, 16, 32, 64}   # DFX_DIST_GROUPS and scalar
    assert any(nc > G > 0 for _, G, nc, _ in LANES)
    assert any(G == 0 and d > 0 for d, G, _, _ in LANES)


def _cfg_key(cfg, d):
    return tuple(sorted(dict(cfg, V_dim=d).items()))


_refs = {}


def _reference(N, agg, cfg, d, sched, stale=False, events=False):
    """computed once per case and left unchanged"""
    key = (N, agg, _cfg_key(cfg, d), sched, stale, events)
    if key not in _refs:
        _refs[key] = X.reference(N, agg, key[2], sched, stale=stale, events=events)
    return _refs[key]


def _contexts(H, DI, N, d, agg, cfg, max_keys=1 << 15):
    ctxs = [H.Context(0, max_keys=max_keys, push_agg=agg, V_dim=d, **cfg) for _ in range(N)]
    return ctxs, [DI.Shard(c, N) for c in ctxs]


def _check_worker(H, ctx, blk, pred, want, tag):
    """one worker's step: predictions, AUC * n, loss, nrows"""
    pr = H.progress(ctx)
    assert pr["nrows"] == blk.size, tag
    if blk.size == 0:
        return
    p = pred.cpu().numpy()
    diff = _first_diff(p, want[2])
    assert diff is None, ("pred", tag, diff)
    assert pr["auc"] == M.auc_times_n(blk.labels, p), ("auc", tag)
    S, tol = M.logloss_sum(blk.labels, p)
    assert abs(pr["loss"] - S) <= tol, ("loss", tag, pr["loss"], S, tol)


def _check_model(H, ctxs, ref, N, agg, tag):
    """every key of the union on its owner, and every server's counters"""
    for c in ctxs:
        c.sync()
    stores = [H.Store(c) for c in ctxs]
    bad = []
    for k, o, e in zip(ref["keys"], ref["own"], ref["entries"]):
        got = stores[o].entry(k)
        if not _entry_eq(got, e):
            bad.append((int(k), int(o), got, e))
    if bad:
        k, o, got, e = bad[0]
        what = "presence"
        if got is not None and e is not None:
            what = ("state", _first_diff(got[0], e[0]))
            if what[1] is None and got[1] is not None and e[1] is not None:
                what = ("V|Vaux", _first_diff(got[1], e[1]))
        raise AssertionError((tag, "%d of %d keys differ" % (len(bad), len(ref["keys"])),
                              "first: key %#x owner %d" % (k, o), what))
    stats = [s.stats() for s in stores]
    if agg == "sum":    # the servers together hold the one Updater's model (_check_servers)
        seed, size, new_w = ref["stats"][0]
        assert all(st["seed"] == seed for st in stats), (tag, stats, seed)
        assert sum(st["n_keys"] for st in stats) == size, tag
        assert sum(st["new_w"] for st in stats) == new_w, tag
        assert [st["n_keys"] for st in stats] == [int(np.sum(ref["own"] == g)) for g in range(N)]
    else:
        for g in range(N):
            assert (stats[g]["seed"], stats[g]["n_keys"], int(stats[g]["new_w"])) == \
                ref["stats"][g], (tag, g, stats[g], ref["stats"][g])
    assert [st["n_vrows"] for st in stats] == ref["vrows"], (tag, stats, ref["vrows"])
    return len(ref["keys"])


def _snapshot(H, ctxs, ref, N):
    """the owners' Get of their keys of the union, and their counters (Get inserts an absent key:
    taken only in schedules whose every step holds the same keys, after the first step)"""
    out = []
    for g in range(N):
        v, l = H.Store(ctxs[g]).pull(ctxs[g].tensor(ref["keys"][ref["own"] == g], torch.int64))
        out.append((_bits(v.cpu().numpy()).copy(), None if l is None else l.cpu().numpy().copy(),
                    H.Store(ctxs[g]).stats()))
    return out


def _same_snapshot(a, b):
    return all(np.array_equal(x[0], y[0]) and (x[1] is None or np.array_equal(x[1], y[1]))
               and x[2] == y[2] for x, y in zip(a, b))


def _sync_case(H, DI, step, N, d, agg, cfg, sched, events=False):
    """N fresh loopback shards on the one GPU through `step` (dist.sharded_step | rsag_step)
    against the oracle: every step's workers, then the whole model"""
    t0 = time.perf_counter()
    ref = _reference(N, agg, cfg, d, sched, events=events)
    t1 = time.perf_counter()
    ctxs, shards = _contexts(H, DI, N, d, agg, cfg)
    comm = DI.LoopbackComm(N)
    dev = {}
    for s, (which, job, cnt) in enumerate(X.SCHEDULES[sched]):
        blocks = X.batches_for(N, which)
        if which not in dev:
            dev[which] = [H.DeviceRowBlock(ctxs[r], blocks[r]) for r in range(N)]
        preds = [torch.zeros(b.size, dtype=torch.float32, device=ctxs[0].device) for b in blocks]
        before = _snapshot(H, ctxs, ref, N) if job != T and s > 0 else None
        step(shards, dev[which], comm, job, push_cnt=cnt, preds=preds)
        for r in range(N):
            _check_worker(H, ctxs[r], blocks[r], preds[r], ref["out"][s][r], (N, d, agg, s, r))
        if before is not None:      # a step without a push leaves the model untouched
            assert _same_snapshot(before, _snapshot(H, ctxs, ref, N)), (N, d, agg, s)
    n = _check_model(H, ctxs, ref, N, agg, (N, d, agg, sched))
    for c in ctxs:
        c.close()
    print("N %d V_dim %d %s %s: %d keys compared; reference %.2f s, device and checks %.2f s"
          % (N, d, agg, sched, n, t1 - t0, time.perf_counter() - t1))
    return ref


# ---------------------------------------------------------------- dist.sharded_step
@pytest.mark.parametrize("agg", ["ranks", "sum"])
@pytest.mark.parametrize("i", range(len(LANES)), ids=lambda i: "d%d" % LANES[i][0])
def test_sharded_step_bit_equal(H, DI, i, agg):
    """N = 3, V_threshold = 0, l1 = 0: steps 0 and 1 push counts (owner_segs, k_dist_feacnt,
    k_dist_pull / _vec), a validation step leaves the model untouched, steps 3 and 4 push no
    counts (k_dist_segs_pull at V_dim % 4 == 0)"""
    d, G, nc, wk = LANES[i]
    assert _vec_group(d) == G and _worker_lanes(d) == wk
    _sync_case(H, DI, DI.sharded_step, 3, d, agg, X.TRAIN, "lanes")


@pytest.mark.parametrize("agg", ["ranks", "sum"])
@pytest.mark.parametrize("i", range(1, len(LANES)), ids=lambda i: "d%d" % LANES[i][0])
def test_sharded_step_lazy_v_bit_equal(H, DI, i, agg):
    """V_threshold = 4, l1 > 0, l1_shrk on, labels flipped on odd steps, at every V_dim > 0 (V_dim 0
    has no V to be lazy about).  Counted on the oracle's state, each > 0: a count push that takes
    a key over the threshold (push_agg=ranks: at a rank > 0, the frank of k_dist_feacnt; sum has
    one Update per key and no frank), an InitV raised by a gradient push, keys pulled with their V
    hidden (record live == 0, vrow >= 0) that get no V update, keys pulled without V that get
    none"""
    d, G, nc, wk = LANES[i]
    assert _vec_group(d) == G and _worker_lanes(d) == wk
    ev = _sync_case(H, DI, DI.sharded_step, 3, d, agg, X.LAZY, "lazy", events=True)["events"]
    assert ev["cross"] > 0 and ev["initv_push"] > 0 and ev["hidden"] > 0 and ev["no_v"] > 0, ev
    if agg == "ranks":
        assert ev["cross_late"] > 0, ev


@pytest.mark.parametrize("agg", ["ranks", "sum"])
@pytest.mark.parametrize("d", [0, 16])
@pytest.mark.parametrize("N", [2, 5])
def test_sharded_step_other_rank_counts_bit_equal(H, DI, N, d, agg):
    """one merge round (N = 2) and three (N = 5: the lone fifth run passes two rounds); the middle
    steps run the variant batch: the last owner receives no key from worker 0 (an empty run
    inside its merge) and one worker's batch is empty (0 rows; at N = 2 owner 1 then receives
    nothing at all)"""
    _sync_case(H, DI, DI.sharded_step, N, d, agg, X.TRAIN, "holes")


# ---------------------------------------------------------------- dist.rsag_step
@pytest.mark.parametrize("d", [0, 16, 260])
def test_rsag_step_bit_equal(H, DI, d):
    """the union-indexed all-gather / reduce-scatter schedule against AggOracle"""
    _sync_case(H, DI, DI.rsag_step, 3, d, "sum", X.TRAIN, "lanes")


# ---------------------------------------------------------------- dist.ShardedPipeline
def _pipe_case(H, DI, N, d, agg, sched, max_keys=1 << 15):
    ref = _reference(N, agg, X.TRAIN, d, sched, stale=True)
    ctxs, shards = _contexts(H, DI, N, d, agg, X.TRAIN, max_keys)
    pipe = DI.ShardedPipeline(shards, DI.LoopbackComm(N))
    live, got, caps = [], [], []
    for s, (which, job, cnt) in enumerate(X.SCHEDULES[sched]):
        blocks = X.batches_for(N, which)
        dbs = [H.DeviceRowBlock(ctxs[r], blocks[r]) for r in range(N)]
        preds = [torch.zeros(b.size, dtype=torch.float32, device=ctxs[0].device) for b in blocks]
        pipe.submit(dbs, job, push_cnt=cnt, preds=preds)
        live.append(dbs)        # batches stay alive until the pipeline is flushed
        got.append(preds)
        if s == 1:              # step 0 has run (its push is pending), step 1 is queued
            caps.append([H.Store(c).probe_stats()[2] for c in ctxs])
    pipe.flush()
    caps.append([H.Store(c).probe_stats()[2] for c in ctxs])
    nrows = [0] * N
    auc = [0.0] * N
    loss = [0.0] * N
    tol = [0.0] * N
    for s, (which, job, cnt) in enumerate(X.SCHEDULES[sched]):
        blocks = X.batches_for(N, which)
        for r in range(N):
            p = got[s][r].cpu().numpy()
            diff = _first_diff(p, ref["out"][s][r][2])
            assert diff is None, ("pred", N, d, agg, s, r, diff)
            nrows[r] += blocks[r].size
            auc[r] += M.auc_times_n(blocks[r].labels, p)      # added per step, in step order
            S, t = M.logloss_sum(blocks[r].labels, p)
            loss[r] += S
            tol[r] += t
    for r in range(N):
        pr = H.progress(ctxs[r])
        assert pr["nrows"] == nrows[r]
        assert pr["auc"] == auc[r], (r, pr["auc"], auc[r])
        assert abs(pr["loss"] - loss[r]) <= tol[r], (r, pr["loss"], loss[r], tol[r])
    _check_model(H, ctxs, ref, N, agg, (N, d, agg, sched))
    for c in ctxs:
        c.close()
    return caps


@pytest.mark.parametrize("agg", ["ranks", "sum"])
@pytest.mark.parametrize("d", [16, 260])
def test_sharded_pipeline_bit_equal(H, DI, d, agg):
    """the 1-step-stale schedule against StaleOracle on test_gpu_dist.PIPE_JOBS' pattern, the
    batch alternating with one of another key universe"""
    _pipe_case(H, DI, 3, d, agg, "pipe")


@pytest.mark.parametrize("agg", ["ranks", "sum"])
def test_sharded_pipeline_growing_table_bit_equal(H, DI, agg):
    """max_keys = 256 and a first step of 12 rows per worker: the owners' tables still have their
    first capacity after step 0 and grow at a later owner_begin, while the other slot (the
    previous step, its push pending) holds table positions: table_rebuild moves them
    (k_remap_segslots)"""
    first, last = _pipe_case(H, DI, 3, 16, agg, "grow", max_keys=256)
    assert all(a < b for a, b in zip(first, last)), (first, last)
    assert all(a == 512 for a in first), first      # table_alloc: 2 * max_keys slots
