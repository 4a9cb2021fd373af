"""The owner-computes split step (csrc/split.hip, dist.split_step, SplitPipeline, SplitStore) at
N > 1 owners, bit for bit, on every lane layout its kernels can take.

Every comparison in this file is np.array_equal on uint32 views (or == on integers and doubles):
there is no tolerance, except the loss, which is held to metric_exact.logloss_sum's own bound
as in tests/test_gpu_split.py.  The yardstick is tests/split_ref.py, the step in numpy in the
device's order (pinned on the CPU by tests/test_split_ref.py): the owners' partial rows
[XV | sum w x | sum_l XXVV_l | 0 0], the workers' predictions and [XV p | p | 0 0 0] rows, and the
model after the owners' backward (tests/backward_ref.py on the concatenated batch).

The batch (split_ref.planted_workers): N workers x 420 rows x 40 nnz (worker 1: 360 rows, so
padded rows exist), even ranks binary, odd valued, every seventh row weight 0.0; every owner holds
keys at exactly 1, 8 | 9, 127 | 128 | 129, 256 | 257, 896 | 897, 1024 | 1025 and 4097
occurrences over the concatenated batch, spread over all workers (a long key's chunks straddle
worker boundaries), so the owner's chunk_plan, k_fm_bwd_chunks, k_chunk_hotgroup and
k_chunk_hotsum run with BwdArgs::p == nullptr (or the k_split_p_compact array); worker 0 also
holds rows of 0, 1, 41, 81 and 700 nnz and one with keys of owner 0 alone.  Every V_dim runs the
whole batch (three reference steps take about a second at V_dim 513).  Every owner's chunk plan
(72 chunks per owner) is asserted through dfx_localize_occ(keys_ready), on a context of its own,
over the owner's received rows as this file rebuilds them in numpy, the way
tests/test_gpu_backward_paths.py does: dfx_split_owner_stats and dfx_prof_counts do not expose
the count of the owners that run the step, so a wrong received-row layout in them would show in
the bit-for-bit comparisons of the partials and the model, not in that assertion.

The cases (TABLE): every forward kernel launch_fwd_fused reaches with FwdArgs::part set (fm.hip
:730-788; lr_lanes is excluded by !a.part), every combine kernel (split.hip:594-598), every
source of p in the backward (row_p, fm.hip:806-809; compact at d >= 64 && d % 32 == 0,
split.hip:682) on one- and two-pass backwards; _layout() restates the rules and the contexts'
defaults (fat_fwd=1, fwd_cpl=8, bwd_cpl=8, bwd_cpl_from=64, bwd_two_pass=1; ctx.hip:62-104) and
every case asserts the layout it names: as in tests/test_gpu_backward_paths.py the layout is
derived, not read from the device, so a changed default needs its row here changed with it."""
import functools
import time

import numpy as np
import pytest
import torch

from oracle import dist_oracle as DO
from oracle import oracle as O
from tests import backward_ref as R
from tests import metric_exact as M
from tests import split_ref as S
from tests.test_gpu_backward_paths import LAZY_L1, _entry_eq
from tests.test_gpu_backward_paths import _layout as _bwd_layout

pytestmark = pytest.mark.gpu

TRAIN = dict(V_threshold=0, l1=0, lr=.05, V_lr=.01)
LAZY = dict(V_threshold=300, l1=LAZY_L1, l1_shrk=1, lr=.05, V_lr=.01)


@pytest.fixture(scope="module")
def H():
    from difacto_amd import hotpath
    return hotpath


@pytest.fixture(scope="module")
def DI():
    from difacto_amd import dist
    return dist


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _first_diff(got, want):
    """-> None when bit-equal, else (differing floats, first index, got, want)"""
    g, w = _bits(got), _bits(want)
    if g.shape != w.shape:
        return ("shape", g.shape, w.shape)
    bad = np.argwhere(g != w)
    if len(bad) == 0:
        return None
    i = tuple(int(v) for v in bad[0])
    return (len(bad), i, float(np.asarray(got)[i]), float(np.asarray(want)[i]))


# ---------------------------------------------------------------- the layouts
def _lanes_for(d, vec=True):
    """lanes_for (fm.hip:679-696) -> (G, CPL, float4)"""
    if d <= 0:
        return 1, 1, False
    if vec and d % 4 == 0:
        cpl = 4
        while d // cpl > 64:
            cpl *= 2
        g = 1
        while g < (d + cpl - 1) // cpl:
            g <<= 1
        return g, cpl, True
    g = 1
    while g < min(d, 64):
        g <<= 1
    cpl = 1
    while cpl < (d + g - 1) // g:
        cpl <<= 1
    return g, cpl, False


def _layout(d, slot_layout="auto", fat_fwd=1, fwd_cpl=8, **kw):
    """-> (forward kernel, combine lanes per row (0: k_split_combine), backward (G, CPL, float4 |
    scalar, passes), source of p, pxv row floats): launch_fwd_fused with part set, fat_es
    (common.h:217-220), dfx_split_combine_rows' G, test_gpu_backward_paths._layout (bwd_lanes,
    bwd_two_pass), the compact-p rule and split_pxv_floats(d, 1) restated"""
    G, CPL, vec = _lanes_for(d)
    es = 0
    if slot_layout != "split" and d >= 4 and d % 4 == 0 and 32 + 4 * d <= 128:
        es = 64 if 32 + 4 * d <= 64 else 128
    if es and fat_fwd and vec and CPL == 4 and 4 * G == d and G in (2, 4):
        fwd = ("walk", G)
    elif vec and CPL == 4 and 4 <= G <= 32:
        if fwd_cpl == 8 and d >= 64 and d % 8 == 0 and G >= 8:
            fwd = ("probe", G // 2, 8)
        else:
            fwd = ("probe", G, 4)
    else:
        fwd = ("fwd", G, CPL, "v" if vec else "s")
    cg = 0
    if d > 0 and d % 4 == 0 and d <= 256:
        cg = 1
        while 4 * cg < d:
            cg <<= 1
    bwd = _bwd_layout(d, slot_layout=slot_layout, **kw)
    assert bwd[4] == es
    psrc = "compact" if d >= 64 and d % 32 == 0 else "row"
    return fwd, cg, bwd[:4], psrc, S.pxv_floats(d)


def _s(g, c):
    return ("fwd", g, c, "s")


# V_dim, owners, context kwargs, the layout
TABLE = [
    (0, 3, {}, (_s(1, 1), 0, (1, 1, "s", 1), "row", 4)),
    (1, 3, {}, (_s(1, 1), 0, (1, 1, "s", 1), "row", 32)),
    (2, 3, {}, (_s(2, 1), 0, (2, 1, "s", 1), "row", 32)),
    (3, 3, {}, (_s(4, 1), 0, (4, 1, "s", 1), "row", 32)),
    (5, 3, {}, (_s(8, 1), 0, (8, 1, "s", 1), "row", 32)),
    (9, 3, {}, (_s(16, 1), 0, (16, 1, "s", 1), "row", 32)),
    (31, 3, {}, (_s(32, 1), 0, (32, 1, "s", 1), "row", 35)),      # pxv stride 35: unaligned rows
    (33, 3, {}, (_s(64, 1), 0, (64, 1, "s", 1), "row", 64)),
    (66, 3, {}, (_s(64, 2), 0, (64, 2, "s", 1), "row", 96)),
    (130, 3, {}, (_s(64, 4), 0, (64, 4, "s", 1), "row", 160)),
    (257, 3, {}, (_s(64, 8), 0, (64, 8, "s", 1), "row", 288)),
    (513, 3, {}, (_s(64, 16), 0, (64, 16, "s", 1), "row", 544)),
    (4, 3, {}, (("fwd", 1, 4, "v"), 1, (1, 4, "v", 1), "row", 32)),       # 64-byte fat slot
    (8, 3, {}, (("walk", 2), 2, (2, 4, "v", 1), "row", 32)),
    (8, 3, dict(fat_fwd=0), (("fwd", 2, 4, "v"), 2, (2, 4, "v", 1), "row", 32)),
    (16, 3, {}, (("walk", 4), 4, (4, 4, "v", 1), "row", 32)),
    (16, 3, dict(slot_layout="split"), (("probe", 4, 4), 4, (4, 4, "v", 1), "row", 32)),
    (16, 3, dict(bwd_cpl_from=16), (("walk", 4), 4, (2, 8, "v", 1), "row", 32)),
    (24, 3, {}, (("probe", 8, 4), 8, (8, 4, "v", 1), "row", 32)),   # 128-byte fat slot, no walk
    (28, 3, {}, (("probe", 8, 4), 8, (8, 4, "v", 1), "row", 32)),   # pxv row 32 floats, p at [28]
    (64, 3, {}, (("probe", 8, 8), 16, (8, 8, "v", 1), "compact", 96)),
    (64, 3, dict(fwd_cpl=4), (("probe", 16, 4), 16, (8, 8, "v", 1), "compact", 96)),
    (72, 3, {}, (("probe", 16, 8), 32, (32, 4, "v", 2), "row", 96)),
    (128, 3, {}, (("probe", 16, 8), 32, (32, 4, "v", 2), "compact", 160)),
    (128, 3, dict(fwd_cpl=4), (("probe", 32, 4), 32, (32, 4, "v", 2), "compact", 160)),
    (128, 3, dict(bwd_two_pass=0), (("probe", 16, 8), 32, (16, 8, "v", 1), "compact", 160)),
    (256, 3, {}, (("fwd", 64, 4, "v"), 64, (64, 4, "v", 2), "compact", 288)),
    (16, 2, {}, (("walk", 4), 4, (4, 4, "v", 1), "row", 32)),
    (16, 8, {}, (("walk", 4), 4, (4, 4, "v", 1), "row", 32)),
    (128, 2, {}, (("probe", 16, 8), 32, (32, 4, "v", 2), "compact", 160)),
    (128, 8, {}, (("probe", 16, 8), 32, (32, 4, "v", 2), "compact", 160)),
]
# the labels flip on odd steps (w returns through zero) in one even and one odd row
FLIP = (15, 22)


def test_split_table_covers_every_layout():
    """the table names what _layout derives, and holds every forward kernel launch_fwd_fused
    reaches in partial mode, every combine kernel and every (p source, passes) of the backward"""
    for d, _, kw, want in TABLE:
        assert _layout(d, **kw) == want, (d, kw)
    assert TABLE[FLIP[0]][0] == 16 and TABLE[FLIP[1]][0] == 72 and FLIP[0] % 2 != FLIP[1] % 2
    fwd = {w[0] for _, _, _, w in TABLE}
    walk = {("walk", 2), ("walk", 4)}
    # k_fm_fwd_probe<G, 4> needs 4 <= G <= 32, <G, 8> V_dim >= 64 (16 lanes or more, halved)
    probe = {("probe", g, 4) for g in (4, 8, 16, 32)} | {("probe", 8, 8), ("probe", 16, 8)}
    # k_fm_fwd<.., kFusedProbe, true, ..>: the scalar set (DFX_SCALAR_SET, fm.hip:698-700) and
    # the float4 set that neither the walk nor the probe takes
    scalar = {_s(g, 1) for g in (1, 2, 4, 8, 16, 32, 64)} | {_s(64, c) for c in (2, 4, 8, 16)}
    vec = {("fwd", 1, 4, "v"), ("fwd", 2, 4, "v"), ("fwd", 64, 4, "v")}
    assert fwd == walk | probe | scalar | vec
    assert {w[1] for _, _, _, w in TABLE} == {0, 1, 2, 4, 8, 16, 32, 64}
    assert {(w[3], w[2][3]) for _, _, _, w in TABLE} == {("row", 1), ("row", 2), ("compact", 1),
                                                         ("compact", 2)}
    assert {w[2] for _, _, _, w in TABLE} >= {(2, 8, "v", 1), (16, 8, "v", 1), (64, 8, "s", 1)}
    assert any(w[4] % 4 for _, _, _, w in TABLE) and any(w[4] == 32 for _, _, _, w in TABLE)
    assert {N for _, N, _, _ in TABLE} == {2, 3, 8}


# ---------------------------------------------------------------- the batch and the reference
@functools.lru_cache(maxsize=None)
def _batch(N):
    """-> (blocks, label-flipped blocks, batch_info, 48 sampled short keys per owner)"""
    blocks = S.planted_workers(N)
    info = S.batch_info(blocks, N)      # the planted counts are exact, no other key chunked
    assert all(n > 0 for n in info["chunks"]) and info["spread"] and info["straddle"]
    rng = np.random.default_rng(5)
    short = info["cnt"] <= R.kChunkOcc
    sample = np.concatenate([rng.choice(info["uniq"][short & (info["own"] == o)], 48,
                                        replace=False) for o in range(N)])
    for b in blocks:
        for a in (b.offs, b.ids, b.vals, b.labels, b.weights):
            if a is not None:
                a.setflags(write=False)
    return blocks, S.flipped(blocks), info, sample


# schedules: per step (batch: 0 the batch | 1 its flipped labels | 2 another batch, job, count push)
def _schedule(name):
    T, V, P = 3, 4, 5   # hotpath.kTraining, kValidation, kPrediction
    if name == "train":
        return [(0, T, True), (0, T, False), (0, T, False)]
    if name == "flip":
        return [(0, T, True), (1, T, False), (0, T, False)]
    if name == "lazy":
        return [(s % 2, T, s == 0) for s in range(5)]
    assert name == "nobwd"
    return [(0, T, True), (0, T, False), (2, V, False), (2, P, False), (0, T, False)]


def _blocks(N, which):
    if which == 2:   # fewer planted keys, so background keys the batch has not: new to the model
        return S.planted_workers(N, S.COUNTS[:9], seed=23)
    return _batch(N)[which]


def _cfg_key(cfg):
    return tuple(sorted(cfg.items()))


@functools.lru_cache(maxsize=None)
def _reference(N, d, cfg_key, sched):
    """the schedule on an oracle Updater through split_ref.split_step -> per step the workers'
    (parts, pred, pxv), and the model after it: per owner Get of its keys of the step, the
    entries of the chunked and the sampled keys, the rand_r state, new_w and the key count; and
    over the steps a later backward reads, the chunked keys met without V / with a hidden V"""
    cfg = dict(cfg_key, V_dim=d)
    _, _, binfo, sample = _batch(N)
    watch = np.concatenate([binfo["chunked_keys"], sample])
    up = O.Updater(**cfg)
    steps = []
    novee = hidden = 0
    sch = _schedule(sched)
    for s, (which, job, cnt) in enumerate(sch):
        blocks = _blocks(N, which)
        info = {}
        before = up.size()
        out = S.split_step(up, blocks, N, push_cnt=cnt, train=job == 3, info=info)
        uniq = info["uniq"]
        own = DO.owner_of(uniq, N)
        gets = [up.get(uniq[own == o]) for o in range(N)]
        steps.append(dict(out=out, uniq=uniq, own=own, gets=gets,
                          entries=[up.entry(k) for k in watch], seed=up.seed,
                          new_w=int(up.new_w), size=up.size(), grew=up.size() - before))
        if d > 0 and s < len(sch) - 1:      # what the next step's backward will read
            ck = binfo["chunked_keys"]
            ent = [up.entry(k) for k in ck]
            ln = up.get(ck)[1]
            novee += sum(e[1] is None for e in ent)
            hidden += sum(e[1] is not None and n == 1 for e, n in zip(ent, ln))
    return steps, watch, novee, hidden


# ---------------------------------------------------------------- the device chunk plan
@pytest.fixture(scope="module")
def plan_ctx(H):
    c = H.Context(0)
    yield c
    c.close()


_plans = {}


def _assert_chunk_plan(H, plan_ctx, N):
    """every owner's device chunk plan (chunk_plan after the owner's Localizer, split.hip:484-485)
    holds the chunks the batch is built for: the owner's received rows — every worker's M
    (padded) rows in rank order, each row's keys of this owner in nnz order — through
    dfx_localize_occ(keys_ready)"""
    if N not in _plans:
        blocks, _, info, _ = _batch(N)
        Mrows = max(b.size for b in blocks)
        got = []
        for o in range(N):
            offs, keys = [np.zeros(1, np.int64)], []
            base = 0
            for b in blocks:
                k = S.reverse_bytes(b.ids)
                mine = DO.owner_of(k, N) == o
                row = np.repeat(np.arange(b.size), np.diff(b.offs.astype(np.int64)))
                per = np.bincount(row[mine], minlength=Mrows)
                offs.append(base + np.cumsum(per))
                base += int(per.sum())
                keys.append(k[mine])
            r = H.localize_occ(plan_ctx, np.concatenate(offs), np.concatenate(keys),
                               keys_ready=True)
            got.append(r["n_chunks"])
        _plans[N] = (got, info["chunks"])
    got, want = _plans[N]
    assert got == want and all(n > 0 for n in want), (N, got, want)
    return got


# ---------------------------------------------------------------- dist.split_step
def _contexts(H, DI, N, d, cfg, kw):
    ctxs = [H.Context(0, max_keys=1 << 16, push_agg="sum", V_dim=d, **cfg, **kw)
            for _ in range(N)]
    return ctxs, [DI.Shard(c, N) for c in ctxs]


def _device_blocks(H, ctxs, N, sched):
    dev = {}
    for which in sorted({w for w, _, _ in _schedule(sched)}):
        blocks = _blocks(N, which)
        dev[which] = (blocks, [H.DeviceRowBlock(ctxs[r], blocks[r]) for r in range(N)])
    return dev


def _check_model(H, ctxs, ref, watch, N, d, tag):
    for c in ctxs:
        c.sync()
    stats = [H.Store(c).stats() for c in ctxs]
    assert all(st["seed"] == ref["seed"] for st in stats), tag
    assert sum(st["new_w"] for st in stats) == ref["new_w"], tag
    assert sum(st["n_keys"] for st in stats) == ref["size"], tag
    for o in range(N):
        keys = ref["uniq"][ref["own"] == o]
        v, l = H.Store(ctxs[o]).pull(ctxs[o].tensor(keys, torch.int64))
        ov, ol = ref["gets"][o]
        if d > 0:
            assert np.array_equal(l.cpu().numpy(), ol), (tag, o)
        assert _first_diff(v.cpu().numpy(), ov) is None, (tag, o, _first_diff(v.cpu().numpy(), ov))
    own = DO.owner_of(watch, N)
    for k, o, e in zip(watch, own, ref["entries"]):
        assert _entry_eq(H.Store(ctxs[o]).entry(k), e), (tag, int(k), int(o))


def _split_case(H, DI, plan_ctx, N, d, cfg, kw, sched):
    """N fresh loopback shards on the one GPU through dist.split_step against the reference,
    after every step"""
    steps, watch, novee, hidden = _reference(N, d, _cfg_key(cfg), sched)
    chunks = _assert_chunk_plan(H, plan_ctx, N)
    ctxs, shards = _contexts(H, DI, N, d, cfg, kw)
    comm = DI.LoopbackComm(N)
    dev = _device_blocks(H, ctxs, N, sched)
    for s, (which, job, cnt) in enumerate(_schedule(sched)):
        blocks, dbs = dev[which]
        ref = steps[s]
        preds = [torch.zeros(b.size, dtype=torch.float32, device=ctxs[0].device) for b in blocks]
        keep = {}
        DI.split_step(shards, dbs, comm, job, push_cnt=cnt, preds=preds, keep=keep)
        Mr, PS, PX = keep["M"], d + 4, S.pxv_floats(d)
        assert Mr == max(b.size for b in blocks) and Mr > min(b.size for b in blocks)
        parts = [t.cpu().numpy().reshape(N, Mr, PS) for t in keep["parts"]]
        rparts = [t.cpu().numpy().reshape(N, Mr, PS) for t in keep["rparts"]]
        pxv = [t.cpu().numpy().reshape(Mr, PX) for t in keep["pxv"]]
        for i, b in enumerate(blocks):
            B = b.size
            rp, rpred, rpxv = ref["out"][i]
            for o in range(N):
                diff = _first_diff(parts[o][i, :B], rp[o])
                assert diff is None, ("partial", s, "owner", o, "worker", i, diff)
                assert not _bits(parts[o][i, B:]).any(), ("padded partial", s, o, i)
                assert np.array_equal(_bits(rparts[i][o]), _bits(parts[o][i])), (s, o, i)
            p = preds[i].cpu().numpy()
            assert _first_diff(p, rpred) is None, ("pred", s, i, _first_diff(p, rpred))
            diff = _first_diff(pxv[i][:B], rpxv)
            assert diff is None, ("pxv", s, "worker", i, diff)
            assert not _bits(pxv[i][B:]).any(), ("padded pxv", s, i)
            pr = H.progress(ctxs[i])
            assert pr["nrows"] == B
            assert pr["auc"] == M.auc_times_n(b.labels, p), (s, i)
            Sx, tol = M.logloss_sum(b.labels, p)
            assert abs(pr["loss"] - Sx) <= tol, (s, i, pr["loss"], Sx, tol)
        _check_model(H, ctxs, ref, watch, N, d, (d, N, s))
    for c in ctxs:
        c.close()
    return steps, chunks, novee, hidden


def _id(i):
    d, N, kw, _ = TABLE[i]
    return "d%d-N%d-%s" % (d, N, "-".join("%s%s" % kv for kv in sorted(kw.items())) or "default")


@pytest.mark.parametrize("i", range(len(TABLE)), ids=_id)
def test_split_step_bit_equal(H, DI, plan_ctx, i):
    d, N, kw, want = TABLE[i]
    assert _layout(d, **kw) == want
    t0 = time.perf_counter()
    _, chunks, _, _ = _split_case(H, DI, plan_ctx, N, d, TRAIN, kw, "flip" if i in FLIP else "train")
    print("layout %s chunks per owner %s (expected and observed) %.1f s"
          % (want, chunks, time.perf_counter() - t0))


@pytest.mark.parametrize("d", [16, 128])
def test_split_lazy_v_bit_equal(H, DI, plan_ctx, d):
    """l1 > 0, V_threshold >= 1, l1_shrk on, labels flipping every step: the owners' backward
    meets chunked keys without V and with a V hidden because w returned to zero (counted on the
    reference's state); the ranked InitV draw over the owners follows the oracle's single rand_r
    sequence while the request counts go from many to none"""
    _, _, novee, hidden = _split_case(H, DI, plan_ctx, 3, d, LAZY, {}, "lazy")
    assert novee > 0 and hidden > 0, (novee, hidden)


def test_split_no_backward_bit_equal(H, DI, plan_ctx):
    """a validation and a prediction step on another batch between training steps: predictions and
    partials exact, the keys met for the first time inserted empty (Get), the model's values
    otherwise unchanged (the checks after every step), n_keys the oracle's"""
    steps, _, _, _ = _split_case(H, DI, plan_ctx, 3, 16, TRAIN, {}, "nobwd")
    assert steps[2]["grew"] > 0 and steps[3]["grew"] == 0 and steps[4]["grew"] == 0
    assert len(np.setdiff1d(steps[2]["uniq"], steps[1]["uniq"])) == steps[2]["grew"]
    # the reference's watched entries (the device's equal them after every step) did not move
    for s in (2, 3):
        assert all(_entry_eq(a, b) for a, b in zip(steps[1]["entries"], steps[s]["entries"]))
    assert not all(_entry_eq(a, b) for a, b in zip(steps[1]["entries"], steps[4]["entries"]))


# ---------------------------------------------------------------- the other drivers
def _driver_case(H, DI, N, d, make, submit, finish):
    """the three-step planted run through another driver: predictions of every step and, after
    the last, the model against the same reference"""
    steps, watch, _, _ = _reference(N, d, _cfg_key(TRAIN), "train")
    ctxs, shards = _contexts(H, DI, N, d, TRAIN, {})
    drv = make(shards)
    dev = _device_blocks(H, ctxs, N, "train")
    blocks, dbs = dev[0]
    preds_all = []
    for s, (_, job, cnt) in enumerate(_schedule("train")):
        preds = [torch.zeros(b.size, dtype=torch.float32, device=ctxs[0].device) for b in blocks]
        submit(drv, dbs, job, cnt, preds)
        preds_all.append(preds)
    finish(drv)
    for c in ctxs:
        c.sync()
    for s, preds in enumerate(preds_all):
        for i in range(N):
            diff = _first_diff(preds[i].cpu().numpy(), steps[s]["out"][i][1])
            assert diff is None, ("pred", s, i, diff)
    _check_model(H, ctxs, steps[-1], watch, N, d, (d, N, "end"))
    return ctxs, drv


@pytest.mark.parametrize("d", [16, 128])
def test_split_pipeline_bit_equal(H, DI, d):
    ctxs, _ = _driver_case(
        H, DI, 3, d, lambda sh: DI.SplitPipeline(sh, DI.LoopbackComm(3)),
        lambda p, dbs, job, cnt, preds: p.submit(dbs, job, push_cnt=cnt, preds=preds),
        lambda p: p.flush())
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("mode", ["sync", "pipelined", "sliced"])
@pytest.mark.parametrize("d", [16, 128])
def test_split_store_bit_equal(H, DI, d, mode):
    """the C++ driver: the synchronous and the pipelined schedule, and the sliced owner forward
    (two slices: slice h's partial exchange beside slice h + 1's forward)"""
    def make(sh):
        st = DI.SplitStore(sh, pipelined=mode != "sync")
        if mode == "sliced":
            st.set_slices(2)
        return st
    ctxs, store = _driver_case(
        H, DI, 3, d, make,
        lambda st, dbs, job, cnt, preds: st.submit(dbs, job, push_cnt=cnt, preds=preds),
        lambda st: st.flush())
    store.close()
    for c in ctxs:
        c.close()
