"""The backward's sums and the updated model, bit for bit, on every path of csrc/fm.hip.

Every comparison in this file is np.array_equal on uint32 views: there is no tolerance.  The
yardstick is tests/backward_ref.py, the backward in numpy in the device's documented order
(pinned on the CPU by tests/test_backward_ref.py): the reference's sequential float sums for a key
of <= kChunkOcc occurrences, chunked double sums rounded once for a longer one.

Constants, by source line:
  kChunkOcc = 128     csrc/internal.h:408   occurrences per chunk; a key of more is chunked
  kHotChunks = 8      csrc/internal.h:411   chunks from which a key is pre-summed in two levels
  kHotGroup = 32      csrc/fm.hip:1657      chunks per level-1 group (k_chunk_hotgroup)
  kHotNT = 1024       csrc/fm.hip:1657      chunks per k_chunk_hotsum tile
  R = 64 / (d + 2)    csrc/fm.hip:1689      level-2 slices (1 when d + 2 > 64); U = 8 unrolled
  UNR = 4             csrc/fm.hip:1550      chunk_one's walk at G < 8 (G >= 8: shuffles, WU = 8)
  UNR = 4 | 2         csrc/fm.hip:813       k_fm_bwd's trips (CPL <= 4 | more)

The batch (backward_ref.planted_batch / PLANTED): 2200 rows x 40 nnz, keys planted at exactly
1, 8 | 9, 127 | 128 | 129, 256 | 257, 896 | 897, 1024 | 1025, 4096 | 4097 occurrences, repeated
inside rows and spread over them, binary and valued, every seventh row weight 0.0; 480 more
two-chunk keys take the chunk table past 1024 chunks, so the hot keys of 897 and 1024 start in
k_chunk_hotsum's first tile and the one of 4097 in its second.  The slice batches hold one key of
ng = 8 R + 1 groups (d = 16: 25 groups, 98,305 occurrences; d = 30: 17 groups, 65,537), which
enters hotsum_key's unrolled loop and leaves the slices unequal.  d = 0 (R = 32) would need a key
of over a million occurrences and is left out.

The fused cases (FUSED below): every (lanes per key G, coordinates per lane CPL, float4 or
scalar, one or two passes, slot layout) that dfx_train_step can instantiate, derived from
lanes_for (fm.hip:679-696), bwd_lanes (:1812-1824), bwd_two_pass (:1859-1864) and fat_es
(common.h:217-220); _layout() restates them and every case asserts the layout it names.  V_dim a
multiple of 4 above 256 has no fused kernel ("unsupported V_dim": launch_bwd_chunks has no
8-per-lane float4 chunk kernel), so 64 lanes x 8 and x 16 run in their scalar forms only (257,
513); those two use the planted keys without the 480 two-chunk ones (SMALL), the rest the batch."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import backward_ref as R

pytestmark = pytest.mark.gpu

SMALL = tuple(c for c in R.PLANTED[:13]) + (4097,)
SLICE = {16: 98305, 30: 65537, 128: 98305}


@pytest.fixture(scope="module")
def H():
    from difacto_amd import hotpath
    return hotpath


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _batch(kind, binary):
    """-> (blk, uniq, cnt, col, chunked mask over the keys, expected chunk count)"""
    if kind == "main":
        blk = R.planted_batch(2200, 40, R.PLANTED, binary, seed=1)
        planted = R.PLANTED
    elif kind == "small":
        blk = R.planted_batch(420, 40, SMALL, binary, seed=2)
        planted = SMALL
    else:  # the slice key, one hot key and one two-chunk key beside it
        planted = (897, int(kind), 129)
        blk = R.planted_batch(4000, 40, planted, binary, seed=3)
    uniq, cnt, col = O.localize(blk.offs, blk.ids)
    cnt = cnt.astype(np.int64)
    # the planted counts are exact, and no other key is chunked
    at = np.searchsorted(uniq, [R.planted_key(i) for i in range(len(planted))])
    assert cnt[at].tolist() == list(planted)
    rest = np.ones(len(uniq), bool)
    rest[at] = False
    assert cnt[rest].max() <= R.kChunkOcc
    for a in (blk.offs, blk.ids, blk.vals, blk.labels, blk.weights, uniq, cnt, col):
        if a is not None:
            a.setflags(write=False)
    return blk, uniq, cnt, col, cnt > R.kChunkOcc, sum(R.n_chunks(int(c)) for c in cnt)


@pytest.fixture(scope="module")
def plan_ctx(H):
    c = H.Context(0)
    yield c
    c.close()


_plans = {}


def _assert_chunk_plan(H, plan_ctx, kind, binary):
    """(c) the device's Localizer plans the chunks this batch is built for"""
    if (kind, binary) not in _plans:
        blk, _, cnt, _, _, nch = _batch(kind, binary)
        r = H.localize_occ(plan_ctx, blk.offs, blk.ids, blk.vals)
        _plans[kind, binary] = (r["n_chunks"], nch)
    got, want = _plans[kind, binary]
    assert got == want and want > 0
    if kind == "main":
        assert want > 1024                      # k_chunk_hotsum's second tile is reached
        _, _, cnt, _, _, _ = _batch(kind, binary)
        first = np.cumsum([R.n_chunks(int(c)) for c in cnt]) - \
            [R.n_chunks(int(c)) for c in cnt]
        hot = np.array([R.n_groups(int(c)) > 0 for c in cnt])
        assert np.sum(hot & (first < 1024)) >= 2 and np.sum(hot & (first >= 1024)) >= 1


def _model(rng, U, d):
    """the interleaved Pull layout, a third of the keys without V, a tenth with w == 0"""
    if d == 0:
        W = (rng.standard_normal(U) * 0.1).astype(np.float32)
        W[rng.random(U) < 0.1] = 0
        return W, None, None
    lens = np.where(rng.random(U) < 0.33, 1, d + 1).astype(np.int32)
    wp, vp = O.get_pos(lens)
    W = (rng.standard_normal(int(lens.sum())) * 0.1).astype(np.float32)
    W[wp[rng.random(U) < 0.1]] = 0
    return W, wp, vp


# ---------------------------------------------------------------- (a) dfx_fm_calcgrad
def _calcgrad_case(H, plan_ctx, kind, d, binary):
    blk, uniq, cnt, col, chunked, _ = _batch(kind, binary)
    _assert_chunk_plan(H, plan_ctx, kind, binary)
    U = len(uniq)
    W, wp, vp = _model(np.random.default_rng(1000 + d), U, d)
    c = H.Context(0)
    db = H.DeviceRowBlock(c, blk)
    dcol, duniq, _ = H.Localizer(c).compact(db)
    assert np.array_equal(H.u32(dcol), col)
    loss = H.FMLoss(c, d)
    tW = c.tensor(W, torch.float32)
    twp = None if wp is None else c.tensor(wp, torch.int32)
    tvp = None if vp is None else c.tensor(vp, torch.int32)
    pred = torch.zeros(blk.size, dtype=torch.float32, device=c.device)
    loss.predict(db, dcol, tW, twp, tvp, pred, U)
    grad = torch.zeros(len(W), dtype=torch.float32, device=c.device)
    loss.calc_grad(db, dcol, tW, twp, tvp, pred, grad, U)
    pred, grad = pred.cpu().numpy(), grad.cpu().numpy()
    c.close()
    opred = O.fm_predict(blk.offs, col, blk.vals, W, wp, vp, d)
    assert np.array_equal(_bits(pred), _bits(opred))
    want = R.backward(blk.offs, col, blk.vals, blk.labels, blk.weights, W, wp, vp, U, d, opred)
    bad = np.nonzero(_bits(grad) != _bits(want))[0]
    assert len(bad) == 0, (len(bad), bad[:8], grad[bad[:8]], want[bad[:8]])
    # (c) the chunked sums are not the reference's sequential float sums: the chunk path ran
    seq = O.fm_calcgrad(blk.offs, col, blk.vals, blk.labels, blk.weights, W, wp, vp, U, d, opred)
    wq = np.arange(U) if wp is None else wp
    assert np.any(_bits(want[wq[chunked]]) != _bits(seq[wq[chunked]]))
    assert np.array_equal(_bits(want[wq[~chunked]]), _bits(seq[wq[~chunked]]))


# d + 2 = 32 | 33 | 64 | 65: R = 2 | 1 and hotsum_key's 64-value block; d = 3 (G = 4): chunk_one's
# UNR walk; d >= 5 (G >= 8): its shuffle walk; d = 100, 200: 2 and 4 coordinates per lane
@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("d", [0, 1, 3, 5, 16, 30, 31, 62, 63, 100, 200])
def test_calcgrad_bit_equal(H, plan_ctx, d, binary):
    _calcgrad_case(H, plan_ctx, "main", d, binary)


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("d", [16, 30])
def test_calcgrad_slices_bit_equal(H, plan_ctx, d, binary):
    assert R.n_groups(SLICE[d]) == 8 * R.n_slices(d) + 1
    _calcgrad_case(H, plan_ctx, str(SLICE[d]), d, binary)


# ---------------------------------------------------------------- (b) the fused step
def _layout(d, bwd_cpl=8, bwd_cpl_from=64, bwd_two_pass=1, slot_layout="auto", **_):
    """-> (G, CPL, 'v' float4 | 's' scalar, passes, slot bytes (0: split)) of dfx_train_step's
    backward: lanes_for(d, true), bwd_two_pass, bwd_lanes and fat_es restated"""
    es = 0
    if slot_layout != "split" and d >= 4 and d % 4 == 0 and 32 + 4 * d <= 128:
        es = 64 if 32 + 4 * d <= 64 else 128
    if d <= 0:
        return 1, 1, "s", 1, es
    if d % 4:
        g = 1
        while g < min(d, 64):
            g <<= 1
        cpl = 1
        while cpl < (d + g - 1) // g:
            cpl <<= 1
        return g, cpl, "s", 1, es
    cpl = 4
    while d // cpl > 64:
        cpl *= 2
    g = 1
    while g < (d + cpl - 1) // cpl:
        g <<= 1
    if cpl == 4 and g >= 32 and bwd_two_pass:
        return g, 4, "v", 2, es
    if cpl == 4 and d >= bwd_cpl_from and d <= 512:
        c = bwd_cpl
        while c >= 8:
            if g * 4 // c >= 2 and d % c == 0:
                return g * 4 // c, c, "v", 1, es
            c //= 2
    return g, cpl, "v", 1, es


ONE = dict(bwd_two_pass=0)
FUSED = [
    # V_dim, context kwargs, (G, CPL, float4 | scalar, passes, fat slot bytes)
    (0, {}, (1, 1, "s", 1, 0)),
    (1, {}, (1, 1, "s", 1, 0)),
    (2, {}, (2, 1, "s", 1, 0)),
    (3, {}, (4, 1, "s", 1, 0)),
    (5, {}, (8, 1, "s", 1, 0)),
    (9, {}, (16, 1, "s", 1, 0)),
    (17, {}, (32, 1, "s", 1, 0)),
    (33, {}, (64, 1, "s", 1, 0)),
    (66, {}, (64, 2, "s", 1, 0)),
    (130, {}, (64, 4, "s", 1, 0)),
    (257, {}, (64, 8, "s", 1, 0)),
    (513, {}, (64, 16, "s", 1, 0)),
    (4, {}, (1, 4, "v", 1, 64)),
    (8, {}, (2, 4, "v", 1, 64)),
    (16, {}, (4, 4, "v", 1, 128)),
    (24, {}, (8, 4, "v", 1, 128)),
    (4, dict(slot_layout="split"), (1, 4, "v", 1, 0)),
    (8, dict(slot_layout="split"), (2, 4, "v", 1, 0)),
    (16, dict(slot_layout="split"), (4, 4, "v", 1, 0)),
    (28, {}, (8, 4, "v", 1, 0)),
    (36, {}, (16, 4, "v", 1, 0)),
    (16, dict(bwd_cpl_from=16), (2, 8, "v", 1, 128)),
    (32, dict(bwd_cpl_from=32), (4, 8, "v", 1, 0)),
    (64, {}, (8, 8, "v", 1, 0)),
    (64, dict(bwd_cpl=16), (4, 16, "v", 1, 0)),
    (72, {}, (32, 4, "v", 2, 0)),
    (72, ONE, (16, 8, "v", 1, 0)),
    (72, dict(ONE, bwd_cpl=4), (32, 4, "v", 1, 0)),
    (128, {}, (32, 4, "v", 2, 0)),
    (128, ONE, (16, 8, "v", 1, 0)),
    (128, dict(ONE, bwd_cpl=16), (8, 16, "v", 1, 0)),
    (256, {}, (64, 4, "v", 2, 0)),
    (256, ONE, (32, 8, "v", 1, 0)),
    (256, dict(ONE, bwd_cpl=16), (16, 16, "v", 1, 0)),
    (256, dict(ONE, bwd_cpl=4), (64, 4, "v", 1, 0)),
]


def test_fused_table_covers_every_layout():
    """the table names what _layout derives, and holds every kernel launch_bwd<true> (fm.hip
    :1842-1848) and launch_bwd_fused (:1894-1897) instantiate that a V_dim can reach"""
    for d, kw, want in FUSED:
        assert _layout(d, **kw) == want, (d, kw)
    have = {w[:4] for _, _, w in FUSED}
    scalar = {(g, 1, "s", 1) for g in (1, 2, 4, 8, 16, 32, 64)} | \
        {(64, c, "s", 1) for c in (2, 4, 8, 16)}
    vec = {(g, 4, "v", 1) for g in (1, 2, 4, 8, 16, 32, 64)} | \
        {(g, 8, "v", 1) for g in (2, 4, 8, 16, 32)} | {(g, 16, "v", 1) for g in (4, 8, 16)}
    two = {(32, 4, "v", 2), (64, 4, "v", 2)}
    assert have == scalar | vec | two
    assert {(w[0], w[4]) for _, _, w in FUSED if w[4]} == {(1, 64), (2, 64), (4, 128), (8, 128),
                                                          (2, 128)}


def _entry_eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    (sa, Va), (sb, Vb) = a, b
    if not np.array_equal(_bits(sa), _bits(sb)) or (Va is None) != (Vb is None):
        return False
    return Va is None or np.array_equal(_bits(Va), _bits(Vb))


def _fused_case(H, plan_ctx, kind, binary, cfg, kw, steps=3, flip=False):
    """a fresh context against an oracle Updater driven by backward_ref.fused_step; step 0 pushes
    the counts, the later steps run with non-zero w, V and Vaux.  flip: odd steps train on the
    negated labels, which takes w back through zero.  -> over the steps a later backward reads,
    the chunked keys met (without V, with a V that Get hides because w == 0)"""
    from difacto_amd import data as D
    blk, uniq, cnt, col, chunked, _ = _batch(kind, binary)
    _assert_chunk_plan(H, plan_ctx, kind, binary)
    neg = D.RowBlock(blk.offs, blk.ids, blk.vals, -blk.labels, blk.weights)
    c = H.Context(0, max_keys=1 << 15, **cfg, **kw)
    st = H.Store(c)
    up, seq = O.Updater(**cfg), O.Updater(**cfg)
    dkeys = c.tensor(uniq, torch.int64)
    rng = np.random.default_rng(5)
    sample = np.concatenate([uniq[chunked], rng.choice(uniq[~chunked], 48, replace=False)])
    dbs = [H.DeviceRowBlock(c, blk), H.DeviceRowBlock(c, neg)]
    hidden = novee = 0
    for step in range(steps):
        b = step % 2 if flip else 0
        want = R.fused_step(up, (blk, neg)[b], push_cnt=(step == 0))
        pred = torch.zeros(blk.size, dtype=torch.float32, device=c.device)
        H.train_step(c, dbs[b], H.kTraining, push_cnt=(step == 0), pred=pred)
        H.progress(c)
        assert np.array_equal(_bits(pred.cpu().numpy()), _bits(want)), step
        v, l = st.pull(dkeys)
        ov, ol = up.get(uniq)
        if cfg["V_dim"] > 0:
            assert np.array_equal(l.cpu().numpy(), ol), step
        v = v.cpu().numpy()
        bad = np.nonzero(_bits(v) != _bits(ov))[0] if len(v) == len(ov) else [-1]
        assert len(bad) == 0, (step, len(bad), bad[:8])
        for k in sample:
            assert _entry_eq(st.entry(k), up.entry(k)), (step, int(k))
        s = st.stats()
        assert (s["seed"], s["new_w"], s["n_keys"]) == (up.seed, int(up.new_w), up.size()), step
        if step == 0:
            # (c) the chunked keys' sums are not the reference's sequential float sums
            seq.train_step(blk.offs, blk.ids, blk.vals, blk.labels, blk.weights, push_cnt=True)
            assert any(not _entry_eq(seq.entry(k), up.entry(k)) for k in uniq[chunked])
            assert all(_entry_eq(seq.entry(k), up.entry(k)) for k in sample[-48:])
        if cfg["V_dim"] > 0 and step < steps - 1:   # what the next step's backward will read
            ent = [up.entry(k) for k in uniq[chunked]]
            ln = ol[chunked]
            novee += sum(e[1] is None for e in ent)
            hidden += sum(e[1] is not None and n == 1 for e, n in zip(ent, ln))
    c.close()
    return novee, hidden


@pytest.mark.parametrize("i", range(len(FUSED)), ids=lambda i: "d%d-%s" % (
    FUSED[i][0], "-".join("%s%s" % kv for kv in sorted(FUSED[i][1].items())) or "default"))
def test_fused_step_bit_equal(H, plan_ctx, i):
    d, kw, want = FUSED[i]
    assert _layout(d, **kw) == want
    cfg = dict(V_dim=d, V_threshold=0, l1=0, lr=.05, V_lr=.01)
    # binary and valued alternate down the table; the widest rows take the planted keys alone
    _fused_case(H, plan_ctx, "small" if d > 256 else "main", i % 2 == 0, cfg, kw)


# chosen on the CPU (the reference alone): at 30 every lazy case below meets both kinds of key
LAZY_L1 = 30.0


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("d,kw", [(16, {}), (128, {})])
def test_fused_lazy_v_bit_equal(H, plan_ctx, d, kw, binary):
    """l1 > 0, V_threshold >= 1, l1_shrk on: chunked keys without V (vq < 0: only the g_w / XXp
    partials are read) and with a V hidden because w returned to zero (the labels flip every
    step), both met by a backward (counted on the reference's state, so by construction)"""
    cfg = dict(V_dim=d, V_threshold=300, l1=LAZY_L1, l1_shrk=1, lr=.05, V_lr=.01)
    novee, hidden = _fused_case(H, plan_ctx, "main", binary, cfg, kw, steps=5, flip=True)
    assert novee > 0 and hidden > 0, (novee, hidden)


@pytest.mark.parametrize("d,binary", [(16, False), (128, True)])
def test_fused_slices_bit_equal(H, plan_ctx, d, binary):
    """the key of 8 R + 1 groups at d = 16 (R = 3) and 769 chunks in plain group order at
    d = 128 (R = 1), through the fused step"""
    cfg = dict(V_dim=d, V_threshold=0, l1=0, lr=.05, V_lr=.01)
    _fused_case(H, plan_ctx, str(SLICE[d]), binary, cfg, {})
