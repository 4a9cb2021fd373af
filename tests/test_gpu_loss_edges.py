"""The clip pred = clamp(pred, -20, 20) (fm_loss.h:118) at each of its five device copies, CalcGrad's
p = -y / (1 + expf(y pred)) [* rw] at every edge of csrc/expf.h's expf on the device, and
ftrl_update's inclusive band z <= l1 && z >= -l1: the inputs of tests/edge_ref.py (shown on the
CPU by tests/test_edge_ref.py to hit what they claim) against the oracle.

Comparison rule, everywhere: np.array_equal on uint32 views.  Where the reference value is NaN the
device value must be NaN (payload and sign are not compared: the host and the device produce
different default NaNs), and every test asserts that the number of elements compared that way is
the count the builder planted, so the rule cannot absorb a wrong finite value.  The only bound is
tests/metric_exact.logloss_sum's own, on the logloss.

Which test pins which clip site (DESIGN.md lists them): k_fm_fwd's (test_clip_predict: kPredict;
test_clip_fused: kFusedProbe at V_dim 5 and 200; test_clip_sharded: kFused over pulled
records), fwd_row_out's (test_clip_fused: the fat walk and every probe), and the three
combines' (test_clip_split).  dfx_train_step always hands the forward the raw feature ids
(FwdArgs::index), so the non-probe kFused form is reached through the sharded store's
launch_fwd_records alone."""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import edge_ref as E
from tests import metric_exact as M
from tests.test_gpu_backward_paths import _entry_eq
from tests.test_gpu_dist_exact import _worker_lanes
from tests.test_gpu_split_exact import _layout

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from difacto_amd import hotpath
    return hotpath


@pytest.fixture(scope="module")
def DI():
    from difacto_amd import dist
    return dist


def _assert_bits(got, want, planted_nan, tag):
    """bit equality, NaN for NaN; the NaN count is the planted one"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan = np.isnan(want)
    assert int(nan.sum()) == planted_nan, (tag, int(nan.sum()), planted_nan)
    assert np.isnan(got[nan]).all(), (tag, "finite where the reference is NaN")
    g, w = E.bits(got)[~nan], E.bits(want)[~nan]
    bad = np.flatnonzero(g != w)
    assert len(bad) == 0, (tag, "%d differ" % len(bad), "first at %d of the non-NaN" % bad[0],
                           "got %#010x want %#010x" % (g[bad[0]], w[bad[0]]))


# ---------------------------------------------------------------- p at expf's edges
@pytest.fixture(scope="module")
def sweep():
    """the sweep and the oracle's two gradients, computed once and left unchanged"""
    blk, pred, labels, rw = E.p_sweep()
    B = blk.size
    col = np.arange(B, dtype=np.uint32)
    W = np.zeros(B, np.float32)
    wp = np.arange(B, dtype=np.int32)
    vp = np.full(B, -1, np.int32)
    want0 = O.fm_calcgrad(blk.offs, col, None, labels, None, W, None, None, B, 0, pred)
    want5 = O.fm_calcgrad(blk.offs, col, blk.vals, labels, rw, W, wp, vp, B, 5, pred)
    for a in (pred, want0, want5):
        a.setflags(write=False)
    return blk, pred, col, W, wp, vp, want0, want5


def test_p_sweep(H, sweep):
    """logit_p on the device against the host's glibc, on every edge of expf: binary and
    unweighted at V_dim 0 the gradient of row i's private key is p itself; valued, with row
    weights, at V_dim 5 with every key lacking V it is ((-y / den) * rw) * x"""
    blk, pred, col, W, wp, vp, want0, want5 = sweep
    B = blk.size
    n_nan = int(np.isnan(pred).sum())
    assert n_nan == sum(int((E.bits(pred) == b).sum()) for b in E.NAN_BITS) > 0
    c = H.Context(0)
    tcol = c.tensor(col, torch.int32)
    tW = c.tensor(W, torch.float32)
    tpred = c.tensor(pred, torch.float32)
    assert np.array_equal(E.bits(tpred.cpu().numpy()), E.bits(pred))    # NaN payloads survive
    db = H.DeviceRowBlock(c, blk)
    vals, weights = db.vals, db.weights
    db.vals = db.weights = None
    grad = torch.zeros(B, dtype=torch.float32, device=c.device)
    H.FMLoss(c, 0).calc_grad(db, tcol, tW, None, None, tpred, grad, B)
    c.sync()
    _assert_bits(grad.cpu().numpy(), want0, n_nan, "binary, V_dim 0")
    db.vals, db.weights = vals, weights
    grad = torch.zeros(B, dtype=torch.float32, device=c.device)
    H.FMLoss(c, 5).calc_grad(db, tcol, tW, c.tensor(wp, torch.int32), c.tensor(vp, torch.int32),
                             tpred, grad, B)
    c.sync()
    _assert_bits(grad.cpu().numpy(), want5, n_nan, "valued, weighted, V_dim 5")
    c.close()


# ---------------------------------------------------------------- the clip: Predict / CalcGrad
_oracles = {}


def _oracle(tmp_path_factory, d, binary):
    """(blk, entries, targets, model file, opred) of one clip case, made once"""
    if (d, binary) not in _oracles:
        blk, entries, tg = E.clip_case(d, binary)
        path = str(tmp_path_factory.mktemp("clip") / ("model_%d_%d" % (d, binary)))
        E.write_model(path, d, entries)
        up = _updater(d, path)
        _, _, opred = up.train_step(blk.offs, blk.ids, blk.vals, blk.labels, train=False,
                                    want_pred=True)
        for a in (blk.offs, blk.ids, blk.labels, opred) + (() if binary else (blk.vals,)):
            a.setflags(write=False)
        _oracles[(d, binary)] = (blk, entries, tg, path, opred)
    return _oracles[(d, binary)]


def _updater(d, path):
    up = O.Updater(V_dim=d, **E.CLIP_CFG)
    up.load(path)
    return up


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "valued"])
@pytest.mark.parametrize("d", E.CLIP_DIMS)
def test_clip_predict(H, tmp_path_factory, d, binary):
    """FMLoss.predict (k_fm_fwd<kPredict>) and calc_grad over the Pull layout of the planted model"""
    blk, entries, tg, path, opred = _oracle(tmp_path_factory, d, binary)
    up = _updater(d, path)
    uniq, _, ocol = O.localize(blk.offs, blk.ids)
    U = len(uniq)
    W, lens = up.get(uniq)
    wp, vp = O.get_pos(lens) if d > 0 else (None, None)
    want = O.fm_predict(blk.offs, ocol, blk.vals, W, wp, vp, d)
    n_nan = len(tg["rows"]["nan"])
    _assert_bits(want, opred, n_nan, "the oracle's step and its Predict")
    og = O.fm_calcgrad(blk.offs, ocol, blk.vals, blk.labels, None, W, wp, vp, U, d, opred)
    c = H.Context(0)
    db = H.DeviceRowBlock(c, blk)
    col, duniq, _ = H.Localizer(c).compact(db)
    assert np.array_equal(H.u64(duniq), uniq)
    tW = c.tensor(W, torch.float32)
    twp = c.tensor(wp, torch.int32)
    tvp = c.tensor(vp, torch.int32)
    pred = torch.zeros(blk.size, dtype=torch.float32, device=c.device)
    H.FMLoss(c, d).predict(db, col, tW, twp, tvp, pred, U)
    grad = torch.zeros(len(W), dtype=torch.float32, device=c.device)
    H.FMLoss(c, d).calc_grad(db, col, tW, twp, tvp, pred, grad, U)
    c.sync()
    _assert_bits(pred.cpu().numpy(), opred, n_nan, ("pred", d, binary))
    _assert_bits(grad.cpu().numpy(), og, tg["nan_grads"], ("grad", d, binary))
    c.close()


# ---------------------------------------------------------------- the clip: the fused step
def _p(g, c):
    return ("probe", g, c)


# V_dim, context kwargs, the forward kernel launch_fwd_fused takes (test_gpu_split_exact._layout;
# V_dim 0 is not in that table's rules: lr_lanes picks between the two)
FUSED = [
    (8, {}, ("walk", 2)),
    (16, {}, ("walk", 4)),
    (0, dict(lr_lanes=1), "lr probe<4, 4>"),
    (0, dict(lr_lanes=0), "k_fm_fwd<1, 1, kFusedProbe>"),
    (16, dict(slot_layout="split"), _p(4, 4)),
    (24, {}, _p(8, 4)),
    (64, dict(fwd_cpl=4), _p(16, 4)),
    (128, dict(fwd_cpl=4), _p(32, 4)),
    (64, {}, _p(8, 8)),
    (128, {}, _p(16, 8)),
    (5, {}, ("fwd", 8, 1, "s")),
    (200, {}, ("fwd", 64, 4, "v")),
]


def _fused_id(i):
    d, kw, _ = FUSED[i]
    return "d%d-%s" % (d, "-".join("%s%s" % kv for kv in sorted(kw.items())) or "default")


def test_fused_table_covers_every_forward():
    fwd = {w for d, _, w in FUSED if d > 0}
    assert fwd >= {("walk", 2), ("walk", 4)} | {_p(g, 4) for g in (4, 8, 16, 32)} | \
        {_p(8, 8), _p(16, 8)}
    assert {w[0] for w in fwd} == {"walk", "probe", "fwd"}
    assert {tuple(kw.items()) for d, kw, _ in FUSED if d == 0} == {(("lr_lanes", 1),),
                                                                   (("lr_lanes", 0),)}


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "valued"])
@pytest.mark.parametrize("i", range(len(FUSED)), ids=_fused_id)
def test_clip_fused(H, tmp_path_factory, i, binary):
    """dfx_train_step on the planted model: a validation step on the whole batch (pred), one on
    the rows whose logloss term is finite (pred, loss, AUC * n), then a training step on the rows
    outside the NaN group: every entry and new_w against O.Updater's"""
    d, kw, want_fwd = FUSED[i]
    if d > 0:
        assert _layout(d, **kw)[0] == want_fwd
    blk, entries, tg, path, opred = _oracle(tmp_path_factory, d, binary)
    n_nan = len(tg["rows"]["nan"])
    c = H.Context(0, max_keys=1 << 12, V_dim=d, **E.CLIP_CFG, **kw)
    H.Store(c).load(path)
    up = _updater(d, path)
    assert H.Store(c).stats()["n_keys"] == up.size() == len(entries)

    def step(b, job):
        db = H.DeviceRowBlock(c, b)
        pred = torch.zeros(b.size, dtype=torch.float32, device=c.device)
        H.train_step(c, db, job, pred=pred)
        c.sync()
        return pred.cpu().numpy(), H.progress(c)

    p, pr = step(blk, H.kValidation)
    assert pr["nrows"] == blk.size
    _assert_bits(p, opred, n_nan, ("pred", d, kw, binary))
    with np.errstate(invalid="ignore"):
        fin = np.flatnonzero(np.isfinite(M.logloss_terms(blk.labels, opred)))
    assert set(tg["rows"]["at"]) | set(tg["rows"]["above"]) | set(tg["rows"]["below"]) <= set(fin)
    assert not set(tg["rows"]["nan"]) & set(fin)
    fb = E.take_rows(blk, fin)
    p, pr = step(fb, H.kValidation)
    _assert_bits(p, opred[fin], 0, ("finite pred", d, kw, binary))
    S, tol = M.logloss_sum(fb.labels, p)
    print("V_dim %d %s %s: loss %.17g yardstick %.17g bound %.3g" % (d, kw, want_fwd, pr["loss"],
                                                                    S, tol))
    assert pr["nrows"] == fb.size and abs(pr["loss"] - S) <= tol, (pr["loss"], S, tol)
    assert pr["auc"] == M.auc_times_n(fb.labels, p)
    tb = E.take_rows(blk, tg["train"])
    up.train_step(tb.offs, tb.ids, tb.vals, tb.labels)
    p, pr = step(tb, H.kTraining)
    _assert_bits(p, opred[tg["train"]], 0, ("training pred", d, kw, binary))
    st = H.Store(c)
    bad = [k for k, *_ in entries if not _entry_eq(st.entry(k), up.entry(k))]
    assert not bad, ("%d of %d entries differ" % (len(bad), len(entries)), "first key %#x" % bad[0],
                     st.entry(bad[0]), up.entry(bad[0]))
    s = st.stats()
    assert s["new_w"] == up.new_w and s["n_keys"] == up.size() and s["seed"] == up.seed
    c.close()


# ---------------------------------------------------------------- the clip: the combines
# V_dim, owners, context kwargs, combine lanes per row (0: k_split_combine), the combine form
SPLIT = [
    (5, 2, {}, 0, "scalar, compact partials"),
    (5, 1, {}, 0, "scalar, one owner's two halves"),
    (16, 2, {}, 4, "float4, compact partials"),
    (16, 1, {}, 4, "float4, one owner's two halves"),
    (16, 2, dict(slot_layout="split"), 4, "float4, compact partials, split slots"),
    (200, 2, {}, 64, "float4, 64 lanes"),
    (0, 2, {}, 0, "scalar, V_dim 0: no clip"),
]


def _shards(H, DI, N, d, kw, entries, tmp_path):
    """N loopback shards holding the planted model, every owner its keys"""
    ctxs = [H.Context(0, max_keys=1 << 12, push_agg="sum", V_dim=d, **E.CLIP_CFG, **kw)
            for _ in range(N)]
    shards = [DI.Shard(c, N) for c in ctxs]
    own = DI.owner_of(np.array([e[0] for e in entries], np.uint64), N)
    assert set(own) == set(range(N))
    prefix = str(tmp_path / "planted")
    for r in range(N):
        E.write_model(DI.model_name(prefix, r), d, [e for e, o in zip(entries, own) if o == r])
        shards[r].load(prefix, r)
    assert sum(H.Store(c).stats()["n_keys"] for c in ctxs) == len(entries)
    return ctxs, shards


def _workers_case(H, DI, step, N, d, kw, binary, tmp_path_factory, tmp_path):
    """the clip batch dealt to N workers row by row through one validation step of `step`:
    every worker's predictions against the oracle's on the whole batch"""
    blk, entries, tg, path, opred = _oracle(tmp_path_factory, d, binary)
    ctxs, shards = _shards(H, DI, N, d, kw, entries, tmp_path)
    rows = [np.arange(r, blk.size, N) for r in range(N)]
    blocks = [E.take_rows(blk, rw) for rw in rows]
    if N > 1:       # rows whose keys lie on different owners: partial sums meet in the combine
        ko = DI.owner_of(E.reverse_bytes(blk.ids), N)
        o = blk.offs.astype(np.int64)
        mixed = [r for r in range(blk.size) if len(set(ko[o[r]:o[r + 1]])) > 1]
        assert mixed and (d == 0 or set(mixed) & set(tg["rows"]["above"]))
    dbs = [H.DeviceRowBlock(ctxs[r], blocks[r]) for r in range(N)]
    preds = [torch.zeros(b.size, dtype=torch.float32, device=ctxs[0].device) for b in blocks]
    step(shards, dbs, DI.LoopbackComm(N), H.kValidation, push_cnt=False, preds=preds)
    for c in ctxs:
        c.sync()
    nan = set(tg["rows"]["nan"])
    seen = 0
    for r in range(N):
        n_nan = len(nan & set(rows[r]))
        seen += n_nan
        _assert_bits(preds[r].cpu().numpy(), opred[rows[r]], n_nan, ("pred", d, N, kw, binary, r))
    assert seen == len(nan) > 0
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "valued"])
@pytest.mark.parametrize("i", range(len(SPLIT)), ids=lambda i: "d%d-N%d-%d" % (SPLIT[i][0],
                                                                               SPLIT[i][1], i))
def test_clip_split(H, DI, tmp_path_factory, tmp_path, i, binary):
    """the owner-computes split's three combine forms (k_split_combine's compact and two-halves
    branches, k_split_combine_vec).  The two-halves form is the one-owner layout of the partials
    (split_part_floats(d, 1)), so it runs at N = 1; the others at N = 2"""
    d, N, kw, cg, _ = SPLIT[i]
    assert _layout(d, **kw)[1] == cg
    _workers_case(H, DI, DI.split_step, N, d, kw, binary, tmp_path_factory, tmp_path)


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "valued"])
@pytest.mark.parametrize("d,lanes", [(5, (8, 1, False)), (16, (4, 4, True))])
def test_clip_sharded(H, DI, tmp_path_factory, tmp_path, d, lanes, binary):
    """the all-to-all sharded step at N = 2: k_fm_fwd<G, CPL, kFused> over the pulled records
    (launch_fwd_records), scalar and float4 lanes"""
    assert _worker_lanes(d) == lanes
    _workers_case(H, DI, DI.sharded_step, 2, d, {}, binary, tmp_path_factory, tmp_path)


# ---------------------------------------------------------------- FTRL's band
@pytest.mark.parametrize("l1_shrk", [0, 1])
@pytest.mark.parametrize("l1,lr,lr_beta", E.FTRL_CASES)
def test_ftrl_edges(H, tmp_path, l1, lr, lr_beta, l1_shrk):
    """Store.push(kFeaCount) then push(kGradient) on the planted entries against O.Updater: z
    exactly on +-l1 gives w = 0, the floats outside leave zero (and draw V past V_threshold)"""
    d, thr = E.FTRL_VDIM, E.FTRL_VTHR
    entries, counts, grads, names = E.ftrl_edges(l1, lr, lr_beta, thr)
    keys = np.array([e[0] for e in entries], np.uint64)
    path = str(tmp_path / "m")
    E.write_model(path, d, entries)
    cfg = dict(V_dim=d, V_threshold=thr, l1=l1, lr=lr, lr_beta=lr_beta, l1_shrk=l1_shrk, V_lr=.01,
               seed=3)
    c = H.Context(0, max_keys=1 << 10, **cfg)
    st = H.Store(c)
    st.load(path)
    up = O.Updater(**cfg)
    up.load(path)
    tk = c.tensor(keys, torch.int64)

    def same(tag):
        c.sync()
        v, l = st.pull(tk)
        ov, ol = up.get(keys)
        assert np.array_equal(l.cpu().numpy(), ol), tag
        _assert_bits(v.cpu().numpy(), ov, 0, (tag, "pulled"))
        bad = [n for n, k in zip(names, keys) if not _entry_eq(st.entry(k), up.entry(k))]
        assert not bad, (tag, bad, [(st.entry(k), up.entry(k)) for n, k in zip(names, keys)
                                    if n == bad[0]])
        s = st.stats()
        assert s["new_w"] == up.new_w and s["seed"] == up.seed and s["n_keys"] == up.size(), tag
        return ol

    same("loaded")
    st.push(tk, H.kFeaCount, c.tensor(counts, torch.float32))
    up.update(keys, O.Updater.kFeaCount, counts)
    lens = same("counts")
    g = []
    for gw, n in zip(grads, lens):
        g += [gw] + [np.float32(0.25)] * (n - 1)
    g = np.array(g, np.float32)
    seed0 = up.seed
    st.push(tk, H.kGradient, c.tensor(g, torch.float32), c.tensor(lens, torch.int32))
    up.update(keys, O.Updater.kGradient, g, lens)
    same("gradient")
    assert up.seed != seed0
    c.close()
