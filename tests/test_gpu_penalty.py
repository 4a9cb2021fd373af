"""Store.evaluate (csrc/store.hip k_penalty: SGDUpdater::Evaluate's penalty and nnz_w) on every slot
layout with l2 > 0, against tests/penalty_ref.penalty: nnz exactly, the penalty within the bound
that file derives from the double sum's own rounding.  tests/test_penalty_ref.py shows on the CPU
that the yardstick is Evaluate and that the planted model tells a wrong V term from the right one
(Vaux for V, V_l2 for l2, no V term, a hidden V skipped: each more than 100 bounds away).
"""
import numpy as np
import pytest

from difacto_amd import data as D
from oracle import oracle as O
from tests import backward_ref as R
from tests import edge_ref as E
from tests import half_ref as HR
from tests import line16_ref as L16
from tests import penalty_ref as PR
from tests.test_gpu_line_slots import LAZY, H, _assert_store, _batch, _bits, _steps  # noqa: F401

pytestmark = pytest.mark.gpu

LAYOUT_IDS = range(len(PR.LAYOUTS))
# the layouts the trained and the rebuilt models run on: (name, V_dim, context kwargs, updater)
TRAINED = [("split", 8, dict(slot_layout="split"), O.Updater), ("fat", 8, {}, O.Updater),
           ("line", 8, dict(slot_layout="line"), O.Updater), ("line16", 16, PR.LINE16, L16.Updater)]
REBUILT = [("split", 5, {}, O.Updater)] + TRAINED[1:]
HALF_TRAINED = [("half%d" % d, d, kw, HR.Updater) for d, kw, _ in PR.HALF_LAYOUTS]


def _check(st, entries, l1, l2, d, tag):
    S, nnz, bound, kinds = PR.penalty(entries, l1, l2, d)
    pen, got = st.evaluate()
    print("%s: penalty %.17g yardstick %.17g bound %.3g nnz %d" % (tag, pen, S, bound, got))
    assert got == nnz, (tag, got, nnz)
    assert abs(pen - S) <= bound, (tag, pen, S, bound)
    return kinds


def _assert_layout(st, d, want):
    """the slot stride and the pool the device allocated are the table row's (es, line)"""
    (tb, pb), cap = st.bytes(), st.capacity()
    assert tb == cap * (32 << want[0]) and (pb == 0) == (d == 0 or want[1] > 0), (tb, pb, cap)


def test_layouts_cover_every_es_and_line():
    """(tests/test_penalty_ref.py holds the same table to es_line over every V_dim)"""
    assert all(PR.es_line(d, **kw) == want for d, kw, want in PR.LAYOUTS)
    assert {w for _, _, w in PR.LAYOUTS} == PR.EVERY_ES_LINE
    assert all(PR.es_line(d, **kw) in PR.EVERY_ES_LINE for _, d, kw, _ in TRAINED + REBUILT)


# ---------------------------------------------------------------- a. planted models
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("i", LAYOUT_IDS, ids=PR.layout_id)
def test_planted_model(H, tmp_path, i, dev):
    """a model file of known w, V and Vaux through either loader: every class of entry, with
    |w| > 2^64 and V ~ 2^60 (huge) and at sums of order 100 (plain)"""
    d, kw, want = PR.LAYOUTS[i]
    for huge in (True, False):
        planted = PR.plant(d, huge)
        path = str(tmp_path / ("m%d" % huge))
        E.write_model(path, d, planted)
        c = H.Context(0, max_keys=1 << 10, V_dim=d, l1=PR.L1, l2=PR.L2, V_l2=PR.V_L2, **kw)
        st = H.Store(c)
        _assert_layout(st, d, want)
        assert st.evaluate() == (0.0, 0)
        st.load(path, device=dev)
        assert st.stats()["n_keys"] == len(planted)
        kinds = _check(st, PR.model_entries(planted), PR.L1, PR.L2, d,
                       "%s %s huge=%d" % (PR.layout_id(i), ("host", "device")[dev], huge))
        for name in PR.KINDS:
            possible = (d > 0 or name not in ("w_v", "zero_v")) and (huge or name != "huge")
            assert (kinds[name] > 0) == possible, (name, kinds)
        # the store holds what was planted: V bit for bit (fp16 Vaux narrows, V beside it does not)
        narrowed = 0
        for key, w, sg, z, V, C in planted[::5]:
            got = st.entry(key)
            assert np.array_equal(_bits(got[0][:3]), _bits([w, sg, z])), key
            assert (got[1] is None) == (V is None), key
            if V is not None:
                keep = L16.nearest_f16(C) if want[1] == 2 else C
                narrowed += int((keep != C).any())
                assert np.array_equal(_bits(got[1]), _bits(np.concatenate([V, keep]))), key
        assert (narrowed > 0) == (want[1] == 2)
        c.close()


@pytest.mark.parametrize("d,kw,want", PR.HALF_LAYOUTS, ids=["half32", "half64"])
def test_planted_model_half(H, tmp_path, d, kw, want):
    """the plain planted model narrowed to fp16 in a vrows=f16 table (k_penalty reads the V half of
    a pool row through v_get): the load is exact, V and Vaux bit for bit (the host loader: the
    device loader refuses a half table)"""
    planted = PR.plant(d, False, narrow=HR.nearest_f16)
    path = str(tmp_path / "m")
    E.write_model(path, d, planted)
    c = H.Context(0, max_keys=1 << 10, V_dim=d, l1=PR.L1, l2=PR.L2, V_l2=PR.V_L2, **kw)
    st = H.Store(c)
    _assert_layout(st, d, want)
    assert st.evaluate() == (0.0, 0)
    st.load(path)
    assert st.stats()["n_keys"] == len(planted)
    kinds = _check(st, PR.model_entries(planted), PR.L1, PR.L2, d, "half V_dim %d" % d)
    for name in PR.KINDS:
        assert (kinds[name] > 0) == (name != "huge"), (name, kinds)
    for key, w, sg, z, V, C in planted[::5]:
        got = st.entry(key)
        assert np.array_equal(_bits(got[0][:3]), _bits([w, sg, z])), key
        assert (got[1] is None) == (V is None), key
        if V is not None:
            assert np.array_equal(_bits(got[1]), _bits(np.concatenate([V, C]))), key
    c.close()


# ---------------------------------------------------------------- b. trained models
@pytest.mark.parametrize("name,d,kw,updater", TRAINED + HALF_TRAINED,
                         ids=[t[0] for t in TRAINED + HALF_TRAINED])
def test_trained_model(H, name, d, kw, updater):
    """a count push and two training steps, the labels flipped in between (test_lazy_v_bit_equal's
    recipe with l2 > 0): the store is the updater's bit for bit, then its penalty the yardstick's
    on the updater's entries — with a V that Get hides and a key without V among them"""
    cfg = dict(PR.LAZY_CFG, V_dim=d)
    assert dict(LAZY, l2=PR.L2, V_dim=d) == cfg
    uniq = _batch(True)[2]
    assert np.array_equal(uniq, PR.lazy_batches()[2])
    c = H.Context(0, max_keys=1 << 12, **kw, **cfg)
    up, st = updater(**cfg), H.Store(c)
    for step in range(3):
        _steps(H, c, up, True, 1, flip=True, first=step)
        kinds = _check(st, PR.entries_of(up, uniq), cfg["l1"], cfg["l2"], d,
                       "trained %s step %d" % (name, step))
    hidden, bare = PR.hidden_and_bare(up, uniq)
    assert hidden > 0 and bare > 0 and kinds["zero_v"] >= hidden and kinds["w_v"] > 0, kinds
    c.close()


# ---------------------------------------------------------------- c. rebuilds
@pytest.mark.parametrize("name,d,kw,updater", REBUILT, ids=[t[0] for t in REBUILT])
def test_rebuilt_tables(H, name, d, kw, updater):
    """test_rebuilds_move_vaux's recipe from max_keys=64 (128 slots: the first launch is one block
    with idle lanes): growth past load 0.5, then table_unclump on clustered keys, the penalty
    after every step.  In the split layout a rebuild leaves the pool rows where they were: slot
    order and row order part ways."""
    cfg = dict(V_dim=d, V_threshold=0, l1=.1, l2=PR.L2, lr=.1, V_lr=.01)
    c = H.Context(0, max_keys=64, **kw, **cfg)
    up, st = updater(**cfg), H.Store(c)
    cap0 = st.capacity()
    assert cap0 < 256 and st.evaluate() == (0.0, 0)
    rng = np.random.default_rng(5)
    seen = np.zeros(0, np.uint64)
    for step in range(5):
        B, k = 400, 8
        ids = rng.integers(0, 1500, B * k).astype(np.uint64)
        if step >= 2:
            ids = ids << np.uint64(40)      # keys that share their top bits: one home slot
        blk = D.RowBlock(np.arange(0, B * k + 1, k, dtype=np.uint64), ids, None,
                         np.where(rng.random(B) < .3, 1, -1).astype(np.float32))
        R.fused_step(up, blk, step == 0)
        H.train_step(c, H.DeviceRowBlock(c, blk), H.kTraining, push_cnt=(step == 0))
        H.progress(c)   # a sync point: the table grows / rehashes here
        seen = np.union1d(seen, O.localize(blk.offs, blk.ids)[0])
        _assert_store(c, st, up, seen, step)
        kinds = _check(st, PR.entries_of(up, seen), cfg["l1"], cfg["l2"], d,
                       "rebuilt %s step %d" % (name, step))
        _, mx, cap = st.probe_stats()
        assert step != 1 or (cap > cap0 and 2 * st.stats()["n_keys"] <= cap)    # it grew
        assert step < 2 or mx < 64 < len(seen)      # unclumped
    assert kinds["w_v"] > 0 and kinds["zero_nov"] > 0, kinds
    c.close()


# ---------------------------------------------------------------- d. empty stores
@pytest.mark.parametrize("i", LAYOUT_IDS, ids=PR.layout_id)
def test_empty_store(H, i):
    d, kw, want = PR.LAYOUTS[i]
    for max_keys in (64, 1 << 10):      # less than one block of slots, and several
        c = H.Context(0, max_keys=max_keys, V_dim=d, l1=PR.L1, l2=PR.L2, **kw)
        st = H.Store(c)
        _assert_layout(st, d, want)
        assert st.evaluate() == (0.0, 0) and st.capacity() == 2 * max_keys
        c.close()


# ---------------------------------------------------------------- e. key-range shards
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("d", [5, 16])
def test_shards(H, tmp_path, d, dev):
    """two key-range servers (tables hashed by the key's position in its range) load their halves
    of one planted file: each half against the yardstick on its own entries"""
    from difacto_amd import dist as DI
    for huge in (True, False):
        planted = PR.plant(d, huge)
        prefix = str(tmp_path / ("m%d" % huge))
        E.write_model(DI.model_name(prefix, 0), d, planted)
        owner = DI.owner_of(np.array([k for k, *_ in planted], np.uint64), 2)
        total = 0
        for g in range(2):
            c = H.Context(0, max_keys=1 << 10, push_agg="sum", V_dim=d, l1=PR.L1, l2=PR.L2,
                          V_l2=PR.V_L2)
            DI.Shard(c, 2).load(prefix, g, saved_ranks=1, device=dev)
            own = [p for p, o in zip(planted, owner) if o == g]
            assert 0 < len(own) < len(planted) and H.Store(c).stats()["n_keys"] == len(own)
            _check(H.Store(c), PR.model_entries(own), PR.L1, PR.L2, d,
                   "shard %d of 2 V_dim %d huge=%d" % (g, d, huge))
            total += H.Store(c).evaluate()[1]
            c.close()
        assert total == PR.penalty(PR.model_entries(planted), PR.L1, PR.L2, d)[1]
