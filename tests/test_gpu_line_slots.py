"""slot_layout=line: a key's entry, V and Vaux in one 128-byte line (V_dim 4, 8, 12), no V pool.

Every comparison is on bit patterns.  The yardsticks are the project's exact ones: the oracle
where no key passes 128 occurrences, tests/backward_ref.fused_step where one does (the chunked
keys' sums are combined from partials in the documented order).
"""
import functools

import numpy as np
import pytest
import torch

from difacto_amd import _lib
from difacto_amd import data as D
from oracle import oracle as O
from tests import backward_ref as R

pytestmark = pytest.mark.gpu

# 1 occurrence, the chunk gate (kChunkOcc = 128) and kHotChunks (8 chunks), each from both sides
PLANTED = (1, 128, 129, 896, 897)
DFX_ERR_ARG = 1


@pytest.fixture(scope="module")
def H():
    from difacto_amd import hotpath
    return hotpath


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _batch(binary):
    """1024 rows x 8 nnz over ~390 ids, ids repeated inside rows, every seventh row weight 0"""
    blk = R.planted_batch(1024, 8, PLANTED, binary, seed=11)
    uniq, cnt, _ = O.localize(blk.offs, blk.ids)
    at = np.searchsorted(uniq, [R.planted_key(i) for i in range(len(PLANTED))])
    assert cnt[at].tolist() == list(PLANTED)
    neg = D.RowBlock(blk.offs, blk.ids, blk.vals, -blk.labels, blk.weights)
    return blk, neg, uniq, sum(R.n_chunks(int(c)) for c in cnt)


def _entry_eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    (sa, Va), (sb, Vb) = a, b
    if not np.array_equal(_bits(sa), _bits(sb)) or (Va is None) != (Vb is None):
        return False
    return Va is None or np.array_equal(_bits(Va), _bits(Vb))


def _record(e):
    """an entry as a model file holds it: without fea_cnt (SGDEntry::SaveEntry)"""
    return (np.append(e[0][:3], np.float32(0)), e[1])


def _assert_store(c, st, up, uniq, tag):
    """Store.pull, every Store.entry (V and Vaux with it), the rand_r seed and new_w"""
    v, l = st.pull(c.tensor(uniq, torch.int64))
    ov, ol = up.get(uniq)
    assert np.array_equal(l.cpu().numpy(), ol), tag
    assert np.array_equal(_bits(v.cpu().numpy()), _bits(ov)), tag
    bad = [int(k) for k in uniq if not _entry_eq(st.entry(k), up.entry(k))]
    assert not bad, (tag, len(bad), bad[:4])
    s = st.stats()
    assert (s["seed"], s["new_w"], s["n_keys"]) == (up.seed, int(up.new_w), up.size()), tag


def _steps(H, c, up, binary, steps, flip=False, first=0):
    blk, neg, uniq, _ = _batch(binary)
    st = H.Store(c)
    dbs = [H.DeviceRowBlock(c, blk), H.DeviceRowBlock(c, neg)]
    for step in range(first, first + steps):
        b = step % 2 if flip else 0
        want = R.fused_step(up, (blk, neg)[b], push_cnt=(step == 0))
        pred = torch.zeros(blk.size, dtype=torch.float32, device=c.device)
        H.train_step(c, dbs[b], H.kTraining, push_cnt=(step == 0), pred=pred)
        H.progress(c)
        assert np.array_equal(_bits(pred.cpu().numpy()), _bits(want)), step
        _assert_store(c, st, up, uniq, step)


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "valued"])
@pytest.mark.parametrize("d", [4, 8, 12])
def test_fused_step_bit_equal(H, d, binary):
    """a count-push step and two training steps: one key, the chunk gate and the hot-key
    pre-sums from both sides, on 1 / 2 / 4 lanes per key"""
    blk, _, _, nch = _batch(binary)
    cfg = dict(V_dim=d, V_threshold=0, l1=0, lr=.05, V_lr=.01)
    c = H.Context(0, max_keys=1 << 12, slot_layout="line", **cfg)
    assert nch == 2 + 7 + 8
    assert H.localize_occ(c, blk.offs, blk.ids, blk.vals)["n_chunks"] == nch
    _steps(H, c, O.Updater(**cfg), binary, 3)
    c.close()


# chosen on the reference alone: with these the batch's keys split into keys that never get V
# (fea_cnt <= V_threshold) and keys whose V Get hides when the flipped labels take w back to 0
LAZY = dict(V_dim=8, V_threshold=10, l1=2.0, l1_shrk=1, lr=.05, V_lr=.01)


def test_lazy_v_bit_equal(H):
    blk, neg, uniq, _ = _batch(True)
    c = H.Context(0, max_keys=1 << 12, slot_layout="line", **LAZY)
    up = O.Updater(**LAZY)
    novee = hidden = 0
    for step in range(3):
        _steps(H, c, up, True, 1, flip=True, first=step)
        ent = [up.entry(k) for k in uniq]
        _, ol = up.get(uniq)
        novee += sum(e[1] is None for e in ent)
        hidden += sum(e[1] is not None and n == 1 for e, n in zip(ent, ol))
    assert novee > 0 and hidden > 0, (novee, hidden)
    c.close()


def test_rebuilds_move_vaux(H):
    """growth past load 0.5 at a sync point, then table_unclump on clustered keys (the recipe of
    test_fused_clustered_keys_rehash): after each, every entry with its V and Vaux is the
    oracle's"""
    cfg = dict(V_dim=12, V_threshold=0, l1=0, lr=.1, V_lr=.01)
    c = H.Context(0, max_keys=64, slot_layout="line", **cfg)
    up, st = O.Updater(**cfg), H.Store(c)
    cap0 = st.probe_stats()[2]
    rng = np.random.default_rng(5)
    seen = np.zeros(0, np.uint64)
    for step in range(5):
        B, k = 400, 8
        ids = rng.integers(0, 1500, B * k).astype(np.uint64)
        if step >= 2:
            ids = ids << np.uint64(40)      # keys that share their top bits: one home slot
        blk = D.RowBlock(np.arange(0, B * k + 1, k, dtype=np.uint64), ids, None,
                         np.where(rng.random(B) < .3, 1, -1).astype(np.float32))
        up.train_step(blk.offs, blk.ids, blk.vals, blk.labels, push_cnt=(step == 0))
        H.train_step(c, H.DeviceRowBlock(c, blk), H.kTraining, push_cnt=(step == 0))
        H.progress(c)   # a sync point: the table grows / rehashes here
        seen = np.union1d(seen, O.localize(blk.offs, blk.ids)[0])
        _assert_store(c, st, up, seen, step)
        _, mx, cap = st.probe_stats()
        if step == 1:
            assert cap > cap0 and 2 * st.stats()["n_keys"] <= cap     # it grew
        if step >= 2:
            assert mx < 64 < len(seen)      # unclumped: no chain as long as the clustered keys
    assert st.bytes()[1] == 0
    c.close()


@pytest.mark.parametrize("d", [4, 12])
def test_model_files_cross_layouts(H, d, tmp_path):
    cfg = dict(V_dim=d, V_threshold=0, l1=0, lr=.05, V_lr=.01)
    blk, _, uniq, _ = _batch(False)
    ups, files, dumps = {}, {}, {}
    for lay in ("line", "split"):
        c = H.Context(0, max_keys=1 << 12, slot_layout=lay, **cfg)
        ups[lay] = O.Updater(**cfg)
        _steps(H, c, ups[lay], False, 3)
        for dev in (False, True):
            p, q = tmp_path / ("m_%s_%d" % (lay, dev)), tmp_path / ("t_%s_%d" % (lay, dev))
            H.Store(c).save(str(p), save_aux=True, device=dev)
            H.Store(c).dump(str(q), dump_aux=True, need_reverse=True, device=dev)
            files[lay, dev], dumps[lay, dev] = p.read_bytes(), sorted(q.read_text().splitlines())
        c.close()
    # the host writers walk slots in order and the slots are the same (same keys, capacity, hash)
    assert len({files[k] for k in files}) == 1 and len(files["line", False]) > 1
    assert all(dumps[k] == dumps["line", False] for k in dumps) and dumps["line", False]
    for dev in (False, True):
        c = H.Context(0, max_keys=1 << 12, slot_layout="line", **cfg)
        H.Store(c).load(str(tmp_path / "m_split_0"), device=dev)
        up, st = ups[("line", "split")[dev]], H.Store(c)    # (each after the same three steps)
        bad = [int(k) for k in uniq if not _entry_eq(_record(st.entry(k)), _record(up.entry(k)))]
        assert not bad, (dev, len(bad))
        # one more step (Load leaves the seed and sets new_w = model_.size(): not compared)
        want = R.fused_step(up, blk, push_cnt=False)
        pred = torch.zeros(blk.size, dtype=torch.float32, device=c.device)
        H.train_step(c, H.DeviceRowBlock(c, blk), H.kTraining, pred=pred)
        H.progress(c)
        assert np.array_equal(_bits(pred.cpu().numpy()), _bits(want)), dev
        bad = [int(k) for k in uniq if not _entry_eq(_record(st.entry(k)), _record(up.entry(k)))]
        assert not bad, (dev, len(bad))
        c.close()


@pytest.mark.parametrize("d", [0, 5, 16, 24])
def test_line_needs_4_8_12(H, d):
    with pytest.raises(_lib.DfxError, match="4, 8 or 12"):
        H.Context(0, slot_layout="line", V_dim=d)


def test_line_is_single_context_and_has_no_pool(H):
    line = H.Context(0, max_keys=1 << 10, slot_layout="line", V_dim=8)
    fat = H.Context(0, max_keys=1 << 10, V_dim=8)
    lib = _lib.lib()
    assert lib.dfx_split_owner_forward(line.h, 0, None) == DFX_ERR_ARG
    assert lib.dfx_dist_owner_pull(line.h, 0, None) == DFX_ERR_ARG
    assert b"slot_layout=line" in lib.dfx_last_error()
    (tl, pl), (tf, pf) = H.Store(line).bytes(), H.Store(fat).bytes()
    assert pl == 0 and tl == (1 << 11) * 128        # 2 * max_keys slots of one line each
    assert tf == (1 << 11) * 64 and pf == (1 << 11) * 8 * 4
    line.close()
    fat.close()
