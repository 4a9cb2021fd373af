"""InitV (sgd_updater.cc:144-152) through every path that draws it (csrc/initv.hip), against the
oracle's single sequential rand_r stream: after each push or step the device's rand_r state,
its V-row count and the model must equal the reference's.  A key ranked one off, or a seed
advanced by a stale request count, shows as a seed mismatch from that step on.

* the ranked pair (count + draw) of the store calls: one tile (4096 flags), a tile and one key,
  several tiles with whole tiles unflagged, no key flagged, more tiles than the grid has blocks;
* V wider than the coordinate-per-thread draw (V_dim > 256): store calls and the fused step
  (the split owner's case is in test_gpu_split.py);
* a request count that changes every step: the fused step (test_gpu_split.py: the split);
* a full V pool: the error at the sync, and no row written for a key that got none."""
import numpy as np
import pytest
import torch

from difacto_amd import data as D
from oracle import oracle as O

pytestmark = pytest.mark.gpu

TILE = 4096  # initv.hip kIvrTile
GRID = 256   # initv.hip kIvrGrid


@pytest.fixture(scope="module")
def H():
    from difacto_amd import hotpath
    return hotpath


def _pull_eq(c, st, up, keys):
    v, l = st.pull(c.tensor(keys, torch.int64))
    ov, ol = up.get(keys)
    assert np.array_equal(l.cpu().numpy(), ol)
    assert np.array_equal(v.cpu().numpy(), ov)


def _count_pushes(H, n, d, layout, few, max_keys=1 << 15, thr=2):
    """n keys with w != 0 and no V (a gradient push at fea_cnt 0), then three Update(kFeaCount):
    every key outside `few` and outside the last tenth crosses V_threshold in the first, the keys
    at the indices `few` in the second, none in the third.  After each: seed, V rows, pull."""
    kw = dict(V_dim=d, V_threshold=thr, l1=0, lr=0.1, V_lr=0.05, V_init_scale=0.5, seed=21,
              l1_shrk=0)
    rng = np.random.default_rng(n + d)
    c = H.Context(0, max_keys=max_keys, slot_layout=layout, **kw)
    st, up = H.Store(c), O.Updater(**kw)
    keys = np.unique(rng.integers(1, 1 << 62, size=n + n // 8 + 8, dtype=np.uint64))[:n]
    assert len(keys) == n
    tk = c.tensor(keys, torch.int64)
    g = (rng.standard_normal(n) + 3).astype(np.float32)  # w leaves 0 for every key
    st.push(tk, H.kGradient, c.tensor(g, torch.float32))
    up.update(keys, O.Updater.kGradient, g)
    never = np.zeros(n, bool)
    never[n - n // 10:] = True
    later = np.zeros(n, bool)
    later[few] = True
    never &= ~later
    first = ~(never | later)
    pushes = [np.where(first, thr + 1, 1), np.where(later, thr, 0), np.where(never, 1, 0)]
    want_rows = [first.sum(), first.sum() + later.sum(), first.sum() + later.sum()]
    for cnt, rows in zip(pushes, want_rows):
        cnt = cnt.astype(np.float32)
        st.push(tk, H.kFeaCount, c.tensor(cnt, torch.float32))
        up.update(keys, O.Updater.kFeaCount, cnt)
        c.sync()
        s = st.stats()
        assert s["seed"] == up.seed
        assert s["n_vrows"] == rows
        _, ol = up.get(keys)
        assert int((ol == d + 1).sum()) == rows  # the oracle's V rows (l1_shrk=0: every V shows)
        _pull_eq(c, st, up, keys)
    c.close()


@pytest.mark.parametrize("layout", ["split", "fat"])
@pytest.mark.parametrize("n", [1, TILE, TILE + 1, 2 * TILE + 37])
def test_initv_ranked_pair_tiles(H, n, layout):
    """the second push flags 20 keys in the middle of the list only: at 4097 keys the last tile
    is empty, at 2 * 4096 + 37 the first and the last"""
    few = np.arange(n // 2, min(n // 2 + 20, n - n // 10))
    _count_pushes(H, n, 8, layout, few)


def test_initv_ranked_pair_grid_stride(H):
    """more tiles than the count / draw grids have blocks: every block takes several tiles.
    One count push flags about 1 % of the keys; the pull is compared on them and on a sample"""
    n = GRID * TILE + TILE + 1
    d = 4
    kw = dict(V_dim=d, V_threshold=2, l1=0, lr=0.1, V_lr=0.05, V_init_scale=0.5, seed=33,
              l1_shrk=0)
    rng = np.random.default_rng(5)
    few = np.sort(rng.choice(n, size=n // 100, replace=False))
    check_keys = np.union1d(few, rng.choice(n, size=10000, replace=False))
    c = H.Context(0, max_keys=1 << 21, **kw)
    st, up = H.Store(c), O.Updater(**kw)
    keys = np.unique(rng.integers(1, 1 << 62, size=n + n // 8, dtype=np.uint64))[:n]
    assert len(keys) == n
    tk = c.tensor(keys, torch.int64)
    g = (rng.standard_normal(n) + 3).astype(np.float32)
    st.push(tk, H.kGradient, c.tensor(g, torch.float32))
    up.update(keys, O.Updater.kGradient, g)
    cnt = np.ones(n, np.float32)
    cnt[few] = 3
    st.push(tk, H.kFeaCount, c.tensor(cnt, torch.float32))
    up.update(keys, O.Updater.kFeaCount, cnt)
    c.sync()
    s = st.stats()
    assert s["seed"] == up.seed
    assert s["n_vrows"] == len(few)
    _pull_eq(c, st, up, keys[check_keys])
    c.close()


def test_initv_wide_v_store(H):
    """V_dim 260 > kIvMaxD: a thread draws a whole row"""
    _count_pushes(H, 300, 260, "split", np.arange(150, 170), max_keys=1 << 10)


def _close(a, b, rtol):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(a), np.abs(b)) + 1e-6)


def test_initv_wide_v_fused(H):
    """(V_dim 257: the fused step has no kernel for 260, "unsupported V_dim")"""
    cfg = dict(V_dim=257, V_threshold=0, l1=0, lr=.1, V_lr=.01)
    c = H.Context(0, max_keys=1 << 13, **cfg)
    up = O.Updater(**cfg)
    seen = []
    for step in range(3):
        blk = D.synthetic(200, 10, 1 << 12, seed=40 + step)
        seen.append(blk)
        loss = up.train_step(blk.offs, blk.ids, blk.vals, blk.labels, push_cnt=(step == 0))[0]
        H.train_step(c, H.DeviceRowBlock(c, blk), H.kTraining, push_cnt=(step == 0))
        p = H.progress(c)
        assert abs(p["loss"] - loss) <= 1e-4 * abs(loss), (step, p["loss"], loss)
        s = H.Store(c).stats()
        assert s["seed"] == up.seed and s["n_keys"] == up.size(), step
    uniq = np.unique(np.concatenate([O.localize(b.offs, b.ids)[0] for b in seen]))
    v, l = H.Store(c).pull(c.tensor(uniq, torch.int64))
    ov, ol = up.get(uniq)
    assert np.array_equal(l.cpu().numpy(), ol)
    assert _close(v.cpu().numpy(), ov, 1e-4)
    c.close()


def oracle_vrows(up, seen, d):
    """V rows of the oracle's model (contexts with l1_shrk=0: Get returns every V there is)"""
    uniq = np.unique(np.concatenate([O.localize(b.offs, b.ids)[0] for b in seen]))
    return int((up.get(uniq)[1] == d + 1).sum())


def test_initv_fused_request_count_changes(H):
    """a count push in every step: the requests go from many to near none, and each step's seed
    advance is that step's count (a stale total of step t - 1 would show at step t)"""
    cfg = dict(V_dim=16, V_threshold=2, l1=0, lr=.1, V_lr=.01, l1_shrk=0)
    c = H.Context(0, max_keys=1 << 18, **cfg)
    up = O.Updater(**cfg)
    seen, rows = [], []
    for step in range(6):
        blk = D.synthetic(3000, 39, 1 << 16, seed=60 + step)
        seen.append(blk)
        up.train_step(blk.offs, blk.ids, blk.vals, blk.labels, push_cnt=True)
        H.train_step(c, H.DeviceRowBlock(c, blk), H.kTraining, push_cnt=True)
        c.sync()
        s = H.Store(c).stats()
        assert s["seed"] == up.seed, step
        rows.append(oracle_vrows(up, seen, 16))
        assert s["n_vrows"] == rows[-1], step
    new = np.diff([0] + rows)  # (the oracle's: what the data asks for, ~16 k, 29 k, ... 0.4 k)
    assert len(set(new)) == 6 and 10 * new[-1] < new[0], new
    c.close()


def test_initv_pool_full(H):
    """autogrow=0 and a V pool of 100 rows, 60 in use: a gradient push whose 300 new keys all
    ask for V raises kErrPoolFull at the sync, and the keys stored before keep their state"""
    kw = dict(V_dim=8, V_threshold=0, l1=0, lr=0.1, V_lr=0.05)
    rng = np.random.default_rng(8)
    c = H.Context(0, max_keys=1024, max_vrows=100, autogrow=0, slot_layout="split", **kw)
    st, up = H.Store(c), O.Updater(**kw)
    old = np.unique(rng.integers(1, 1 << 62, size=60, dtype=np.uint64))
    new = np.setdiff1d(np.unique(rng.integers(1, 1 << 62, size=300, dtype=np.uint64)), old)
    for keys in (old, new):  # fea_cnt > V_threshold; w == 0 still, so no V yet
        cnt = np.ones(len(keys), np.float32)
        st.push(c.tensor(keys, torch.int64), H.kFeaCount, c.tensor(cnt, torch.float32))
        up.update(keys, O.Updater.kFeaCount, cnt)
    tk = c.tensor(old, torch.int64)
    for _ in range(2):  # the first draws the old keys' V
        ov, ol = up.get(old)
        g = (rng.standard_normal(len(ov)) + 3).astype(np.float32)
        st.push(tk, H.kGradient, c.tensor(g, torch.float32), c.tensor(ol, torch.int32))
        up.update(old, O.Updater.kGradient, g, ol)
    c.sync()
    s = st.stats()
    assert s["n_vrows"] == len(old) and s["seed"] == up.seed
    _pull_eq(c, st, up, old)
    before = st.pull(tk)[0].cpu().numpy().copy()
    g = (rng.standard_normal(len(new)) + 3).astype(np.float32)
    st.push(c.tensor(new, torch.int64), H.kGradient, c.tensor(g, torch.float32),
            c.tensor(np.ones(len(new), np.int32), torch.int32))
    with pytest.raises(H._lib.DfxError):
        c.sync()
    assert st.stats()["n_vrows"] == 100  # the pool's end
    after = st.pull(tk)[0].cpu().numpy()
    assert np.array_equal(before, after)
    c.close()
