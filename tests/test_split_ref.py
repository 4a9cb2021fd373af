"""tests/split_ref.py (the owner-computes split step in numpy, in the device's order) pinned on
the CPU: its batch is what tests/test_gpu_split_exact.py needs, it stays within the split's 1e-5
bars of the oracle, it is NOT the oracle bit for bit (the regrouping by owner is visible), and
each documented ordering matters: a deliberate mis-ordering changes a prediction or a model float
on the committed batch.  At N = 1 split_step refuses (one owner is backward_ref.fused_step)."""
import functools

import numpy as np
import pytest

from oracle import dist_oracle as DO
from oracle import oracle as O
from tests import backward_ref as R
from tests import split_ref as S

CFG = dict(V_dim=16, V_threshold=0, l1=0, lr=.05, V_lr=.01)


def close(a, b, rtol=1e-5):
    """tests/test_gpu_split.py::close"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    floor = 1e-6 * max(1.0, float(np.max(np.abs(b))) if b.size else 1.0)
    return np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(a), np.abs(b)) + floor)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _workers(N):
    return S.planted_workers(N)


@pytest.mark.parametrize("N", [2, 3, 8])
def test_batch_is_what_the_split_tests_need(N):
    blocks = _workers(N)
    info = S.batch_info(blocks, N)      # asserts the planted counts, from O.localize alone
    assert all(n > 0 for n in info["chunks"])
    assert info["chunks"] == [sum(R.n_chunks(c) for c in S.COUNTS)] * N == [72] * N
    assert info["chunked_keys"].size == N * sum(c > R.kChunkOcc for c in S.COUNTS) == 8 * N
    sizes = [b.size for b in blocks]
    assert sizes[0] == S.ROWS + len(S.APPENDED) + 1 and sizes[1] == S.SHORT < max(sizes)
    assert all((b.vals is None) == (r % 2 == 0) for r, b in enumerate(blocks))
    assert all(50 <= np.sum(b.weights == 0) <= 61 for b in blocks)   # every seventh row
    lens = np.diff(blocks[0].offs.astype(np.int64))[S.ROWS:]
    assert lens.tolist() == list(S.APPENDED) + [S.LONE]
    lone = S.reverse_bytes(blocks[0].ids[-S.LONE:])
    assert np.all(DO.owner_of(lone, N) == 0)    # a row with no key of owners 1 .. N - 1
    # every planted key of 127 occurrences or more is met by every worker, and every chunked
    # key has a chunk whose occurrences (in (worker, row, nnz) order) come from two workers
    assert info["spread"] and info["straddle"]


def _run(N, steps, variant=None, cfg=CFG, bars=False):
    blocks = _workers(N)
    up, one = O.Updater(**cfg), O.Updater(**cfg)
    cat = S.concat(blocks)
    uniq, _, col = O.localize(cat.offs, cat.ids)
    preds, differ = [], []
    for s in range(steps):
        info = {}
        out = S.split_step(up, blocks, N, push_cnt=(s == 0), variant=variant, info=info)
        pred = np.concatenate([o[1] for o in out])
        preds.append(pred)
        if bars:     # O.fm_predict on the state the step read; the oracle's own steps beside it
            assert close(pred, info["oracle_pred"]), (N, s)
            differ.append(float(np.mean(_bits(pred) != _bits(info["oracle_pred"]))))
            _, _, opred = one.train_step(cat.offs, cat.ids, cat.vals, cat.labels, cat.weights,
                                         push_cnt=(s == 0), want_pred=True)
            assert close(pred, opred), (N, s)
    model = up.get(uniq)
    if bars:
        ov, ol = one.get(uniq)
        assert np.array_equal(model[1], ol) and close(model[0], ov), N
        assert up.seed == one.seed and up.size() == one.size()
    return preds, model, differ


@pytest.mark.parametrize("N", [2, 3, 8])
def test_reference_within_the_split_bars_and_regrouped(N):
    """predictions within 1e-5 of the oracle's at every step, the model after three steps within
    1e-5 of O.Updater.train_step's (keys, V rows and the rand_r state exact); and the regrouping by
    owner is visible: once w and V are non-zero, more than half the rows differ from the oracle in
    their last bits (measured on this batch, steps 1 and 2: 0.78, 0.73 of the rows at N = 2;
    0.73, 0.79 at N = 3; 0.72, 0.67 at N = 8)"""
    _, _, differ = _run(N, 3, bars=True)
    print("rows whose prediction differs from the oracle's, per step:", differ)
    assert differ[-1] > 0.5, differ


@functools.lru_cache(maxsize=None)
def _base():
    return _run(3, 3)


def _changed(a, b):
    return any(not np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[0], b[0])) or \
        not np.array_equal(_bits(a[1][0]), _bits(b[1][0]))


@pytest.mark.parametrize("variant", ["rev_owners", "xxvv_coord", "row_worker"])
def test_every_documented_order_matters(variant):
    """(a) owners combined in reverse rank order, (b) XXVV summed across owners per coordinate,
    then over l, (c) a key's occurrences in (row, worker) order: each changes a prediction or a
    model float, bitwise, at N = 3, V_dim 16"""
    assert _changed(_base(), _run(3, 3, variant))


def test_chunked_sums_matter(monkeypatch):
    """(d) the chunked keys summed sequentially in float (no key counts as long)"""
    base = _base()
    monkeypatch.setattr(R, "kChunkOcc", 1 << 30)
    assert _changed(base, _run(3, 3))


def test_one_owner_is_refused():
    """N = 1 has another partial layout and is the fused step: split_step refuses it"""
    with pytest.raises(ValueError):
        S.split_step(O.Updater(**CFG), _workers(2)[:1], 1, push_cnt=True)
