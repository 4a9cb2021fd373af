"""The numpy Localizer reference (tests/localizer_ref.py) pinned on the CPU: against the oracle's
Localizer::Compact and the reference's own known answers on rcv1-100, against the oracle on
seeded blocks (max_index = 1000, the all-ones id), and its chunk arithmetic by hand."""
import numpy as np

from oracle import oracle as O

from tests import localizer_ref as R

ALL = (1 << 64) - 1


def _check_against_oracle(offs, ids, max_index):
    uniq, cnt, col = O.localize(offs, ids, max_index=max_index)
    r = R.localize(offs, ids, max_index=max_index)
    assert np.array_equal(r["uniq"], uniq)
    assert np.array_equal(r["cnt"], cnt.astype(np.int64))
    assert np.array_equal(np.diff(r["segstart"].astype(np.int64)), r["cnt"])
    # every occurrence of segment u is an nnz whose col is u, in position (so row) order
    nnz = len(ids)
    offs64 = np.asarray(offs, dtype=np.int64)
    row = np.repeat(np.arange(len(offs) - 1, dtype=np.uint32), np.diff(offs64))
    order = np.lexsort((np.arange(nnz), col))
    assert np.array_equal(r["occ_row"], row[order])
    return r


def test_reverse_bytes_is_the_oracles():
    xs = np.array([0, 1, 0x1B8, 0x0123456789ABCDEF, ALL, 1 << 63], dtype=np.uint64)
    assert R.reverse_bytes(xs).tolist() == [O.reverse_bytes(int(x)) for x in xs]
    assert int(R.reverse_bytes(xs)[3]) == 0xFEDCBA9876543210


def test_rcv1_known_answers(rcv1, known):
    for name in ("localizer_base", "localizer_hash1000"):
        k = known[name]
        r = _check_against_oracle(rcv1.offs, rcv1.ids, k.get("max_index", ALL))
        assert int(R.reverse_bytes(r["uniq"]).sum()) == k["sum_uidx"]
        assert int(r["cnt"].sum()) == k["sum_freq"]
        assert int(r["segstart"][-1]) == rcv1.nnz


def test_seeded_blocks():
    rng = np.random.default_rng(11)
    for B, per, space, mx in ((50, 7, 40, ALL), (64, 5, 1 << 40, 1000), (33, 9, 1 << 62, ALL),
                              (1, 5, 3, ALL)):
        lens = rng.integers(0, 2 * per, B)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        ids = rng.integers(0, space, int(offs[-1]), dtype=np.uint64)
        if len(ids) > 3:
            ids[1] = ids[-1] = np.uint64(ALL)  # the all-ones id: key 0 when max_index is all ones
            ids[2] = 0
        vals = rng.standard_normal(len(ids)).astype(np.float32)
        r = _check_against_oracle(offs, ids, mx)
        rv = R.localize(offs, ids, vals, max_index=mx)
        keys = R.keys_of(ids, mx)
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(rv["occ_x"], vals.view(np.uint32)[order])
        assert np.array_equal(np.repeat(r["uniq"], r["cnt"]), keys[order])
        if mx == ALL and len(ids) > 3:
            n0 = int(np.sum(ids == 0) + np.sum(ids == np.uint64(ALL)))  # both map to key 0
            assert n0 >= 3 and r["uniq"][0] == 0 and r["cnt"][0] == n0


def test_keys_ready_and_values_bits():
    ids = np.array([5, ALL, 0, 5, 1 << 63], dtype=np.uint64)
    vals = np.array([-0.0, np.inf, 1e-45, np.nan, -np.inf], dtype=np.float32)
    r = R.localize([0, 2, 2, 5], ids, vals, keys_ready=True)
    assert r["uniq"].tolist() == [0, 5, 1 << 63, ALL]
    assert r["segstart"].tolist() == [0, 1, 3, 4, 5]
    assert r["occ_row"].tolist() == [2, 0, 2, 2, 0]
    assert np.array_equal(r["occ_x"], vals.view(np.uint32)[[2, 0, 3, 4, 1]])
    e = R.localize([0], np.zeros(0, np.uint64))
    assert e["U"] == 0 and e["segstart"].tolist() == [0] and e["n_chunks"] == 0


def test_chunk_arithmetic():
    lens = [1, 128, 129, 256, 257, 2048, 2049]
    n, choff, seg = R.chunk_plan(lens)
    per = [0, 0, 2, 2, 3, 16, 17]
    assert n == sum(per) == 40
    assert choff.tolist() == [0, 0, 0, 2, 4, 7, 23]
    assert seg.tolist() == [2] * 2 + [3] * 2 + [4] * 3 + [5] * 16 + [6] * 17
    assert R.chunk_plan([128] * 5)[0] == 0 and len(R.chunk_plan([128] * 5)[2]) == 0
