"""The CPU half of the device reshuffler's tests: csrc/reshuffle.h (the text the kernels compile
for the per-epoch row permutation) against its numpy restatement tests/reshuffle_ref.py
(tools/reshuffle_check.cc -> build/reshuffle_check), the properties a shuffle needs of that
permutation, and reshuffle_ref.reshuffle on a hand-written list.  No HIP call."""
import os
import subprocess

import numpy as np
import pytest

from tests import reshuffle_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "build", "reshuffle_check")
SIZES = (1, 2, 3, 4, 5, 255, 256, 257, 65535, 65536, 65537, 1000003)
KEYS = (0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1, 20261020)


@pytest.fixture(scope="module")
def check():
    subprocess.check_call(["make", "-s", "build/reshuffle_check"], cwd=ROOT)
    return CHECK


@pytest.mark.parametrize("N", SIZES)
def test_header_equals_numpy(check, N):
    """build/reshuffle_check N KEY prints what reshuffle_ref.perm(N, KEY) holds"""
    for key in KEYS[:2] if N > 100000 else KEYS:
        out = subprocess.run([check, str(N), str(key)], capture_output=True, text=True,
                             timeout=120, check=True).stdout
        got = np.array(out.split(), np.uint32)
        assert got.shape == (N,) and np.array_equal(got, R.perm(N, key)), (N, key)


def test_epoch_key_equals_numpy(check):
    seen = set()
    for seed, epoch, lst in ((0, 0, 0), (0, 1, 0), (0, 1, 1), (7, 19, 3), ((1 << 64) - 1, 2, 9)):
        out = subprocess.run([check, "key", str(seed), str(epoch), str(lst)],
                             capture_output=True, text=True, timeout=60, check=True).stdout
        assert int(out) == R.epoch_key(seed, epoch, lst), (seed, epoch, lst)
        seen.add(int(out))
    assert len(seen) == 5


@pytest.mark.parametrize("N", SIZES)
def test_perm_is_a_bijection(N):
    for key in KEYS[:2] if N > 100000 else KEYS:
        p = R.perm(N, key)
        assert p.dtype == np.uint32 and p.shape == (N,)
        assert np.array_equal(np.sort(p), np.arange(N, dtype=np.uint32)), (N, key)
    assert N > 1 or np.array_equal(R.perm(1, 12345), [0])


def test_domain_stays_below_4n():
    for N in SIZES[1:] + (6, 16, 17, 1 << 20, (1 << 20) + 1, (1 << 31) - 1):
        _, h = R.net(N, 0)
        assert N <= 1 << (2 * h) < 4 * N, (N, h)
    assert R.net(1, 0)[1] == 0 and R.net(0, 0)[1] == 0


@pytest.mark.parametrize("N", (65535, 65536, 65537, 1000003))
def test_two_keys_agree_at_fewer_than_one_percent(N):
    a, b = R.perm(N, 1), R.perm(N, 2)
    assert np.count_nonzero(a == b) < N // 100


def test_batches_mix_their_sources():
    """N = 30,000 as 30 source batches of 1000 rows and 30 output batches of 1000 rows, 5 keys:
    every output batch holds rows of all 30 sources, none takes more than 80 rows from one
    source (expectation 33), at most 8 fixed points"""
    for epoch in range(5):
        p = R.perm(30000, R.epoch_key(0, epoch + 1, 0)).astype(np.int64)
        counts = np.zeros((30, 30), np.int64)
        np.add.at(counts, (np.arange(30000) // 1000, p // 1000), 1)
        fixed = int(np.count_nonzero(p == np.arange(30000)))
        print("epoch", epoch, "min", counts.min(), "max", counts.max(), "fixed", fixed)
        assert counts.min() > 0
        assert counts.max() <= 80
        assert fixed <= 8


def _hand_list():
    """3 batches: binary; valued with weights and an empty row; binary and empty"""
    u64, f32 = np.uint64, np.float32
    return [
        {"offs": np.array([0, 2, 3], u64), "ids": np.array([10, 11, 12], u64), "vals": None,
         "labels": np.array([1, -1], f32), "weights": None},
        {"offs": np.array([0, 0, 1, 4], u64), "ids": np.array([20, 21, 22, 23], u64),
         "vals": np.array([.5, 1.5, 2.5, 3.5], f32), "labels": np.array([-1, 1, 1], f32),
         "weights": np.array([2, 3, 4], f32)},
        {"offs": np.array([0], u64), "ids": np.zeros(0, u64), "vals": None,
         "labels": np.zeros(0, f32), "weights": None},
    ]


def _rows(batches, valued, weighted):
    """the multiset of rows as sorted tuples (ids, values, label, weight)"""
    out = []
    for b in batches:
        offs = b["offs"].astype(np.int64)
        for r in range(len(offs) - 1):
            a, e = offs[r], offs[r + 1]
            vals = b["vals"][a:e] if b["vals"] is not None else np.ones(e - a, np.float32)
            w = b["weights"][r] if b["weights"] is not None else 1.0
            out.append((tuple(b["ids"][a:e].tolist()), tuple(vals.tolist()) if valued else (),
                        float(b["labels"][r]), float(w) if weighted else 1.0))
    return sorted(out)


def test_reshuffle_keeps_rows_rebases_offsets_and_reads_binary_as_ones():
    src = _hand_list()
    for key in (0, 5, 99):
        out = R.reshuffle(src, 2, key)
        assert [len(b["labels"]) for b in out] == [2, 2, 1]
        assert _rows(out, True, True) == _rows(src, True, True)
        for b in out:
            assert b["offs"][0] == 0 and b["offs"][-1] == len(b["ids"]) == len(b["vals"])
            assert b["offs"].dtype == np.uint64 and np.all(np.diff(b["offs"].astype(np.int64)) >= 0)
            assert b["vals"].dtype == np.float32 and b["weights"].dtype == np.float32
            for r in range(len(b["labels"])):  # the binary batch's rows: ones, weight 1
                ids = b["ids"][int(b["offs"][r]):int(b["offs"][r + 1])]
                if len(ids) and ids[0] < 20:
                    assert np.all(b["vals"][int(b["offs"][r]):int(b["offs"][r + 1])] == 1)
                    assert b["weights"][r] == 1
    assert {tuple(np.concatenate([b["ids"] for b in R.reshuffle(src, 2, k)]).tolist())
            for k in range(8)} != {tuple(np.concatenate([b["ids"] for b in src]).tolist())}
    # a binary, unweighted list stays binary and unweighted; one batch larger than the list
    out = R.reshuffle([src[0], src[2]], 5, 3)
    assert len(out) == 1 and out[0]["vals"] is None and out[0]["weights"] is None
    assert _rows(out, False, False) == _rows([src[0]], False, False)
    assert R.reshuffle([src[2]], 4, 1) == []
