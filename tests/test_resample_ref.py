"""The CPU half of the per-epoch down-sample's tests: csrc/reshuffle.h's rs_draw and rs_dropped
(the text the kernels compile) against their numpy restatement tests/resample_ref.py
(tools/resample_check.cc -> build/resample_check), the properties a sample needs of that draw,
and epoch_resample's option rules (tests/host/train_options_resample_tests.cc).  No HIP call."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import resample_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "build", "resample_check")
SIZES = (1, 2, 255, 256, 257, 65537, 1000003)
RATES = (0.25, 0.5, 0.9)
KEYS = (0, 1, 2, 12345, (1 << 63) + 7)


@pytest.fixture(scope="module")
def check():
    subprocess.check_call(["make", "-s", "build/resample_check"], cwd=ROOT)
    return CHECK


@pytest.mark.parametrize("N", SIZES)
def test_header_equals_numpy(check, N):
    """build/resample_check N KEY NEG_SAMPLING prints resample_ref's draw bits and drop flags"""
    rows = np.arange(N)
    for i, ns in enumerate(RATES):
        key = KEYS[(i + N) % len(KEYS)]
        out = subprocess.run([check, str(N), str(key), repr(ns)], capture_output=True, text=True,
                             timeout=120, check=True).stdout
        got = np.array(out.split(), np.uint32).reshape(-1, 2)
        assert got.shape == (N, 2), (N, key, ns)
        u = S.draw(key, rows)
        assert u.dtype == np.float32
        assert np.array_equal(got[:, 0], u.view(np.uint32)), (N, key, ns)
        assert np.array_equal(got[:, 1] != 0, S.dropped(key, rows, np.zeros(N, np.float32), ns)), \
            (N, key, ns)


def test_draw_is_a_multiple_of_2_to_minus_24_below_one():
    u = S.draw(3, np.arange(100000))
    assert u.min() >= 0 and u.max() < 1
    scaled = u.astype(np.float64) * (1 << 24)
    assert np.array_equal(scaled, np.floor(scaled))


@pytest.mark.parametrize("ns", RATES)
def test_drop_rate_is_within_four_sigma(ns):
    """N = 100,000 negative rows: the dropped count against the binomial N p, p = neg_sampling
    (the reader's inequality drops a negative with probability neg_sampling)"""
    N = 100000
    sigma = math.sqrt(N * ns * (1 - ns))
    labels = np.full(N, -1, np.float32)
    for key in KEYS:
        n = int(np.count_nonzero(S.dropped(key, np.arange(N), labels, ns)))
        print("neg_sampling", ns, "key", key, "dropped", n, "sigmas", (n - N * ns) / sigma)
        assert abs(n - N * ns) <= 4 * sigma, (ns, key, n)


def test_two_keys_are_independent():
    """keys 5 and 6 at 0.5 agree on about half of the rows"""
    N = 100000
    labels = np.zeros(N, np.float32)
    a = S.dropped(5, np.arange(N), labels, 0.5)
    b = S.dropped(6, np.arange(N), labels, 0.5)
    agree = np.count_nonzero(a == b) / N
    print("agree", agree)
    assert 0.499 <= agree <= 0.505


def test_labels_and_rates_that_drop_nothing():
    N = 10000
    rows = np.arange(N)
    for ns in RATES + (0.0,):
        assert not S.dropped(7, rows, np.ones(N, np.float32), ns).any()       # positive rows
        assert not S.dropped(7, rows, np.full(N, .5, np.float32), ns).any()
    for ns in (1.0, 1.5, float("inf")):
        assert not S.dropped(7, rows, np.zeros(N, np.float32), ns).any()
        assert not S.dropped(7, rows, np.full(N, -1, np.float32), ns).any()
    # label 0 counts as negative, as in the reader (label <= 0)
    assert S.dropped(7, rows, np.zeros(N, np.float32), 0.9).sum() > 8000
    # neg_sampling = 0: u > 1 never holds
    assert not S.dropped(7, rows, np.zeros(N, np.float32), 0.0).any()


def test_resample_filters_the_permuted_order():
    """the sampled epoch is the reshuffled epoch's rows without the dropped ones, in order"""
    from tests import reshuffle_ref as R
    rng = np.random.default_rng(1)
    u64, f32 = np.uint64, np.float32
    src = []
    for n in (5, 0, 9):
        lens = rng.integers(0, 4, size=n)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(u64)
        src.append({"offs": offs, "ids": rng.integers(0, 99, size=int(offs[-1])).astype(u64),
                    "vals": None, "labels": rng.choice([-1, 1], size=n).astype(f32),
                    "weights": None})
    labels = np.concatenate([b["labels"] for b in src])
    for key in (0, 4):
        full = R.reshuffle(src, 14, key)[0]
        keep = S.kept_rows(src, key, 0.5)
        p = R.perm(14, key).astype(np.int64)
        mask = ~S.dropped(key, p, labels[p], 0.5)
        assert np.array_equal(keep, p[mask]) and set(p[labels[p] > 0]) <= set(keep)
        out = S.resample(src, 4, key, 0.5)
        assert [len(b["labels"]) for b in out] == [4] * (len(keep) // 4) + \
            ([len(keep) % 4] if len(keep) % 4 else [])
        assert np.array_equal(np.concatenate([b["labels"] for b in out]), full["labels"][mask])
        lens = np.diff(full["offs"].astype(np.int64))[mask]
        assert np.array_equal(np.concatenate([np.diff(b["offs"].astype(np.int64)) for b in out]),
                              lens)
        for b in out:
            assert b["offs"][0] == 0 and b["offs"][-1] == len(b["ids"])
            assert b["vals"] is None and b["weights"] is None
    # nothing dropped at 1: reshuffle_ref's batches
    a, b = S.resample(src, 4, 9, 1.0), R.reshuffle(src, 4, 9)
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert all(np.array_equal(x[k], y[k]) for k in ("offs", "ids", "labels"))


def test_option_rules():
    """epoch_resample's refusals stand behind epoch_shuffle's; the table of every other option
    (build/train_options_tests) passes unchanged"""
    for name in ("train_options_resample_tests", "train_options_tests"):
        subprocess.check_call(["make", "-s", "build/" + name], cwd=ROOT)
        out = subprocess.run([os.path.join(ROOT, "build", name)], capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
