"""tests/metric_exact.py against what it restates: a brute-force pair count, the oracle's
stable-tie AUC (exactly), and the reference's own float AUC / logloss within the reference's
float accumulation.  No GPU: these pin the yardstick that test_gpu_metric_exact.py holds the
device to."""
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import metric_exact as M


def _brute_auc_times_n(label, pred):
    """O(n^2): a negative counts the positives strictly before it in (value, input index)
    order; values compare as floats do (-0 == +0, subnormals distinct, +-inf ordered)"""
    pred = np.asarray(pred, np.float32)
    pos = np.asarray(label, np.float32) > 0
    n = len(pred)
    P = int(pos.sum())
    if P in (0, n):
        return 1.0
    area = 0
    for j in range(n):
        if pos[j]:
            continue
        for i in range(n):
            if pos[i] and (pred[i] < pred[j] or (pred[i] == pred[j] and i < j)):
                area += 1
    a = float(area) / (float(P) * (float(n) - float(P)))
    return ((1 - a) if a < 0.5 else a) * float(n)


_EDGE_VALUES = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 3e-39, 1.0,
                         -1.0, 1.5, 20.0, -20.0], np.float32)


def _small_cases():
    rng = np.random.default_rng(7)
    for n in (1, 2, 3, 17, 64, 65, 300):
        for odd in (False, True):
            label = M.labels_odd(rng, n) if odd else M.labels_pm1(rng, n)
            yield label, rng.choice(_EDGE_VALUES, size=n)               # heavy ties, edges
            yield label, rng.choice(_EDGE_VALUES[:9], size=n)           # zeros and subnormals
            yield label, (np.round(rng.standard_normal(n) * 2) / 2).astype(np.float32)
            for name in M.PATTERNS:
                yield label, M.make_pred(name, rng, n, label)
    yield np.array([1, -1, -1], np.float32), np.array([0, 1, 2], np.float32)  # first
    yield np.array([-1, -1, 1], np.float32), np.array([0, 1, 2], np.float32)  # last
    yield np.array([-1, 1, -1], np.float32), np.array([0, 1, 2], np.float32)  # a = 0.5


def test_auc_times_n_equals_brute_force_and_oracle_stable_ties():
    k = 0
    for label, pred in _small_cases():
        got = M.auc_times_n(label, pred)
        assert got == _brute_auc_times_n(label, pred), (k, label, pred)
        assert got == O.auc_stable_ties(label, pred), (k, label, pred)
        k += 1
    assert k > 150


def test_auc_times_n_degenerate_and_middle():
    one = np.ones(5, np.float32)
    p = np.arange(5, dtype=np.float32)
    assert M.auc_times_n(one, p) == 1.0 and M.auc_times_n(-one, p) == 1.0
    assert M.auc_times_n(np.zeros(5, np.float32), p) == 1.0   # 0 is not positive
    # one positive in the exact middle: a = 0.5 exactly, not flipped
    assert M.auc_times_n(np.array([-1, 1, -1], np.float32), np.array([0, 1, 2], np.float32)) == 1.5
    assert M.auc_times_n(np.array([1, -1, -1], np.float32), np.array([0, 1, 2], np.float32)) == 3.0
    assert M.auc_times_n(np.array([-1, -1, 1], np.float32), np.array([0, 1, 2], np.float32)) == 3.0


@pytest.mark.parametrize("n", [1000, 12289, 100003])
def test_auc_times_n_against_reference_on_tie_free_inputs(n):
    """the reference accumulates the area in float: 1e-4 * n is its bar throughout the suite"""
    for name in M.NORMAL_PATTERNS:
        label, pred = M.standalone_case(name, n)
        keep = np.unique(pred, return_index=True)[1]   # drop the few float32 collisions
        keep.sort()
        label, pred = label[keep], pred[keep]
        assert not O.has_ties(pred)
        assert abs(M.auc_times_n(label, pred) - O.auc(label, pred)) <= 1e-4 * len(pred)
        assert M.auc_times_n(label, pred) == O.auc_stable_ties(label, pred)


@pytest.mark.parametrize("n", [1, 1000, 100003])
def test_logloss_sum_against_reference(n):
    """the reference's Evaluate accumulates in float: the suite's 1e-4 relative bar"""
    for name in ["correlated", "anti", "eighths", "saturated", "subnormal"]:
        for odd in (False, True):
            label, pred = M.standalone_case(name, n, odd)
            S, tol = M.logloss_sum(label, pred)
            assert abs(S - O.evaluate(label, pred)) <= 1e-4 * max(S, 1.0), (name, n)


def test_logloss_tol_is_below_one_row():
    """what makes a dropped or doubled row visible: tol < the smallest term, at every size of
    the GPU tests' standard-normal inputs"""
    for n in M.SIZES:
        for name in M.NORMAL_PATTERNS:
            for odd in (False, True):
                label, pred = M.standalone_case(name, n, odd)
                S, tol = M.logloss_sum(label, pred)
                assert tol < M.logloss_terms(label, pred).min(), (name, n)
    # at test_auc_and_evaluate's n = 20,000 even the smallest term any row can have, at the
    # +-20 clip, is above tol
    S, tol = M.logloss_sum(*M.standalone_case("correlated", 20000))
    assert tol < math.log(1.0 + math.exp(-20.0))
    # infinite terms (exp overflows in double as it does on the device) give S = tol = inf
    S, tol = M.logloss_sum(*M.standalone_case("inf", 100))
    assert math.isinf(S) and math.isinf(tol)
