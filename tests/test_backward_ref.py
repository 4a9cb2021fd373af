"""The numpy backward in the device's summation order (tests/backward_ref.py) pinned on the CPU:
where no key passes kChunkOcc occurrences it is the oracle's CalcGrad bit for bit, and a step
driven by it leaves an oracle Updater in the state Updater.train_step leaves; where keys are
chunked, every restated double sum stays within the recursive-summation bound of math.fsum over
the same terms; the chunk / group / slice plans are asserted by hand."""
import math

import numpy as np
import pytest

from difacto_amd import data as D
from oracle import oracle as O
from tests import backward_ref as R


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _model(rng, U, d):
    """the interleaved Pull layout, a third of the keys without V, a tenth with w == 0"""
    if d == 0:
        return (rng.standard_normal(U) * 0.1).astype(np.float32), None, None
    lens = np.where(rng.random(U) < 0.33, 1, d + 1).astype(np.int32)
    wp, vp = O.get_pos(lens)
    W = (rng.standard_normal(int(lens.sum())) * 0.1).astype(np.float32)
    W[wp[rng.random(U) < 0.1]] = 0
    return W, wp, vp


def _weights(rng, B):
    w = (rng.random(B) + 0.5).astype(np.float32)
    w[::5] = 0
    return w


def _blocks(rcv1):
    yield "rcv1", rcv1
    yield "binary", D.synthetic(700, 25, 1500, binary=True, seed=3, ragged=True)
    yield "valued", D.synthetic(700, 25, 1500, binary=False, seed=4, ragged=True)


@pytest.mark.parametrize("d", [0, 3, 16])
def test_no_chunks_equals_oracle(rcv1, d):
    for name, blk in _blocks(rcv1):
        rng = np.random.default_rng(10 + d)
        uniq, cnt, col = O.localize(blk.offs, blk.ids)
        assert cnt.max() <= R.kChunkOcc
        U = len(uniq)
        W, wp, vp = _model(rng, U, d)
        for rw in (None, _weights(rng, blk.size)):
            pred = O.fm_predict(blk.offs, col, blk.vals, W, wp, vp, d)
            og = O.fm_calcgrad(blk.offs, col, blk.vals, blk.labels, rw, W, wp, vp, U, d, pred)
            g = R.backward(blk.offs, col, blk.vals, blk.labels, rw, W, wp, vp, U, d, pred)
            assert np.array_equal(_bits(g), _bits(og)), (name, d, rw is None)


@pytest.mark.parametrize("cfg", [
    dict(V_dim=0, l1=.01, lr=.1),
    dict(V_dim=4, V_threshold=2, lr=.1, V_lr=.01, l1=.1),       # lazy V, w back to zero
    dict(V_dim=16, V_threshold=0, l1=0, lr=.1, V_lr=.01),
])
def test_fused_step_leaves_the_updaters_state(rcv1, cfg):
    for name, blk in _blocks(rcv1):
        blk = D.RowBlock(blk.offs, blk.ids, blk.vals, blk.labels,
                         _weights(np.random.default_rng(5), blk.size))
        a, b = O.Updater(**cfg), O.Updater(**cfg)
        uniq, _, _ = O.localize(blk.offs, blk.ids)
        for step in range(4):
            _, _, want = a.train_step(blk.offs, blk.ids, blk.vals, blk.labels, blk.weights,
                                      push_cnt=(step == 0), want_pred=True)
            got = R.fused_step(b, blk, push_cnt=(step == 0))
            assert np.array_equal(_bits(got), _bits(want)), (name, step)
            (va, la), (vb, lb) = a.get(uniq), b.get(uniq)
            assert np.array_equal(_bits(va), _bits(vb)) and np.array_equal(la, lb), (name, step)
            assert a.seed == b.seed and a.new_w == b.new_w and a.size() == b.size()
        for k in uniq:
            (sa, Va), (sb, Vb) = a.entry(k), b.entry(k)
            assert np.array_equal(_bits(sa), _bits(sb))
            assert (Va is None) == (Vb is None)
            assert Va is None or np.array_equal(_bits(Va), _bits(Vb))


def _fsum_bound(terms):
    """|any recursive double summation of n terms - their exact sum| <= (n - 1) u sum |t| + O(u^2)
    with u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4, which holds
    for every order of the additions); n u sum |t| covers the second-order term for n < 2^26"""
    t = [float(v) for v in terms]
    return math.fsum(t), len(t) * 2.0 ** -53 * math.fsum(abs(v) for v in t)


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("d", [0, 5, 30])
def test_chunked_sums_within_the_summation_bound(d, binary):
    counts = (129, 257, 896, 897, 1025, 4097, 8200)   # 2, 3, 7, 8, 9, 33, 65 chunks
    blk = R.planted_batch(600, 40, counts, binary, seed=21 + d)
    uniq, cnt, col = O.localize(blk.offs, blk.ids)
    U = len(uniq)
    W, wp, vp = _model(np.random.default_rng(d), U, d)
    pred = O.fm_predict(blk.offs, col, blk.vals, W, wp, vp, d)
    g, dbg = R.backward(blk.offs, col, blk.vals, blk.labels, blk.weights, W, wp, vp, U, d, pred,
                        debug=True)
    assert sorted(int(c) for c in cnt[dbg["long"]]) == sorted(counts)
    assert not np.all(dbg["nz"]) and np.any(dbg["nz"])          # both sides of p != 0
    seen_v = 0
    for u in dbg["long"]:
        s0, s1 = int(dbg["seg"][u]), int(dbg["seg"][u + 1])
        S = dbg["sums"][int(u)]
        nz = dbg["nz"][s0:s1]
        for j, terms in ((0, dbg["px"][s0:s1][nz]), (1, dbg["pxx"][s0:s1][nz])):
            exact, bound = _fsum_bound(terms)
            assert abs(S[j] - exact) <= bound, (int(u), j, S[j], exact, bound)
        if d > 0 and dbg["hasv"][u]:
            seen_v += 1
            for k in range(d):
                exact, bound = _fsum_bound(dbg["T"][s0:s1, k])
                assert abs(S[2 + k] - exact) <= bound, (int(u), k, S[2 + k], exact, bound)
    assert d == 0 or seen_v >= 2
    # the keys that are not chunked are still the oracle's, bit for bit
    og = O.fm_calcgrad(blk.offs, col, blk.vals, blk.labels, blk.weights, W, wp, vp, U, d, pred)
    short = np.ones(U, bool)
    short[dbg["long"]] = False
    wq = np.arange(U) if wp is None else wp
    assert np.array_equal(_bits(g[wq[short]]), _bits(og[wq[short]]))
    # and the chunked ones differ from its sequential float sums somewhere
    assert np.any(_bits(g[wq[~short]]) != _bits(og[wq[~short]]))


def test_plans_by_hand():
    chunks = {128: 0, 129: 2, 896: 7, 897: 8, 4096: 32, 4097: 33, 98305: 769, 65537: 513}
    groups = {128: 0, 129: 0, 896: 0, 897: 1, 4096: 1, 4097: 2, 98305: 25, 65537: 17}
    for n in chunks:
        assert R.n_chunks(n) == chunks[n] and R.n_groups(n) == groups[n], n
    for P, want in ((2, 32), (18, 3), (32, 2), (33, 1), (64, 1), (65, 1)):
        assert R.n_slices(P - 2) == want, P
    assert [R.planted_key(i) for i in range(2)] == [1 << 24, 2 << 24]


def test_combine_orders():
    """combine() against the three orders written out on integers-as-doubles whose sums are exact,
    with one value per chunk so large that a dropped, doubled or misplaced chunk shows"""
    for nc, d in ((7, 0), (8, 0), (33, 16), (769, 16), (513, 30), (100, 62), (100, 200)):
        P = d + 2
        parts = np.arange(nc * P, dtype=np.float64).reshape(nc, P) * 3 + 1
        assert np.array_equal(R.combine(parts, d), parts.sum(axis=0)), (nc, d)
    # an order-sensitive case: 1e16 + 1 - 1e16 depends on where the large terms meet
    parts = np.zeros((96, 18))
    parts[0, 0], parts[32, 0], parts[64, 0] = 1e16, 1.0, -1e16     # three groups, R = 3 slices
    assert R.combine(parts, 16)[0] == 0.0      # (1e16) + (1) = 1e16, + (-1e16) = 0: slice order
    parts = np.zeros((128, 18))
    parts[0, 0], parts[32, 0], parts[64, 0], parts[96, 0] = 1e16, -1e16, 1.0, 1.0
    # four groups in R = 3 slices: slice 0 = g0 + g3 = 1e16 + 1 = 1e16, slice 1 = -1e16, slice 2 = 1
    assert R.combine(parts, 16)[0] == 1.0
    # in plain group order (d + 2 > 64) the same partials give 2.0
    big = np.zeros((128, 66))
    big[:, 0] = parts[:, 0]
    assert R.combine(big, 64)[0] == 2.0
