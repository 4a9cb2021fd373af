"""tests/dist_ref.py on the CPU: the planted batches hold the classes tests/test_gpu_dist_exact.py
relies on, the merge's tile boundaries fall between equal keys of two ranks, and the oracle's
result depends, bit for bit, on the order a key's records are applied in — so a device that
applied them in another order could not pass an exact comparison.  No class may be empty and no
case is skipped on a condition computed from the data: dist_ref.SEEDS holds seeds for which every
assertion here holds."""
import functools

import numpy as np
import pytest

from oracle import dist_oracle as DO
from tests import dist_ref as X
from tests.localizer_ref import reverse_bytes

NS = (2, 3, 5)      # every N tests/test_gpu_dist_exact.py runs
TRAIN = dict(V_threshold=0, l1=0, lr=.05, V_lr=.01)


@functools.lru_cache(maxsize=None)
def _info(N, which=0):
    blocks = X.batches_for(N, which)
    return blocks, X.batch_info(blocks, N)


@pytest.mark.parametrize("N", NS)
def test_planted_shape(N):
    blocks, info = _info(N)
    assert [b.size for b in blocks] == [X.SHORT if w == 1 else X.ROWS for w in range(N)]
    for w, b in enumerate(blocks):
        assert np.array_equal(np.diff(b.offs.astype(np.int64)), np.full(b.size, X.NNZ))
        assert (b.vals is None) == (w % 2 == 0)
        assert np.all(b.weights[::7] == 0) and np.all(b.weights[np.arange(b.size) % 7 != 0] > 0)
    other = X.planted_workers(N, binary_even=False, seed=X.SEEDS[N])
    assert [b.vals is None for b in other] == [w % 2 == 1 for w in range(N)]
    # worker 0's long keys: exactly 129 and 1025 occurrences, owners 0 and 1, nothing else long
    assert info["long"][:2] == (X.LONG[1], X.LONG[0]) and info["long"][2] < 64
    uniq, cnt = info["loc"][0][0], info["loc"][0][1]
    assert DO.owner_of(uniq[cnt == X.LONG[0]], N).tolist() == [0]
    assert DO.owner_of(uniq[cnt == X.LONG[1]], N).tolist() == [1]
    for r in range(1, N):
        assert info["loc"][r][1].max() < 64


@pytest.mark.parametrize("N", NS)
def test_planted_classes(N):
    """every owner: >= 8 keys of every non-empty subset of the workers (N <= 3), of every number
    of pushing workers (N = 5); the bulk from every worker; every key on the owner it was planted
    for (the key sets are recomputed with O.localize and owner_of)"""
    _, info = _info(N)
    lay = X.layout(N, X.SEEDS[N])
    for o in range(N):
        keys, sets = lay[o]
        assert np.all(DO.owner_of(keys, N) == o)
        mine = info["uniq"][info["own"] == o]
        assert np.array_equal(np.sort(keys), mine)
        at = np.searchsorted(info["uniq"], keys)
        for k, s in zip(at, sets):
            assert set(np.nonzero(info["has"][k])[0].tolist()) == set(s)
        if N <= 3:
            assert all(info["sets"][o].get(c, 0) >= X.CLASS for c in range(1, 1 << N)), (N, o)
            assert len(info["sets"][o]) == (1 << N) - 1
        else:
            assert all(info["by_count"][o].get(m, 0) >= X.CLASS for m in range(1, N + 1)), (N, o)
        want = X.bulk_per_owner(N)
        assert all(n >= want for n in info["run_len"][o]), (N, o, info["run_len"][o])
    assert X.bulk_per_owner(2) == X.bulk_per_owner(3) == 1100
    # N <= 3: round 1's pair and the last round's pair span two tiles on every owner
    if N <= 3:
        for o in range(N):
            rl = info["run_len"][o]
            assert rl[0] + rl[1] > X.kMrgTile and sum(rl) > X.kMrgTile
    else:   # 5 x 1100 keys do not fit 260 x 16 slots: rounds 2 and 3 span two tiles
        for o in range(N):
            rl = info["run_len"][o]
            assert sum(rl[:4]) > X.kMrgTile and sum(rl) > X.kMrgTile


def test_hole_and_empty_batch():
    """the variant step at N = 5: the last owner receives no key from worker 0, worker 3's batch
    is empty; at N = 2 worker 1's batch is empty, so owner runs of one rank alone"""
    blocks, info = _info(5, 2)
    assert [b.size for b in blocks] == [300, 260, 300, 0, 300]
    assert info["run_len"][4][0] == 0 and all(n > 0 for n in info["run_len"][4][1:3])
    assert all(rl[3] == 0 for rl in info["run_len"])
    assert all(info["run_len"][o][0] > 0 for o in range(4))
    blocks, info = _info(2, 2)
    assert [b.size for b in blocks] == [300, 0]
    assert info["run_len"][1] == [0, 0] and info["run_len"][0][0] > 0
    # another universe shares no key with the batch
    a, b = _info(3)[1]["uniq"], _info(3, 3)[1]["uniq"]
    assert len(np.intersect1d(a, b)) == 0
    assert len(_info(3, 4)[1]["uniq"]) <= 3 * X.HEAD * X.NNZ


def test_received_is_the_exchange():
    """received() against a plain restatement: owner g gets, from every rank in rank order, that
    rank's sorted unique keys of g's range"""
    for N in NS:
        blocks, info = _info(N)
        runs = X.received(info["loc"], N)
        for r, b in enumerate(blocks):
            k = np.unique(reverse_bytes(b.ids))
            own = DO.owner_of(k, N)
            for g in range(N):
                assert np.array_equal(runs[g][r], k[own == g])


def _ties_by_hand(runs):
    """merge_runs' rounds with Python lists and sorted() (stable): (key, round-local source)"""
    cur = [[int(k) for k in r] for r in runs]
    ties = 0
    while len(cur) > 1:
        nxt = []
        for p in range(0, len(cur) - 1, 2):
            m = sorted([(k, 0) for k in cur[p]] + [(k, 1) for k in cur[p + 1]],
                       key=lambda t: t[0])
            ties += sum(m[t - 1] == (m[t][0], 0) and m[t][1] == 1
                        for t in range(X.kMrgTile, len(m), X.kMrgTile))
            nxt.append([k for k, _ in m])
        if len(cur) % 2:
            nxt.append(cur[-1])
        cur = nxt
    return ties


def test_merge_tile_ties():
    # by hand: A = 0 .. 2047 and B = [2047]: the boundary after 2048 outputs splits 2047A | 2047B
    a = np.arange(2048, dtype=np.uint64)
    assert X.merge_tile_ties([a, a[-1:]]) == 1
    assert X.merge_tile_ties([a, a[-1:] + np.uint64(1)]) == 0     # different keys
    assert X.merge_tile_ties([a[:-1], a[-2:]]) == 0              # 2046A 2046B | 2047B
    assert X.merge_tile_ties([a[:1], a]) == 0                    # one tile and one item
    # three runs: round 1 merges (0, 1) into one tile, run 2 passes; round 2's A holds two copies
    # of each key: ... 1023A 1023A | 1023B, and one item fewer leaves a single tile
    assert X.merge_tile_ties([a[:1024], a[:1024], a[1023:1024]]) == 1
    assert X.merge_tile_ties([a[:1024], a[:1023], a[1023:1024]]) == 0
    for N in NS:
        _, info = _info(N)
        runs = X.received(info["loc"], N)
        assert info["ties"] == [_ties_by_hand(rr) for rr in runs]
    # every owner at N = 3, overall at N = 2 and N = 5
    assert all(t >= 1 for t in _info(3)[1]["ties"]), _info(3)[1]["ties"]
    assert sum(_info(2)[1]["ties"]) >= 1 and sum(_info(5)[1]["ties"]) >= 1


@functools.lru_cache(maxsize=None)
def _teeth(N, agg, d):
    cfg = tuple(sorted(dict(TRAIN, V_dim=d).items()))
    a = X.reference(N, agg, cfg, "teeth")
    b = X.reference(N, agg, cfg, "teeth", rank_order=X.reversed_order(N))
    diff = X.entries_differ(a, b)
    return a, b, [int(diff[a["own"] == o].sum()) for o in range(N)]


@pytest.mark.parametrize("d", [0, 16, 260])
@pytest.mark.parametrize("agg,N", [("ranks", 2), ("ranks", 3), ("sum", 3), ("sum", 5)])
def test_reversed_order_changes_bits(agg, N, d):
    """three steps with every key's records applied last rank first: the model of every owner
    differs in some bit from the rank-order one — the comparison of tests/test_gpu_dist_exact.py
    sees the order"""
    a, b, per_owner = _teeth(N, agg, d)
    assert all(n >= 1 for n in per_owner), (agg, N, d, per_owner)
    print(agg, N, d, "keys whose bits change per owner", per_owner, "of", len(a["keys"]))


@pytest.mark.parametrize("d", [0, 16])
def test_reversed_order_sum_two_workers_changes_nothing(d):
    """push_agg=sum at N = 2: a key's gradient is a + b or b + a, the same float (IEEE addition is
    commutative), its count likewise, and the InitV draws are ranked in key order whatever the
    workers' order — so no bit can move, and sum mode is pinned only by keys that three or more
    workers push (N = 3 and N = 5 above)"""
    a, b, per_owner = _teeth(2, "sum", d)
    assert per_owner == [0, 0]
    assert a["stats"] == b["stats"]


def test_rank_order_default_is_rank_order():
    cfg = tuple(sorted(dict(TRAIN, V_dim=16).items()))
    for agg in ("ranks", "sum"):
        a = X.reference(3, agg, cfg, "teeth")
        b = X.reference(3, agg, cfg, "teeth", rank_order=[0, 1, 2])
        assert not X.entries_differ(a, b).any() and a["stats"] == b["stats"]
        for oa, ob in zip(a["out"], b["out"]):
            for (_, _, pa), (_, _, pb) in zip(oa, ob):
                assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32))
    with pytest.raises(AssertionError):
        DO.ShardedOracle(3, rank_order=[0, 0, 1], V_dim=0)


@pytest.mark.parametrize("agg", ["ranks", "sum"])
def test_lazy_run_meets_its_events(agg):
    """the lazy configuration of the GPU file on the planted batch meets, on the oracle's state:
    a count push that crosses V_threshold (ranks: at a rank > 0, k_dist_feacnt's frank), an InitV
    raised by a gradient push, keys pulled with their V hidden that get no V update, and keys
    pulled without V that get none"""
    cfg = tuple(sorted(dict(X.LAZY, V_dim=16).items()))
    ev = X.reference(3, agg, cfg, "lazy", events=True)["events"]
    assert ev["cross"] > 0 and ev["initv_push"] > 0 and ev["hidden"] > 0 and ev["no_v"] > 0, ev
    if agg == "ranks":
        assert ev["cross_late"] > 0, ev
