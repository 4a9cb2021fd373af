"""Batches and bookkeeping for the bit-for-bit tests of the all-to-all sharded store (csrc/dist.hip,
dist.sharded_step / ShardedPipeline / rsag_step).  Plain numpy, run on the CPU; test
infrastructure.  Pinned by tests/test_dist_ref.py; used by tests/test_gpu_dist_exact.py.

The store promises that a key's records are applied in worker-rank order (dist.hip:10-28).  Whether
a test can see that order depends on the batch alone, so the batch is built for it:

planted_workers(N): one RowBlock per worker, ROWS x NNZ slots (worker 1: SHORT rows), even ranks
binary, odd ranks valued, every seventh row weight 0.0.  Every key's owner and pushing workers are
known by construction (backward_ref.planted_key(i, N) lies in owner i % N's range).  Per owner:
  * CLASS keys for every non-empty proper subset of the workers at N <= 3 (all 7 subsets at N = 3
    with the bulk); at N > 3, CLASS keys pushed by exactly m workers for every m < N (the workers
    of key j of owner o: (o + j + t) % N, t < m) and the bulk by all N;
  * a bulk of keys common to all workers: bulk_per_owner(N) = 1100 at N <= 3, so round 1's pair
    and the last round's pair of merge_runs each span two kMrgTile-item tiles.  At N = 5 a worker
    of 260 x 16 = 4160 slots cannot hold 5 x 1100 keys: the bulk is 700 per owner, which leaves
    round 1's pairs in one tile and rounds 2 and 3 in two;
  * worker 0 holds one bulk key of owner 0 at LONG[0] = 129 occurrences and one of owner 1 at
    LONG[1] = 1025: the a2a worker backward has no chunk plan (launch_bwd_positions, choff ==
    nullptr) and sums them sequentially in float32.
Which key index belongs to which class is drawn from the seed, so the merged positions of the
classes (and with them which keys sit across a tile boundary) vary with it.  universe: disjoint key
sets for different values (new keys for a table that must grow).  hole: worker 0 holds no key of
the last owner (an empty run in that owner's merge); empty: that worker's batch has 0 rows.

received(loc, N): per owner the ranks' runs as the exchange delivers them.
merge_tile_ties(runs): sort.hip merge_runs' pairing restated (pairs (2p, 2p + 1), a lone last run
passes a round unchanged, tiles of kMrgTile outputs of a pair) -> the tile boundaries of every round
that fall between two equal keys, the first taken from A and the second from B: the one place
where the stability of the merge (A wins ties, merge_split / takeA, sort.hip:421-432, :470) can
break without a key leaving its place.
reversed_order(N): the rank_order argument of oracle.dist_oracle's ShardedOracle / AggOracle /
StaleOracle that applies every key's records (count pushes, gradient pushes, AggOracle's row
sums) last rank first, nothing else changed."""
import functools
import itertools

import numpy as np

from difacto_amd import data as D
from oracle import dist_oracle as DO
from oracle import oracle as O
from tests import backward_ref as R
from tests.localizer_ref import reverse_bytes

f32 = np.float32

kMrgTile = 2048          # csrc/sort.hip:411 (kMrgNT * kMrgItems)
ROWS, NNZ, SHORT = 300, 16, 260
CLASS = 8                # keys per (owner, class)
LONG = (129, 1025)       # occurrences of worker 0's two long keys (owners 0 and 1)
STRIDE = 4096            # key indices per owner and universe


def bulk_per_owner(N):
    return 1100 if N <= 3 else 700


def classes(N, o=0):
    """-> the worker sets of owner o's class keys, CLASS of each in a row"""
    if N <= 3:
        sets = [s for m in range(1, N) for s in itertools.combinations(range(N), m)]
        return [frozenset(s) for s in sets for _ in range(CLASS)]
    return [frozenset((o + j + t) % N for t in range(m)) for m in range(1, N)
            for j in range(CLASS)]


def layout(N, seed=7, universe=0):
    """-> per owner (keys u64 sorted by class position, worker set per key): the class keys first
    (classes(N, o)), then the bulk (all workers); key = planted_key(o + N * j) with the j drawn
    without replacement from the owner's STRIDE indices of this universe"""
    rng = np.random.default_rng(seed)
    full = frozenset(range(N))
    out = []
    for o in range(N):
        sets = classes(N, o) + [full] * bulk_per_owner(N)
        j = rng.permutation(STRIDE)[:len(sets)] + universe * STRIDE
        keys = np.array([R.planted_key(o + N * int(v), N) for v in j], np.uint64)
        out.append((keys, sets))
    return out


def planted_workers(N, binary_even=True, seed=7, universe=0, hole=False, empty=None):
    """-> N RowBlocks (see the module docstring)"""
    assert N >= 2
    lay = layout(N, seed, universe)
    rng = np.random.default_rng(seed + 1000)
    nb = len(classes(N))
    long_keys = (lay[0][0][nb], lay[1][0][nb])      # the first bulk key of owners 0 and 1
    blocks = []
    for w in range(N):
        rows = SHORT if w == 1 else ROWS
        if empty is not None and w == empty:
            rows = 0
        n = rows * NNZ
        mine = []
        for o in range(N):
            if hole and w == 0 and o == N - 1:
                continue
            keys, sets = lay[o]
            mine.append(keys[np.array([w in s for s in sets])])
        mine = np.concatenate(mine)
        slots = [mine]
        if w == 0:     # (the hole at N = 2 is owner 1: its long key goes with it)
            reps = [c - 1 if not (hole and o == N - 1) else 0 for o, c in zip((0, 1), LONG)]
            slots += [np.repeat(np.array(long_keys, np.uint64), reps)]
        used = sum(len(s) for s in slots)
        if rows:
            assert used <= n, (N, w, used, n)
            fill = mine[~np.isin(mine, np.array(long_keys, np.uint64))]
            slots.append(rng.choice(fill, n - used))
            keys = np.concatenate(slots)[rng.permutation(n)]
        else:
            keys = np.zeros(0, np.uint64)
        offs = (np.arange(rows + 1) * NNZ).astype(np.uint64)
        binary = (w % 2 == 0) == bool(binary_even)
        vals = None if binary else (1.0 - rng.random(n, dtype=np.float32)).astype(f32)
        labels = np.where(rng.random(rows) < 0.3, 1.0, -1.0).astype(f32)
        wts = (1.5 - rng.random(rows)).astype(f32)
        wts[::7] = 0
        blocks.append(D.RowBlock(offs, reverse_bytes(keys), vals, labels, wts))
    return blocks


def flipped(blocks):
    """the same batches with the labels negated (training on them takes w back through zero)"""
    return [D.RowBlock(b.offs, b.ids, b.vals, -b.labels, b.weights) for b in blocks]


def head(blocks, rows):
    """the first `rows` rows of every worker's batch"""
    return [b.slice(0, min(rows, b.size)) for b in blocks]


def localized(blocks, N):
    """every worker's Localizer::Compact as ShardedOracle.begin keeps it: (uniq, cnt, col, owner
    bounds)"""
    loc = []
    for b in blocks:
        uniq, cnt, col = O.localize(b.offs, b.ids, want_cnt=True)
        loc.append((uniq, cnt, col, DO.owner_bounds(uniq, N)))
    return loc


def received(loc, N):
    """-> per owner the list of the ranks' sorted key runs, in rank order (dist.sharded_step's
    alltoallv of the keys)"""
    return [[loc[r][0][loc[r][3][g]:loc[r][3][g + 1]] for r in range(N)] for g in range(N)]


def pushers(loc, N):
    """-> (union keys u64 sorted, owner per key, bool[U, N]: worker r pushes key u)"""
    uk = np.unique(np.concatenate([l[0] for l in loc]))
    has = np.zeros((len(uk), N), bool)
    for r in range(N):
        has[np.searchsorted(uk, loc[r][0]), r] = True
    return uk, DO.owner_of(uk, N), has


def merge_tile_ties(runs):
    """runs: one owner's received runs -> the number of tile boundaries, over all rounds of
    merge_runs, between two equal keys of which the first came from the pair's A and the second
    from its B"""
    cur = [np.asarray(r, np.uint64) for r in runs]
    ties = 0
    while len(cur) > 1:
        nxt = []
        for p in range(0, len(cur), 2):
            if p + 1 == len(cur):               # the lone last run: copied, nothing to merge
                nxt.append(cur[p])
                continue
            a, b = cur[p], cur[p + 1]
            k = np.concatenate([a, b])
            src = np.concatenate([np.zeros(len(a), np.int8), np.ones(len(b), np.int8)])
            order = np.argsort(k, kind="stable")   # A before B on equal keys
            k, src = k[order], src[order]
            for t in range(kMrgTile, len(k), kMrgTile):
                ties += int(k[t - 1] == k[t] and src[t - 1] == 0 and src[t] == 1)
            nxt.append(k)
        cur = nxt
    return ties


def reversed_order(N):
    return list(range(N - 1, -1, -1))


def batch_info(blocks, N):
    """what the batch is built for, recomputed from O.localize and owner_of alone -> dict: loc,
    uniq, own, has (pushers), per owner the number of keys per exact worker set (sets) and per
    number of pushing workers (by_count), the keys every owner receives from every worker
    (run_len), the ties per owner, worker 0's three largest occurrence counts (long)"""
    loc = localized(blocks, N)
    uk, own, has = pushers(loc, N)
    sets, by_count = [], []
    for o in range(N):
        h = has[own == o]
        code = h @ (1 << np.arange(N))
        sets.append({int(c): int(n) for c, n in zip(*np.unique(code, return_counts=True))})
        m = h.sum(axis=1)
        by_count.append({int(c): int(n) for c, n in zip(*np.unique(m, return_counts=True))})
    runs = received(loc, N)
    cnt0 = np.sort(loc[0][1].astype(np.int64))[::-1] if len(loc[0][0]) else np.zeros(2, np.int64)
    return dict(loc=loc, uniq=uk, own=own, has=has, sets=sets, by_count=by_count,
                run_len=[[len(r) for r in rr] for rr in runs],
                ties=[merge_tile_ties(rr) for rr in runs], long=tuple(int(c) for c in cnt0[:3]))


# ---- schedules and the reference run ---------------------------------------------------------
T, V = 3, 4     # hotpath.kTraining, kValidation
SEEDS = {2: 7, 3: 9, 5: 12}   # chosen on the CPU: tests/test_dist_ref.py's counts hold for them

# per step (batch, job, count push).  batches: 0 the planted batch | 1 its flipped labels | 2 the
# hole / empty-batch variant | 3 another key universe | 4 the first HEAD rows of batch 0
SCHEDULES = {
    # steps 0, 1 push counts (owner_segs, k_dist_feacnt, k_dist_pull*), a validation step, steps
    # 3, 4 push none (the fused k_dist_segs_pull at V_dim % 4 == 0)
    "lanes": [(0, T, True), (0, T, True), (0, V, False), (0, T, False), (0, T, False)],
    "lazy": [(0, T, True), (1, T, True), (0, V, False), (1, T, False), (0, T, False)],
    "holes": [(0, T, True), (2, T, True), (2, T, False), (0, T, False)],
    "teeth": [(0, T, True), (0, T, True), (0, T, False)],
    # test_gpu_dist.PIPE_JOBS' pattern
    "pipe": [(0, T, True), (3, T, True), (0, T, False), (3, V, False), (0, T, False),
             (3, T, False)],
    "grow": [(4, T, True), (3, T, True), (0, T, False), (3, V, False), (0, T, False),
             (3, T, False)],
}
HEAD = 12
TRAIN = dict(V_threshold=0, l1=0, lr=.05, V_lr=.01)
# chosen on the CPU (the oracle alone): tests/test_dist_ref.py test_lazy_run_meets_its_events.  A
# bulk key's count is 1 per worker and step, so at N = 3 it stands at 3 after step 0 and crosses 4
# at rank 1 of step 1's count push; |g| of such a key is below 1.5 per worker, so l1 = 0.6 keeps
# part of the keys at w == 0
LAZY = dict(V_threshold=4, l1=0.6, l1_shrk=1, lr=.05, V_lr=.01)


def _freeze(blocks):
    for b in blocks:
        for a in (b.offs, b.ids, b.vals, b.labels, b.weights):
            if a is not None:
                a.setflags(write=False)
    return blocks


@functools.lru_cache(maxsize=None)
def batches_for(N, which):
    """the batches of a schedule (read-only, shared by the reference and the device run)"""
    return _freeze(_batches_for(N, which))


def _batches_for(N, which):
    seed = SEEDS[N]
    if which == 0:
        return planted_workers(N, seed=seed)
    if which == 1:
        return flipped(planted_workers(N, seed=seed))
    if which == 2:
        return planted_workers(N, seed=seed + 100, hole=True, empty=N - 2 if N > 2 else 1)
    if which == 3:
        return planted_workers(N, seed=seed + 200, universe=1)
    assert which == 4
    return head(planted_workers(N, seed=seed), HEAD)


def make_oracle(N, agg, cfg, stale=False, rank_order=None):
    if stale:
        return DO.StaleOracle(N, agg=agg, rank_order=rank_order, **cfg)
    cls = DO.AggOracle if agg == "sum" else DO.ShardedOracle
    return cls(N, rank_order=rank_order, **cfg)


def _has_v(so, keys):
    return np.array([(lambda e: e is not None and e[1] is not None)(so.entry(k)) for k in keys])


def _count_events(so, st, N, thr, before, ev, agg):
    """the lazy run's events of one training step, on the oracle's state.  before: the union
    keys' (entry or None) before the step's count push"""
    loc = st["loc"]
    uk, own, has = pushers(loc, N)
    if before is not None:            # a count push ran: whose Update crossed the threshold
        for i, k in enumerate(uk):
            e = before[i]
            if e is None or e[1] is not None or e[0][0] == 0:
                continue
            fc = f32(e[0][3])
            for r in range(N):
                if not has[i, r]:
                    continue
                c = loc[r][1][np.searchsorted(loc[r][0], k)]
                fc = f32(fc + c)
                if fc > thr:
                    ev["cross"] += 1
                    ev["cross_late"] += int(r > 0)
                    break
    return uk


def reference(N, agg, cfg_items, sched, stale=False, rank_order=None, events=False):
    """the schedule on the oracle -> dict: out (per step, per worker (loss, auc * n, pred)), keys
    (the union of all batches' keys, sorted), own, entries (so.entry per key after the last step),
    stats (per server (seed, n_keys, new_w) | the one updater's), vrows per owner, events"""
    cfg = dict(cfg_items)
    so = make_oracle(N, agg, cfg, stale, rank_order)
    thr = cfg.get("V_threshold", 0)
    ev = dict(cross=0, cross_late=0, initv_push=0, hidden=0, no_v=0)
    out, allk = [], []
    cache = {}
    for which, job, cnt in SCHEDULES[sched]:
        if which not in cache:
            cache[which] = batches_for(N, which)
        blocks = cache[which]
        train = job == T
        if stale:
            out.append(so.submit(blocks, push_cnt=cnt, train=train))
            allk.append(np.concatenate([O.localize(b.offs, b.ids)[0] for b in blocks]))
            continue
        before = None
        if events and train:
            uk0 = np.unique(np.concatenate([O.localize(b.offs, b.ids)[0] for b in blocks]))
            if cnt:
                before = [so.entry(k) for k in uk0]
        st = so.begin(blocks, cnt and train, (1 << 64) - 1)
        so.pull(st)
        out.append(so.compute(st, train))
        allk.append(np.concatenate([l[0] for l in st["loc"]]))
        if train:
            if events:
                uk = _count_events(so, st, N, thr, before, ev, agg)
                hv0 = _has_v(so, uk)
                live = np.zeros(len(uk), bool)      # some worker pulled the key's V
                for r in range(N):
                    lens = st["pulled"][r][1]
                    live[np.searchsorted(uk, st["loc"][r][0])] |= lens > 1
                v0 = [so.entry(k)[1] for k in uk]
            so.push(st)
            if events:
                hv1 = _has_v(so, uk)
                ev["initv_push"] += int(np.sum(~hv0 & hv1))
                ev["no_v"] += int(np.sum(~hv0 & ~hv1))
                for i in np.nonzero(hv0 & ~live)[0]:
                    same = np.array_equal(v0[i].view(np.uint32),
                                          so.entry(uk[i])[1].view(np.uint32))
                    ev["hidden"] += int(same)
                    assert same, "a V that no worker pulled was updated"
    if stale:
        so.flush()
    keys = np.unique(np.concatenate(allk))
    own = DO.owner_of(keys, N)
    entries = [so.entry(k) for k in keys]
    ups = so.up
    stats = [(u.seed, u.size(), int(u.new_w)) for u in ups]
    vrows = [int(sum(e is not None and e[1] is not None for e, o in zip(entries, own) if o == g))
             for g in range(N)]
    return dict(out=out, keys=keys, own=own, entries=entries, stats=stats, vrows=vrows, events=ev)


def entries_differ(a, b):
    """-> bool per key: the two references' entries differ in some bit"""
    def bits(x):
        return None if x is None else np.ascontiguousarray(x, f32).view(np.uint32)

    def eq(p, q):
        if p is None or q is None:
            return p is None and q is None
        if not np.array_equal(bits(p[0]), bits(q[0])) or (p[1] is None) != (q[1] is None):
            return False
        return p[1] is None or np.array_equal(bits(p[1]), bits(q[1]))
    return np.array([not eq(p, q) for p, q in zip(a["entries"], b["entries"])])
