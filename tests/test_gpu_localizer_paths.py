"""The Localizer's own outputs (dfx_localize_occ: uniq, segstart, occ_row, occ_x and the chunk
plan, as the fused step and the split owner consume them) against the numpy reference
(tests/localizer_ref.py), at every size and state where csrc/locbucket.hip, localize.hip or
sort.hip change path.  Every comparison is np.array_equal on integers and bit patterns.

Every case runs on bucket-sort contexts (loc_bucket=1) and on radix-sort contexts
(loc_bucket=0; sort_pack=0 and loc_xpay=0 for the other payload forms); valued cases at
lb_gather = 0, 1, 2; the cases where the scatter's row windows matter (W) also at lb_hnt = 256,
512, 1024.  A bucket case asserts from the entry's stats that the path it is named for was taken
(used, lb_over, the hint words, the map flag, the launch plan): none passes by falling back.

Constants are named by the source line they are read from (csrc/ = difacto_amd/csrc/)."""
import numpy as np
import pytest

from tests import localizer_ref as R

pytestmark = pytest.mark.gpu

ALL = (1 << 64) - 1
kLbCap = 2048        # locbucket.hip:48   items of a bucket sorted in LDS
kLbMaxBits = 13      # locbucket.hip:49
kLbMaxRows = 2048    # locbucket.hip:50   rows per hist / scatter tile, at most
kLbOverRadix = 2     # locbucket.hip:52   more oversize buckets than this: radix next
kLbRetry = 64        # locbucket.hip:53   ... and the bucket sort again after this many
kLbHotMax = 1024     # locbucket.hip:147  the hot-key list's capacity
kLbTiles = 128       # locbucket.hip:1341 row tiles, at most (before the rt cap)
kChunkOcc = 128      # internal.h:398     occurrences per chunk of a long segment
kList = 256          # localize.hip:295   k_chunk_write's block-wide list
kListMin = 16        # localize.hip:317   segments of more chunks than this go through it


def lb_wbits(nnz):
    """locbucket.hip:1308-1309: the least wbits >= 1 with 1024 << wbits >= nnz"""
    w = 1
    while w < kLbMaxBits and (1024 << w) < nnz:
        w += 1
    return w


def lb_tiles(B, nnz):
    """locbucket.hip:1342-1344 -> (rt, ntiles)"""
    nt = min(kLbTiles, max(1, nnz // 4096))
    rt = min(kLbMaxRows, max(1, -(-B // nt)))
    return rt, -(-B // rt)


def lb_hot_th(nnz):
    """locbucket.hip:1393-1394: a hot key's occurrences, at least"""
    return max(64, min(nnz // (1 << lb_wbits(nnz)) // 2, kLbCap))


def bitlen(x):
    return int(x).bit_length()


@pytest.fixture(scope="module")
def H():
    from difacto_amd import hotpath
    return hotpath


BUCKET_BIN = [dict(loc_bucket=1)]
BUCKET_BIN_W = BUCKET_BIN + [dict(loc_bucket=1, lb_hnt=h) for h in (256, 512, 1024)]
RADIX_BIN = [dict(loc_bucket=0), dict(loc_bucket=0, sort_pack=0)]
BUCKET_VAL = [dict(loc_bucket=1, lb_gather=g) for g in (0, 1, 2)]
BUCKET_VAL_W = BUCKET_VAL + [dict(loc_bucket=1, lb_gather=2, lb_hnt=h) for h in (256, 512, 1024)]
RADIX_VAL = [dict(loc_bucket=0), dict(loc_bucket=0, loc_xpay=0)]


class Ctxs:
    """small contexts (no model access), closed on exit"""

    def __init__(self, H, kws):
        self.H, self.kws = H, kws

    def __enter__(self):
        self.cs = [(kw, self.H.Context(0, max_keys=4096, **kw)) for kw in self.kws]
        return self.cs

    def __exit__(self, *exc):
        for _, c in self.cs:
            c.close()


def _ctxs(H, valued, windows=False, radix=True):
    if valued:
        kws = (BUCKET_VAL_W if windows else BUCKET_VAL) + (RADIX_VAL if radix else [])
    else:
        kws = (BUCKET_BIN_W if windows else BUCKET_BIN) + (RADIX_BIN if radix else [])
    return Ctxs(H, kws)


class Batch:
    def __init__(self, lens, ids, vals=None, max_index=ALL, keys_ready=False):
        self.offs = np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]) \
            .astype(np.uint64)
        self.ids = np.ascontiguousarray(ids, dtype=np.uint64)
        assert int(self.offs[-1]) == len(self.ids)
        self.vals = None if vals is None else np.ascontiguousarray(vals, dtype=np.float32)
        self.max_index, self.keys_ready = max_index, keys_ready
        self.B, self.nnz = len(self.offs) - 1, len(self.ids)
        self._ref = None

    def ref(self):  # computed once, shared by every context
        if self._ref is None:
            self._ref = R.localize(self.offs, self.ids, self.vals, self.max_index,
                                   self.keys_ready)
        return self._ref


def even(B, nnz):
    lens = np.full(B, nnz // B, dtype=np.int64)
    lens[:nnz % B] += 1
    return lens


def ragged(rng, B, nnz):
    """B rows of random lengths (some empty) summing to nnz"""
    cuts = np.sort(rng.integers(0, nnz + 1, B - 1))
    return np.diff(np.concatenate([[0], cuts, [nnz]]))


def ids_of(keys):
    """the ids whose keys these are (ReverseBytes is its own inverse; max_index all ones)"""
    return R.reverse_bytes(np.asarray(keys, dtype=np.uint64))


def vals_of(rng, n):
    return rng.standard_normal(n).astype(np.float32)


def _same(out, ref, what):
    assert out["U"] == ref["U"], what
    assert np.array_equal(out["uniq"], ref["uniq"]), what
    assert np.array_equal(out["segstart"], ref["segstart"]), what
    assert np.array_equal(out["occ_row"], ref["occ_row"]), what
    if ref["occ_x"] is not None:
        assert np.array_equal(out["occ_x"], ref["occ_x"]), what
    assert out["n_chunks"] == ref["n_chunks"], what
    if ref["n_chunks"] > 0:
        assert np.array_equal(out["choff"], ref["choff"]), what
        assert np.array_equal(out["chunk_seg"], ref["chunk_seg"]), what
        assert out["stats"]["n_init"] != 0, what  # (the plan's gate was open)


def _expect(st, expect, what):
    for k, v in (expect or {}).items():
        if callable(v):
            assert v(st[k]), (what, k, st)
        else:
            assert st[k] == v, (what, k, v, st)


def run(H, cs, b, what, expect=None, expect_all=None, used=1):
    """one batch on every context: outputs equal the reference; bucket contexts took the bucket
    sort (used) and the path `expect` names; `expect_all` holds on the radix contexts too"""
    ref = b.ref()
    sts = []
    for kw, c in cs:
        out = H.localize_occ(c, b.offs, b.ids, b.vals, b.max_index, b.keys_ready)
        st = out["stats"]
        w = (what, kw)
        _same(out, ref, w)
        _expect(st, expect_all, w)
        if kw["loc_bucket"]:
            assert st["used"] == used, (w, st)
            if used:
                assert st["wbits"] in (lb_wbits(b.nnz), min(lb_wbits(b.nnz) + 1, kLbMaxBits)), w
                assert (st["rt"], st["ntiles"]) == lb_tiles(b.B, b.nnz), (w, st)
                _expect(st, expect, w)
        else:
            assert st["used"] == 0, (w, st)
        sts.append(st)
    return sts


# ---------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("valued", [False, True])
def test_sizes_and_bucket_count_steps(H, valued):
    """nnz = 1; B = 1 with one id five times (rb = 0, diff = 0); the bucket-count steps
    (locbucket.hip:1309: nnz = 2048 | 2049, 4096 | 4097), one tile to two (:1342: nnz = 8191 |
    8192); empty first and last rows; all rows empty but one; no rows; rows without items"""
    rng = np.random.default_rng(1)
    v = (lambda n: vals_of(rng, n)) if valued else (lambda n: None)
    with _ctxs(H, valued) as cs:
        run(H, cs, Batch([1], [12345], v(1)), "nnz=1", dict(wbits=1, hint2=1, lb_over=0))
    with _ctxs(H, valued) as cs:
        run(H, cs, Batch([5], [77] * 5, v(5)), "B=1 x5", dict(wbits=1, hint2=1, lb_over=0))
    for nnz, wb, nt in ((2048, 1, 1), (2049, 2, 1), (4096, 2, 1), (4097, 3, 1), (8191, 3, 1),
                        (8192, 3, 2)):
        ids = rng.integers(0, 1 << 24, nnz, dtype=np.uint64)  # keys vary in their top 24 bits
        with _ctxs(H, valued) as cs:
            run(H, cs, Batch(ragged(rng, 300, nnz), ids, v(nnz)), ("nnz", nnz),
                dict(wbits=wb, ntiles=nt, hint2=1, lb_over=0))
    lens = ragged(rng, 200, 3000)
    with _ctxs(H, valued) as cs:
        run(H, cs, Batch(np.concatenate([[0, 0, 0], lens, [0, 0]]),
                         rng.integers(0, 1 << 24, 3000, dtype=np.uint64), v(3000)),
            "empty first and last rows", dict(wbits=2, lb_over=0))
    lens = np.zeros(500, dtype=np.int64)
    lens[321] = 2500
    with _ctxs(H, valued) as cs:
        run(H, cs, Batch(lens, rng.integers(0, 1 << 24, 2500, dtype=np.uint64), v(2500)),
            "all rows empty but one", dict(wbits=2, lb_over=0))
        # the same contexts after a batch: no rows, then rows without items, then a batch again
        run(H, cs, Batch([], [], v(0)), "B=0", used=0, expect_all=dict(U=0, n_chunks=0))
        run(H, cs, Batch([0] * 70, [], v(0)), "nnz=0", used=0, expect_all=dict(U=0, n_chunks=0))
        run(H, cs, Batch([3], [9, 8, 9], v(3)), "after empty")
    with _ctxs(H, valued) as cs:  # ... and as a context's first batches
        run(H, cs, Batch([0] * 3, [], v(0)), "nnz=0 first", used=0, expect_all=dict(U=0))
        run(H, cs, Batch([], [], v(0)), "B=0 first", used=0, expect_all=dict(U=0))


# ------------------------------------------------------------------------- bucket capacity
def _cap_batch(rng, totals, packed, valued, B=64):
    """fresh contexts place a key by its top bits (locbucket.hip:124-126): nnz = 4096 gives four
    buckets, chosen by key bits 63..62.  packed: 12 more bits vary, at bit 50; else 62"""
    ks = []
    for bk, n in enumerate(totals):
        low = (rng.integers(0, 1 << 12, n, dtype=np.uint64) << np.uint64(50)) if packed else \
            rng.integers(0, 1 << 62, n, dtype=np.uint64)
        ks.append((np.uint64(bk) << np.uint64(62)) | low)
    keys = np.concatenate(ks)
    if packed:
        keys[0] |= np.uint64(1 << 50)  # (the lowest varying bit is bit 50)
    keys = keys[rng.permutation(len(keys))]
    return Batch(even(B, len(keys)), ids_of(keys), vals_of(rng, len(keys)) if valued else None)


@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("packed", [True, False])
def test_bucket_capacity(H, valued, packed):
    """exactly kLbCap items in a bucket (the one-wave LDS sort) against kLbCap + 1
    (lb_needs_global, locbucket.hip:740: k_lb_big through global memory), and one bucket of all"""
    rng = np.random.default_rng(2)
    for totals, over in (((kLbCap, kLbCap, 0, 0), 0), ((kLbCap + 1, kLbCap - 1, 0, 0), 1),
                         ((0, kLbCap - 1, 0, kLbCap + 1), 1), ((2 * kLbCap, 0, 0, 0), 1)):
        b = _cap_batch(rng, totals, packed, valued)
        assert b.nnz == 4096 and lb_wbits(b.nnz) == 2
        with _ctxs(H, valued) as cs:
            run(H, cs, b, ("totals", totals, packed),
                dict(wbits=2, lb_over=over, hint0=over, hint2=1 if packed else 2))


# ---------------------------------------------------------------- radix fallback and retry
def _three_hot(rng, nnz=8000, occ=2100):
    """three keys of `occ` occurrences in three different buckets of the eight (fresh: key bits
    63..61; a fitted map keeps keys this far apart in different buckets too)"""
    hot = [np.uint64((bk << 61) | (3 << 40)) for bk in (1, 4, 6)]
    fill = rng.integers(0, 1 << 24, nnz - 3 * occ, dtype=np.uint64) << np.uint64(40)
    keys = np.concatenate([np.repeat(np.array(hot, dtype=np.uint64), occ), fill])
    keys = keys[rng.permutation(nnz)]
    return Batch(ragged(rng, 250, nnz), ids_of(keys), vals_of(rng, nnz))


@pytest.mark.parametrize("gather", [0, 1, 2])
def test_radix_fallback_and_retry(H, gather):
    """hint[0] = 3 > kLbOverRadix (locbucket.hip:1302) sends the next kLbRetry - 1 = 63 batches
    to the radix sort; the 64th runs the bucket sort again; all 65 results equal the reference
    (valued batches: a binary one would build a hot-key map, which clears hint[0])"""
    rng = np.random.default_rng(3)
    bs = [_three_hot(rng) for _ in range(3)]
    assert all(lb_wbits(b.nnz) == 3 for b in bs) and 3 > kLbOverRadix
    with Ctxs(H, [dict(loc_bucket=1, lb_gather=gather)]) as cs:
        run(H, cs, bs[0], "call 0", dict(lb_over=3, hint0=3, hint1=0))
        for i in range(1, kLbRetry):
            run(H, cs, bs[i % 3], ("call", i), used=0, expect_all=dict(hint0=3, hint1=i))
        run(H, cs, bs[kLbRetry % 3], "the 64th", dict(lb_over=3, hint0=3, hint1=0))
    with Ctxs(H, RADIX_VAL) as cs:
        for b in bs:
            run(H, cs, b, "radix")


# ------------------------------------------------------------------------------ item form
def _span_batch(rng, nnz, B, span, valued):
    """keys in [base, base + span], both ends present and bit 0 varying: lb_pack
    (locbucket.hip:214-222) sees bitlen(span) key bits"""
    base = np.uint64(5 << 56)
    keys = base + (rng.integers(0, 1 << 62, nnz, dtype=np.uint64) % np.uint64(span + 1))
    keys[0], keys[1], keys[2] = base, base + np.uint64(span), base + np.uint64(1)
    keys = keys[rng.permutation(nnz)]
    return Batch(even(B, nnz), ids_of(keys), vals_of(rng, nnz) if valued else None)


@pytest.mark.parametrize("valued", [False, True])
def test_item_form_flips_at_63_bits(H, valued):
    """varying key bits + row bits = 63 packs, 64 does not (locbucket.hip:220); the row bits
    come from B - 1 for binary batches and from nnz - 1 for valued ones (:444)"""
    rng = np.random.default_rng(4)
    nnz, B = 1500, 1024
    rb = bitlen(nnz - 1) if valued else bitlen(B - 1)
    assert rb == (11 if valued else 10)
    for span, form in (((1 << (63 - rb)) - 1, 1), (1 << (63 - rb), 2),
                       ((1 << (64 - rb)) - 1, 2)):
        assert bitlen(span) + rb == (63 if form == 1 else 64)
        with _ctxs(H, valued) as cs:
            run(H, cs, _span_batch(rng, nnz, B, span, valued), ("span bits", bitlen(span)),
                dict(hint2=form, lb_over=0))


def _form_batch(rng, wide, valued, nnz=3000, B=200):
    ids = rng.integers(0, ALL, nnz, dtype=np.uint64) if wide else \
        rng.integers(0, 1 << 20, nnz, dtype=np.uint64)
    return Batch(ragged(rng, B, nnz), ids, vals_of(rng, nnz) if valued else None)


@pytest.mark.parametrize("valued", [False, True])
def test_item_form_first_guess_and_switches(H, valued):
    """a first batch's form is guessed on the host (locbucket.hip:1314-1328) from max_index /
    keys_ready; later launches follow the previous batch's form (q_lds, :1437), so a batch of
    the other form is sorted by the launch meant for the previous one"""
    rng = np.random.default_rng(5)
    nnz = 3000
    v = (lambda: vals_of(rng, nnz)) if valued else (lambda: None)
    wide_ids = rng.integers(0, ALL, nnz, dtype=np.uint64)
    small_ids = rng.integers(0, 1 << 20, nnz, dtype=np.uint64)
    firsts = [("max_index=1000", Batch(ragged(rng, 200, nnz), wide_ids, v(), 1000), 1, 1),
              ("small ids", Batch(ragged(rng, 200, nnz), small_ids, v()), 2, 1),
              ("64-bit ids", Batch(ragged(rng, 200, nnz), wide_ids, v()), 2, 2),
              ("keys_ready small", Batch(ragged(rng, 200, nnz), small_ids << np.uint64(30), v(),
                                         keys_ready=True), 2, 1),
              ("keys_ready wide", Batch(ragged(rng, 200, nnz), wide_ids, v(), keys_ready=True),
               2, 2)]
    for what, b, guess, form in firsts:
        with _ctxs(H, valued) as cs:
            # the launch's form: the host's guess, or the device's word when that came first
            run(H, cs, b, what, dict(hint2=form, q_lds=lambda q: q in (guess == 2, form == 2)))
    with _ctxs(H, valued) as cs:
        prev = None
        for i, wide in enumerate([False, True, True, False, True]):
            form = 2 if wide else 1
            ok = (lambda q, p=prev, f=form: q in (p == 2, f == 2)) if prev else (lambda q: True)
            run(H, cs, _form_batch(rng, wide, valued), ("switch", i, wide),
                dict(hint2=form, q_lds=ok))
            prev = form


# --------------------------------------------------------------------------------- key map
def _range_batch(rng, lo, hi, valued, nnz=3000, B=200):
    keys = np.uint64(lo) + rng.integers(0, hi - lo, nnz, dtype=np.uint64)
    return Batch(ragged(rng, B, nnz), ids_of(keys), vals_of(rng, nnz) if valued else None)


@pytest.mark.parametrize("valued", [False, True])
def test_key_map_follows_the_previous_batch(H, valued):
    """one context: pk_min / pk_max of a batch fit the next batch's bucket map (lb_map,
    locbucket.hip:117-134): the same range spreads; a range above clamps into the last bucket,
    one below (every key <= base) into the first; one distinct key (range 0, shift 0); the
    extreme keys together; max_index = 1000 with the all-ones id"""
    rng = np.random.default_rng(6)
    nnz = 3000
    v = (lambda n=nnz: vals_of(rng, n)) if valued else (lambda n=nnz: None)
    with _ctxs(H, valued) as cs:
        run(H, cs, _range_batch(rng, 1 << 40, 1 << 41, valued), "range, top-bit map",
            dict(lb_over=1, pk_valid=1))  # fresh: all keys share their top bits
        run(H, cs, _range_batch(rng, 1 << 40, 1 << 41, valued), "same range", dict(lb_over=0))
        run(H, cs, _range_batch(rng, 1 << 50, (1 << 50) + (1 << 41), valued), "above",
            dict(lb_over=1))
        run(H, cs, _range_batch(rng, 1 << 30, 1 << 31, valued), "below", dict(lb_over=1))
        run(H, cs, Batch(ragged(rng, 200, nnz), ids_of(np.full(nnz, 0x1234567890, np.uint64)),
                         v()), "one key", dict(lb_over=1), expect_all=dict(U=1, n_chunks=24))
        # (binary contexts now hold a hot-key map of that key; the rest must equal all the same)
        ext = np.where(rng.integers(0, 2, nnz) == 1, np.uint64(ALL), np.uint64(0))
        run(H, cs, Batch(ragged(rng, 200, nnz), ext, v(), keys_ready=True),
            "keys 0 and 2^64-1", dict(hint2=2), expect_all=dict(U=2))
        run(H, cs, Batch(ragged(rng, 200, nnz), np.where(ext == 0, np.uint64(0), np.uint64(ALL)),
                         v()), "ids 0 and all ones: key 0", expect_all=dict(U=1))
        ids = rng.integers(0, ALL, nnz, dtype=np.uint64)
        ids[::7] = np.uint64(ALL)
        run(H, cs, Batch(ragged(rng, 200, nnz), ids, v(), 1000), "max_index=1000, all-ones id",
            dict(hint2=1))
        run(H, cs, _range_batch(rng, 1 << 40, 1 << 41, valued), "the range again")


# ------------------------------------------------------------------------ rows and windows
def _w_cases(rng):
    """(name, lens) of the row shapes the scatter's windows meet (locbucket.hip:460-504)"""
    one = np.ones(3000, dtype=np.int64)
    gaps = np.zeros(900, dtype=np.int64)
    gaps[::90] = 300  # ten rows of 300 with runs of 89 empty rows between
    gaps[45] = 1
    longrow = np.ones(600, dtype=np.int64)
    longrow[150] = 9000  # more than a round of the largest block (8 * 1024 items)
    mixed = rng.integers(0, 3, 5000)  # empty, one, two: the next 64 rows start inside the window
    return [("one nnz per row", one), ("runs of empty rows", gaps),
            ("one long row among short", longrow), ("rows of 0-2", mixed)]


@pytest.mark.parametrize("valued", [False, True])
def test_row_windows(H, valued):
    """(W) rows of one nnz; runs of 64 and more empty rows; one row longer than a block's round
    among short ones; B = rt * ntiles exactly and one more"""
    rng = np.random.default_rng(7)
    cases = _w_cases(rng)
    for B in (1000, 1001):  # nnz = 9000: two tiles (locbucket.hip:1342); rt = 500 | 501
        lens = even(B, 9000)
        assert lb_tiles(B, 9000) == ((B + 1) // 2, 2)
        cases.append((("B", B), lens))
    for name, lens in cases:
        nnz = int(np.sum(lens))
        ids = rng.integers(0, 1 << 24, nnz, dtype=np.uint64)
        with _ctxs(H, valued, windows=True) as cs:
            run(H, cs, Batch(lens, ids, vals_of(rng, nnz) if valued else None), name,
                dict(lb_over=0, hint2=1))


@pytest.mark.parametrize("valued", [False, True])
def test_row_tile_cap(H, valued):
    """(W) B = 128 * 2048 + 1 rows of one nnz: rt hits kLbMaxRows (locbucket.hip:1343) and the
    tile count passes kLbTiles"""
    rng = np.random.default_rng(8)
    B = kLbTiles * kLbMaxRows + 1
    assert lb_tiles(B, B) == (kLbMaxRows, kLbTiles + 1)
    b = Batch(np.ones(B, dtype=np.int64), rng.integers(0, 1 << 24, B, dtype=np.uint64),
              vals_of(rng, B) if valued else None)
    kws = (BUCKET_VAL_W + RADIX_VAL[:1]) if valued else (BUCKET_BIN_W + RADIX_BIN[:1])
    with Ctxs(H, kws) as cs:
        run(H, cs, b, "tile cap", dict(rt=kLbMaxRows, ntiles=kLbTiles + 1, wbits=9, lb_over=0))


# ------------------------------------------------------------- long segments and the plan
def _seg_batch(rng, nnz, hot_bucket_total, hot_occ, valued, B=100):
    """nnz = 3000 | 4096 on fresh contexts: four buckets by key bits 63..62.  Bucket 1 holds
    hot_bucket_total items, hot_occ of them one key; the rest spread over the other buckets"""
    hot = np.uint64((1 << 62) | (5 << 50))
    n1 = hot_bucket_total - hot_occ
    near = (np.uint64(1 << 62) | (rng.integers(8, 1 << 11, n1, dtype=np.uint64) << np.uint64(50)))
    rest = nnz - hot_bucket_total
    oth = (rng.choice(np.array([0, 2, 3], dtype=np.uint64), rest) << np.uint64(62)) | \
        (rng.integers(0, 1 << 12, rest, dtype=np.uint64) << np.uint64(50))
    keys = np.concatenate([np.full(hot_occ, hot, np.uint64), near, oth])
    keys = keys[rng.permutation(nnz)]
    return Batch(ragged(rng, B, nnz), ids_of(keys), vals_of(rng, nnz) if valued else None)


@pytest.mark.parametrize("valued", [False, True])
def test_long_segment_gate(H, valued):
    """a key of kChunkOcc occurrences plans no chunk and leaves the gate shut; kChunkOcc + 1
    plans two (k_lb_wbucket's longseg, locbucket.hip:1035; k_loc_heads, localize.hip:167) — in a
    bucket the LDS sort takes and in an oversize one (the heads read from global memory)"""
    rng = np.random.default_rng(9)
    for nnz, total, over in ((3000, 700, 0), (4096, kLbCap + 52, 1)):
        for occ, nch in ((kChunkOcc, 0), (kChunkOcc + 1, 2)):
            b = _seg_batch(rng, nnz, total, occ, valued)
            assert int(b.ref()["cnt"].max()) == occ
            with _ctxs(H, valued) as cs:
                run(H, cs, b, ("long", nnz, occ), dict(lb_over=over, wbits=2),
                    expect_all=dict(n_chunks=nch, n_init=1 if nch else 0))


@pytest.mark.parametrize("valued", [False, True])
def test_chunk_table_block_wide_list(H, valued):
    """2048 occurrences: 16 chunks, written by the segment's own thread; 2049: 17, through
    k_chunk_write's block-wide list (localize.hip:317).  The key fills its bucket alone: exactly
    kLbCap (LDS sort) and kLbCap + 1 (oversize)"""
    rng = np.random.default_rng(10)
    for occ, nch, over in ((kLbCap, kListMin, 0), (kLbCap + 1, kListMin + 1, 1)):
        b = _seg_batch(rng, 4096, occ, occ, valued)
        with _ctxs(H, valued) as cs:
            run(H, cs, b, ("occ", occ), dict(lb_over=over), expect_all=dict(n_chunks=nch))


@pytest.mark.parametrize("valued", [False, True])
def test_chunk_list_overflows(H, valued):
    """~0.6 M nnz with 260 keys of 2100 occurrences (17 chunks each), the smallest keys of the
    batch, so one k_chunk_write tile lists more than its kList = 256 entries (localize.hip:295,
    319, 325); each hot key oversizes its own bucket (k_lb_big's looping blocks)"""
    rng = np.random.default_rng(11)
    nhot, occ, nnz = kList + 4, 2100, 600000
    assert lb_wbits(nnz) == 10
    hot = (np.arange(nhot, dtype=np.uint64) << np.uint64(54)) | np.uint64(1 << 30)
    fill = (rng.integers(nhot, 1 << 10, nnz - nhot * occ, dtype=np.uint64) << np.uint64(54)) | \
        (rng.integers(0, 1 << 20, nnz - nhot * occ, dtype=np.uint64) << np.uint64(30))
    keys = np.concatenate([np.repeat(hot, occ), fill])
    keys = keys[rng.permutation(nnz)]
    b = Batch(even(15000, nnz), ids_of(keys), vals_of(rng, nnz) if valued else None)
    assert np.all(b.ref()["cnt"][:nhot] == occ) and b.ref()["n_chunks"] >= nhot * 17
    kws = (BUCKET_VAL + RADIX_VAL[:1]) if valued else (BUCKET_BIN + RADIX_BIN[:1])
    with Ctxs(H, kws) as cs:
        run(H, cs, b, "260 hot keys", dict(lb_over=nhot, wbits=10))


# ------------------------------------------------------------------------------ hot-key map
def _hot_batch(rng, nnz, hots, valued=False, B=128, spread=None):
    """binary batch: `hots` = [(r, occurrences)] among fillers; keys are r << 44, r < 2^20.
    spread: the first hot key's occurrences split evenly over the two halves of the positions"""
    nh = sum(n for _, n in hots)
    fill = rng.integers(1, (1 << 20) - 1, nnz - nh, dtype=np.uint64)
    fill = fill[~np.isin(fill, [r for r, _ in hots])]
    fill = np.concatenate([fill, np.full(nnz - nh - len(fill), 7, np.uint64)])
    r = np.concatenate([np.full(n, k, np.uint64) for k, n in hots] + [fill])
    r = r[rng.permutation(nnz)]
    if spread:
        k, n = hots[0]
        cold = r[r != k]
        half = nnz // 2
        first = np.concatenate([np.full(n // 2, k, np.uint64), cold[:half - n // 2]])
        second = np.concatenate([np.full(n - n // 2, k, np.uint64), cold[half - n // 2:]])
        r = np.concatenate([first[rng.permutation(len(first))],
                            second[rng.permutation(len(second))]])
    return Batch(even(B, nnz), ids_of(r << np.uint64(44)),
                 vals_of(rng, nnz) if valued else None)


def test_hot_key_map(H):
    """binary batches of one context.  nnz = 4096 (the smallest wbits at which a map can exist:
    eight buckets allow one hot key, locbucket.hip:1193) and 8192 (sixteen: three).  A batch
    with a key of >= hot_th occurrences builds the map (hint[3]); the next is placed by it"""
    rng = np.random.default_rng(12)
    n4, n8 = 4096, 8192
    assert lb_hot_th(n4) == 512 and lb_hot_th(n8) == 512 and lb_wbits(n4) == 2
    K, KMIN, KMAX = 0x54321, 0, (1 << 20) - 1
    built = dict(hint3=1)
    by_map = dict(mapped=1, wbits=3)
    with Ctxs(H, [dict(loc_bucket=1), dict(loc_bucket=1, lb_hnt=256)] + RADIX_BIN[:1]) as cs:
        run(H, cs, _hot_batch(rng, n4, [(K, 1000)]), "first", dict(mapped=0, wbits=2, **built))
        run(H, cs, _hot_batch(rng, n4, [(K, 1000)]), "second", dict(**by_map, **built))
        run(H, cs, _hot_batch(rng, n4, [(K, 1000)]), "third", dict(**by_map, **built))
        run(H, cs, _hot_batch(rng, n4, []), "hot key absent", dict(hint3=0, **by_map))
        run(H, cs, _hot_batch(rng, n4, [(K, 1000)]), "again", dict(mapped=0, wbits=2, **built))
        run(H, cs, _hot_batch(rng, n4, [(K, 2000)]), "twice as frequent",
            dict(**by_map, **built))
        # a continued run: the map (W = 2 buckets for K) splits 200 occurrences by position into
        # parts of 100 <= kChunkOcc; only k_lb_bscan's continuation opens the plan's gate
        run(H, cs, _hot_batch(rng, n4, [(K, 200)], spread=True), "continued run",
            dict(hint3=0, **by_map), expect_all=dict(n_chunks=2, n_init=1))
        for name, k in (("smallest", KMIN), ("largest", KMAX)):
            run(H, cs, _hot_batch(rng, n4, [(k, 1000)]), (name, "builds"), built)
            run(H, cs, _hot_batch(rng, n4, [(k, 1000)]), (name, "placed"),
                dict(**by_map, **built))
        # a valued batch ignores the map (locbucket.hip:1333) and leaves it in place
    with Ctxs(H, [dict(loc_bucket=1, lb_gather=2)] + RADIX_BIN[:1]) as cs:
        run(H, cs, _hot_batch(rng, n4, [(K, 1000)]), "build", dict(mapped=0, **built))
        run(H, cs, _hot_batch(rng, n4, [(K, 900)], valued=True), "valued after a map",
            dict(mapped=0, wbits=2, hint3=1))
        run(H, cs, _hot_batch(rng, n4, [(K, 1000)]), "binary again", dict(**by_map, **built))
        # another size: the launch holds the map's LDS and one more bucket bit (:1335), but the
        # map was built for 2^3 buckets (lb_hot_on, :156): the key map places the batch
        run(H, cs, _hot_batch(rng, n8, [(K, 1000)]), "another wbits",
            dict(mapped=0, wbits=4, **built))
        run(H, cs, _hot_batch(rng, n8, [(K, 1000), (K + 1, 1000)]), "two hot keys, builds",
            dict(mapped=1, wbits=4, **built))
        run(H, cs, _hot_batch(rng, n8, [(K, 1000), (K + 1, 1000)]), "two adjacent, placed",
            dict(mapped=1, wbits=4, **built))
        run(H, cs, _hot_batch(rng, n8, [(K, 700), (K + 1, 700), (9, 700)]), "three: still on",
            dict(mapped=1, wbits=4, **built))
        # 2 * nh == nbk / 2 (:1193): four hot keys at sixteen buckets switch the map off
        run(H, cs, _hot_batch(rng, n8, [(K, 600), (K + 1, 600), (9, 600), (KMAX, 600)]),
            "four: off", dict(mapped=1, wbits=4, hint3=0))
        run(H, cs, _hot_batch(rng, n8, [(K, 1000)]), "after off", dict(mapped=0, wbits=3, **built))


def test_hot_list_overflows(H):
    """~2.2 M nnz with 1100 keys of more than hot_th occurrences: k_lb_hotlist counts past
    kLbHotMax (locbucket.hip:1169, 1193), no map is built and the next batch keeps the key map;
    1000 such keys fit, and the batch after them is placed by their map"""
    rng = np.random.default_rng(13)
    nnz, B = 2200000, 55000
    th = lb_hot_th(nnz)
    assert lb_wbits(nnz) == 12 and th == 268

    def batch(nhot):
        hot = (np.arange(nhot, dtype=np.uint64) * np.uint64(3) + np.uint64(1)) << np.uint64(52)
        nf = nnz - nhot * (th + 2)
        fill = (rng.integers(0, 1 << 24, nf, dtype=np.uint64) << np.uint64(40)) | \
            np.uint64(1 << 39)
        keys = np.concatenate([np.repeat(hot, th + 2), fill])
        b = Batch(even(B, nnz), ids_of(keys[rng.permutation(nnz)]))
        assert int(np.sum(b.ref()["cnt"] >= th)) == nhot
        return b

    with Ctxs(H, BUCKET_BIN + RADIX_BIN[:1]) as cs:
        over = batch(kLbHotMax + 76)
        run(H, cs, over, "1100 hot keys", dict(mapped=0, wbits=12, hint3=0, lb_over=0))
        run(H, cs, over, "again: the key map", dict(mapped=0, wbits=12, hint3=0, lb_over=0))
        fits = batch(kLbHotMax - 24)
        run(H, cs, fits, "1000 hot keys", dict(mapped=0, wbits=12, hint3=1))
        run(H, cs, fits, "placed by their map", dict(mapped=1, wbits=13, hint3=1))


# ----------------------------------------------------------------------------------- values
def test_value_bit_patterns(H):
    """-0.0, a subnormal, +-inf and NaN payloads among the values, carried bit for bit on every
    lb_gather and both sorts — through the LDS sort and, in the oversize bucket, k_lb_big"""
    rng = np.random.default_rng(14)
    b = _cap_batch(rng, (kLbCap + 52, kLbCap - 52, 0, 0), True, True)
    bits = b.vals.view(np.uint32)
    special = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001,
                        0xFFFFFFFF, 0x7F800001, 0x00000000], dtype=np.uint32)
    bits[::5] = np.resize(special, len(bits[::5]))
    with _ctxs(H, True) as cs:
        run(H, cs, b, "special values", dict(lb_over=1))
    b2 = Batch(even(64, b.nnz), rng.integers(0, ALL - 1, b.nnz, dtype=np.uint64), b.vals,
               keys_ready=True)  # 64-bit keys: unpacked items
    with _ctxs(H, True) as cs:
        run(H, cs, b2, "special values, unpacked", dict(hint2=2))


# ------------------------------------------------------------------------ split owner's form
@pytest.mark.parametrize("valued", [False, True])
def test_split_owner_form(H, valued):
    """keys_ready = 1 with full 64-bit keys (dfx_split_owner_begin's call, split.hip:474):
    twice on one context, so the second batch runs on a fitted map and the unpacked launch"""
    rng = np.random.default_rng(15)
    nnz = 5000
    with _ctxs(H, valued) as cs:
        for i in range(2):
            keys = rng.integers(0, ALL - 1, nnz, dtype=np.uint64)
            keys[::11] = keys[3]  # a segment of 455 occurrences: four chunks
            b = Batch(ragged(rng, 300, nnz), keys, vals_of(rng, nnz) if valued else None,
                      keys_ready=True)
            run(H, cs, b, ("owner", i), dict(hint2=2, wbits=lambda w: w in (3, 4)),
                expect_all=dict(n_chunks=4))
