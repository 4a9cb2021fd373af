"""A fresh negative down-sample per reshuffled epoch (dfx_reshuffle_begin_epoch_sampled in
difacto_amd/csrc/reshuffle.hip, hotpath.Reshuffler.begin_epoch_sampled, dfx_train
epoch_resample=1): a sampled epoch's batches equal tests/resample_ref.py's byte for byte (the
permuted order filtered by the keyed draw on the source row, cut every batch_rows kept rows),
at the sizes where the compaction's scan changes shape; K = 0, K below and at a multiple of
batch_rows; neg_sampling 1 is dfx_reshuffle_begin_epoch bit for bit; scratch that does not fit
is reported and not an error; misuse is DFX_ERR_ARG; training through a sampled reshuffler
equals training on the reference's batches bit for bit; and the driver's option gives every
epoch its own sample, reproducibly.  Every comparison is array_equal or equality of doubles."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from tests import reshuffle_ref as R
from tests import resample_ref as S
import tests.test_gpu_batchcache as BC
import tests.test_gpu_reshuffle as G

pytestmark = pytest.mark.gpu

TILE = 2048  # kTile of reshuffle.hip: positions per block of the compaction's scan
RATES = (0.25, 0.9)
KEYS = (R.epoch_key(0, 1, 0), 3)


@pytest.fixture(scope="module")
def ctx():
    from difacto_amd import hotpath as H
    c = H.Context(0, V_dim=0, max_keys=1 << 12)
    yield c
    c.close()


def _sources(N, kind, seed):
    """a list of N rows as source batches of 1, 7, 64 and 65 rows in turn (the last one cut to
    fit), an empty batch after the second, rows of 0..8 ids (so some are empty)"""
    rng = np.random.default_rng(seed)
    blks, left, i = [], N, 0
    while left > 0:
        n = min((1, 7, 64, 65)[i % 4], left)
        valued = kind == "valued" or (kind == "mixed" and i % 2 == 1)
        weighted = kind == "valued" or (kind == "mixed" and i % 3 == 0)
        blks.append(G._blk(rng.integers(0, 9, size=n), seed * 1000 + i, valued=valued,
                           weighted=weighted))
        left -= n
        i += 1
        if i == 2:
            blks.append(G._blk([], seed * 1000 + 999))
    return blks


def _assert_sampled_epoch(rs, key, ns, want, where):
    nb, rows = rs.begin_epoch_sampled(key, ns)
    assert (nb, rows) == (len(want), sum(len(w["labels"]) for w in want)), where
    for i, w in enumerate(want):
        b = rs.next()
        assert b is not None, (where, i)
        G._assert_batch(b, w, (where, i))
        rs.consumed()
    assert rs.next() is None and rs.next() is None, where


SIZES = (1, 2, 63, 64, 65, 1000, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


@pytest.mark.parametrize("kind", ["binary", "valued", "mixed"])
@pytest.mark.parametrize("N", SIZES)
def test_sampled_batches_equal_the_reference(ctx, N, kind):
    from difacto_amd import hotpath as H
    blks = _sources(N, kind, 7 + N % 5)
    assert sum(b.size for b in blks) == N
    bc = G._record(H, ctx, blks)
    # batch_rows 1, 7, 64 and N at every size.  Small batch_rows at a large N hand out
    # hundreds of batches, each checked from Python, so there they run fewer of the four
    # (rate, key) pairs; batch_rows 1 above 65 rows runs at one size only, a tile and a row
    # (many of the per-batch scan's blocks then lie past K)
    rows_list = (1, 7, 64, N) if N <= 65 or N == TILE + 1 else (7, 64, N)
    seen = set()
    for batch_rows in sorted(set(rows_list)):
        rs = H.Reshuffler(bc, 0, batch_rows, 2 + batch_rows % 3)
        assert rs.kept
        pairs = [(ns, key) for ns in RATES for key in KEYS]
        if N > 65 and batch_rows == 1:
            pairs = pairs[3:]
        elif N > 1000 and batch_rows == 7:
            pairs = pairs[0::3]
        for ns, key in pairs:
            want = S.resample(blks, batch_rows, key, ns)
            K = sum(len(w["labels"]) for w in want)
            assert len(want) == -(-K // batch_rows) and K <= N
            _assert_sampled_epoch(rs, key, ns, want, (N, kind, batch_rows, ns, key))
            seen.add((ns, key, K))
        st = rs.stats()
        assert st["rows"] == N and st["batches"] == -(-N // min(batch_rows, N))
        rs.close()
    if N >= 63:  # the two keys keep other rows, the two rates other counts
        assert len({k for _, _, k in seen}) >= 2, seen
    for i, blk in enumerate(blks):  # after these epochs the sources are the bytes they were
        BC._assert_holds(bc.get(0, i), blk)
    bc.close()


def test_more_tiles_than_one_round_of_the_tile_scan(ctx):
    """N = 2048 * 2048 + 5 one-id rows: 2049 tiles, so k_rs_tiles, one block that scans 2048
    tiles a round, takes a second round with a carry, and the per-batch scan walks 2^20 rows a
    block.  The reference is resample_ref.kept_rows, compared a batch at a time as arrays"""
    from difacto_amd import hotpath as H
    N, batch_rows = TILE * TILE + 5, 1 << 20
    blks = [G._blk(np.ones(n, np.int64), 500 + i) for i, n in enumerate((N - 70000, 70000))]
    ids = np.concatenate([b.ids for b in blks])
    labels = np.concatenate([b.labels for b in blks])
    bc = G._record(H, ctx, blks, budget=1 << 30, block=1 << 26)
    rs = H.Reshuffler(bc, 0, batch_rows, 2)
    assert rs.kept
    for ns, key in ((0.25, 21), (0.9, 22)):
        keep = S.kept_rows(blks, key, ns)
        K = len(keep)
        assert TILE * TILE * (1 - ns) * .6 < K < N
        assert rs.begin_epoch_sampled(key, ns) == (-(-K // batch_rows), K)
        for k0 in range(0, K, batch_rows):
            rows = keep[k0:k0 + batch_rows]
            b = rs.next()
            a = b.arrays()
            assert b.size == b.nnz == len(rows), (key, k0)
            assert np.array_equal(a["offs"], np.arange(len(rows) + 1, dtype=np.uint64)), (key, k0)
            assert np.array_equal(a["ids"], ids[rows]), (key, k0)
            assert np.array_equal(a["labels"], labels[rows]), (key, k0)
            assert a["vals"] is None and a["weights"] is None
            rs.consumed()
        assert rs.next() is None
    rs.close()
    bc.close()


def _labelled(lens, seed, labels):
    b = G._blk(lens, seed)
    b.labels[:] = labels
    return b


def test_edge_counts_of_kept_rows(ctx):
    from difacto_amd import hotpath as H
    rng = np.random.default_rng(3)
    blks = [G._blk(rng.integers(0, 6, size=n), 200 + n) for n in (120, 80)]
    bc = G._record(H, ctx, blks)
    # K an exact multiple of batch_rows: a key picked from the reference
    key = next(k for k in range(1, 200) if len(S.kept_rows(blks, k, 0.25)) % 10 == 0)
    want = S.resample(blks, 10, key, 0.25)
    assert all(len(w["labels"]) == 10 for w in want) and 10 < len(want) < 20
    rs = H.Reshuffler(bc, 0, 10, 2)
    _assert_sampled_epoch(rs, key, 0.25, want, "multiple")
    rs.close()
    # K < batch_rows: one short batch
    rs = H.Reshuffler(bc, 0, 200, 2)
    want = S.resample(blks, 200, 5, 0.9)
    assert len(want) == 1 and 0 < len(want[0]["labels"]) < 200
    _assert_sampled_epoch(rs, 5, 0.9, want, "short")
    rs.close()
    bc.close()
    # K = 0: three negative rows, neg_sampling 0.9, key 0 -- numpy says all three are dropped
    neg = _labelled([2, 0, 5], 210, -1)
    assert S.dropped(0, np.arange(3), neg.labels, 0.9).all()
    assert S.resample([neg], 2, 0, 0.9) == []
    bc = G._record(H, ctx, [neg])
    rs = H.Reshuffler(bc, 0, 2, 2)
    assert rs.begin_epoch_sampled(0, 0.9) == (0, 0)
    assert rs.next() is None and rs.next() is None
    G._assert_epoch(rs, (0, R.reshuffle([neg], 2, 0)), "plain after K = 0")
    key = next(k for k in range(1, 50) if len(S.kept_rows([neg], k, 0.9)))
    _assert_sampled_epoch(rs, key, 0.9, S.resample([neg], 2, key, 0.9), "some key keeps a row")
    rs.close()
    bc.close()
    # an all-positive list: nothing is dropped at any rate
    pos = [_labelled(rng.integers(0, 6, size=n), 220 + n, 1) for n in (70, 30)]
    bc = G._record(H, ctx, pos)
    rs = H.Reshuffler(bc, 0, 32, 2)
    for ns in (0.0, 0.25, 0.9):
        want = R.reshuffle(pos, 32, 9)
        assert sum(len(w["labels"]) for w in want) == 100
        _assert_sampled_epoch(rs, 9, ns, want, ("positive", ns))
    rs.close()
    bc.close()


def _collect(rs, n):
    out = []
    for _ in range(n):
        b = rs.next()
        out.append((b.size, b.nnz, b.arrays()))
        rs.consumed()
    assert rs.next() is None
    return out


def test_neg_sampling_one_is_begin_epoch_bit_for_bit(ctx):
    from difacto_amd import hotpath as H
    rng = np.random.default_rng(4)
    blks = [G._blk(rng.integers(0, 9, size=n), 300 + n, valued=n == 65, weighted=n == 7)
            for n in (7, 2100, 65)]
    N = sum(b.size for b in blks)
    bc = G._record(H, ctx, blks)
    rs = H.Reshuffler(bc, 0, 100, 3)
    nb = -(-N // 100)
    for key in KEYS:
        assert rs.begin_epoch(key) == nb
        plain = _collect(rs, nb)
        for ns in (1.0, 2.5, float("inf")):
            assert rs.begin_epoch_sampled(key, ns) == (nb, N)
            sampled = _collect(rs, nb)
            for p, s in zip(plain, sampled):
                assert p[:2] == s[:2]
                for k in G.NAMES:
                    assert (p[2][k] is None) == (s[2][k] is None)
                    assert p[2][k] is None or p[2][k].tobytes() == s[2][k].tobytes(), k
    # a sampled epoch, then a plain one, then a sampled one: each is still right
    _assert_sampled_epoch(rs, 11, 0.25, S.resample(blks, 100, 11, 0.25), "sampled")
    G._assert_epoch(rs, (11, R.reshuffle(blks, 100, 11)), "plain after sampled")
    _assert_sampled_epoch(rs, 12, 0.9, S.resample(blks, 100, 12, 0.9), "sampled again")
    rs.close()
    bc.close()


def test_scratch_that_does_not_fit_is_reported(ctx):
    """a budget that holds the list, the table, the scratch and the ring, and 256 bytes more:
    the compacted arrays (8 bytes a row) do not fit -> n_batches = -1 with DFX_OK, nothing is
    taken, the cache is untouched and a plain epoch still works"""
    from difacto_amd import hotpath as H
    blk = G._blk([1] * 2000, 400)
    bc = G._record(H, ctx, [blk])
    rs = H.Reshuffler(bc, 0, 100, 2)
    with_rs = bc.stats()["bytes"]
    scratch = rs.stats()["scratch_bytes"]
    assert rs.begin_epoch_sampled(1, 0.5)[0] == len(S.resample([blk], 100, 1, 0.5))
    grown = rs.stats()["scratch_bytes"] - scratch
    assert grown >= 2000 * 8 and grown % 256 == 0     # counted once they are allocated
    assert bc.stats()["bytes"] == with_rs + grown
    rs.close()
    bc.close()
    bc = G._record(H, ctx, [blk], budget=with_rs + 256)
    rs = H.Reshuffler(bc, 0, 100, 2)
    assert rs.kept and bc.stats()["bytes"] == with_rs
    assert rs.begin_epoch_sampled(1, 0.5) == (-1, 0)
    assert bc.stats()["bytes"] == with_rs and rs.stats()["scratch_bytes"] == scratch
    BC._arg_error(rs.next)                             # no epoch is open
    BC._assert_holds(bc.get(0, 0), blk)
    G._assert_epoch(rs, (1, R.reshuffle([blk], 100, 1)), "plain")
    assert rs.begin_epoch_sampled(2, 0.5) == (-1, 0)   # asked again: the same answer
    rs.close()
    bc.close()


def test_misuse_is_err_arg(ctx):
    from difacto_amd import _lib
    from difacto_amd import hotpath as H
    blk = G._blk([2, 1, 4, 0, 3], 410)
    bc = G._record(H, ctx, [blk])
    rs = H.Reshuffler(bc, 0, 2, 2)
    f = _lib.lib().dfx_reshuffle_begin_epoch_sampled
    n, r = ctypes.c_int64(7), ctypes.c_int64(7)
    half = ctypes.c_float(0.5)
    held = bc.stats()["bytes"]
    assert f(None, 0, half, ctypes.byref(n), ctypes.byref(r)) == 1
    assert f(rs.h, 0, half, None, ctypes.byref(r)) == 1
    assert f(rs.h, 0, half, ctypes.byref(n), None) == 1
    assert b"null" in _lib.lib().dfx_last_error()
    BC._arg_error(rs.begin_epoch_sampled, 0, float("nan"))
    BC._arg_error(rs.begin_epoch_sampled, 0, -0.25)
    BC._arg_error(rs.begin_epoch_sampled, 0, float("-inf"))
    assert (n.value, r.value) == (7, 7) and bc.stats()["bytes"] == held   # nothing was taken
    BC._arg_error(rs.next)                             # a rejected call opens no epoch
    # ... and leaves an open one as it was
    want = S.resample([blk], 2, 6, 0.25)
    nb, rows = rs.begin_epoch_sampled(6, 0.25)
    assert nb == len(want) >= 1
    BC._arg_error(rs.begin_epoch_sampled, 0, float("nan"))
    BC._arg_error(rs.consumed)                         # consumed with no batch handed out
    for i, w in enumerate(want):
        G._assert_batch(rs.next(), w, i)
        rs.consumed()
        BC._arg_error(rs.consumed)
    assert rs.next() is None
    rs.close()
    bc.close()


@pytest.mark.parametrize("case", ["fm16", "logit_valued"])
def test_training_through_a_sampled_reshuffler_equals_the_reference_batches(case):
    """context A steps three epochs through a sampled reshuffler over its cached list; a fresh
    context B steps over resample_ref's batches uploaded as plain tensors: equal progress
    (doubles), seed, key count and pulls"""
    from difacto_amd import data as D
    from difacto_amd import hotpath as H
    if case == "fm16":
        cfg = dict(V_dim=16, V_threshold=0, l1=0, lr=.1, V_lr=.01, max_keys=1 << 16)
        blks = [D.synthetic(500, 10, 1 << 12, seed=190 + i) for i in range(4)]
    else:
        cfg = dict(V_dim=0, l1=0, lr=.1, max_keys=1 << 16)
        blks = [D.synthetic(500, 10, 1 << 12, seed=195 + i, binary=False, ragged=True)
                for i in range(4)]
    labels = np.concatenate([b.labels for b in blks])
    assert 200 < np.count_nonzero(labels <= 0) < 1800     # both classes: some rows are dropped
    A, B = H.Context(0, **cfg), H.Context(0, **cfg)
    bc = G._record(H, A, blks)
    rs = H.Reshuffler(bc, 0, 300, 3)
    kept = []
    for epoch in range(3):
        key = R.epoch_key(9, epoch, 0)
        want = S.resample(blks, 300, key, 0.5)
        K = sum(len(w["labels"]) for w in want)
        kept.append(K)
        assert rs.begin_epoch_sampled(key, 0.5) == (len(want), K)
        for w in want:
            H.train_step(A, rs.next(), H.kTraining, push_cnt=(epoch == 0))
            rs.consumed()
            wb = D.RowBlock(w["offs"], w["ids"], w["vals"], w["labels"], w["weights"])
            H.train_step(B, H.DeviceRowBlock(B, wb), H.kTraining, push_cnt=(epoch == 0))
        assert rs.next() is None
        pa, pb = H.progress(A), H.progress(B)
        assert pa["nrows"] == pb["nrows"] == K < 2000
        assert pa["loss"] == pb["loss"] and pa["auc"] == pb["auc"], (epoch, pa, pb)
        sa, sb = H.Store(A).stats(), H.Store(B).stats()
        assert sa["seed"] == sb["seed"] and sa["n_keys"] == sb["n_keys"] > 0, (epoch, sa, sb)
    assert len(set(kept)) > 1, kept                        # every epoch its own sample
    _, uniq, _ = H.Localizer(A).compact(H.DeviceRowBlock(A, D.concat(blks)), want_cnt=False)
    (va, la), (vb, lb) = H.Store(A).pull(uniq), H.Store(B).pull(uniq)
    assert va.cpu().numpy().tobytes() == vb.cpu().numpy().tobytes()
    assert (la is None) == (lb is None)
    if la is not None:
        assert la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes()
    rs.close()
    bc.close()
    A.close()
    B.close()


# ---- the driver -----------------------------------------------------------------------------
CFG = dict(V_dim=4, V_threshold=1, max_keys=262144)
NS = 0.5
KW = ["batch_size=256", "num_jobs_per_epoch=4", "max_num_epochs=3", "stop_rel_objv=0",
      "shuffle=0", "neg_sampling=%g" % NS, "data_format=criteo", "has_aux=1", "cache=device",
      "epoch_shuffle=1", "epoch_resample=1"] + ["%s=%s" % kv for kv in CFG.items()]
EPOCH_LINE = r"^  epoch_resample: (\d+) of (\d+) rows kept in (\d+) parts(.*)$"


def _stable(out):
    """a run's lines without what a clock decides: the rates and seconds in parentheses at the
    end of a line, the line of the host's waits"""
    return [re.sub(r"  \(.*\)$", "", l) for l in out.splitlines()
            if "the host waited" not in l and not l.startswith("  reader:")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """4,000 generated Criteo rows; the runs of dfx_train the tests below compare"""
    d = tmp_path_factory.mktemp("rsm")
    path = str(d / "c.txt")
    subprocess.check_call([BC.GEN_BIN, path, "4000", "65536", "0"])
    outs = {}
    for name, extra in (("a", []), ("b", []), ("seed7", ["shuffle_seed=7"]),
                        ("device_parse", ["parse=auto"]), ("small", ["cache_mb=200"])):
        outs[name] = BC._train(["data_in=" + path, "model_out=" + str(d / ("m_" + name))]
                               + KW + extra)
    return path, d, outs


@pytest.fixture(scope="module")
def reference(driver):
    """the parts' recorded lists (file order, 256 rows a batch) and, per seed, hotpath stepped
    over resample_ref's batches of every epoch: the Training lines, the rows kept per epoch and
    part, the saved model"""
    from difacto_amd import data as D
    from difacto_amd import hotpath as H
    path, d, _ = driver
    ctx = H.Context(0, V_dim=0, max_keys=1 << 12)
    parts = [H.parse_criteo(ctx, p)[0] for p in G._parts(open(path, "rb").read(), 4)]
    ctx.close()
    assert sum(p.size for p in parts) == 4000
    lists = [[p.slice(i, min(i + 256, p.size)) for i in range(0, p.size, 256)] for p in parts]
    out = {"parts": parts}
    for seed in (0, 7):
        c = H.Context(0, **CFG)
        lines, kept = [], []
        for epoch in range(3):
            tot = {"nrows": 0., "loss": 0., "auc": 0.}
            kept.append([])
            for part, recorded in enumerate(lists):
                want = S.resample(recorded, 256, R.epoch_key(seed, epoch, part), NS)
                kept[-1].append(sum(len(w["labels"]) for w in want))
                for w in want:
                    b = D.RowBlock(w["offs"], w["ids"], w["vals"], w["labels"])
                    H.train_step(c, H.DeviceRowBlock(c, b), H.kTraining, push_cnt=(epoch == 0))
                p = H.progress(c)
                for k in tot:
                    tot[k] += p[k]
            lines.append("Rows = %.0f, loss = %.9g, AUC = %.9g"
                         % (tot["nrows"], tot["loss"] / tot["nrows"], tot["auc"] / tot["nrows"]))
        model = str(d / ("ref_%d" % seed))
        H.Store(c).save(model, True)
        c.close()
        out[seed] = (lines, kept, model)
    return out


def test_driver_is_reproducible_and_every_epoch_has_its_own_sample(driver, reference):
    path, d, outs = driver
    assert _stable(outs["a"]) == _stable(outs["b"]) != _stable(outs["seed7"])
    assert len(_stable(outs["a"])) >= 3 + 3 + 3
    f = {k: BC._fields(v, "Training") for k, v in outs.items()}
    print(f)
    assert all(len(v) == 3 for v in f.values())
    assert f["a"] == f["b"] and f["a"] == f["device_parse"]
    assert all(x != y for x, y in zip(f["a"], f["seed7"]))       # another seed, another run
    # the same model: the same keys with bit-equal entries (a model file lists the entries in
    # the table's slot order, which is not part of the contract)
    from difacto_amd import data as D
    from oracle import oracle as O
    keys = O.localize(*[getattr(D.concat(reference["parts"]), n) for n in ("offs", "ids")])[0]
    kw = {k: CFG[k] for k in ("V_dim", "V_threshold")}
    n, size = BC._assert_models_equal(str(d / "m_a_part-0"), str(d / "m_b_part-0"), keys, **kw)
    assert n == size
    with pytest.raises(AssertionError):
        BC._assert_models_equal(str(d / "m_a_part-0"), str(d / "m_seed7_part-0"), keys, **kw)
    for name, seed in (("a", 0), ("seed7", 7), ("device_parse", 0)):
        m = re.findall(EPOCH_LINE, outs[name], re.M)
        kept = reference[seed][1]
        assert [(int(a), int(b), int(c), t) for a, b, c, t in m] == \
            [(sum(k), 4000, 4, "") for k in kept], (name, m, kept)
        assert len({sum(k) for k in kept}) == 3, kept           # per-epoch K varies
        one = re.findall(r"^epoch_resample=1: (\d+) of (\d+) training parts resample", outs[name],
                         re.M)
        assert one == [("4", "4")], outs[name]
        assert outs[name].index("cache=device:") < outs[name].index("epoch_resample=1:")
        assert "read through" not in outs[name]
    rows = [l.split(",")[0] for l in f["a"]]
    assert rows == ["Rows = %d" % sum(k) for k in reference[0][1]]
    assert all(sum(k) < 4000 for k in reference[0][1])


def test_driver_lines_and_model_equal_hotpath_on_the_reference_batches(driver, reference):
    from difacto_amd import data as D
    from oracle import oracle as O
    path, d, outs = driver
    keys = O.localize(*[getattr(D.concat(reference["parts"]), n) for n in ("offs", "ids")])[0]
    for name, seed in (("a", 0), ("seed7", 7), ("device_parse", 0)):
        lines, _, model = reference[seed]
        assert lines == BC._fields(outs[name], "Training"), (name, lines)
        n, size = BC._assert_models_equal(str(d / ("m_%s_part-0" % name)), model, keys, **{
            k: CFG[k] for k in ("V_dim", "V_threshold")})
        assert n == size


def test_driver_reads_a_part_that_does_not_fit_through_its_reader(driver, reference):
    """cache_mb=200 holds three of the four parts' 64 MiB blocks: part 3 is read through its
    reader, with the reader's own sample, in every epoch, and the run says so"""
    path, d, outs = driver
    out = outs["small"]
    assert BC._cache_line(out)[2:] == (1, 4)
    assert re.findall(r"^epoch_resample=1: (\d+) of (\d+) training parts resample.*, 1 read "
                      r"through its reader", out, re.M) == [("3", "4")], out
    m = re.findall(EPOCH_LINE, out, re.M)
    kept = reference[0][1]
    held = sum(p.size for p in reference["parts"][:3])
    assert [(int(a), int(b), int(c), t) for a, b, c, t in m] == \
        [(sum(k[:3]), held, 3, ", 1 part read through its reader") for k in kept], (m, kept)
    rows = [int(l.split(",")[0].split("= ")[1]) for l in BC._fields(out, "Training")]
    # part 3's rows come from the reader: the same sample in every epoch
    extra = {r - sum(k[:3]) for r, k in zip(rows, kept)}
    assert len(extra) == 1 and 0 < extra.pop() < reference["parts"][3].size, (rows, kept)


def test_driver_refusals():
    for args, text in (
            (["epoch_resample=1", "cache=device", "neg_sampling=0.5"],
             "epoch_resample=1 needs epoch_shuffle=1 (the rows are drawn out of the reshuffled "
             "cache)"),
            (["epoch_resample=1", "epoch_shuffle=1", "cache=device"],
             "epoch_resample=1 needs neg_sampling < 1")):
        r = subprocess.run([BC.TRAIN_BIN, "data_in=/nonexistent"] + args, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode == 2 and r.stderr.strip() == text, (r.returncode, r.stderr)
