"""The device reshuffler (difacto_amd/csrc/reshuffle.hip, hotpath.Reshuffler, dfx_train
epoch_shuffle=1): a reshuffled epoch's batches equal tests/reshuffle_ref.py's byte for byte,
the ring is reused and regrown, the cached sources stay the bytes they were, training through a
reshuffler equals training on the reference's batches bit for bit, what does not fit the budget
is reported and not an error, misuse is DFX_ERR_ARG, and the driver's option reshuffles the
later epochs reproducibly.  Every comparison is array_equal or equality of doubles: the
reference is exact, so none has a tolerance."""
import ctypes

import numpy as np
import pytest

from tests import reshuffle_ref as R
import tests.test_gpu_batchcache as BC

pytestmark = pytest.mark.gpu

NAMES = ("offs", "ids", "vals", "labels", "weights")
BLOCK = 4096


def _blk(lens, seed, valued=False, weighted=False):
    """a RowBlock of the given row lengths; a block with no ids is never valued (its value
    tensor would be empty, i.e. a NULL pointer, on the device)"""
    lens = np.asarray(lens, np.int64)
    return BC._block(lens, seed, valued=valued and lens.sum() > 0,
                     weighted=weighted and len(lens) > 0)


def _record(H, ctx, blks, budget=1 << 26, list_id=0, block=BLOCK):
    bc = H.BatchCache(ctx, budget, block)
    bc.begin(list_id)
    for b in blks:
        assert bc.append(H.DeviceRowBlock(ctx, b))
    assert bc.seal() == len(blks)
    return bc


def _assert_batch(got, want, where):
    a = got.arrays()
    B = len(want["labels"])
    assert got.size == B and got.nnz == len(want["ids"]), where
    for k in NAMES:
        assert (a[k] is None) == (want[k] is None), (where, k)
        if want[k] is not None:
            assert a[k].dtype == want[k].dtype and np.array_equal(a[k], want[k]), (where, k)
    assert a["offs"][0] == 0 and got.nnz == int(a["offs"][B]), where
    for k, p in got.pointers().items():
        assert p is None or p % 256 == 0, (where, k, p)


def _assert_epoch(rs, want, where=""):
    assert rs.begin_epoch(want[0]) == len(want[1]), where
    for i, w in enumerate(want[1]):
        b = rs.next()
        assert b is not None, (where, i)
        _assert_batch(b, w, (where, i))
        rs.consumed()
    assert rs.next() is None and rs.next() is None, where


@pytest.fixture(scope="module")
def ctx():
    from difacto_amd import hotpath as H
    c = H.Context(0, V_dim=0, max_keys=1 << 12)
    yield c
    c.close()


def _lists():
    rng = np.random.default_rng(5)
    ragged = lambda n: rng.integers(0, 9, size=n)  # noqa: E731
    long_rows = np.array([1, 64, 65, 129, 1000, 0, 3], np.int64)
    sizes = [ragged(1), ragged(7), ragged(64), [], ragged(65),
             np.concatenate([ragged(400), np.zeros(70, np.int64), long_rows, ragged(523)])]
    assert [len(s) for s in sizes] == [1, 7, 64, 0, 65, 1000]
    out = {}
    # (blocks, batch_rows, nring)
    out["sizes_binary"] = ([_blk(s, 10 + i) for i, s in enumerate(sizes)], 100, 3)
    out["sizes_valued"] = ([_blk(s, 20 + i, valued=True, weighted=True)
                            for i, s in enumerate(sizes)], 64, 2)
    out["mixed_values"] = ([_blk(s, 30 + i, valued=i % 2 == 1) for i, s in enumerate(sizes)],
                           65, 4)
    out["some_weights"] = ([_blk(s, 40 + i, weighted=i in (1, 5)) for i, s in enumerate(sizes)],
                           257, 2)
    out["one_row"] = ([_blk([3], 50)], 1, 2)
    out["fewer_rows_than_a_batch"] = ([_blk([2, 0, 5], 51, valued=True)], 5, 2)
    out["all_rows_empty"] = ([_blk([0] * 70, 52), _blk([0] * 3, 53)], 16, 2)
    out["three_batches_exactly"] = ([_blk(ragged(100), 54), _blk(ragged(50), 55)], 50, 2)
    out["three_batches_and_one"] = ([_blk(ragged(100), 56), _blk(ragged(51), 57)], 50, 2)
    out["crosses_bit_widths"] = ([_blk([1] * 65000, 58), _blk([1] * 537, 59)], 20000, 2)
    return out


LISTS = _lists()


@pytest.mark.parametrize("name", sorted(LISTS))
def test_reshuffled_batches_equal_the_reference(ctx, name):
    from difacto_amd import hotpath as H
    blks, batch_rows, nring = LISTS[name]
    bc = _record(H, ctx, blks)
    rs = H.Reshuffler(bc, 0, batch_rows, nring)
    assert rs.kept
    N = sum(b.size for b in blks)
    for key in (R.epoch_key(0, 1, 0), 3):
        want = R.reshuffle(blks, batch_rows, key)
        assert len(want) == -(-N // batch_rows)
        _assert_epoch(rs, (key, want), (name, key))
    st = rs.stats()
    assert st["rows"] == N and st["batches"] == -(-N // batch_rows)
    rs.close()
    bc.close()


def test_ring_entries_are_reused(ctx):
    """nring = 2 and 7 output batches: a batch is checked when it is handed out, and its ring
    entry holds the batch two further on after consumed and two more next calls"""
    from difacto_amd import hotpath as H
    rng = np.random.default_rng(6)
    blks = [_blk(rng.integers(0, 12, size=n), 60 + n, valued=True) for n in (150, 155)]
    bc = _record(H, ctx, blks)
    rs = H.Reshuffler(bc, 0, 50, 2)
    want = R.reshuffle(blks, 50, 11)
    assert len(want) == 7 and rs.begin_epoch(11) == 7
    got = []
    for i in range(7):
        got.append(rs.next())
        _assert_batch(got[i], want[i], i)
        rs.consumed()
        if i >= 2:
            assert got[i].pointers() == got[i - 2].pointers()
            assert got[i].pointers() != got[i - 1].pointers()
            # the entry batch i - 2 was in now holds batch i, and still does after consumed
            _assert_batch(got[i], want[i], ("again", i))
            old = got[i - 2].arrays()
            n = min(got[i - 2].size, got[i].size)
            assert np.array_equal(old["labels"][:n], want[i]["labels"][:n])
            assert np.array_equal(old["offs"][:n + 1], want[i]["offs"][:n + 1])
    rs.close()
    bc.close()


def test_keys_and_read_only_sources(ctx):
    from difacto_amd import hotpath as H
    rng = np.random.default_rng(7)
    blks = [_blk(rng.integers(0, 6, size=n), 70 + n, valued=n == 90, weighted=n == 40)
            for n in (40, 90, 33)]
    bc = _record(H, ctx, blks)
    rs = H.Reshuffler(bc, 0, 32, 2)

    def epoch(key):
        out = []
        assert rs.begin_epoch(key) == 6
        for _ in range(6):
            out.append(rs.next().arrays())
            rs.consumed()
        return out

    a, b, c = epoch(5), epoch(5), epoch(6)
    for x, y in zip(a, b):
        for k in NAMES:
            assert np.array_equal(x[k], y[k]), k
    assert any(not np.array_equal(x["ids"], y["ids"]) for x, y in zip(a, c))
    for i, blk in enumerate(blks):  # the cached sources are the bytes they were
        BC._assert_holds(bc.get(0, i), blk)
    rs.close()
    bc.close()


def _long_row_keys():
    """2000 rows of one id but rows 700 and 1500 of 5000; two keys, picked from the reference:
    the first sends the long rows to different batches of 300, the second to one batch"""
    lens = np.ones(2000, np.int64)
    lens[[700, 1500]] = 5000
    apart = together = None
    for key in range(1, 400):
        p = R.perm(2000, key).astype(np.int64)
        where = np.argsort(p)[[700, 1500]] // 300  # the output batches of rows 700 and 1500
        if where[0] != where[1] and apart is None:
            apart = key
        if where[0] == where[1] and together is None:
            together = key
        if apart is not None and together is not None:
            return lens, apart, together
    raise AssertionError("no such keys below 400")


def test_ring_grows_for_a_larger_batch(ctx):
    from difacto_amd import hotpath as H
    lens, apart, together = _long_row_keys()
    blks = [_blk(lens[:1200], 80), _blk(lens[1200:], 81)]
    bc = _record(H, ctx, blks)
    rs = H.Reshuffler(bc, 0, 300, 2)
    first, second = R.reshuffle(blks, 300, apart), R.reshuffle(blks, 300, together)
    big = [max(len(b["ids"]) for b in e) for e in (first, second)]
    assert big[0] < 5300 < 10000 <= big[1]
    _assert_epoch(rs, (apart, first), "apart")
    ring0 = rs.stats()["ring_bytes"]
    _assert_epoch(rs, (together, second), "together")
    assert rs.stats()["ring_bytes"] > ring0 >= 2 * big[0] * 8
    _assert_epoch(rs, (apart, first), "apart again")
    rs.close()
    bc.close()


@pytest.mark.parametrize("case", ["fm16_chunked", "logit_valued"])
def test_training_through_a_reshuffler_equals_the_reference_batches(case):
    """context A steps three epochs through a reshuffler over its cached list; a fresh context
    B steps over reshuffle_ref's batches uploaded as plain tensors: equal progress (doubles),
    seed, key count and pulls"""
    from difacto_amd import data as D
    from difacto_amd import hotpath as H
    if case == "fm16_chunked":
        cfg = dict(V_dim=16, V_threshold=0, l1=0, lr=.1, V_lr=.01, max_keys=1 << 16)
        blks = [D.synthetic(500, 10, 1 << 12, seed=90 + i) for i in range(4)]
        for b in blks:
            b.ids[::10] = 7  # one key in every row: 300 occurrences a batch, the chunk plan
    else:
        cfg = dict(V_dim=0, l1=0, lr=.1, max_keys=1 << 16)
        blks = [D.synthetic(500, 10, 1 << 12, seed=95 + i, binary=False, ragged=True)
                for i in range(4)]
    A, B = H.Context(0, **cfg), H.Context(0, **cfg)
    bc = _record(H, A, blks)
    rs = H.Reshuffler(bc, 0, 300, 3)
    for epoch in range(3):
        key = R.epoch_key(9, epoch, 0)
        want = R.reshuffle(blks, 300, key)
        assert len(want) == 7
        if case == "fm16_chunked":
            assert min(int(np.count_nonzero(w["ids"] == 7)) for w in want[:-1]) > 128
        assert rs.begin_epoch(key) == 7
        for w in want:
            H.train_step(A, rs.next(), H.kTraining, push_cnt=(epoch == 0))
            rs.consumed()
            wb = D.RowBlock(w["offs"], w["ids"], w["vals"], w["labels"], w["weights"])
            H.train_step(B, H.DeviceRowBlock(B, wb), H.kTraining, push_cnt=(epoch == 0))
        pa, pb = H.progress(A), H.progress(B)
        assert pa["nrows"] == pb["nrows"] == 2000
        assert pa["loss"] == pb["loss"] and pa["auc"] == pb["auc"], (epoch, pa, pb)
        sa, sb = H.Store(A).stats(), H.Store(B).stats()
        assert sa["seed"] == sb["seed"] and sa["n_keys"] == sb["n_keys"] > 0, (epoch, sa, sb)
    _, uniq, _ = H.Localizer(A).compact(H.DeviceRowBlock(A, D.concat(blks)), want_cnt=False)
    assert uniq.numel() == H.Store(A).stats()["n_keys"]
    (va, la), (vb, lb) = H.Store(A).pull(uniq), H.Store(B).pull(uniq)
    assert va.cpu().numpy().tobytes() == vb.cpu().numpy().tobytes()
    assert (la is None) == (lb is None)
    if la is not None:
        assert la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes()
    rs.close()
    bc.close()
    A.close()
    B.close()


@pytest.mark.parametrize("extra", [256, 2048])
def test_a_budget_without_room_for_the_ring_keeps_nothing(ctx, extra):
    """the list takes one block of 4096; the table and the scratch need 2048 more and the ring
    more still: kept = 0 with DFX_OK, nothing stays allocated, the cache still replays"""
    from difacto_amd import hotpath as H
    blk = _blk([3] * 100, 100)
    bc = _record(H, ctx, [blk], budget=BLOCK + extra)
    assert bc.stats()["bytes"] == BLOCK
    rs = H.Reshuffler(bc, 0, 10, 2)
    assert rs.kept is False and rs.h is None
    assert bc.stats()["bytes"] == BLOCK
    BC._assert_holds(bc.get(0, 0), blk)
    rs.close()
    bc.close()


def test_misuse_is_err_arg(ctx):
    """every misuse of include/difacto_amd.h's list but a list of 2^31 rows, which no test can
    afford to record (its offsets alone are 16 GB)"""
    from difacto_amd import _lib
    from difacto_amd import hotpath as H
    blk = _blk([2, 1, 4], 110)
    bc = H.BatchCache(ctx, 2 * BLOCK + 8192, BLOCK)
    BC._arg_error(H.Reshuffler, bc, 0, 2)           # an unknown list
    bc.begin(0)
    assert bc.append(H.DeviceRowBlock(ctx, blk))
    BC._arg_error(H.Reshuffler, bc, 0, 2)           # an open list
    assert bc.seal() == 1
    bc.begin(1)
    assert bc.append(H.DeviceRowBlock(ctx, _blk([400] * 40, 111))) is False  # over the budget
    assert bc.seal() == -1
    BC._arg_error(H.Reshuffler, bc, 1, 2)           # a dropped list
    BC._arg_error(H.Reshuffler, bc, 0, 0)           # batch_rows <= 0
    BC._arg_error(H.Reshuffler, bc, 0, -3)
    BC._arg_error(H.Reshuffler, bc, 0, 2, 1)        # nring outside 2..8
    BC._arg_error(H.Reshuffler, bc, 0, 2, 9)
    held = bc.stats()["bytes"]
    rs = H.Reshuffler(bc, 0, 2, 2)
    assert rs.kept and bc.stats()["bytes"] > held
    BC._arg_error(rs.next)                          # next before begin_epoch
    BC._arg_error(rs.consumed)                      # consumed with no batch handed out
    assert rs.begin_epoch(1) == 2
    BC._arg_error(rs.consumed)
    assert rs.next() is not None
    rs.consumed()
    BC._arg_error(rs.consumed)                      # ... twice for one batch
    # the cache's destroy with a live reshuffler: refused, the cache stays usable
    assert _lib.lib().dfx_batchcache_destroy(bc.h) == 1
    assert b"reshuffler" in _lib.lib().dfx_last_error()
    BC._assert_holds(bc.get(0, 0), blk)
    _assert_epoch(rs, (4, R.reshuffle([blk], 2, 4)))
    n = ctypes.c_int64(0)
    assert _lib.lib().dfx_reshuffle_begin_epoch(None, 0, ctypes.byref(n)) == 1
    rs.close()
    assert bc.stats()["bytes"] == held              # the ring and the scratch are given back
    bc.close()


# ---- the driver -----------------------------------------------------------------------------
CFG = dict(V_dim=4, V_threshold=1, max_keys=262144)
KW = ["batch_size=100", "num_jobs_per_epoch=2", "max_num_epochs=3", "stop_rel_objv=0",
      "shuffle=0", "neg_sampling=1", "data_format=criteo", "has_aux=1", "cache=device"] + \
     ["%s=%s" % kv for kv in CFG.items()]


def _parts(data, nparts):
    """TextReader's cut of a text file: [size k / n, size (k + 1) / n), both ends moved to the
    next line start"""
    size = len(data)

    def line_start(at):
        if at == 0 or at >= size:
            return size if at >= size else 0
        nl = data.find(b"\n", at - 1)
        return nl + 1 if nl >= 0 else size
    return [data[line_start(size * k // nparts):line_start(size * (k + 1) // nparts)]
            for k in range(nparts)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """2,000 generated Criteo rows; the runs of dfx_train the tests below compare"""
    import subprocess
    d = tmp_path_factory.mktemp("rs")
    path = str(d / "c.txt")
    subprocess.check_call([BC.GEN_BIN, path, "2000", "65536", "0"])
    outs = {}
    for name, extra in (("plain", []), ("a", ["epoch_shuffle=1"]), ("b", ["epoch_shuffle=1"]),
                        ("seed7", ["epoch_shuffle=1", "shuffle_seed=7"])):
        outs[name] = BC._train(["data_in=" + path, "model_out=" + str(d / ("m_" + name))]
                               + KW + extra)
    return path, d, outs


def test_driver_reshuffles_later_epochs_reproducibly(driver):
    import re
    from difacto_amd import hotpath as H
    from oracle import oracle as O
    path, d, outs = driver
    f = {k: BC._fields(v, "Training") for k, v in outs.items()}
    print(f)
    assert all(len(v) == 3 for v in f.values())
    assert f["a"] == f["b"]                                  # the same seed: the same run
    assert f["a"][0] == f["plain"][0] == f["seed7"][0]       # the recording epoch is unchanged
    for k in (1, 2):
        rows = [x[k].split(",")[0] for x in (f["plain"], f["a"], f["seed7"])]
        assert rows[0] == rows[1] == rows[2] == "Rows = 2000"
        assert len({f["plain"][k], f["a"][k], f["seed7"][k]}) == 3   # other batches, other loss
    m = re.findall(r"^epoch_shuffle=1: (\d+) of (\d+) training parts reshuffle, rings ([\d.]+) MB",
                   outs["a"], re.M)
    assert len(m) == 1 and m[0][:2] == ("2", "2") and float(m[0][2]) > 0, outs["a"]
    assert "epoch_shuffle" not in outs["plain"]
    assert outs["a"].count("parts reshuffled, the host waited") == 2
    ctx = H.Context(0, V_dim=0, max_keys=1 << 12)
    blocks = [H.parse_criteo(ctx, p)[0] for p in _parts(open(path, "rb").read(), 2)]
    ctx.close()
    from difacto_amd import data as D
    keys = O.localize(*[getattr(D.concat(blocks), n) for n in ("offs", "ids")])[0]
    n, size = BC._assert_models_equal(str(d / "m_a_part-0"), str(d / "m_b_part-0"), keys,
                                      V_dim=4, V_threshold=1)
    assert n == size


def test_driver_lines_equal_hotpath_on_the_reference_batches(driver):
    """the recording epoch steps the parts' rows in file order, 100 a batch (shuffle=0,
    neg_sampling=1); epochs 1 and 2 step reshuffle_ref's batches of those lists under
    epoch_key(seed, epoch, list): the driver's three Training lines, from hotpath"""
    from difacto_amd import data as D
    from difacto_amd import hotpath as H
    path, d, outs = driver
    ctx = H.Context(0, **CFG)
    parts = [H.parse_criteo(ctx, p)[0] for p in _parts(open(path, "rb").read(), 2)]
    assert sum(p.size for p in parts) == 2000
    lists = [[p.slice(i, min(i + 100, p.size)) for i in range(0, p.size, 100)] for p in parts]
    for seed, name in ((0, "a"), (7, "seed7")):
        c = H.Context(0, **CFG)
        lines = []
        for epoch in range(3):
            tot = {"nrows": 0., "loss": 0., "auc": 0.}
            for part, recorded in enumerate(lists):
                if epoch == 0:
                    batches = recorded
                else:
                    batches = [D.RowBlock(w["offs"], w["ids"], w["vals"], w["labels"])
                               for w in R.reshuffle(recorded, 100, R.epoch_key(seed, epoch, part))]
                for b in batches:
                    H.train_step(c, H.DeviceRowBlock(c, b), H.kTraining, push_cnt=(epoch == 0))
                p = H.progress(c)
                for k in tot:
                    tot[k] += p[k]
            lines.append("Rows = %.0f, loss = %.9g, AUC = %.9g"
                         % (tot["nrows"], tot["loss"] / tot["nrows"], tot["auc"] / tot["nrows"]))
        c.close()
        assert lines == BC._fields(outs[name], "Training"), (name, lines)
    ctx.close()
