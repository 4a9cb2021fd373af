"""The device batch cache (difacto_amd/csrc/batchcache.hip, hotpath.BatchCache, dfx_train
cache=device): cached batches are their sources byte for byte, replaying them trains the same
model, a list over the budget is dropped and not the run, misuse is DFX_ERR_ARG, and the
driver prints the same losses and saves the same models with the cache on and off.  Every
check compares two runs of the project (or source bytes), so none has a tolerance."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

TRAIN_BIN = os.path.join(ROOT, "build", "dfx_train")
GEN_BIN = os.path.join(ROOT, "build", "gen_criteo")
CONV_BIN = os.path.join(ROOT, "build", "dfx_convert")
RCV1 = os.path.join(GOLDEN, "rcv1_100.libsvm")
BLOCK = 4096
NAMES = ("offs", "ids", "vals", "labels", "weights")


def _block(lens, seed, valued=False, weighted=False):
    from difacto_amd.data import RowBlock
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    offs = np.zeros(len(lens) + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    nnz = int(offs[-1])
    ids = rng.integers(0, 1 << 63, size=nnz, dtype=np.uint64)
    vals = rng.random(nnz, dtype=np.float32) + np.float32(.5) if valued else None
    labels = np.where(rng.random(len(lens)) < .3, 1., -1.).astype(np.float32)
    weights = rng.random(len(lens), dtype=np.float32) + np.float32(1) if weighted else None
    return RowBlock(offs, ids, vals, labels, weights)


def _source_arrays(blk):
    """what the cache must hold: the block's arrays; None where the source pointer is NULL
    (no array, or an empty tensor, whose data_ptr() is 0)"""
    src = dict(zip(NAMES, (blk.offs, blk.ids, blk.vals, blk.labels, blk.weights)))
    return {k: (None if v is None or v.size == 0 else v) for k, v in src.items()}


def _assert_holds(cached, blk):
    got, want = cached.arrays(), _source_arrays(blk)
    assert cached.size == blk.size and cached.nnz == blk.nnz
    for k in NAMES:
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is not None:
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    for k, p in cached.pointers().items():
        assert p is None or p % 256 == 0, (k, p)


def _scribble(dblk):
    """other bytes into a source batch's tensors, on the context's (torch's current) stream"""
    import torch
    for t in (dblk.offs, dblk.ids, dblk.vals, dblk.labels, dblk.weights):
        if t is not None and t.numel():
            t.view(dtype=torch.uint8).fill_(0xA5)


def _arg_error(fn, *args):
    """fn(*args) fails with DFX_ERR_ARG (status 1) and a message from dfx_last_error()"""
    from difacto_amd._lib import DfxError
    with pytest.raises(DfxError) as e:
        fn(*args)
    m = re.match(r"libdifacto_amd: status 1: (.+)", str(e.value), re.S)
    assert m and m.group(1).strip() not in ("", "?"), str(e.value)


# ---- 1 ---------------------------------------------------------------------------------------
def test_cached_batches_are_their_sources():
    """one list, blocks of 4096 bytes: B=1 nnz=1 binary; row lengths [0, 2, 0] valued and
    weighted; B=257 nnz=1001 binary; B=0; nnz=2000 (index alone exceeds a block).  After the
    sources are overwritten every cached array equals the original bit for bit, NULL value /
    weight stay NULL, every pointer is a multiple of 256"""
    from difacto_amd import hotpath as H
    rng = np.random.default_rng(3)
    lens257 = rng.multinomial(1001, np.full(257, 1 / 257))
    blks = [_block([1], 1), _block([0, 2, 0], 2, valued=True, weighted=True),
            _block(lens257, 3), _block([], 4), _block([20] * 100, 5)]
    assert [b.size for b in blks] == [1, 3, 257, 0, 100]
    assert [b.nnz for b in blks] == [1, 2, 1001, 0, 2000]
    ctx = H.Context(0, V_dim=0, max_keys=1 << 12)
    bc = H.BatchCache(ctx, 1 << 24, BLOCK)
    dblks = [H.DeviceRowBlock(ctx, b) for b in blks]
    assert bc.count(7) == -2
    bc.begin(7)
    for d in dblks:
        assert bc.append(d) is True
    assert bc.seal() == len(blks)
    for d in dblks:
        _scribble(d)
    ctx.sync()
    assert bc.count(7) == len(blks)
    for i, b in enumerate(blks):
        _assert_holds(bc.get(7, i), b)
    assert bc.get(7, 0).arrays()["vals"] is None and bc.get(7, 1).arrays()["vals"] is not None
    assert bc.get(7, 1).arrays()["weights"] is not None
    st = bc.stats()
    assert (st["sealed"], st["dropped"], st["batches"]) == (1, 0, len(blks))
    assert st["bytes"] % 256 == 0 and st["bytes"] >= 2000 * 8
    bc.close()
    ctx.close()


# ---- 2 ---------------------------------------------------------------------------------------
def test_replay_trains_the_same_model():
    """context A steps from freshly uploaded batches in each of 3 epochs; context B records in
    epoch 0 while stepping from the sources, then steps from get() in epochs 1 and 2: equal
    progress (loss and AUC as doubles) and store stats after every epoch, bit-equal pulls of
    all keys at the end"""
    from difacto_amd import data as D
    from difacto_amd import hotpath as H
    cfg = dict(V_dim=4, V_threshold=1, l1=0, lr=.1, V_lr=.01, max_keys=1 << 16)
    blks = [D.synthetic(200, 10, 1 << 12, seed=11 + i) for i in range(4)]
    A, B = H.Context(0, **cfg), H.Context(0, **cfg)
    bc = H.BatchCache(B, 1 << 24, BLOCK)
    for epoch in range(3):
        for b in blks:
            H.train_step(A, H.DeviceRowBlock(A, b), H.kTraining, push_cnt=(epoch == 0))
        if epoch == 0:
            bc.begin(0)
            for b in blks:
                d = H.DeviceRowBlock(B, b)
                assert bc.append(d)
                H.train_step(B, d, H.kTraining, push_cnt=True)
            assert bc.seal() == len(blks)
        else:
            for i in range(bc.count(0)):
                H.train_step(B, bc.get(0, i), H.kTraining, push_cnt=False)
        pa, pb = H.progress(A), H.progress(B)
        assert pa["nrows"] == pb["nrows"] == 800
        assert pa["loss"] == pb["loss"] and pa["auc"] == pb["auc"], (epoch, pa, pb)
        sa, sb = H.Store(A).stats(), H.Store(B).stats()
        assert sa["seed"] == sb["seed"] and sa["n_keys"] == sb["n_keys"] > 0, (epoch, sa, sb)
    allb = D.concat(blks)
    _, uniq, _ = H.Localizer(A).compact(H.DeviceRowBlock(A, allb), want_cnt=False)
    assert uniq.numel() == H.Store(A).stats()["n_keys"]
    va, la = H.Store(A).pull(uniq)
    vb, lb = H.Store(B).pull(uniq)
    assert va.cpu().numpy().tobytes() == vb.cpu().numpy().tobytes()
    assert la.cpu().numpy().tobytes() == lb.cpu().numpy().tobytes()
    bc.close()
    A.close()
    B.close()


# ---- 3 ---------------------------------------------------------------------------------------
def test_list_over_budget_is_dropped_not_the_run():
    """budget = 3 blocks of 4096: list 0 fits, list 1 grows until an append is refused and is
    dropped (seal -1, get DFX_ERR_ARG, its bytes given back), list 2 then records and replays,
    list 0 still holds its sources"""
    from difacto_amd import hotpath as H
    cfg = dict(V_dim=4, V_threshold=1, l1=0, lr=.1, V_lr=.01, max_keys=1 << 14)
    A, B = H.Context(0, **cfg), H.Context(0, **cfg)
    bc = H.BatchCache(B, 3 * BLOCK, BLOCK)
    b0 = _block([3] * 10, 20)
    bc.begin(0)
    assert bc.append(H.DeviceRowBlock(B, b0))
    assert bc.seal() == 1
    before = bc.stats()
    assert before["bytes"] == BLOCK
    bc.begin(1)
    kept = []
    for i in range(64):  # 3 arrays of 256 bytes a batch: two more blocks hold 10 batches
        kept.append(bc.append(H.DeviceRowBlock(B, _block([3] * 10, 30 + i))))
        if not kept[-1]:
            break
    assert kept == [True] * 10 + [False], kept
    assert bc.append(H.DeviceRowBlock(B, b0)) is False  # later appends are no-ops
    assert bc.stats()["bytes"] == before["bytes"]
    assert bc.seal() == -1
    assert bc.count(1) == -1
    _arg_error(bc.get, 1, 0)
    st = bc.stats()
    assert (st["sealed"], st["dropped"], st["batches"], st["bytes"]) == (1, 1, 1, BLOCK)
    b2 = _block([4] * 50, 21)
    bc.begin(2)
    d2 = H.DeviceRowBlock(B, b2)
    assert bc.append(d2)
    assert bc.seal() == 1
    _scribble(d2)
    B.sync()
    _assert_holds(bc.get(2, 0), b2)
    _assert_holds(bc.get(0, 0), b0)
    H.train_step(A, H.DeviceRowBlock(A, b2), H.kTraining, push_cnt=True)
    H.train_step(B, bc.get(2, 0), H.kTraining, push_cnt=True)
    pa, pb = H.progress(A), H.progress(B)
    assert pa["nrows"] == pb["nrows"] == 50 and pa["loss"] == pb["loss"] and pa["auc"] == pb["auc"]
    st = bc.stats()
    assert (st["sealed"], st["dropped"], st["batches"]) == (2, 1, 2)
    assert BLOCK < st["bytes"] <= 3 * BLOCK
    bc.close()
    A.close()
    B.close()


# ---- 4 ---------------------------------------------------------------------------------------
class _Raw:
    def __init__(self, b):
        self.b = b

    def as_batch(self):
        return self.b


def test_misuse_is_err_arg():
    import ctypes
    from difacto_amd import _lib
    from difacto_amd import hotpath as H
    ctx = H.Context(0, V_dim=0, max_keys=1 << 12)
    blk = _block([2, 1], 40)
    d = H.DeviceRowBlock(ctx, blk)
    _arg_error(H.BatchCache, ctx, -1)          # negative sizes
    _arg_error(H.BatchCache, ctx, 1 << 20, -1)
    bc = H.BatchCache(ctx, BLOCK, BLOCK)
    _arg_error(bc.append, d)                   # no open list
    _arg_error(bc.seal)
    _arg_error(bc.begin, -1)
    bc.begin(0)
    _arg_error(bc.begin, 1)                    # begin while a list is open
    _arg_error(bc.get, 0, 0)                   # get on an open list
    good = d.as_batch()
    for field, val in (("size", -1), ("nnz", -1), ("offset", None), ("label", None)):
        bad = _lib.Batch(good.size, good.nnz, good.offset, good.index, good.value, good.label,
                         good.weight)
        setattr(bad, field, val)
        _arg_error(bc.append, _Raw(bad))
    assert bc.append(d)
    assert bc.seal() == 1
    _arg_error(bc.begin, 0)                    # already sealed
    _arg_error(bc.get, 0, 1)                   # i out of range
    _arg_error(bc.get, 0, -1)
    _arg_error(bc.get, 5, 0)                   # never begun
    bc.begin(1)
    assert bc.append(H.DeviceRowBlock(ctx, _block([200] * 10, 41))) is False  # over the budget
    assert bc.seal() == -1
    _arg_error(bc.begin, 1)                    # already dropped
    _arg_error(bc.get, 1, 0)
    out = ctypes.c_int64(0)
    assert _lib.lib().dfx_batchcache_count(None, 0, ctypes.byref(out)) == 1
    assert _lib.lib().dfx_last_error()
    _assert_holds(bc.get(0, 0), blk)
    bc.close()
    ctx.close()


# ---- 5, 6: the driver ------------------------------------------------------------------------
def _train(args, timeout=120):
    r = subprocess.run([TRAIN_BIN] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _fields(out, tag):
    got = [l.split(tag + ": ")[1].split("  (")[0] for l in out.splitlines() if tag + ":" in l]
    assert got, out
    return got


def _cache_line(out):
    """-> (batches, MB, parts not cached, parts) of the one line the recording epoch prints"""
    m = re.findall(r"^cache=device: (\d+) batches, ([\d.]+) MB held, (\d+) of (\d+) parts not "
                   r"cached$", out, re.M)
    assert len(m) == 1, out
    return int(m[0][0]), float(m[0][1]), int(m[0][2]), int(m[0][3])


def _assert_models_equal(path_a, path_b, keys, **kw):
    """the same keys with bit-equal entries (slot order is not part of the contract)"""
    from oracle import oracle as O
    a, b = O.Updater(**kw), O.Updater(**kw)
    a.load(path_a)
    b.load(path_b)
    assert a.size() == b.size() > 0
    n = 0
    for k in keys:
        ea, eb = a.entry(k), b.entry(k)
        assert (ea is None) == (eb is None), k
        if ea is None:
            continue
        n += 1
        assert ea[0].tobytes() == eb[0].tobytes(), k
        assert (ea[1] is None) == (eb[1] is None), k
        if ea[1] is not None:
            assert ea[1].tobytes() == eb[1].tobytes(), k
    return n, a.size()


@pytest.fixture(scope="module")
def criteo(tmp_path_factory):
    """3,000 generated rows and their localized keys"""
    from oracle import oracle as O
    d = tmp_path_factory.mktemp("bc")
    path = str(d / "c.txt")
    subprocess.check_call([GEN_BIN, path, "3000", "65536", "0"])
    subprocess.check_call([CONV_BIN, "data_in=" + path, "data_format=criteo",
                           "data_out=" + str(d / "c.libsvm"), "data_out_format=libsvm"],
                          stdout=subprocess.DEVNULL)
    offs, ids = [0], []
    for line in open(d / "c.libsvm"):
        ids.extend(int(t) for t in line.split()[1:])
        offs.append(len(ids))
    keys = O.localize(np.array(offs, np.uint64), np.array(ids, np.uint64))[0]
    return path, keys


KW = ["V_dim=4", "V_threshold=1", "batch_size=250", "num_jobs_per_epoch=2", "max_num_epochs=3",
      "stop_rel_objv=0", "shuffle=3", "neg_sampling=0.7", "data_format=criteo",
      "max_keys=262144", "has_aux=1"]


@pytest.mark.parametrize("parse", ["host", "device"])
def test_driver_fused_cache_equals_no_cache(tmp_path, criteo, parse):
    """dfx_train on 3,000 rows, shuffled and down-sampled, 2 parts, with validation, 3 epochs:
    cache=device, and cache=device with a budget below one block (nothing cached), print the
    Training / Validation fields of cache=none in every epoch and save the same model"""
    data, keys = criteo
    outs = {}
    for name, extra in (("none", ["cache=none"]), ("device", ["cache=device"]),
                        ("tiny", ["cache=device", "cache_mb=1"])):
        outs[name] = _train(["data_in=" + data, "data_val=" + data, "parse=" + parse,
                             "model_out=" + str(tmp_path / ("m_" + name))] + extra + KW)
    assert "cache=device" not in outs["none"]
    for name in ("device", "tiny"):
        for tag in ("Training", "Validation"):
            a, b = _fields(outs["none"], tag), _fields(outs[name], tag)
            print(parse, name, tag, len(a), "epochs")
            assert len(a) >= 2 and a == b, (name, tag, a, b)
        n, size = _assert_models_equal(str(tmp_path / "m_none_part-0"),
                                       str(tmp_path / ("m_" + name + "_part-0")), keys,
                                       V_dim=4, V_threshold=1)
        assert n == size
    batches, mb, missed, parts = _cache_line(outs["device"])
    assert (missed, parts) == (0, 4) and batches > 2 and mb > 0
    assert _cache_line(outs["tiny"]) == (0, 0.0, 4, 4)


def test_driver_fused_cache_valued_libsvm(tmp_path):
    """valued batches through the host feeder: rcv1_100.libsvm, batch_size=7"""
    from difacto_amd import data as D
    from oracle import oracle as O
    blk = D.read_libsvm(RCV1)
    assert not np.all(blk.vals == 1)
    keys = O.localize(blk.offs, blk.ids)[0]
    kw = ["data_in=" + RCV1, "data_val=" + RCV1, "data_format=libsvm", "batch_size=7",
          "V_dim=4", "V_threshold=1", "num_jobs_per_epoch=2", "max_num_epochs=3",
          "stop_rel_objv=0", "max_keys=65536", "has_aux=1"]
    outs = {}
    for c in ("none", "device"):
        outs[c] = _train(kw + ["cache=" + c, "model_out=" + str(tmp_path / ("m_" + c))])
    for tag in ("Training", "Validation"):
        a, b = _fields(outs["none"], tag), _fields(outs["device"], tag)
        assert len(a) >= 2 and a == b, (tag, a, b)
    n, size = _assert_models_equal(str(tmp_path / "m_none_part-0"),
                                   str(tmp_path / "m_device_part-0"), keys, V_dim=4,
                                   V_threshold=1)
    assert n == size
    assert _cache_line(outs["device"])[2:] == (0, 4)


def test_driver_sharded_cache_equals_no_cache(tmp_path, criteo):
    """shards=2 exchange=a2a pipelined=1, 3 epochs: the printed fields and both servers' model
    parts are equal with cache=device and cache=none"""
    data, keys = criteo
    outs = {}
    for c in ("none", "device"):
        outs[c] = _train(["data_in=" + data, "shards=2", "exchange=a2a", "pipelined=1",
                          "cache=" + c, "model_out=" + str(tmp_path / ("m_" + c))] + KW)
    a, b = _fields(outs["none"], "Training"), _fields(outs["device"], "Training")
    assert len(a) == 3 and a == b, (a, b)
    total = 0
    for r in (0, 1):
        n, size = _assert_models_equal(str(tmp_path / ("m_none_part-%d" % r)),
                                       str(tmp_path / ("m_device_part-%d" % r)), keys, V_dim=4,
                                       V_threshold=1)
        assert n == size
        total += n
    assert total > 0
    batches, mb, missed, parts = _cache_line(outs["device"])
    assert (missed, parts) == (0, 4) and batches > 2 and mb > 0
