"""Model files loaded on the device (csrc/modelload.hip, dfx_store_load_dev) against the host
loader dfx_store_load_part, which is the yardstick (test_gpu_r3.py pins it to the oracle).  Both
insert in parallel, so two stores are equal when their counters (n_keys, n_vrows, new_w), their
capacity and their save(save_aux=True) records, key by key, are equal; every comparison is exact.

Files are crafted from a seed: records with and without V mixed at random, and a fifth of the V
and Vaux dwords set to the integers 1 and d + 1, so chains that start inside a payload stay
alive.  MIN_TILE is the smallest tile_dwords: at 32 dwords every file here spans more than one
group of 128 tiles, and a V_dim 260 record (526 dwords with aux) is longer than 16 tiles."""
import os
import struct
import subprocess

import numpy as np
import pytest

from difacto_amd import data as D
from difacto_amd._lib import DfxError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_BIN = os.path.join(ROOT, "build", "dfx_train")
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
MODELS = [(0, "auto"), (4, "auto"), (16, "auto"), (28, "auto"), (260, "split")]
MIN_TILE, GROUP, N = 32, 128, 3000


@pytest.fixture(scope="module")
def H():
    from difacto_amd import hotpath
    return hotpath


def _craft(d, aux, keys, seed):
    """SGDUpdater::Save's bytes for `keys` -> (the file, each record's offset)"""
    rng = np.random.default_rng(seed)
    out, offs, at = [bytes([aux])], [], 1
    for k in keys:
        has_v = d > 0 and rng.random() < .5
        rec = struct.pack("<Qi", int(k), d + 1 if has_v else 1)
        rec += rng.standard_normal(1 + 2 * aux).astype(np.float32).tobytes()
        if has_v:
            v = rng.standard_normal(d * (1 + aux)).astype(np.float32).view(np.uint32)
            v[rng.random(v.size) < .1] = 1
            v[rng.random(v.size) < .1] = d + 1
            rec += v.tobytes()
        out.append(rec)
        offs.append(at)
        at += len(rec)
    return b"".join(out), offs


def _keys(n, seed):
    rng = np.random.default_rng(seed)  # (the high end is exclusive: never the reserved key)
    return rng.permutation(np.unique(rng.integers(0, 2 ** 64 - 1, n, dtype=np.uint64)))


def _records(data, d):
    """a Save file -> {key: record bytes}"""
    aux, out, i = data[0], {}, 1
    while i < len(data):
        key, size = struct.unpack_from("<Qi", data, i)
        n = 16 + 8 * aux + (4 * d * (1 + aux) if size > 1 else 0)
        assert key not in out
        out[key] = data[i:i + n]
        i += n
    assert i == len(data)
    return out


def _state(H, c, tmp):
    s = H.Store(c)
    p = str(tmp / "state.bin")
    s.save(p, True)
    st = s.stats()
    return (st["n_keys"], st["n_vrows"], st["new_w"], s.capacity()), \
        _records(open(p, "rb").read(), c.V_dim)


def _loaded(H, tmp, path, d, layout, **kw):
    """the state of a fresh store (far smaller than the file: the load grows it) after one load"""
    c = H.Context(0, max_keys=1 << 8, slot_layout=layout, V_dim=d)
    st = H.Store(c).load(path, **kw)
    out = _state(H, c, tmp)
    c.close()
    return out, st


@pytest.fixture(scope="module")
def crafted(H, tmp_path_factory):
    """(V_dim, layout, aux) -> (the file's path, the host-loaded state), made once"""
    tmp, made = tmp_path_factory.mktemp("model_load"), {}

    def get(d, layout, aux):
        if (d, layout, aux) not in made:
            p = str(tmp / ("m_%d_%d" % (d, aux)))
            open(p, "wb").write(_craft(d, aux, _keys(N, 7 + d), 11 * d + aux)[0])
            made[(d, layout, aux)] = (p, _loaded(H, tmp, p, d, layout)[0])
        return made[(d, layout, aux)]
    return get


@pytest.mark.parametrize("tile", [MIN_TILE, 0])
@pytest.mark.parametrize("aux", [0, 1])
@pytest.mark.parametrize("d,layout", MODELS)
def test_parity(H, crafted, tmp_path, d, layout, aux, tile):
    path, want = crafted(d, layout, aux)
    got, st = _loaded(H, tmp_path, path, d, layout, device=True, tile_dwords=tile)
    print(st)
    n = len(want[1])
    assert N - 2 <= n <= N and want[0][0] == n
    assert got[0] == want[0]
    assert got[1] == want[1]
    assert st["records"] == st["owned"] == n and st["host_loaded"] == 0
    assert st["owned_v"] == want[0][1] and (d == 0 or 0 < st["owned_v"] < n)
    assert st["tile_dwords"] == (tile or (4096 if d < 260 else 8192))
    assert st["tiles"] == -(-((os.path.getsize(path) - 1) // 4) // st["tile_dwords"])
    if tile:
        assert st["tiles"] > GROUP


@pytest.mark.parametrize("what", ["one_record", "stray_tail", "aux_byte", "zero_bytes"])
def test_tiny_files(H, tmp_path, what):
    """stray_tail: under 8 bytes behind the last record, where the host's loop just ends"""
    p = str(tmp_path / "tiny.bin")
    one = _craft(4, 1, [77], 1)[0]
    open(p, "wb").write({"one_record": one, "stray_tail": one + b"\x01" * 7, "aux_byte": one[:1],
                         "zero_bytes": b""}[what])
    want = _loaded(H, tmp_path, p, 4, "auto")[0]
    assert want[0][0] == (what in ("one_record", "stray_tail"))
    for tile in (MIN_TILE, 0):
        assert _loaded(H, tmp_path, p, 4, "auto", device=True, tile_dwords=tile)[0] == want


def test_rank_filter(H, crafted, tmp_path):
    path, whole = crafted(4, "auto", 1)
    owned = 0
    for rank in range(3):
        want = _loaded(H, tmp_path, path, 4, "auto", rank=rank, nranks=3)[0]
        got, st = _loaded(H, tmp_path, path, 4, "auto", rank=rank, nranks=3, device=True,
                          tile_dwords=MIN_TILE)
        assert got == want and st["owned"] == want[0][0] > 0
        assert st["records"] == len(whole[1])
        owned += st["owned"]
    assert owned == len(whole[1])


@pytest.mark.parametrize("layout", ["auto", "split"])
def test_into_a_live_store(H, tmp_path, layout):
    """a file without aux over a trained store, half of its keys trained ones: sqrt_g and z
    (and fea_cnt) of those stay, as SGDEntry::LoadEntry has it"""
    d, states = 4, []
    for device in (False, True):
        c = H.Context(0, max_keys=1 << 12, slot_layout=layout, V_dim=d, V_threshold=2, l1=0.02,
                      lr=.1, V_lr=.02)
        for step in range(3):
            blk = D.synthetic(500, 20, 1 << 11, binary=(step % 2 == 0), seed=60 + step)
            H.train_step(c, H.DeviceRowBlock(c, blk), H.kTraining, push_cnt=(step < 2))
        H.progress(c)
        before = _state(H, c, tmp_path)
        trained = sorted(before[1])
        assert len(trained) > 500
        keys = np.concatenate([np.array(trained[::2], np.uint64), _keys(len(trained) // 2, 5)])
        p = str(tmp_path / "half.bin")
        open(p, "wb").write(_craft(d, 0, keys, 9)[0])
        H.Store(c).load(p, device=device, tile_dwords=MIN_TILE)
        after = _state(H, c, tmp_path)
        assert after[0][0] == before[0][0] + len(trained) // 2
        k = trained[0]  # (a trained key of the file: w is the file's, the aux state stays)
        assert after[1][k][12:16] != before[1][k][12:16]
        assert after[1][k][16:24] == before[1][k][16:24]
        cnt = H.Store(c).entry(k)[0]
        assert cnt[3] > 0
        states.append((before, after, cnt.tobytes()))
        c.close()
    assert states[0] == states[1]


@pytest.mark.parametrize("what", ["short_1", "in_head", "in_V", "size", "key"])
def test_refusals(H, tmp_path, what):
    d, keys = 4, _keys(1500, 3)
    data, offs = _craft(d, 1, keys, 4)
    with_v = [i for i in range(len(offs) - 1) if offs[i + 1] - offs[i] > 24]
    i = with_v[len(with_v) // 2]
    bad = {"short_1": data[:-1], "in_head": data[:offs[i] + 10],
           "in_V": data[:offs[i] + 24 + 6],
           "size": data[:offs[i] + 8] + struct.pack("<i", d + 2) + data[offs[i] + 12:],
           "key": data[:offs[i]] + b"\xff" * 8 + data[offs[i] + 8:]}[what]
    p, good = str(tmp_path / "bad.bin"), str(tmp_path / "good.bin")
    open(p, "wb").write(bad)
    open(good, "wb").write(_craft(d, 1, _keys(100, 8), 8)[0])
    c = H.Context(0, max_keys=1 << 8, V_dim=d)
    s = H.Store(c)
    s.load(good)
    want = _state(H, c, tmp_path)
    errs = []
    for kw in (dict(), dict(device=True, tile_dwords=MIN_TILE), dict(device=True)):
        with pytest.raises(DfxError) as e:
            s.load(p, **kw)
        errs.append(str(e.value))
        assert _state(H, c, tmp_path) == want
    assert errs[0] == errs[1] == errs[2], errs
    for tile in (8, 40, 16384, -32):
        with pytest.raises(DfxError, match="status 1:"):
            s.load(good, device=True, tile_dwords=tile)
    assert _state(H, c, tmp_path) == want
    c.close()


def _run(args, rc=0):
    assert os.path.exists(TRAIN_BIN), "build/dfx_train missing: run make"
    r = subprocess.run([TRAIN_BIN] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == rc, r.stdout + r.stderr
    return r


def test_driver(tmp_path):
    """task=2 from a 2-part model: the single-GPU run (part 0), and three shards that each keep
    their keys of both parts - the prediction files under model_read=device are the host's"""
    kw = ["V_dim=4", "V_threshold=1", "lr=0.1", "V_lr=0.05", "l1=0.1", "seed=7", "max_keys=65536",
          "num_jobs_per_epoch=1"]
    model = str(tmp_path / "m")
    _run(["data_in=" + DATA, "shards=2", "shuffle=0", "batch_size=10", "max_num_epochs=2",
          "stop_rel_objv=0", "has_aux=1", "model_out=" + model] + kw)
    for name, args, parts in (("one", [], 1), ("three", ["shards=3", "model_in_parts=2"], 3)):
        preds = {}
        for reader in ("host", "device"):
            out = str(tmp_path / (name + reader))
            r = _run(["task=2", "data_val=" + DATA, "model_in=" + model, "pred_out=" + out,
                      "model_read=" + reader] + args + kw)
            assert (reader == "device") == ("model_read=device: " in r.stdout), r.stdout
            preds[reader] = [open("%s_part-%d" % (out, k), "rb").read() for k in range(parts)]
        assert preds["host"] == preds["device"] and all(len(x) > 0 for x in preds["host"])
    r = _run(["task=2", "data_val=" + DATA, "model_in=" + model, "model_read=bogus"] + kw, rc=2)
    assert r.stderr.strip().splitlines()[-1] == "model_read must be host or device"
