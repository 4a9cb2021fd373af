"""The model files written from the device (csrc/modelfile.hip, csrc/modeltext.h):
dfx_store_save_dev and dfx_store_dump_dev against the host writers dfx_store_save and dfx_store_dump on the same
context, byte for byte.  The host writers are the yardstick: test_gpu_r3.py pins them to the
oracle (test_dump_text_equals_oracle, and the save / load round trips).

The trained models are that test's own recipe - 4 fused steps of D.synthetic(1500, 20, 1 << 13,
seed=60 + step), V_threshold=2, l1=0.02, lr=.1, V_lr=.02, max_keys=1 << 16 - at V_dim 0, 4, 8,
16 and 28, the fat-slot sizes in both layouts.  On the CPU oracle that recipe dumps 8133-8189
lines with no float outside csrc/fmtg.h's domain and none longer than 713 bytes, so the device
must format every chunk itself: a writer that hands its chunks to the host loop fails here.

Chunk sizes: the default, one tile of 256 slots, a slot past it, 16 tiles, the whole table; the
tiny table adds chunks of 1, 63, 64 and 65 slots, where a chunk may hold no entry or one."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from difacto_amd import data as D

pytestmark = pytest.mark.gpu

CHECK = os.path.join(ROOT, "build", "fmtg_check")
EDGE_KEYS = [0, 1, 9, 10, 99, 10 ** 19 - 1, 10 ** 19, 2 ** 63, 2 ** 64 - 2]
CFG = dict(V_threshold=2, l1=0.02, lr=.1, V_lr=.02)
MODELS = [(0, "auto"), (4, "auto"), (4, "split"), (8, "auto"), (8, "split"), (16, "auto"),
          (16, "split"), (28, "auto")]
GUARD = 64


@pytest.fixture(scope="module")
def H():
    from difacto_amd import hotpath
    return hotpath


def _train(H, V_dim, layout, steps=4, max_keys=1 << 16, **over):
    cfg = dict(CFG, V_dim=V_dim)
    cfg.update(over)
    c = H.Context(0, max_keys=max_keys, slot_layout=layout, **cfg)
    for step in range(steps):
        blk = D.synthetic(1500, 20, 1 << 13, binary=(step % 2 == 0), seed=60 + step)
        H.train_step(c, H.DeviceRowBlock(c, blk), H.kTraining, push_cnt=(step < 2))
    H.progress(c)
    return c


@pytest.fixture(scope="module")
def models(H, tmp_path_factory):
    """(V_dim, layout) -> the trained context; host(key) -> the host writer's file of it, made
    once and left unchanged"""
    tmp = tmp_path_factory.mktemp("modelfile")
    ctxs, files = {}, {}

    def ctx(V_dim, layout):
        if (V_dim, layout) not in ctxs:
            ctxs[(V_dim, layout)] = _train(H, V_dim, layout)
        return ctxs[(V_dim, layout)]

    def host(V_dim, layout, kind, aux, rev=0):
        k = (V_dim, layout, kind, aux, rev)
        if k not in files:
            p = str(tmp / ("host_%d_%s_%s_%d_%d" % k))
            s = H.Store(ctx(V_dim, layout))
            if kind == "save":
                s.save(p, bool(aux))
            else:
                s.dump(p, bool(aux), bool(rev))
            files[k] = open(p, "rb").read()
        return files[k]

    yield ctx, host
    for c in ctxs.values():
        c.close()


def _chunks(cap):
    return [0, 256, 257, 4096, cap]


def _check_stats(st, data, text, chunk, cap):
    assert st["bytes"] == len(data)
    if text:
        assert st["entries"] == data.count(b"\n")
    # (a chunk is cut to the staging budget: the whole table at V_dim 28 is two chunks)
    assert st["chunks"] >= max(1, -(-cap // chunk) if chunk else 1)
    if 0 < chunk <= 4096:
        assert st["chunks"] == -(-cap // chunk)


@pytest.mark.parametrize("aux", [0, 1])
@pytest.mark.parametrize("V_dim,layout", MODELS)
def test_trained_save(H, models, tmp_path, V_dim, layout, aux):
    ctx, host = models
    c = ctx(V_dim, layout)
    want = host(V_dim, layout, "save", aux)
    assert len(want) > 8000 * 16
    s = H.Store(c)
    cap = s.capacity()
    entries = set()
    for chunk in _chunks(cap):
        p = str(tmp_path / ("dev_%d" % chunk))
        st = s.save(p, bool(aux), device=True, chunk_slots=chunk)
        got = open(p, "rb").read()
        assert len(got) == len(want), (chunk, st)
        assert got == want, chunk
        assert st["host_chunks"] == 0
        _check_stats(st, got, False, chunk, cap)
        entries.add(st["entries"])
    assert len(entries) == 1 and 8000 < entries.pop() < 8200


@pytest.mark.parametrize("aux,rev", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("V_dim,layout", MODELS)
def test_trained_dump(H, models, tmp_path, V_dim, layout, aux, rev):
    ctx, host = models
    c = ctx(V_dim, layout)
    want = host(V_dim, layout, "dump", aux, rev)
    assert 8000 < want.count(b"\n") < 8200
    s = H.Store(c)
    cap = s.capacity()
    for chunk in _chunks(cap):
        p = str(tmp_path / ("dev_%d" % chunk))
        st = s.dump(p, bool(aux), bool(rev), device=True, chunk_slots=chunk)
        got = open(p, "rb").read()
        assert len(got) == len(want), (chunk, st)
        assert got == want, chunk
        # every float of these models is inside the formatter's domain: no chunk is the host's
        assert st["host_chunks"] == 0, (chunk, st)
        _check_stats(st, got, True, chunk, cap)


def test_vdim_260(H, tmp_path):
    """records of 2104 bytes and lines of 523 fields: longer than a wave's stride, longer than
    a tile's round of 256 fields.  Split layout, aux, one training step of the store (the fused
    step stops at V_dim 256): the counts, a gradient on w that draws V, a gradient on w and V.
    (A step's AdaGrad accumulators may be tiny: a chunk may fall to the host; the files are the
    host's either way, and the binary file never needs it.)"""
    c = H.Context(0, max_keys=1 << 12, slot_layout="split", V_dim=260, V_threshold=1, l1=0,
                  lr=.1, V_lr=.02)
    rng = np.random.default_rng(260)
    keys = np.unique(rng.integers(0, 1 << 62, size=300, dtype=np.uint64))
    tk = c.tensor(keys, torch.int64)
    st = H.Store(c)
    st.push(tk, H.kFeaCount, c.tensor(np.full(len(keys), 3, np.float32), torch.float32))
    st.push(tk, H.kGradient, c.tensor(rng.standard_normal(len(keys)).astype(np.float32),
                                      torch.float32))
    v, lens = st.pull(tk)
    assert int(lens.min()) == 261
    st.push(tk, H.kGradient, c.tensor(rng.standard_normal(v.numel()).astype(np.float32),
                                      torch.float32), lens)
    c.sync()
    s = H.Store(c)
    hs, hd = str(tmp_path / "h.bin"), str(tmp_path / "h.txt")
    s.save(hs, True)
    s.dump(hd, True, False)
    want_s, want_d = open(hs, "rb").read(), open(hd, "rb").read()
    assert len(want_s) > 100 * 2104
    for chunk in (0, 257):
        p = str(tmp_path / "d.bin")
        st = s.save(p, True, device=True, chunk_slots=chunk)
        assert open(p, "rb").read() == want_s
        assert st["host_chunks"] == 0 and st["bytes"] == len(want_s)
        p = str(tmp_path / "d.txt")
        st = s.dump(p, True, False, device=True, chunk_slots=chunk)
        print("V_dim 260 dump, chunk_slots %d: %s" % (chunk, st))
        assert open(p, "rb").read() == want_d
        assert st["entries"] == want_d.count(b"\n")
    c.close()


@pytest.mark.parametrize("chunk", [1, 63, 64, 65])
def test_tiny_table(H, tmp_path, chunk):
    """max_keys = 1 << 8: chunks with no survivor, and a survivor alone in its chunk"""
    c = H.Context(0, max_keys=1 << 8, V_dim=4, V_threshold=1, l1=0.02, lr=.1, V_lr=.02)
    blk = D.synthetic(40, 4, 1 << 5, seed=3)
    for step in range(2):
        H.train_step(c, H.DeviceRowBlock(c, blk), H.kTraining, push_cnt=True)
    H.progress(c)
    s = H.Store(c)
    cap = s.capacity()
    for aux in (0, 1):
        hs, hd = str(tmp_path / "h.bin"), str(tmp_path / "h.txt")
        s.save(hs, bool(aux))
        s.dump(hd, bool(aux), True)
        want_s, want_d = open(hs, "rb").read(), open(hd, "rb").read()
        assert 0 < want_d.count(b"\n") < cap  # some chunks of one slot hold nothing
        ps, pd = str(tmp_path / "d.bin"), str(tmp_path / "d.txt")
        st = s.save(ps, bool(aux), device=True, chunk_slots=chunk)
        assert open(ps, "rb").read() == want_s
        assert st["chunks"] == -(-cap // chunk) and st["entries"] == want_d.count(b"\n")
        st = s.dump(pd, bool(aux), True, device=True, chunk_slots=chunk)
        assert open(pd, "rb").read() == want_d
        assert st["chunks"] == -(-cap // chunk) and st["host_chunks"] == 0
    c.close()


def test_empty_store(H, tmp_path):
    c = H.Context(0, max_keys=1 << 8, V_dim=4)
    s = H.Store(c)
    for aux in (0, 1):
        p = str(tmp_path / "e.bin")
        st = s.save(p, bool(aux), device=True)
        assert open(p, "rb").read() == bytes([aux])
        assert st["entries"] == 0 and st["bytes"] == 1 and st["host_chunks"] == 0
        p = str(tmp_path / "e.txt")
        st = s.dump(p, bool(aux), False, device=True)
        assert open(p, "rb").read() == b""
        assert st["entries"] == 0 and st["bytes"] == 0 and st["host_chunks"] == 0
    c.close()


# ---- a crafted model ------------------------------------------------------------------------
def _edge_floats(tmp):
    p = str(tmp / "edges.f32")
    subprocess.run([CHECK, "edgelist", p], check=True, timeout=60)
    return np.fromfile(p, np.float32)


def _in_domain(x):
    a = np.abs(x.astype(np.float64))
    return np.isfinite(a) & ((a == 0) | ((a >= 1e-12) & (a < 1e12)))


def _write_model(path, d, entries):
    """SGDUpdater::Save's format with aux: entries of (key, w, sqrt_g, z, V | None, Vaux | None)"""
    with open(path, "wb") as f:
        f.write(b"\x01")
        for key, w, sg, z, V, C in entries:
            f.write(struct.pack("<Qi", key, 1 + d if V is not None else 1))
            f.write(np.float32([w, sg, z]).tobytes())
            if V is not None:
                f.write(np.float32(V).tobytes() + np.float32(C).tobytes())


def _crafted(tmp, d, floats, seed):
    """the edge keys; w = 0 and w = -0.0 without V (neither is written); w = -0.0 with V (it
    is); then each float alone in w, sqrt_g, z, V[0], V[d-1], Vaux[0] and Vaux[d-1] of an entry
    of its own -> (entries, those the files hold)"""
    rng = np.random.RandomState(seed)
    base = np.float32([.25, -1.5, 3, 1e-3][:d] + [2.0] * max(0, d - 4))
    ent = [(k, np.float32(.5 + i), np.float32(1), np.float32(2), base + i, base * 2)
           for i, k in enumerate(EDGE_KEYS)]
    ent.append((12345, np.float32(0), np.float32(1), np.float32(2), None, None))
    ent.append((12346, np.float32(-0.0), np.float32(1), np.float32(2), None, None))
    ent.append((12347, np.float32(-0.0), np.float32(1), np.float32(2), base, base))
    held = len(ent) - 2
    keys = set(k for k, *_ in ent)
    for x in floats:
        for pos in range(7):
            k = int(rng.randint(1, 2 ** 62)) * 2 + 1
            while k in keys:
                k += 2
            keys.add(k)
            st = [np.float32(1.5), np.float32(1), np.float32(2)]
            V, C = base.copy(), (base * 2).copy()
            if pos < 3:
                st[pos] = x
            elif pos < 5:
                V[0 if pos == 3 else d - 1] = x
            else:
                C[0 if pos == 5 else d - 1] = x
            ent.append((k, st[0], st[1], st[2], V, C))
            held += 1
    return ent, held


@pytest.mark.parametrize("bad", [False, True])
def test_crafted_model(H, tmp_path, bad):
    d = 4
    edges = _edge_floats(tmp_path)
    floats = list(edges[_in_domain(edges)])
    bad_floats = [np.float32(np.inf), np.float32(np.nan), np.float32(1e-20), np.float32(1e-40),
                  np.float32(1e13)]
    if bad:
        floats = floats[::7] + bad_floats
    ent, held = _crafted(tmp_path, d, floats, seed=5)
    src = str(tmp_path / "crafted.bin")
    _write_model(src, d, ent)
    c = H.Context(0, max_keys=1 << 12, V_dim=d)
    s = H.Store(c)
    s.load(src)
    cap = s.capacity()
    n_bad = 7 * len(bad_floats) if bad else 0
    for aux in (0, 1):
        hs = str(tmp_path / "h.bin")
        s.save(hs, bool(aux))
        want_s = open(hs, "rb").read()
        assert len(want_s) == 1 + held * (16 + 8 * aux + 4 * d * (1 + aux))
        for rev in (0, 1):
            hd = str(tmp_path / "h.txt")
            s.dump(hd, bool(aux), bool(rev))
            want_d = open(hd, "rb").read()
            assert want_d.count(b"\n") == held
            for chunk in (16, 256, cap):
                p = str(tmp_path / "d.txt")
                st = s.dump(p, bool(aux), bool(rev), device=True, chunk_slots=chunk)
                assert open(p, "rb").read() == want_d, (aux, rev, chunk)
                assert st["entries"] == held
                h = st["host_chunks"]
                # without aux, sqrt_g, z and Vaux are not printed: 3 of the 7 places remain
                nb = n_bad if aux else 3 * len(bad_floats) if bad else 0
                if not bad:
                    assert h == 0
                elif chunk == cap:
                    assert h == 1 and st["chunks"] == 1
                else:
                    assert 1 <= h <= nb, (h, nb)
        for chunk in (16, 256, cap):
            p = str(tmp_path / "d.bin")
            st = s.save(p, bool(aux), device=True, chunk_slots=chunk)
            assert open(p, "rb").read() == want_s
            assert st["host_chunks"] == 0 and st["entries"] == held
    c.close()


def _records(data, d):
    """a Save file -> (aux, {key: record bytes})"""
    aux = data[0]
    out, i = {}, 1
    while i < len(data):
        key, size = struct.unpack_from("<Qi", data, i)
        n = 16 + 8 * aux + (4 * d * (1 + aux) if size > 1 else 0)
        assert size in (1, d + 1) and key not in out
        out[key] = data[i:i + n]
        i += n
    assert i == len(data)
    return aux, out


def test_round_trip(H, models, tmp_path):
    """a device-saved file, loaded into a fresh context and saved by the host, reproduces
    itself: the same length and, key by key, the same records (the loader inserts the keys in
    parallel, so keys that share a home slot may swap places in the fresh table)"""
    ctx, _ = models
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    H.Store(ctx(8, "auto")).save(a, True, device=True)
    c = H.Context(0, max_keys=1 << 16, slot_layout="auto", **dict(CFG, V_dim=8))
    H.Store(c).load(a)
    H.Store(c).save(b, True)
    da, db = open(a, "rb").read(), open(b, "rb").read()
    assert len(da) == len(db)
    assert _records(da, 8) == _records(db, 8)
    c.close()


# ---- one chunk into caller memory -----------------------------------------------------------
def _one_chunk(H, c, text, aux, slot0, n, cap_bytes, size):
    out = torch.full((size + GUARD,), 0xA5, dtype=torch.uint8, device=c.device)
    if text:
        stat = H.model_format(c, slot0, n, aux, True, out, cap_bytes)
    else:
        stat = H.model_pack(c, slot0, n, aux, out, cap_bytes)
    return stat, bytes(out.cpu().numpy().tobytes())


@pytest.mark.parametrize("text", [False, True])
@pytest.mark.parametrize("V_dim,layout", [(4, "auto"), (28, "auto")])
def test_one_chunk_capacity(H, models, V_dim, layout, text):
    """the whole table as one chunk: capacity exact, one byte short, one record / line short,
    64 guard bytes behind; nothing at or past the capacity is written and stat reports the need"""
    ctx, host = models
    c = ctx(V_dim, layout)
    want = host(V_dim, layout, "dump", 1, 1) if text else host(V_dim, layout, "save", 1)[1:]
    need = len(want)
    n_ent = host(V_dim, layout, "dump", 1, 1).count(b"\n")
    cap = H.Store(c).capacity()
    if text:
        last = need - (want.rfind(b"\n", 0, need - 1) + 1)
    else:
        i = 0
        while i < need:  # records of 24 bytes, or with V and Vaux behind
            last = 24 + (8 * V_dim if struct.unpack_from("<i", want, i + 8)[0] > 1 else 0)
            i += last
        assert i == need
    for cb in (need, need - 1, need - last):
        stat, out = _one_chunk(H, c, text, 1, 0, cap, cb, need)
        assert stat == [need, cb, n_ent, 0], (cb, stat)
        assert out[:cb] == want[:cb]
        assert out[cb:] == b"\xa5" * (need - cb + GUARD)
    # three ranges laid end to end are the file
    cuts = [0, 1000, 1777, cap]
    got = b""
    for lo, hi in zip(cuts, cuts[1:]):
        stat, out = _one_chunk(H, c, text, 1, lo, hi - lo, need, need)
        assert stat[1] == stat[0] and out[stat[0]:] == b"\xa5" * (need - stat[0] + GUARD)
        got += out[:stat[0]]
    assert got == want


def test_one_chunk_rejects(H, models):
    ctx, _ = models
    c = ctx(4, "auto")
    cap = H.Store(c).capacity()
    out = torch.zeros(64, dtype=torch.uint8, device=c.device)
    from difacto_amd._lib import DfxError
    for slot0, n in ((-1, 1), (0, cap + 1), (cap, 1)):
        with pytest.raises(DfxError):
            H.model_pack(c, slot0, n, 1, out, 64)
        with pytest.raises(DfxError):
            H.model_format(c, slot0, n, 1, 0, out, 64)
    with pytest.raises(DfxError):
        H.model_pack(c, 0, 1, 1, out[1:], 32)  # not dword aligned
