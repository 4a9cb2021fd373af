"""Criteo text parsed and batched on the device (difacto_amd/csrc/textparse.hip,
difacto_amd/host/device_reader.cc) against the host reader, which is the yardstick everywhere:
ParseCriteo, GatherRows, BatchReader and TextReader of difacto_amd/host/reader.cc.  The C++
driver is tests/host/textparse_tests.cc (build/textparse_tests); its CPU modes (the batch
planner, the raw-mode chunk cuts, the shared CityHash64) run without a GPU."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "textparse_tests")
TRAIN_BIN = os.path.join(ROOT, "build", "dfx_train")
GEN_BIN = os.path.join(ROOT, "build", "gen_criteo")
CONV_BIN = os.path.join(ROOT, "build", "dfx_convert")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cityhash_cells.json")


def _make(*targets):
    subprocess.check_call(["make", "-s"] + list(targets), cwd=ROOT)


def _gen(path, rows, seed=0):
    _make("build/gen_criteo")
    subprocess.check_call([GEN_BIN, str(path), str(rows), "65536", str(seed)])
    return str(path)


def _run(*args, timeout=120):
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=timeout)
    print(r.stdout[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    return r.stdout


# ---- CPU -----------------------------------------------------------------------------------
def test_planner_plans_batch_readers_batches(tmp_path):
    """BatchPlanner fed the host-parsed chunks' lengths and labels, its plan carried out with
    host GatherRows: the batches equal BatchReader's, batch by batch (5,000 rows, batch 257,
    64 KB chunks so most batches straddle chunks, shuffle 0 / 3, neg_sampling 1 / 0.7, parts
    0/1 and 1/2).  No HIP call."""
    _make("build/textparse_tests")
    out = _run("plan", _gen(tmp_path / "c.txt", 5000))
    assert out.count("batches ok") == 8


def test_text_reader_raw_mode_cuts(tmp_path):
    """TextReader::NextRaw cuts the chunks TextReader::Next parses: the raw chunks parsed by
    ParseCriteo equal the parsed chunks one by one, over chunk sizes, parts, both formats and a
    file without its last newline"""
    _make("build/textparse_tests")
    _run("cuts", _gen(tmp_path / "c.txt", 5000), tmp_path)


def test_cityhash_shared_header_keeps_the_hashes():
    """CityHash64 through csrc/cityhash.h (the text reader.cc and the device parser both
    compile) gives the values the reader gave before the move, for cells of every length of the
    sweep: 1..200 bytes, every length branch and several trips of the 64-byte loop"""
    _make("build/textparse_tests")
    want = json.load(open(GOLDEN))
    out = subprocess.check_output([BIN, "hashcells"], text=True, timeout=60)
    cells = [l.split("\t") for l in out.splitlines()]
    assert len(cells) == 15 * 39
    assert {len(c) for c, _ in cells} == {1, 3, 4, 7, 8, 16, 17, 32, 33, 64, 65, 127, 128, 129,
                                          200}
    for cell, h in cells:
        assert want[cell] == h, cell


# ---- GPU -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_parse_equals_host_parser():
    """dfx_parse_criteo == ParseCriteo exactly (offset, index, label; is_train 1 and 0) with
    needs_host == 0 on generated rows, the cell-length sweep, 0..39 / 45 columns, one row and
    70,000 rows; capacities one too small; nbytes 0 and 2^31"""
    assert os.path.exists(BIN), "build/textparse_tests missing: run make"
    out = _run("parse")
    for tag in ("(a)", "(b)", "(c)", "(d)", "(e)", "(f)", "(g)"):
        assert "parse " + tag in out, tag


@pytest.mark.gpu
def test_fallback_forms_flagged_or_equal():
    """CRLF, blank lines, labels 1.5 / abc / empty / +1 and an unterminated last line: each
    result is needs_host == 1 or exactly ParseCriteo's output"""
    assert os.path.exists(BIN), "build/textparse_tests missing: run make"
    out = _run("fallback")
    assert "fallback label +1 is_train=1: equal" in out


@pytest.mark.gpu
def test_gather_equals_host_gather():
    """dfx_gather_rows == GatherRows: a range, a permuted list, a list with gaps, n = 0,
    appending at r0 > 0, zero-length source rows"""
    assert os.path.exists(BIN), "build/textparse_tests missing: run make"
    _run("gather")


@pytest.mark.gpu
def test_device_batch_reader_equals_batch_reader(tmp_path):
    """DeviceBatchReader == BatchReader batch by batch on 5,000 generated rows (the grid of
    the planner test), every chunk as one batch, and a file whose chunks the device hands back
    to the host parser"""
    assert os.path.exists(BIN), "build/textparse_tests missing: run make"
    out = _run("batches", _gen(tmp_path / "c.txt", 5000), tmp_path)
    assert out.count("batches ok") == 8 and "chunks parsed by the host ok" in out


def _train(args, timeout=120):
    r = subprocess.run([TRAIN_BIN] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _fields(out, tag):
    """the printed "Rows = .., loss = .., AUC = .." of every line of a kind"""
    got = [l.split(tag + ": ")[1].split("  (")[0] for l in out.splitlines() if tag + ":" in l]
    assert got, out
    return got


def _read_bare_libsvm(path):
    """dfx_convert's libsvm text of binary rows: "label id id ..." (data.read_libsvm wants
    id:val)"""
    offs, ids, labels = [0], [], []
    for line in open(path):
        tok = line.split()
        labels.append(float(tok[0]))
        ids.extend(int(t) for t in tok[1:])
        offs.append(len(ids))
    return (np.array(offs, np.uint64), np.array(ids, np.uint64), np.array(labels, np.float32))


@pytest.mark.gpu
def test_driver_parse_device_equals_parse_host(tmp_path):
    """dfx_train parse=device against parse=host on 3,000 rows, shuffled and down-sampled,
    with validation: the same printed loss / AUC fields, models with the same keys and
    bit-equal entries, byte-identical prediction files; parse=device with libsvm exits 2"""
    from oracle import oracle as O
    data = _gen(tmp_path / "c.txt", 3000)
    kw = ["V_dim=4", "V_threshold=1", "batch_size=250", "num_jobs_per_epoch=2",
          "max_num_epochs=2", "stop_rel_objv=0", "shuffle=3", "neg_sampling=0.7",
          "data_format=criteo", "max_keys=262144", "has_aux=1"]
    outs = {}
    for parse in ("host", "device"):
        outs[parse] = _train(["data_in=" + data, "data_val=" + data, "parse=" + parse,
                              "model_out=" + str(tmp_path / ("m_" + parse))] + kw)
    for tag in ("Training", "Validation"):
        a, b = _fields(outs["host"], tag), _fields(outs["device"], tag)
        assert len(a) == 2 and a == b, (tag, a, b)
    assert "parsed by the host" not in outs["device"]
    # the models: the same keys, bit-equal entries (slot order is not part of the contract)
    subprocess.check_call([CONV_BIN, "data_in=" + data, "data_format=criteo",
                           "data_out=" + str(tmp_path / "c.libsvm"), "data_out_format=libsvm"],
                          stdout=subprocess.DEVNULL)
    offs, ids, _ = _read_bare_libsvm(tmp_path / "c.libsvm")
    ups = {}
    for parse in ("host", "device"):
        ups[parse] = O.Updater(V_dim=4, V_threshold=1)
        ups[parse].load(str(tmp_path / ("m_" + parse)) + "_part-0")
    assert ups["host"].size() == ups["device"].size() > 0
    n = 0
    for k in O.localize(offs, ids)[0]:
        a, b = ups["host"].entry(k), ups["device"].entry(k)
        assert (a is None) == (b is None), k
        if a is None:
            continue
        n += 1
        assert a[0].tobytes() == b[0].tobytes(), k
        assert (a[1] is None) == (b[1] is None), k
        if a[1] is not None:
            assert a[1].tobytes() == b[1].tobytes(), k
    assert n == ups["host"].size()
    # prediction
    pred = {}
    for parse in ("host", "device"):
        p = str(tmp_path / ("pred_" + parse))
        out = _train(["task=2", "data_val=" + data, "model_in=" + str(tmp_path / "m_host"),
                      "pred_out=" + p, "num_jobs_per_epoch=2", "parse=" + parse, "V_dim=4",
                      "V_threshold=1", "data_format=criteo", "max_keys=262144"])
        assert "Prediction:" in out
        pred[parse] = open(p + "_part-0", "rb").read()
    assert len(pred["host"].splitlines()) == 3000
    assert pred["host"] == pred["device"]
    # no silent fall-back
    for bad in (["data_format=libsvm"], ["data_format=criteo", "fused=0"],
                ["data_format=criteo", "shards=2"]):
        r = subprocess.run([TRAIN_BIN, "data_in=" + data, "parse=device"] + bad,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "parse=device" in r.stderr, (bad, r.stdout, r.stderr)


@pytest.mark.gpu
def test_hotpath_parse_criteo(tmp_path):
    """hotpath.parse_criteo on 200 rows against the host reader's rows, written by
    dfx_convert data_out_format=libsvm and read back here"""
    from difacto_amd import hotpath as H
    data = _gen(tmp_path / "c.txt", 200, seed=5)
    subprocess.check_call([CONV_BIN, "data_in=" + data, "data_format=criteo",
                           "data_out=" + str(tmp_path / "c.libsvm"), "data_out_format=libsvm"],
                          stdout=subprocess.DEVNULL)
    offs, ids, labels = _read_bare_libsvm(tmp_path / "c.libsvm")
    ctx = H.Context(0, V_dim=0, max_keys=1024)
    blk, needs_host = H.parse_criteo(ctx, open(data, "rb").read())
    assert not needs_host and blk.size == 200
    assert np.array_equal(blk.offs, offs) and np.array_equal(blk.ids, ids)
    assert np.array_equal(blk.labels, labels) and blk.vals is None
    test_blk, needs_host = H.parse_criteo(ctx, open(data, "rb").read(), is_train=False)
    assert not needs_host and test_blk.size == 200 and not test_blk.labels.any()
    assert test_blk.nnz >= blk.nnz  # the label column is a feature column there
    _, needs_host = H.parse_criteo(ctx, b"1\t5\r\n")
    assert needs_host
    ctx.close()
