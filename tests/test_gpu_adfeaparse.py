"""adfea text parsed and batched on the device (difacto_amd/csrc/adfeaparse.hip, the adfea text
feed in textfeed.hip, difacto_amd/host/device_reader.cc, dfx_train parse_adfea=1) against the
host reader, which is the yardstick everywhere: ParseAdfea, GatherRows, BatchReader and
TextReader of difacto_amd/host/reader.cc.  Every comparison is exact.  The C++ driver is
tests/host/adfeaparse_tests.cc (build/adfeaparse_tests)."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

from tests import adfea_ref as A
from tests.test_gpu_sharded_parse_driver import _records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "adfeaparse_tests")
TRAIN_BIN = os.path.join(ROOT, "build", "dfx_train")
GEN_BIN = os.path.join(ROOT, "build", "gen_adfea")


def _gen(path, rows, seed, *shape):
    assert os.path.exists(GEN_BIN), "build/gen_adfea missing: run make"
    subprocess.check_call([GEN_BIN, str(path), str(rows), str(seed)] + [str(s) for s in shape])
    return str(path)


def _run(*args, timeout=120):
    assert os.path.exists(BIN), "build/adfeaparse_tests missing: run make"
    r = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True,
                       timeout=timeout)
    print(r.stdout[-6000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    return r.stdout


def test_parse_equals_host_parser():
    """dfx_parse_adfea == ParseAdfea exactly (offset, index, label) with needs_host == 0: the
    three-row sample, the smallest texts, every part of a feature token on the 16-byte and 4 KiB
    boundaries, a line over three tiles, the 64-byte token, blank runs, the id edges, the label
    rule, more than 1024 tiles, capacities one too small"""
    out = _run("parse")
    for tag in ("(a)", "(b)", "(c)", "(d)", "(e)", "(f)", "(g)", "(h)", "(i)", "(j)"):
        assert "parse " + tag in out, tag
    assert "parse (c) 30 boundary placements ok" in out


def test_fallback_forms_flagged_or_equal():
    """empty and blank-only lines, fewer than three tokens, a token without ':' at a feature
    place and one with ':' at a head place (the host's continued row) must be flagged; CRLF, an
    unterminated last line, the 65-byte token and the misshapen tokens are needs_host == 1 or
    exactly ParseAdfea's output"""
    out = _run("fallback")
    for must in ("empty line", "leading empty line", "blank-only line", "two tokens", "one token",
                 "no ':' at token 3", "no ':' at token 4", "':' at token 0", "':' at token 1",
                 "':' at token 2 (a continued row)"):
        assert "fallback %s: needs_host" % must in out, must
    assert "fallback a 65-byte token:" in out and out.count("fallback \"") == 14


def test_device_batch_reader_adfea_equals_batch_reader(tmp_path):
    """DeviceBatchReader("adfea") == BatchReader batch by batch, every batch unvalued, on the CPU
    planner test's file and grid, every chunk as one batch, a file whose 50,000-feature rows make
    the ring entry and the shuffle buffer grow mid-run, a file with flagged chunks, and a chunk
    that needs more features than its ':' bytes bound"""
    out = _run("batches", _gen(tmp_path / "rows.adfea", 5000, 7, 5, 15, 24, 39), tmp_path)
    assert out.count("batches (unvalued) ok") == 8 and "chunks parsed by the host ok" in out
    assert out.count("grow file") == 2 and "batches whole chunks:" in out
    assert "batches over_bound file:" in out


def test_textfeed_adfea_rejects_values_and_stays_usable():
    """on an adfea feed a value array and valued != 0 are DFX_ERR_ARG with a message and queue
    nothing; a three-row chunk then goes through the feed and equals the host's block, and a
    host-parsed chunk through _upload with value == NULL; the Criteo and libsvm feeds behave as
    before"""
    out = _run("feedargs")
    assert "feedargs criteo:" in out and "feedargs libsvm:" in out and "feedargs adfea:" in out


# ---- Python --------------------------------------------------------------------------------
def test_hotpath_parse_adfea(tmp_path):
    """hotpath.parse_adfea on the sample, the id edges and 300 generated rows with 64-bit ids
    against ParseAdfea's restatement (tests/adfea_ref.py); a CRLF chunk and a continued row are
    handed back"""
    from difacto_amd import hotpath as H
    ctx = H.Context(0, V_dim=0, max_keys=1024)
    gen = open(_gen(tmp_path / "g.adfea", 300, 3, 0, 9, 64, 4096), "rb").read()
    edges = (b"1 4 1 0:0 000017:0004095 4503599627370495:4095 4503599627370496:4096\n"
             b"2 3 10 18446744073709551615:1 18446744073709551616:18446744073709551616 "
             b"1234567890123456789012345:7\n3 0 01\n")
    for data in (b"1 3 1 17:2 123456789:4095 5:1\n2 1 0 9:7\n3 0 1\n", edges, gen, b""):
        want = A.parse(data)
        offs, ids, labels, stat = H.parse_adfea(ctx, data)
        assert not stat["needs_host"] and stat["rows"] == len(want[2])
        assert stat["nnz"] == len(want[1])
        assert np.array_equal(offs, np.array(want[0], np.uint64))
        assert np.array_equal(ids, np.array(want[1], np.uint64))
        assert labels.tobytes() == np.array(want[2], np.float32).tobytes()
    assert H.parse_adfea(ctx, b"1 1 1 5:2\r\n")[3]["needs_host"]
    assert H.parse_adfea(ctx, b"1 2 1 5:2\n6:3\n")[3]["needs_host"]
    ctx.close()


# ---- the driver ----------------------------------------------------------------------------
COMMON = ["data_format=adfea", "V_dim=4", "V_threshold=1", "num_jobs_per_epoch=2",
          "max_num_epochs=2", "stop_rel_objv=0", "stop_val_auc=-1", "max_keys=262144",
          "has_aux=1", "batch_size=50", "l1=0.01"]  # l1 small: 400 rows leave weights to save
DEVICE = ["parse=auto", "parse_adfea=1"]


@pytest.fixture(scope="module")
def rows400(tmp_path_factory):
    return _gen(tmp_path_factory.mktemp("adfea") / "rows400.adfea", 400, 5, 5, 15, 20, 39)


def _train(args, timeout=120):
    r = subprocess.run([TRAIN_BIN] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _fields(out, tag):
    """the printed "Rows = .., loss = .., AUC = .." of every line of a kind"""
    got = [l.split(tag + ": ")[1].split("  (")[0] for l in out.splitlines() if tag + ":" in l]
    assert got, out
    return got


def _same_models(tmp_path, a, b, parts=1):
    """the same keys with the same bytes each, aux words included (a model file lists the
    table's slots in order, and which slot a key takes is not part of the contract)"""
    for g in range(parts):
        ra = _records(str(tmp_path / ("%s_part-%d" % (a, g))))
        rb = _records(str(tmp_path / ("%s_part-%d" % (b, g))))
        assert len(ra) > 0 and ra.keys() == rb.keys(), g
        assert [k for k in ra if ra[k] != rb[k]] == [], g


def _pair(tmp_path, data, extra, device=DEVICE, line="parse: device (adfea)", parts=1,
          device_extra=()):
    """the command with parse=host and on the device parser: the start line, equal Training and
    Validation fields over two epochs, models equal entry for entry"""
    args = ["data_in=" + data, "data_val=" + data] + COMMON + list(extra)
    host = _train(args + ["parse=host", "model_out=" + str(tmp_path / "h")])
    dev = _train(args + list(device) + list(device_extra) + ["model_out=" + str(tmp_path / "d")])
    assert dev.splitlines()[0] == line, dev[:300]
    assert "parse:" not in host and "parsed by the host" not in dev
    for kind in ("Training", "Validation"):
        a, b = _fields(host, kind), _fields(dev, kind)
        assert len(a) == 2 and a == b, (kind, a, b)
    _same_models(tmp_path, "h", "d", parts)
    return host, dev


@pytest.mark.parametrize("mix", ["shuffle=0", "default shuffle", "neg_sampling=0.5"])
def test_driver_parse_adfea_equals_parse_host(tmp_path, rows400, mix):
    """dfx_train parse=auto parse_adfea=1 against parse=host on 400 generated rows (batch_size=50,
    validation, 2 epochs): the start line says device (adfea), the Training / Validation fields
    and the saved model, entry for entry, are parse=host's"""
    extra = [] if mix == "default shuffle" else [mix]
    host, _ = _pair(tmp_path, rows400, extra)
    rows = int(re.match(r"Rows = (\d+),", _fields(host, "Training")[0]).group(1))
    assert rows == 400 if mix != "neg_sampling=0.5" else 100 < rows < 400


def test_driver_parse_adfea_with_the_device_cache(tmp_path, rows400):
    """the same with cache=device: the recording epoch appends the adfea feed's batches, every
    part is cached, and the second epoch replays them"""
    _, dev = _pair(tmp_path, rows400, [], device_extra=["cache=device"])
    m = re.search(r"^cache=device: (\d+) batches, .* MB held, (\d+) of (\d+) parts not cached$",
                  dev, re.M)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) == 0, dev


def test_driver_parse_adfea_prediction_files_equal(tmp_path, rows400):
    """task=2 with pred_out: byte-equal prediction files"""
    _train(["data_in=" + rows400, "parse=host", "model_out=" + str(tmp_path / "m")] + COMMON)
    outs = {}
    for tag, parse in (("h", ["parse=host"]), ("d", DEVICE)):
        outs[tag] = _train(["task=2", "data_val=" + rows400, "model_in=" + str(tmp_path / "m"),
                            "pred_out=" + str(tmp_path / ("p" + tag)), "data_format=adfea",
                            "num_jobs_per_epoch=2", "V_dim=4", "V_threshold=1",
                            "max_keys=262144"] + parse)
        assert "Prediction:" in outs[tag]
    assert outs["d"].splitlines()[0] == "parse: device (adfea)", outs["d"][:300]
    a, b = str(tmp_path / "ph_part-0"), str(tmp_path / "pd_part-0")
    assert filecmp.cmp(a, b, shallow=False)
    assert len(open(a).read().splitlines()) == 400


@pytest.mark.parametrize("exchange", ["split", "a2a"])
def test_driver_parse_adfea_sharded(tmp_path, rows400, exchange):
    """parse=auto-sharded shards=2 parse_adfea=1: rank 0 prints device (adfea, 2 shards) and the
    run computes what parse=host computes, both exchanges"""
    _pair(tmp_path, rows400, ["shards=2", "exchange=" + exchange, "push_agg=sum"],
          device=["parse=auto-sharded", "parse_adfea=1"], line="parse: device (adfea, 2 shards)",
          parts=2)


def test_driver_parse_adfea_refusals(tmp_path, rows400):
    """no silent fall-back: parse_adfea=1 with another format or another parse value exits 2"""
    for args, need in ((["data_format=libsvm", "parse=auto"], "needs data_format=adfea"),
                       (["data_format=adfea", "parse=host"], "needs parse=auto or"),
                       (["data_format=adfea", "parse=device"], "needs parse=auto or")):
        r = subprocess.run([TRAIN_BIN, "data_in=" + rows400, "parse_adfea=1"] + args,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "parse_adfea=1 " + need in r.stderr, r.stderr
