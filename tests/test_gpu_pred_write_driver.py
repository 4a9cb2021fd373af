"""dfx_train task=2 pred_write=device from the command line: every <pred_out>_part-<rank> is
byte-identical to pred_write=host's (the parent's writer) and the "Prediction:" line is the
same, on the single-GPU fused path with parse=host and parse=device (Criteo) or parse=auto
(libsvm), pred_prob 0 and 1, and on two loopback shards with both exchanges; a batch holding a
prediction outside the device formatter's domain is written by the host loop in its place and
counted."""
import filecmp
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_BIN = os.path.join(ROOT, "build", "dfx_train")
GEN_BIN = os.path.join(ROOT, "build", "gen_criteo")
RCV1 = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
CRITEO_KW = ["V_dim=4", "V_threshold=1", "max_keys=262144"]
RCV1_KW = ["V_dim=4", "V_threshold=1", "lr=0.1", "V_lr=0.05", "l1=0.1", "seed=7",
           "max_keys=65536"]


def _run(args):
    assert os.path.exists(TRAIN_BIN), "build/dfx_train missing: run make"
    r = subprocess.run([TRAIN_BIN] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _prediction_line(out):
    pl = [l for l in out.splitlines() if l.startswith("Prediction: ")]
    assert len(pl) == 1, out
    return pl[0]


def _writer_line(out):
    """(rows, host batches) of the device writer's lines"""
    m = re.findall(r"^pred_write=device: (\d+) rows, pass [\d.]+ s, the host waited [\d.]+ s for "
                   r"text$", out, re.M)
    assert len(m) == 1, out
    hb = re.findall(r"^pred_write=device: (\d+) batch(?:es)? written by the host", out, re.M)
    assert len(hb) <= 1, out
    return int(m[0]), int(hb[0]) if hb else 0


def _both_writers(tmp_path, args, ranks=(0,), rows=None, host_batches=0):
    """the same task=2 run with either writer: equal files, equal Prediction lines"""
    outs = {}
    for w in ("host", "device"):
        outs[w] = _run(["task=2", "pred_out=" + str(tmp_path / w), "pred_write=" + w] + args)
    assert _prediction_line(outs["host"]) == _prediction_line(outs["device"])
    assert "pred_write=device" not in outs["host"]
    got_rows, got_hb = _writer_line(outs["device"])
    total = 0
    for g in ranks:
        a, b = str(tmp_path / ("host_part-%d" % g)), str(tmp_path / ("device_part-%d" % g))
        assert filecmp.cmp(a, b, shallow=False), g
        total += len(open(a).read().splitlines())
    assert total == rows and got_rows == rows
    assert got_hb == host_batches
    return outs


@pytest.fixture(scope="module")
def criteo(tmp_path_factory):
    """3000 generated Criteo rows and a small FM trained on them"""
    d = tmp_path_factory.mktemp("criteo")
    data, model = str(d / "c.txt"), str(d / "m")
    subprocess.check_call([GEN_BIN, data, "3000", "65536", "0"])
    _run(["data_in=" + data, "data_format=criteo", "max_num_epochs=2", "num_jobs_per_epoch=1",
          "batch_size=100", "model_out=" + model] + CRITEO_KW)
    return data, model


@pytest.mark.parametrize("prob", [0, 1])
@pytest.mark.parametrize("parse", ["host", "device"])
def test_criteo_files_equal(tmp_path, criteo, parse, prob):
    data, model = criteo
    _both_writers(tmp_path, ["data_val=" + data, "data_format=criteo", "model_in=" + model,
                             "num_jobs_per_epoch=2", "parse=" + parse, "pred_prob=%d" % prob]
                  + CRITEO_KW, rows=3000)


@pytest.fixture(scope="module")
def rcv1_model(tmp_path_factory):
    m = str(tmp_path_factory.mktemp("rcv1") / "m")
    _run(["data_in=" + RCV1, "num_jobs_per_epoch=1", "shuffle=0", "batch_size=30",
          "max_num_epochs=3", "stop_rel_objv=0", "model_out=" + m] + RCV1_KW)
    return m


@pytest.mark.parametrize("prob", [0, 1])
@pytest.mark.parametrize("parse", ["host", "auto"])
def test_rcv1_files_equal(tmp_path, rcv1_model, parse, prob):
    _both_writers(tmp_path, ["data_val=" + RCV1, "model_in=" + rcv1_model,
                             "num_jobs_per_epoch=2", "parse=" + parse, "pred_prob=%d" % prob]
                  + RCV1_KW, rows=100)


def test_a_batch_outside_the_domain_is_written_by_the_host(tmp_path):
    """a logistic regression (no clip of the prediction) and one row whose feature values are
    1e15: its raw prediction leaves 1e-12 <= |x| < 1e12, the batch (part 0 of 2) is written by
    the host loop, the other by the device, and the file is still the host writer's"""
    kw = ["loss=logit", "lr=0.1", "l1=0", "seed=7", "max_keys=65536"]
    m = str(tmp_path / "m")
    _run(["data_in=" + RCV1, "num_jobs_per_epoch=1", "shuffle=0", "batch_size=30",
          "max_num_epochs=3", "stop_rel_objv=0", "model_out=" + m] + kw)
    lines = open(RCV1).read().splitlines()
    first = lines[0].split()
    big = " ".join([first[0]] + [t.split(":")[0] + ":1e15" for t in first[1:]])
    val = tmp_path / "val.libsvm"
    val.write_text("\n".join([big] + lines) + "\n")
    outs = _both_writers(tmp_path, ["data_val=" + str(val), "model_in=" + m,
                                    "num_jobs_per_epoch=2", "pred_prob=0"] + kw,
                         rows=101, host_batches=1)
    row0 = open(str(tmp_path / "host_part-0")).readline().split("\t")
    assert not (1e-12 <= abs(float(row0[1])) < 1e12), row0
    assert "1 batch written by the host" in outs["device"]


@pytest.mark.parametrize("exchange", ["a2a", "split"])
def test_two_shards_files_equal(tmp_path, rcv1_model, exchange):
    _both_writers(tmp_path, ["data_val=" + RCV1, "model_in=" + rcv1_model, "model_in_parts=1",
                             "num_jobs_per_epoch=2", "pred_prob=1", "shards=2",
                             "exchange=" + exchange, "pipelined=1", "push_agg=sum"] + RCV1_KW,
                  ranks=(0, 1), rows=100)


def test_without_task_2_the_option_does_nothing(tmp_path):
    a = _run(["data_in=" + RCV1, "num_jobs_per_epoch=1", "shuffle=0", "batch_size=30",
              "max_num_epochs=1", "pred_write=device"] + RCV1_KW)
    assert "pred_write" not in a and "Epoch[0] Training:" in a
