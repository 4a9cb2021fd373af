"""dfx_train's model_write=host|device and task=1, from the command line, on
tests/golden/rcv1_100.libsvm with 2 epochs and V_dim=4: model_out under the device writer
against the host writer's on every path (the single-GPU run with fused=1 and fused=0, two
loopback shards with both exchanges, every part), task=1's name_dump under both writers with
need_reverse and dump_aux against each other and against Store.dump of the loaded model, the
refusals, and the printed lines.

Two invocations are two processes, each with a table of its own, and keys that share a home slot
sit in the order their parallel inserts won (the fused step's and the loader's alike): files of
two processes are compared entry by entry - the same length, and for every key the same record
or line - which is byte equality up to that order.  Byte equality on one table is
tests/test_gpu_modelfile.py's."""
import os
import re
import struct
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_BIN = os.path.join(ROOT, "build", "dfx_train")
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
D = 4
KWARGS = ["V_dim=%d" % D, "V_threshold=1", "lr=0.1", "V_lr=0.05", "l1=0.1", "seed=7",
          "max_keys=65536"]
TRAIN = ["data_in=" + DATA, "num_jobs_per_epoch=1", "shuffle=0", "batch_size=10",
         "max_num_epochs=2", "stop_rel_objv=0", "has_aux=1"] + KWARGS
PATHS = {"fused1": (["fused=1"], 1), "fused0": (["fused=0"], 1),
         "a2a": (["shards=2", "exchange=a2a"], 2), "split": (["shards=2", "exchange=split"], 2)}
WRITE_LINE = re.compile(r"^model_write=device: (\d+) entries, (\d+\.\d) MB in (\d+\.\d{3}) s, "
                        r"the host waited (\d+\.\d{3}) s for chunks$", re.M)
DUMP_LINE = re.compile(r"^Dump: (\d+) entries, (\d+) bytes in (\d+\.\d{3}) s$", re.M)


def _run(args, rc=0):
    assert os.path.exists(TRAIN_BIN), "build/dfx_train missing: run make"
    r = subprocess.run([TRAIN_BIN] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == rc, r.stdout + r.stderr
    return r


def _records(data):
    """a Save file -> (aux, {key: record bytes})"""
    aux = data[0]
    out, i = {}, 1
    while i < len(data):
        key, size = struct.unpack_from("<Qi", data, i)
        n = 16 + 8 * aux + (4 * D * (1 + aux) if size > 1 else 0)
        assert size in (1, D + 1) and key not in out
        out[key] = data[i:i + n]
        i += n
    assert i == len(data)
    return aux, out


def _lines(text):
    """a Dump file -> {key: line}"""
    out = {}
    for line in text.split(b"\n")[:-1]:
        key = int(line.split(b"\t")[0])
        assert key not in out
        out[key] = line
    assert text.endswith(b"\n") and len(out) == text.count(b"\n")
    return out


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """path name -> (host run's stdout, device run's stdout, [host part files], [device's])"""
    tmp = tmp_path_factory.mktemp("model_write")
    out = {}
    for name, (args, parts) in PATHS.items():
        h, d = str(tmp / (name + "_host")), str(tmp / (name + "_dev"))
        rh = _run(TRAIN + args + ["model_out=" + h])
        rd = _run(TRAIN + args + ["model_out=" + d, "model_write=device"])
        out[name] = (rh.stdout, rd.stdout, ["%s_part-%d" % (h, r) for r in range(parts)],
                     ["%s_part-%d" % (d, r) for r in range(parts)])
    return out


@pytest.mark.parametrize("name", list(PATHS))
def test_model_out_equals_the_host_writers(trained, name):
    host_out, dev_out, host_files, dev_files = trained[name]
    entries = nbytes = 0
    for hf, df in zip(host_files, dev_files):
        a, b = open(hf, "rb").read(), open(df, "rb").read()
        assert len(a) == len(b) > 1
        ra, rb = _records(a), _records(b)
        assert ra[0] == 1 and ra == rb
        entries += len(rb[1])
        nbytes += len(b)
    assert entries > 1000
    # the device run says what it wrote; the default run prints what it printed before
    m = WRITE_LINE.findall(dev_out)
    assert len(m) == 1, dev_out
    assert int(m[0][0]) == entries and abs(float(m[0][1]) - nbytes / 2 ** 20) <= 0.05
    assert float(m[0][3]) <= float(m[0][2])
    assert "model_write" not in host_out
    heads = lambda s: [l.split(":")[0] for l in s.splitlines()  # noqa: E731
                       if not l.startswith("model_write=device")]
    assert heads(dev_out) == heads(host_out) and "Epoch[1] Training" in heads(host_out)


def test_model_write_without_model_out_does_nothing(tmp_path):
    r = _run(TRAIN + ["model_write=device", "max_num_epochs=1"])
    assert "model_write" not in r.stdout and "Epoch[0] Training" in r.stdout


@pytest.fixture(scope="module")
def store_dumps(trained, tmp_path_factory):
    """(dump_aux, need_reverse) -> Store.dump of the model loaded in this process"""
    from difacto_amd import hotpath as H
    tmp = tmp_path_factory.mktemp("store_dump")
    c = H.Context(0, V_dim=D, max_keys=65536)
    H.Store(c).load(trained["fused1"][2][0])
    out = {}
    for aux in (0, 1):
        for rev in (0, 1):
            p = str(tmp / ("d%d%d.txt" % (aux, rev)))
            H.Store(c).dump(p, bool(aux), bool(rev))
            out[(aux, rev)] = open(p, "rb").read()
    c.close()
    return out


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("aux", [0, 1])
def test_task1_dumps_the_model(trained, store_dumps, tmp_path, aux, rev):
    model = trained["fused1"][2][0]
    want = store_dumps[(aux, rev)]
    got = {}
    for writer in ("host", "device"):
        p = str(tmp_path / (writer + ".txt"))
        r = _run(["task=1", "model_in=" + model, "V_dim=%d" % D, "max_keys=65536",
                  "name_dump=" + p, "dump_aux=%d" % aux, "need_reverse=%d" % rev,
                  "model_write=" + writer])
        got[writer] = open(p, "rb").read()
        m = DUMP_LINE.findall(r.stdout)
        assert len(m) == 1, r.stdout
        assert int(m[0][0]) == got[writer].count(b"\n") and int(m[0][1]) == len(got[writer])
        # every float of this model is inside the device formatter's domain
        assert "written by the host" not in r.stdout
        assert "Epoch[" not in r.stdout
    assert len(got["host"]) == len(got["device"]) == len(want) > 0
    assert _lines(got["host"]) == _lines(got["device"]) == _lines(want)
    n_fields = set(l.count(b"\t") for l in _lines(want).values())
    assert n_fields == ({2 + 2 * aux, 2 + 2 * aux + D * (1 + aux)})


def test_task1_default_name_and_no_data_in(trained, tmp_path):
    """name_dump defaults to dump.txt (in the working directory); data_in is not asked for"""
    r = subprocess.run([TRAIN_BIN, "task=1", "model_in=" + trained["fused1"][2][0],
                        "V_dim=%d" % D], capture_output=True, text=True, timeout=120,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout + r.stderr
    assert DUMP_LINE.search(r.stdout)
    assert os.path.getsize(str(tmp_path / "dump.txt")) > 0


@pytest.mark.parametrize("args,message", [
    (TRAIN + ["model_write=gpu"], "model_write must be host or device"),
    (TRAIN + ["model_write=gpu", "model_out=x"], "model_write must be host or device"),
    (["task=1"], "dump needs model_in"),
    (["task=1", "data_in=" + DATA], "dump needs model_in"),
    (["task=1", "model_in=x", "shards=2"], "task=1 needs the single-GPU run (shards=0)"),
])
def test_refusals(args, message):
    r = _run(args, rc=2)
    assert r.stderr.strip().splitlines()[-1] == message
    assert "Epoch[" not in r.stdout and "Dump:" not in r.stdout
