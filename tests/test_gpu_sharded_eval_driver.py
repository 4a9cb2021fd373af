"""dfx_train's sharded runs validate (data_val) and predict (task=2), from the command line, on
loopback shards of one GPU (and one RCCL shard at world size 1): the Validation line against
the sharded oracle of the run's schedule, the stop rules, the per-rank prediction files against
the single-GPU run, and the batch cache's validation lists.

Bounds, all the project's own: a printed loss within 1e-5 relative of the oracle's (what
tests/test_host_cpp.py holds the sharded training loss to), the AUC within rel 1e-4 / abs 1e-6
(tests/test_gpu_dist.py:112); written predictions through test_gpu_dist's `close` at rtol 2e-5 =
its 1e-5 plus %g's rounding (six digits: 5e-6 relative on each side)."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_gpu_dist import close
from tests.test_host_cpp import _part_rows, _slice

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_BIN = os.path.join(ROOT, "build", "dfx_train")
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")
KW = dict(V_dim=4, V_threshold=1, lr=0.1, V_lr=0.05, l1=0.1, seed=7)
KWARGS = ["%s=%s" % kv for kv in KW.items()] + ["max_keys=65536"]
BS, EPOCHS = 10, 3
TRAIN = ["data_in=" + DATA, "num_jobs_per_epoch=1", "shuffle=0", "batch_size=%d" % BS,
         "max_num_epochs=%d" % EPOCHS, "stop_rel_objv=0", "stop_val_auc=-1"] + KWARGS


def _run(args, env=None):
    assert os.path.exists(TRAIN_BIN), "build/dfx_train missing: run make"
    r = subprocess.run([TRAIN_BIN] + args, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _fields(out, tag):
    """the reference's part of every `tag` line: 'Rows = .., loss = .., AUC = ..'"""
    return [l.split(tag + ": ")[1].split("  (")[0] for l in out.splitlines() if tag + ":" in l]


def _nums(field):
    m = re.fullmatch(r"Rows = (\d+), loss = (\S+), AUC = (\S+)", field)
    assert m, field
    return int(m.group(1)), float(m.group(2)), float(m.group(3))


def _shard_args(shards, exchange, pipelined):
    return ["shards=%d" % shards, "exchange=" + exchange, "pipelined=%d" % pipelined,
            "push_agg=sum"]


def _oracle_epochs(N, stale):
    """per epoch (train loss, val loss, val auc), all per row: the driver's schedule on the
    batches it forms — shard g trains part g of N in batches of BS (the shards step together),
    the store is flushed, then one validation step on the shards' whole parts"""
    from difacto_amd import data as D
    from oracle import dist_oracle as DO
    from oracle import oracle as O
    blk = D.read_libsvm(DATA)
    parts = [_part_rows(DATA, p, N) for p in range(N)]
    nsteps = max((len(p) + BS - 1) // BS for p in parts)
    so = DO.StaleOracle(N, agg="sum", **KW) if stale else DO.AggOracle(N, **KW)
    out = []
    for ep in range(EPOCHS):
        loss = 0.0
        for t in range(nsteps):
            step = [_slice(blk, parts[p][t * BS:(t + 1) * BS]) for p in range(N)]
            o = so.submit(step, push_cnt=ep == 0) if stale else so.step(step, push_cnt=ep == 0)
            loss += sum(x[0] for x in o)
        if stale:
            so.flush()
        val = [_slice(blk, parts[p]) for p in range(N)]
        o = so.submit(val, train=False) if stale else so.step(val, train=False)
        vauc = 0.0
        for b, x in zip(val, o):
            if b.size:
                vauc += O.auc_stable_ties(b.labels, x[2]) if O.has_ties(x[2]) else x[1]
        out.append((loss / blk.size, sum(x[0] for x in o) / blk.size, vauc / blk.size))
    return out


_ORACLE = {}


def _oracle(N, stale):
    if (N, stale) not in _ORACLE:
        _ORACLE[(N, stale)] = _oracle_epochs(N, stale)
    return _ORACLE[(N, stale)]


def _check_validation(tmp_path, shards, exchange, pipelined, env=None, without_too=True):
    N = abs(shards)
    sh = _shard_args(shards, exchange, pipelined)
    with_val = _run(TRAIN + sh + ["data_val=" + DATA, "has_aux=1",
                                  "model_out=" + str(tmp_path / "v")], env)
    tr, va = _fields(with_val, "Training"), _fields(with_val, "Validation")
    assert len(tr) == EPOCHS and len(va) == EPOCHS, with_val
    # every Validation line directly after its Training line
    lines = [l for l in with_val.splitlines() if l.startswith("Epoch[")]
    assert [l.split(":")[0].split("] ")[1] for l in lines] == ["Training", "Validation"] * EPOCHS
    # the split's pipelined schedule equals the synchronous one; a2a's is 1-step stale
    want = _oracle(N, stale=bool(pipelined) and exchange == "a2a")
    for ep in range(EPOCHS):
        rows, loss, auc = _nums(va[ep])
        print(exchange, pipelined, shards, ep, "val loss", loss, want[ep][1], "auc", auc,
              want[ep][2])
        assert rows == 100
        assert abs(_nums(tr[ep])[1] - want[ep][0]) <= 1e-5 * abs(want[ep][0]), (ep, tr[ep])
        assert abs(loss - want[ep][1]) <= 1e-5 * abs(want[ep][1]), (ep, loss, want[ep][1])
        assert auc == pytest.approx(want[ep][2], rel=1e-4, abs=1e-6), (ep, auc, want[ep][2])
    if not without_too:
        return
    # validation changes nothing the training sees
    without = _run(TRAIN + sh + ["has_aux=1", "model_out=" + str(tmp_path / "t")], env)
    assert tr == _fields(without, "Training")
    for g in range(N):
        assert filecmp.cmp(str(tmp_path / ("v_part-%d" % g)), str(tmp_path / ("t_part-%d" % g)),
                           shallow=False), g


@pytest.mark.parametrize("pipelined", [0, 1])
@pytest.mark.parametrize("exchange", ["a2a", "split"])
def test_validation_matches_oracle(tmp_path, exchange, pipelined):
    _check_validation(tmp_path, 3, exchange, pipelined)


def test_validation_two_shards(tmp_path):
    _check_validation(tmp_path, 2, "a2a", 1)


def test_validation_rccl_world1(tmp_path):
    """shards=-1: one shard over RCCL at world size 1.  One run (the communicators take most
    of its seconds): the Training and Validation lines against the 1-shard stale oracle; the
    comparison with the run without data_val is the loopback cases'"""
    env = dict(os.environ, DFX_COMM_ID_FILE=str(tmp_path / "id"))
    env.pop("WORLD_SIZE", None)
    _check_validation(tmp_path, -1, "a2a", 1, env, without_too=False)
    assert not os.path.exists(str(tmp_path / "id"))


@pytest.mark.parametrize("exchange", ["a2a", "split"])
def test_rank_without_validation_rows(tmp_path, exchange):
    """data_val of two lines over three shards: one shard reads no row and steps along with
    empty batches; the run ends (the subprocess timeout is the hang check)"""
    val = tmp_path / "two.libsvm"
    val.write_text("".join(open(DATA).readlines()[:2]))
    parts = [_part_rows(str(val), p, 3) for p in range(3)]
    assert sorted(len(p) for p in parts)[0] == 0 and sum(len(p) for p in parts) == 2
    out = _run(TRAIN + _shard_args(3, exchange, 1) + ["data_val=" + str(val),
                                                      "max_num_epochs=2"])
    va = _fields(out, "Validation")
    assert len(va) == 2 and all(_nums(v)[0] == 2 for v in va), out


@pytest.mark.parametrize("exchange", ["a2a", "split"])
def test_validation_auc_stop_rule(exchange):
    """no AUC gain reaches stop_val_auc=1e9: every shard leaves after epoch 0's validation"""
    out = _run([a for a in TRAIN if not a.startswith("stop_val_auc")] +
               _shard_args(3, exchange, 1) + ["data_val=" + DATA, "stop_val_auc=1e9"])
    assert len(_fields(out, "Training")) == 1 and len(_fields(out, "Validation")) == 1, out


# ---- prediction ------------------------------------------------------------------------------
def _read_pred(path):
    rows = [l.split("\t") for l in open(path).read().splitlines()]
    return [r[0] for r in rows], [r[1] for r in rows]


def _reassemble(prefix, N, J, data=DATA):
    """the ranks' files in the single-GPU order: part p of J * N belongs to rank p mod N at
    job p div N, and a rank writes its parts' rows in the order it read them"""
    files = [_read_pred("%s_part-%d" % (prefix, g)) for g in range(N)]
    at = [0] * N
    labels, preds = [], []
    for p in range(J * N):
        g, n = p % N, len(_part_rows(data, p, J * N))
        labels += files[g][0][at[g]:at[g] + n]
        preds += files[g][1][at[g]:at[g] + n]
        at[g] += n
    assert at == [len(f[0]) for f in files], (at, [len(f[0]) for f in files])
    return labels, np.array([float(x) for x in preds])


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    """a model trained on one GPU, and its own task=2 predictions at 3 and 6 parts"""
    d = tmp_path_factory.mktemp("single")
    m = str(d / "m")
    _run(["data_in=" + DATA, "num_jobs_per_epoch=1", "shuffle=0", "batch_size=30",
          "max_num_epochs=3", "stop_rel_objv=0", "model_out=" + m] + KWARGS)
    ref = {}
    for jobs, prob in ((3, 0), (6, 0), (3, 1)):
        out = str(d / ("p%d_%d" % (jobs, prob)))
        _run(["task=2", "data_val=" + DATA, "model_in=" + m, "pred_out=" + out,
              "num_jobs_per_epoch=%d" % jobs, "pred_prob=%d" % prob] + KWARGS)
        labels, preds = _read_pred(out + "_part-0")
        ref[(jobs, prob)] = (labels, np.array([float(x) for x in preds]))
        assert len(labels) == 100
    return m, ref


@pytest.mark.parametrize("jobs,prob", [(1, 0), (2, 0), (1, 1)])
@pytest.mark.parametrize("exchange", ["a2a", "split"])
def test_sharded_prediction_matches_single_gpu(tmp_path, single, exchange, jobs, prob):
    m, ref = single
    N = 3
    out = str(tmp_path / "p")
    text = _run(["task=2", "data_val=" + DATA, "model_in=" + m, "model_in_parts=1",
                 "pred_out=" + out, "num_jobs_per_epoch=%d" % jobs, "pred_prob=%d" % prob,
                 "cache=device" if exchange == "a2a" else "cache=none"] +
                _shard_args(N, exchange, 1) + KWARGS)
    assert sorted(f for f in os.listdir(str(tmp_path))) == ["p_part-%d" % g for g in range(N)]
    pl = [l for l in text.splitlines() if l.startswith("Prediction: ")]
    assert len(pl) == 1 and _nums(pl[0][len("Prediction: "):])[0] == 100, text
    labels, preds = _reassemble(out, N, jobs)
    want_labels, want = ref[(jobs * N, prob)]
    assert labels == want_labels
    print(exchange, jobs, prob, "max |diff|", float(np.max(np.abs(preds - want))))
    assert close(preds, want, rtol=2e-5)


@pytest.mark.parametrize("exchange", ["a2a", "split"])
def test_sharded_model_predicts_from_its_own_parts(tmp_path, exchange):
    """a model three servers saved, used by three shards as it is and by two shards through
    model_in_parts=3"""
    s = str(tmp_path / "s")
    sh3, sh2 = _shard_args(3, exchange, 1), _shard_args(2, exchange, 1)
    _run(TRAIN + sh3 + ["model_out=" + s])
    common = ["task=2", "data_val=" + DATA, "model_in=" + s, "num_jobs_per_epoch=1",
              "pred_prob=0"] + KWARGS
    _run(common + sh3 + ["pred_out=" + str(tmp_path / "a")])
    _run(common + sh2 + ["model_in_parts=3", "pred_out=" + str(tmp_path / "b")])
    la, pa = _reassemble(str(tmp_path / "a"), 3, 1)
    lb, pb = _reassemble(str(tmp_path / "b"), 2, 1)
    assert len(la) == 100 and la == lb
    assert np.any(pa != 0)
    assert close(pa, pb, rtol=2e-5)


def test_empty_rank_still_writes_its_file(tmp_path, single):
    m, _ = single
    val = tmp_path / "two.libsvm"
    val.write_text("".join(open(DATA).readlines()[:2]))
    out = str(tmp_path / "p")
    text = _run(["task=2", "data_val=" + str(val), "model_in=" + m, "model_in_parts=1",
                 "pred_out=" + out, "num_jobs_per_epoch=1"] + _shard_args(3, "a2a", 1) + KWARGS)
    sizes = [len(open("%s_part-%d" % (out, g)).read().splitlines()) for g in range(3)]
    assert sorted(sizes)[0] == 0 and sum(sizes) == 2, sizes
    assert "Prediction: Rows = 2," in text


# ---- the batch cache's validation lists ----------------------------------------------------
def _cache_line(out):
    m = re.findall(r"^cache=device: (\d+) batches, ([\d.]+) MB held, (\d+) of (\d+) parts not "
                   r"cached$", out, re.M)
    assert len(m) == 1, out
    return int(m[0][0]), int(m[0][2]), int(m[0][3])


def test_batch_cache_replays_validation(tmp_path):
    """cache=device exchange=a2a data_val=F, 3 epochs: the printed fields and the model parts
    equal cache=none's, and the cache holds the validation batches too (one per shard: a
    shard's validation part is one chunk) in lists of their own"""
    sh = _shard_args(3, "a2a", 1)
    outs = {}
    for c in ("none", "device"):
        outs[c] = _run(TRAIN + sh + ["data_val=" + DATA, "cache=" + c, "has_aux=1",
                                     "model_out=" + str(tmp_path / ("m_" + c))])
    for tag in ("Training", "Validation"):
        a, b = _fields(outs["none"], tag), _fields(outs["device"], tag)
        assert len(a) == EPOCHS and a == b, (tag, a, b)
    for g in range(3):
        assert filecmp.cmp(str(tmp_path / ("m_none_part-%d" % g)),
                           str(tmp_path / ("m_device_part-%d" % g)), shallow=False), g
    train_only = _cache_line(_run(TRAIN + sh + ["cache=device"]))
    both = _cache_line(outs["device"])
    assert train_only[1] == 0 and both[1] == 0
    assert both[0] == train_only[0] + 3, (both, train_only)
    assert both[2] == train_only[2] + 3, (both, train_only)  # parts: 3 training + 3 validation
