"""dfx_train cache=auto from the command line: exchange=split runs record their batches in the
first epoch and replay them from the device batch cache afterwards, and compute what the same
command computes with cache=none; on the paths cache=device already serves, cache=auto is
cache=device; with fused=0 it is no cache.

Data and settings are tests/test_gpu_sharded_eval_driver.py's (rcv1_100.libsvm, batch_size=10,
V_dim=4 V_threshold=1 max_keys=65536, 3 epochs, stop_rel_objv=0 stop_val_auc=-1, push_agg=sum).
"Equal" is what that file demands of two sharded runs of one command: equal Training /
Validation fields and filecmp-equal <model_out>_part-<g> with has_aux=1.  A replayed batch is
the bytes the reader's batch was uploaded as, and the split step computes the same bits from
the same bytes in the same order, so nothing here has a tolerance.  Two cache=none runs of each
command used here (shards=3 at pipelined 0 and 1, shards=2 num_jobs_per_epoch=2, the two-line
data_val over three shards, shards=-1) were compared once on an MI355X and met this."""
import filecmp
import os
import re

import pytest

from tests.test_gpu_sharded_eval_driver import (DATA, EPOCHS, KWARGS, TRAIN, _cache_line, _fields,
                                                _nums, _oracle, _run, _shard_args)
from tests.test_host_cpp import _part_rows

pytestmark = pytest.mark.gpu


def _pair(tmp_path, args, a, b, N, env=None):
    """the command with cache=a and with cache=b ('' : no cache key): outputs, equal fields,
    equal model parts"""
    outs = []
    for tag, c in (("a", a), ("b", b)):
        outs.append(_run(args + (["cache=" + c] if c else []) +
                         ["has_aux=1", "model_out=" + str(tmp_path / tag)], env))
    for tag in ("Training", "Validation"):
        fa, fb = _fields(outs[0], tag), _fields(outs[1], tag)
        assert fa == fb, (tag, fa, fb)
    assert len(_fields(outs[0], "Training")) == EPOCHS, outs[0]
    for g in range(N):
        assert filecmp.cmp(str(tmp_path / ("a_part-%d" % g)), str(tmp_path / ("b_part-%d" % g)),
                           shallow=False), g
    return outs


def _jobs(args, n):
    return [a for a in args if not a.startswith("num_jobs_per_epoch")] + \
        ["num_jobs_per_epoch=%d" % n]


@pytest.mark.parametrize("pipelined", [0, 1])
def test_split_replays_and_equals_no_cache(tmp_path, pipelined):
    args = TRAIN + _shard_args(3, "split", pipelined) + ["data_val=" + DATA]
    auto, none = _pair(tmp_path, args, "auto", "none", 3)
    assert auto.splitlines()[0] == "cache: device (exchange=split)", auto
    assert not none.startswith("cache:")
    # the report follows epoch 0's lines: every part cached, 3 shards x (train, val)
    lines = auto.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("cache=device:")]
    assert len(at) == 1 and lines[at[0] - 1].startswith("Epoch[0] Validation:"), auto
    assert not any(l.startswith("Epoch[1]") for l in lines[:at[0]]), auto
    batches, dropped, parts = _cache_line(auto)
    assert (dropped, parts) == (0, 6), auto
    # a shard's part in batches of 10, and its validation part in one chunk
    want = sum((len(_part_rows(DATA, p, 3)) + 9) // 10 for p in range(3)) + 3
    assert batches == want, (batches, want)
    tr, va = _fields(auto, "Training"), _fields(auto, "Validation")
    assert len(va) == EPOCHS
    ora = _oracle(3, stale=False)  # the split's pipelined schedule equals the synchronous one
    for ep in range(EPOCHS):
        rows, loss, auc = _nums(va[ep])
        assert rows == 100 and _nums(tr[ep])[0] == 100
        assert abs(_nums(tr[ep])[1] - ora[ep][0]) <= 1e-5 * abs(ora[ep][0]), (ep, tr[ep])
        assert abs(loss - ora[ep][1]) <= 1e-5 * abs(ora[ep][1]), (ep, loss, ora[ep][1])
        assert auc == pytest.approx(ora[ep][2], rel=1e-4, abs=1e-6), (ep, auc, ora[ep][2])


def test_partly_cached_parts_are_read(tmp_path):
    """cache_mb=64 is one of the cache's 64 MiB blocks per shard, and a list owns its blocks:
    each shard keeps its first list (training job 0) and drops the three that follow; those
    parts are read while job 0 replays"""
    args = _jobs(TRAIN, 2) + _shard_args(2, "split", 1) + ["data_val=" + DATA, "cache_mb=64"]
    auto, _ = _pair(tmp_path, args, "auto", "none", 2)
    batches, dropped, parts = _cache_line(auto)
    assert (dropped, parts) == (6, 8), auto
    assert batches == sum((len(_part_rows(DATA, p, 4)) + 9) // 10 for p in (0, 1)), auto


def test_zero_budget_drops_everything(tmp_path):
    args = TRAIN + _shard_args(2, "split", 1) + ["data_val=" + DATA, "cache_mb=0"]
    auto, _ = _pair(tmp_path, args, "auto", "none", 2)
    assert _cache_line(auto) == (0, 4, 4), auto


def test_rank_with_an_empty_cached_validation_list(tmp_path):
    """data_val of two lines over three shards: one shard caches an empty validation list and
    steps along with empty batches in the replayed epochs (the subprocess timeout is the hang
    check)"""
    val = tmp_path / "two.libsvm"
    val.write_text("".join(open(DATA).readlines()[:2]))
    parts = [_part_rows(str(val), p, 3) for p in range(3)]
    assert sorted(len(p) for p in parts)[0] == 0 and sum(len(p) for p in parts) == 2
    args = TRAIN + _shard_args(3, "split", 1) + ["data_val=" + str(val)]
    auto, _ = _pair(tmp_path, args, "auto", "none", 3)
    va = _fields(auto, "Validation")
    assert len(va) == EPOCHS and all(_nums(v)[0] == 2 for v in va), auto
    assert _cache_line(auto)[1:] == (0, 6), auto  # the empty list is sealed, not dropped


def test_rccl_world1(tmp_path):
    """shards=-1: one shard over RCCL at world size 1"""
    env = dict(os.environ, DFX_COMM_ID_FILE=str(tmp_path / "id"))
    env.pop("WORLD_SIZE", None)
    args = TRAIN + _shard_args(-1, "split", 1) + ["data_val=" + DATA]
    auto, _ = _pair(tmp_path, args, "auto", "none", 1, env)
    assert auto.splitlines()[0] == "cache: device (exchange=split)", auto
    assert _cache_line(auto)[1:] == (0, 2), auto


@pytest.mark.parametrize("path", ["fused", "a2a"])
def test_auto_is_device_where_device_runs(tmp_path, path):
    sh = _shard_args(2, "a2a", 1) if path == "a2a" else []
    auto, dev = _pair(tmp_path, TRAIN + sh + ["data_val=" + DATA], "auto", "device",
                      2 if path == "a2a" else 1)
    assert auto.splitlines()[0] == "cache: device (%s)" % ("exchange=a2a" if sh else "fused"), auto
    assert _cache_line(auto) == _cache_line(dev)
    assert _cache_line(auto)[1] == 0


def test_auto_without_the_fused_path_is_no_cache(tmp_path):
    auto, plain = _pair(tmp_path, TRAIN + ["data_val=" + DATA, "fused=0"], "auto", "", 1)
    assert auto.splitlines()[0] == "cache: none (fused=0)", auto
    assert "cache=device:" not in auto
    assert _nums(_fields(auto, "Training")[0])[0] == 100
    # it trains: the loss falls
    assert _nums(_fields(auto, "Training")[-1])[1] < _nums(_fields(auto, "Training")[0])[1]
    assert not plain.startswith("cache:")


def test_prediction_accepts_the_key(tmp_path):
    """task=2 is one pass: cache=auto is accepted, no cache is made, the files are the same"""
    sh = _shard_args(3, "split", 1)
    m = str(tmp_path / "m")
    _run(TRAIN + sh + ["model_out=" + m])
    common = ["task=2", "data_val=" + DATA, "model_in=" + m, "num_jobs_per_epoch=1",
              "pred_prob=0"] + KWARGS + sh
    out_a = _run(common + ["cache=auto", "pred_out=" + str(tmp_path / "pa")])
    out_n = _run(common + ["cache=none", "pred_out=" + str(tmp_path / "pn")])
    assert out_a.splitlines()[0] == "cache: none (task=2)", out_a
    assert "cache=device:" not in out_a
    assert re.search(r"^Prediction: Rows = 100,", out_a, re.M), out_a
    assert out_a.splitlines()[1:] == out_n.splitlines()
    for g in range(3):
        assert os.path.getsize(str(tmp_path / ("pa_part-%d" % g))) > 0
        assert filecmp.cmp(str(tmp_path / ("pa_part-%d" % g)), str(tmp_path / ("pn_part-%d" % g)),
                           shallow=False), g
