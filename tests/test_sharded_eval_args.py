"""dfx_train's argument checks for evaluation in sharded runs: everything here is decided
before any context is created, so it runs without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_BIN = os.path.join(ROOT, "build", "dfx_train")
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")


def _run(args):
    assert os.path.exists(TRAIN_BIN), "build/dfx_train missing: run make"
    # no device is visible to the child: reaching dfx_ctx_create could not end in these exits
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return subprocess.run([TRAIN_BIN] + args, capture_output=True, text=True, timeout=60, env=env)


def test_sharded_prediction_needs_model_and_data(tmp_path):
    """task=2 shards=2 without model_in, without data_val, and with exchange=split: exit 2
    with the single path's message, and no longer the 'training only' refusal"""
    model = "model_in=" + str(tmp_path / "m")
    for args in (["task=2", "shards=2", "data_val=" + DATA],
                 ["task=2", "shards=2", model],
                 ["task=2", "shards=2", "exchange=split", "data_val=" + DATA],
                 ["task=2", "shards=2", "exchange=split", model]):
        r = _run(args)
        assert r.returncode == 2, (args, r.returncode, r.stderr)
        assert "prediction needs model_in and data_val" in r.stderr, (args, r.stderr)
        assert "training only" not in r.stderr, (args, r.stderr)


def test_stop_val_auc_is_a_numeric_key():
    """stop_val_auc=abc is rejected where the other numeric keys are (while the arguments are
    parsed, as stop_rel_objv=abc is), not taken for an updater kwarg"""
    bad = _run(["data_in=" + DATA, "shards=2", "stop_val_auc=abc"])
    ref = _run(["data_in=" + DATA, "shards=2", "stop_rel_objv=abc"])
    assert ref.returncode != 0
    assert bad.returncode == ref.returncode, (bad.returncode, ref.returncode, bad.stderr)
    assert "Epoch" not in bad.stdout
    assert "dfx_ctx_create" not in bad.stderr and "hip" not in bad.stderr.lower(), bad.stderr
