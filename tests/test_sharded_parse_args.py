"""dfx_train parse=auto-sharded: the argument checks, which run in main before any context is
made (no GPU).  The value is accepted, the checks of the keys it is combined with still fire
with their own messages, and an unknown value's message lists it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_BIN = os.path.join(ROOT, "build", "dfx_train")
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")


def _fail(args):
    assert os.path.exists(TRAIN_BIN), "build/dfx_train missing: run make"
    r = subprocess.run([TRAIN_BIN, "data_in=" + DATA] + args, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    return r.stderr


def test_negative_cache_budget_is_named():
    err = _fail(["parse=auto-sharded", "shards=2", "cache=auto", "cache_mb=-1"])
    assert "cache" in err and "parse must be" not in err, err


def test_prediction_without_a_model():
    err = _fail(["parse=auto-sharded", "task=2", "shards=2"])
    assert "prediction needs" in err, err


def test_unknown_value_lists_the_new_one():
    err = _fail(["parse=bogus"])
    assert "parse must be" in err and "auto-sharded" in err, err


def test_old_values_keep_their_errors():
    """parse=device in a sharded run stays an error of its own"""
    err = _fail(["parse=device", "data_format=criteo", "shards=2"])
    assert "parse=device needs" in err, err
