"""dfx_train's epoch_shuffle= argument is checked in main before any context, learner or
exchange is created, so a refused combination exits 2 without a GPU and names what the option
needs (no silent run in the recorded order)."""
import os
import subprocess

import pytest

from conftest import ROOT

TRAIN = os.path.join(ROOT, "build", "dfx_train")


def run(*args):
    return subprocess.run([TRAIN, "data_in=x"] + list(args), capture_output=True, text=True,
                          timeout=60)


@pytest.mark.parametrize("args,need", [
    (("epoch_shuffle=1",), "cache=device"),
    (("epoch_shuffle=1", "cache=none", "shuffle_seed=3"), "cache=device"),
    (("epoch_shuffle=1", "cache=device", "cache_loc=1"), "cache_loc=0"),
    (("epoch_shuffle=1", "cache=device", "fused=0"), "fused=1"),
    (("epoch_shuffle=1", "cache=device", "task=2"), "task=2"),
    (("epoch_shuffle=1", "cache=device", "shards=2"), "shards=0"),
    (("epoch_shuffle=1", "cache=device", "shards=2", "exchange=split"), "shards=0"),
], ids=["no_cache", "cache_none", "cache_loc", "fused_0", "task_2", "sharded", "sharded_split"])
def test_refused_epoch_shuffle_arguments_exit_2(args, need):
    r = run(*args)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "epoch_shuffle=1 needs" in r.stderr and need in r.stderr, r.stderr


def test_python_binding_declares_the_reshuffle_entry_points():
    from difacto_amd import _lib
    from difacto_amd import hotpath as H
    for name in ("dfx_reshuffle_create", "dfx_reshuffle_destroy", "dfx_reshuffle_begin_epoch",
                 "dfx_reshuffle_next", "dfx_reshuffle_consumed", "dfx_reshuffle_stats"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name)
    assert hasattr(H, "Reshuffler")
