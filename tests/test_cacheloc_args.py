"""dfx_train's cache_loc= argument is checked in main before any context, learner or exchange
is created, so a refused combination exits 2 without a GPU and names what the option needs (no
silent run without the kept Localizer outputs)."""
import os
import subprocess

import pytest

from conftest import ROOT

TRAIN = os.path.join(ROOT, "build", "dfx_train")


def run(*args):
    return subprocess.run([TRAIN, "data_in=x"] + list(args), capture_output=True, text=True,
                          timeout=60)


@pytest.mark.parametrize("args,need", [
    (("cache_loc=1",), "cache=device"),
    (("cache_loc=1", "cache=none"), "cache=device"),
    (("cache_loc=1", "cache=device", "fused=0"), "fused=1"),
    (("cache_loc=1", "cache=device", "task=2"), "task=2"),
    (("cache_loc=1", "cache=device", "shards=2"), "shards=0"),
    (("cache_loc=1", "cache=device", "shards=2", "exchange=split"), "shards=0"),
], ids=["no_cache", "cache_none", "fused_0", "task_2", "sharded", "sharded_split"])
def test_refused_cache_loc_arguments_exit_2(args, need):
    r = run(*args)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "cache_loc=1 needs" in r.stderr and need in r.stderr, r.stderr


def test_python_binding_declares_the_loc_entry_points():
    """the prototypes of _lib.py and a dfx_loc of the header's layout (8 pointers, 4 int64, a
    uint64, two int32, a pointer: 128 bytes)"""
    import ctypes
    from difacto_amd import _lib
    for name in ("dfx_batchcache_append_loc", "dfx_batchcache_get_loc",
                 "dfx_batchcache_stats_loc", "dfx_train_step_loc"):
        assert name in _lib.EXPORTED
    assert ctypes.sizeof(_lib.Loc) == 8 * 8 + 4 * 8 + 8 + 2 * 4 + 8
    assert _lib.Loc.form.offset == 104 and _lib.Loc.served.offset == 112
