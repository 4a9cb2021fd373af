"""dfx_train's cache= arguments are checked in main before any context, learner or exchange is
created, so a refused combination exits 2 without a GPU (no silent run without the cache)."""
import os
import subprocess

import pytest

from conftest import ROOT

TRAIN = os.path.join(ROOT, "build", "dfx_train")


def run(*args):
    return subprocess.run([TRAIN, "data_in=x"] + list(args), capture_output=True, text=True,
                          timeout=60)


@pytest.mark.parametrize("args", [
    ("cache=bogus",),
    ("cache=device", "shards=2", "exchange=split"),
    ("cache=device", "fused=0"),
], ids=["unknown_value", "exchange_split", "fused_0"])
def test_refused_cache_arguments_exit_2(args):
    r = run(*args)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "cache" in r.stderr, r.stderr
