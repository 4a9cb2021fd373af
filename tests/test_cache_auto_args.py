"""dfx_train's cache=auto is checked in main before any context is made, as cache=device is: a
negative budget exits 2 without a GPU, on every path cache=auto could take."""
import os
import subprocess

import pytest

from conftest import ROOT

TRAIN = os.path.join(ROOT, "build", "dfx_train")


def run(*args):
    return subprocess.run([TRAIN, "data_in=x"] + list(args), capture_output=True, text=True,
                          timeout=60)


@pytest.mark.parametrize("args", [
    (),
    ("shards=2", "exchange=split"),
    ("shards=2", "exchange=a2a"),
    ("fused=0",),
], ids=["fused", "exchange_split", "exchange_a2a", "fused_0"])
def test_negative_budget_exits_2(args):
    r = run("cache=auto", "cache_mb=-1", *args)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "cache" in r.stderr, r.stderr
    assert r.stdout == "", r.stdout  # refused before the line that names the path
