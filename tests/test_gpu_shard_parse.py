"""Both sharded stores fed by DeviceBatchReaders, driven from C++
(tests/host/shard_parse_tests.cc): GpuShardedStore (a2a) and GpuSplitLearner (split) on
loopback N = 3, pipelined 0 and 1, over rcv1-100 and 500 generated Criteo rows with
chunk_bytes=4096 and batch_size=5, so every text slot and ring entry of the 4-deep feeds is
reused many times while the stores mark a batch one step late.

Every comparison is of bits and is made by the binary, one line per comparison: the shards'
progress sums and saved model files against the same stores fed the host reader's blocks.  The
feed's batches are the host reader's bytes and the stores compute the same bits from the same
bytes, so nothing here has a tolerance.  The last lines are the case that omits the marks: the
reader throws after handing out a ring's worth of batches (all but one slot, for whole chunks)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "shard_parse_tests")
GEN_BIN = os.path.join(ROOT, "build", "gen_criteo")
RCV1 = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    assert os.path.exists(BIN), "build/shard_parse_tests missing: run make"
    d = tmp_path_factory.mktemp("shard_parse")
    criteo = str(d / "c.txt")
    subprocess.check_call([GEN_BIN, criteo, "500", "65536", "0"])
    r = subprocess.run([BIN, RCV1, criteo, str(d)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    print(r.stderr[-4000:])
    return r


def test_binary_passes(run):
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "ALL PASSED" in run.stdout and "DIFFER" not in run.stdout


# data x store x pipelined
CONFIGS = 2 * 2 * 2


@pytest.mark.parametrize("what", ["steps", "progress", "models",
                                  "(every batch marked after the flush)",
                                  "(the host run stepped: every row validated, some trained)"])
def test_every_comparison_ran_and_is_equal(run, what):
    lines = [l for l in run.stdout.splitlines() if l.startswith("data=") and
             l.endswith(" " + what + " equal")]
    assert len(lines) == CONFIGS, (what, run.stdout[-3000:])


def test_omitted_marks_throw(run):
    assert "omitted marks, minibatches: 4 handed out, threw" in run.stdout
    assert "omitted marks, whole chunks: 3 handed out, threw" in run.stdout
