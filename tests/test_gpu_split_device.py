"""GpuSplitLearner's device entry driven from C++ (tests/host/split_device_tests.cc):
ProcessDeviceBatches on loopback N = 3 and N = 1 with batches of 7, 64 and 65 rows of 1-40 ids
and a hot id, FM V_dim = 4 and logit, valued and binary.

Every comparison is of bits and is made by the binary, which prints one line per comparison:
(a) steps fed device arrays after the first against the same steps fed host blocks (every
pulled word, the progress), (b) mixed steps (device, host, none), (c) the validation
predictions, (d) the recorded batches copied back against the host blocks, and the schedule
replayed from the caches against the host run of the doubled schedule, (e) 12 pipelined steps
alternating host and device items on 3 staging slots.  A device item reaches the split store
as the same bytes the feeder would have uploaded, so the step computes the same bits: nothing
here has a tolerance."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "split_device_tests")


@pytest.fixture(scope="module")
def run():
    assert os.path.exists(BIN), "build/split_device_tests missing: run make"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    print(r.stderr[-4000:])
    return r


def _lines(r, tag):
    return [l for l in r.stdout.splitlines() if " " + tag + " " in l]


def test_binary_passes(run):
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "ALL PASSED" in run.stdout and "DIFFER" not in run.stdout


# configurations: valued x loss x (N = 3: pipelined 0 and 1; N = 1: pipelined 1)
CONFIGS = 2 * 2 * 3


@pytest.mark.parametrize("tag,count", [
    ("(a) device", CONFIGS), ("(c) device", CONFIGS),
    ("(b) mixed", 2 * 2 * 2 * 2),       # N = 3 only, two lines each
    ("(d) record", CONFIGS), ("(d) replay", CONFIGS),
    ("(e) alternate", 2 * 2 * 2),       # pipelined only
])
def test_every_comparison_ran_and_is_equal(run, tag, count):
    lines = _lines(run, tag)
    assert len(lines) == count, (tag, lines)
    assert all(l.endswith(" equal") for l in lines), lines
