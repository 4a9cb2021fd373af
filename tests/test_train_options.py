"""dfx_train's option rules on the CPU: ResolveOptions (difacto_amd/host/train_options.h), the one
function that holds every refusal, its precedence and the "parse:" / "cache:" lines, against the
truth table tests/host/train_options_tests.cc (no GPU, no library)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "train_options_tests")


def test_train_options_truth_table():
    subprocess.check_call(["make", "-s", "build/train_options_tests"], cwd=ROOT)
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr
