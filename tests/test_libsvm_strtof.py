"""The CPU half of the device libsvm parser's tests: csrc/strtof.h (the text the device parser
compiles for its labels, values and ids) against the host's strtof / strtoull bit for bit
(tools/strtof_check.cc -> build/strtof_check), and the batch planner on valued rows with the
row-flag mirroring against BatchReader (tests/host/libsvmparse_tests.cc, mode plan).  The
yardstick is libc and the host reader, never Python's float()."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "build", "strtof_check")
GEN = os.path.join(ROOT, "build", "gen_libsvm")
BIN = os.path.join(ROOT, "build", "libsvmparse_tests")


def _make(*targets):
    subprocess.check_call(["make", "-s"] + list(targets), cwd=ROOT)


def _run(cmd, timeout=300):
    r = subprocess.run([str(a) for a in cmd], capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-4000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    return r.stdout


def test_strtof_random_strings_of_the_fast_grammar():
    """2,000,000 random strings per seed, every shape of the grammar (1-19 digits, the point at
    every position, leading and trailing zeros, q over [-27, 27], both signs, one in eight just
    outside): 0 differences from strtof, every string outside reported not fast"""
    _make("build/strtof_check")
    for seed in (1, 20261020):
        out = _run([CHECK, "sample", 2000000, seed])
        assert "2000000 strings" in out and " 0 differences" in out


def test_strtof_every_4099th_float():
    """every 4099th float bit pattern printed with %.9g: fast exactly when in the grammar, and
    then the float it was printed from"""
    _make("build/strtof_check")
    out = _run([CHECK, "floats", 4099])
    assert " 0 differences" in out
    assert int(out.split("strings, ")[1].split(" fast")[0]) > 500000


def test_strtof_edges_and_ids():
    """ties to even, FLT_MAX and the first inf inside |q| <= 27, the q = 27 | 28 and 19 | 20
    digit boundaries, signed zeros, the not-fast forms; ids of 19 / 20 / 30 digits, 2^64 - 1 and
    2^64 against strtoull"""
    _make("build/strtof_check")
    out = _run([CHECK, "edges"])
    assert " 0 differences; ids: 0 differences" in out


def test_planner_on_valued_rows_drops_values_where_batch_reader_does(tmp_path):
    """BatchPlanner fed the host-parsed libsvm chunks' lengths and labels, its plan carried out
    with host GatherRows and the row flags mirrored chunk -> shuffle buffer -> batch: the
    batches equal BatchReader's, including which ones have their values dropped (5,000 rows in
    blocks of valued and all-ones rows, batch 257, 64 KB chunks, shuffle 0 / 3, neg_sampling
    1 / 0.7, parts 0/1 and 1/2).  No HIP call."""
    _make("build/gen_libsvm", "build/libsvmparse_tests")
    data = tmp_path / "mixed.libsvm"
    subprocess.check_call([GEN, str(data), "5000", "7", "5", "15", "24", "3"])
    out = _run([BIN, "plan", data])
    assert out.count("batches ok") == 8
