"""csrc/modeltext.h, the device model dump's lines, on the CPU: build/modeltext_check
(tools/modeltext_check.cc, plain g++) compares it with a real std::ostream, which is what
SGDUpdater::Dump and dfx_store_dump print through.  The floats come from `fmtg_check edgelist`
(every boundary of csrc/fmtg.h) and from random bit patterns: a line inside the formatter's
domain is the stream's bytes, a line outside answers "needs host"."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_KEYS = [0, 1, 9, 10, 99, 10 ** 19 - 1, 10 ** 19, 2 ** 63, 2 ** 64 - 2]


def _tool(name):
    subprocess.check_call(["make", "-s", "build/" + name], cwd=ROOT)
    return os.path.join(ROOT, "build", name)


def _run(*args):
    r = subprocess.run([_tool("modeltext_check")] + [str(a) for a in args], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    return r.stdout


def test_edge_keys():
    """keys 0, 1, 9, 10, 99, 10^19 - 1, 10^19, 2^63 and 2^64 - 2, as stored and reversed"""
    out = _run("keys")
    rows = re.findall(r"^key (\d+) rev ([01]) length (\d+)$", out, re.M)
    assert sorted(set(int(k) for k, _, _ in rows)) == sorted(EDGE_KEYS)
    assert len(rows) == 2 * len(EDGE_KEYS)
    for k, rev, n in rows:
        if rev == "0":
            assert int(n) == len(str(int(k)))
    assert "keys: 18 checked, 0 differ" in out


def test_u64_lengths():
    """the least and the greatest key of every decimal length 1..20"""
    out = _run("lens")
    rows = [tuple(int(x) for x in l.split()) for l in out.splitlines()
            if re.match(r"^\d+ \d+ \d+$", l)]
    assert len(rows) == 40
    assert sorted(set(r[0] for r in rows)) == list(range(1, 21))
    for L, v, n in rows:
        assert n == L == len(str(v)), (L, v, n)
    assert (20, 2 ** 64 - 1, 20) in rows and (1, 0, 1) in rows
    assert "lens: 0 differ" in out


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("aux", [0, 1])
@pytest.mark.parametrize("D", [0, 4, 16])
def test_lines(tmp_path, D, aux, rev):
    edges = str(tmp_path / "edges.f32")
    subprocess.run([_tool("fmtg_check"), "edgelist", edges], check=True, timeout=60)
    out = _run("lines", 20000, 1000 + 8 * D + 2 * aux + rev, D, aux, rev, edges)
    m = re.search(r"lines: (\d+) equal, (\d+) need the host, 0 differ, longest (\d+) of (\d+)", out)
    assert m, out[-500:]
    same, host, longest, worst = (int(g) for g in m.groups())
    assert same + host == 20000
    assert same > 10000 and host > 500  # both kinds of line were seen
    assert longest <= worst
