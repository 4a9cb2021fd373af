"""parse_adfea's option rules on the CPU: ResolveOptions (difacto_amd/host/train_options.h)
against the truth table tests/host/train_options_adfea_tests.cc (the key across the parse values,
shards, fused and the data formats; no GPU, no library), the table of every other option passing
unchanged, and the binding of the new entry point."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_adfea_truth_table():
    for name in ("train_options_adfea_tests", "train_options_tests"):
        subprocess.check_call(["make", "-s", "build/" + name], cwd=ROOT)
        r = subprocess.run([os.path.join(ROOT, "build", name)], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0 and "ALL PASSED" in r.stdout, r.stdout + r.stderr


def test_python_binding_declares_the_adfea_parser():
    from difacto_amd import _lib, hotpath
    assert "dfx_parse_adfea" in _lib.EXPORTED
    assert callable(hotpath.parse_adfea)
    header = open(os.path.join(ROOT, "include", "difacto_amd.h")).read()
    assert "DFX_TEXT_ADFEA = 2" in header
