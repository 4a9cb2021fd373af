"""model_write's and task=1's option rules on the CPU: ResolveOptions
(difacto_amd/host/train_options.h) against the truth table
tests/host/train_options_model_tests.cc (the model_write value, task=1 with and without model_in,
sharded, and with no data_in; no GPU, no library), the tables of every older option passing
unchanged, and the bindings and the header declaring the new entry points."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dfx_model_pack", "dfx_model_format", "dfx_store_save_dev", "dfx_store_dump_dev")


# each table's own success line
TABLES = {"train_options_model_tests": "train_options_model_tests: ALL PASSED (",
          "train_options_tests": "ALL PASSED (",
          "train_options_adfea_tests": "train_options_adfea_tests: ALL PASSED (",
          "train_options_resample_tests": "train_options_resample_tests: all passed"}


def test_model_write_truth_table():
    for name, line in TABLES.items():
        subprocess.check_call(["make", "-s", "build/" + name], cwd=ROOT)
        r = subprocess.run([os.path.join(ROOT, "build", name)], capture_output=True, text=True,
                           timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.strip().splitlines()[-1].startswith(line), r.stdout
        assert "FAILED" not in r.stdout


def test_bindings_and_header_declare_the_entry_points():
    from difacto_amd import _lib, hotpath
    header = open(os.path.join(ROOT, "include", "difacto_amd.h")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTED
        assert re.search(r"^int %s\(dfx_ctx\* ctx," % name, header, re.M), name
    assert callable(hotpath.model_pack) and callable(hotpath.model_format)
    import inspect
    for fn, keys in ((hotpath.Store.save, ("device", "chunk_slots")),
                     (hotpath.Store.dump, ("device", "chunk_slots"))):
        params = inspect.signature(fn).parameters
        assert all(k in params and params[k].default in (False, 0) for k in keys)
    from difacto_amd import dist
    assert inspect.signature(dist.Shard.save).parameters["device"].default is False
