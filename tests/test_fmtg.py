"""csrc/fmtg.h, the text of a prediction row as the device writer forms it (pred_write=device),
against the host's snprintf("%g") and the driver's probability expression, on the CPU
(build/fmtg_check, tools/fmtg_check.cc): every output is glibc's bytes or flagged, and inside
the guaranteed domain (+-0, 1e-12 <= |x| < 1e12) nothing is flagged.  Also dfx_train's
pred_write= argument, which is checked in main before any context exists, and the binding."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CHECK = os.path.join(ROOT, "build", "fmtg_check")
TRAIN = os.path.join(ROOT, "build", "dfx_train")


def check(*args):
    r = subprocess.run([CHECK] + list(args), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ALL PASSED" in r.stdout, (r.returncode, r.stdout, r.stderr)
    m = re.search(r"(\d+) checked, (\d+) flagged, (\d+) bad", r.stdout)
    assert m and int(m.group(3)) == 0, r.stdout
    return int(m.group(1)), int(m.group(2))


def test_edges():
    checked, flagged = check("edges")
    # the list holds subnormals, non-finite values and values past both ends: some are flagged,
    # most are not
    assert checked > 8000 and 0 < flagged < 100


@pytest.mark.parametrize("mode", ["floats", "probs"])
def test_every_4099th_float(mode):
    checked, flagged = check(mode, "4099")  # 2^32 / 4099: 1 047 809 floats
    assert checked == 1047809
    if mode == "probs":
        # a probability leaves the domain only below 1e-14, above it is 1 or nearly
        assert flagged < checked // 100


def test_sample():
    checked, flagged = check("sample", "1000000", "1")
    # log-uniform over 26 decades: about one decade (1e-13 .. 1e-14 is formatted) and the top
    # one lie outside the formatter's domain
    assert checked == 1000000 and flagged < checked // 10


@pytest.mark.parametrize("args,need", [
    (("pred_write=x",), "pred_write must be host or device"),
    (("pred_write=device", "fused=0"), "fused=1"),
    (("pred_write=device", "fused=0", "task=2", "model_in=m", "data_val=v"), "fused=1"),
], ids=["bad_value", "fused_0", "fused_0_task_2"])
def test_refused_pred_write_arguments_exit_2(args, need):
    r = subprocess.run([TRAIN, "data_in=x"] + list(args), capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2, (r.returncode, r.stdout, r.stderr)
    assert "pred_write" in r.stderr and need in r.stderr, r.stderr


def test_python_binding_declares_the_predtext_entry_points():
    from difacto_amd import _lib
    from difacto_amd import hotpath as H
    for name in ("dfx_format_pred", "dfx_predtext_create", "dfx_predtext_submit",
                 "dfx_predtext_take", "dfx_predtext_destroy"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name)
    assert hasattr(H, "format_pred") and hasattr(H, "PredText")
