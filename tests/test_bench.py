"""bench.py's plain run and --dump-outputs (the fused step; the sharded bench's options are
exercised in test_gpu_dist.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "3001", "--key-bits", "14"] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_dumps_reproducible_outputs(tmp_path):
    """A plain run reports the headline fields and nothing that takes a run of its own;
    --dump-outputs writes the last timed step's predictions, the timed steps' progress and
    the pulled model sample as float32 / float64 .npy files under 64 MB, and two runs with the
    same arguments (seeded inputs, a deterministic step) write identical arrays."""
    outs, dumps = [], []
    for name in ("a", "b"):
        d = tmp_path / name
        outs.append(_bench("--dump-outputs", str(d)))
        dumps.append({f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(str(d)))})
    out = outs[0]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "train examples/sec" and out["higher_is_better"] is True
    assert out["dtype"] == "f32" and out["value"] > 0
    # (ms_per_step is rounded to 1e-4 ms: 5e-3 covers a step of 0.01 ms)
    assert out["value"] == pytest.approx(3001 / (out["ms_per_step"] * 1e-3), rel=5e-3)
    for moved in ("cpu_baseline", "roofline", "roofline_forward", "step_window", "lanes_ms",
                  "host_call_ms_idle_device"):
        assert moved not in out, moved
    a, b = dumps
    assert set(a) == set(b) == {"pred", "progress", "model_vals", "model_lens"}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.isfinite(a[k]).all(), k
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert a["pred"].shape == (3001,) and a["pred"].dtype == np.float32
    rows, loss, auc = a["progress"]
    assert rows == 3 * 3001
    assert loss / rows == pytest.approx(out["train_loss_per_row"], abs=1e-6)
    assert auc / rows == pytest.approx(out["train_auc"], abs=1e-6)
    # Store::Pull's layout: w alone, or [w | V(16)] for a key counted in the count-push epoch
    lens = a["model_lens"]
    assert lens.size > 0 and np.isin(lens, (1, 17)).all() and (lens == 17).any()
    assert a["model_vals"].size == int(lens.sum())
    assert np.abs(a["model_vals"]).max() > 0
