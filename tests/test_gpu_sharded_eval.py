"""The sharded stores' evaluation paths driven from C++ (tests/host/shard_eval_tests.cc):
GpuShardedStore::Submit with a validation job and prediction buffers, and GpuSplitLearner's
prediction output, on N = 1, 2, 3 loopback shards holding one loaded model, against the single
context's dfx_train_step(.., DFX_JOB_VALIDATION, .., pred_out) on the same rows.

The a2a path is pinned bit for bit.  Read from the kernels: a worker's forward on pulled
records (dfx_dist_fwd_bwd -> launch_fwd_records) is k_fm_fwd<G, CPL, kFused>, the fused step's
(launch_fwd_fused) the same template in kFusedProbe mode, or the probe / walk kernels whose
sums fm.hip states to be bit-identical to it; both walk a row's nnz in order into the same
accumulators, then reduce over the coordinates serially.  What they read is the same words: the
pull record [V | w | live] carries `live = vrow >= 0 && !(l1_shrk && w == 0)` (dist.hip
k_dist_pull*), which is the fused forward's own gate.  The number of shards does not enter: each
worker computes its own rows whole.

The split path at N > 1 adds the owners' per-row partials in rank order, another order of the
same sums: it keeps test_gpu_dist.py's `close` (relative 1e-5 plus the floor 1e-6 max(1,
max|b|)).  At N = 1 there is one owner and no exchange; it is held to the same tolerance.

Progress, as tests/test_gpu_dist.py:113-116: AUC * n equals metric_exact.auc_times_n on the
shard's own predictions exactly, the loss is within logloss_sum's bound."""
import os
import subprocess

import numpy as np
import pytest

from tests import metric_exact as M
from tests.test_gpu_dist import close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "shard_eval_tests")
DATA = os.path.join(ROOT, "tests", "golden", "rcv1_100.libsvm")


def _parse(out):
    cases, seqs = [], []
    for line in out.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "case":
            cases.append(dict(kv.split("=") for kv in w[2:]))
            cases[-1]["shards"] = {}
        elif w[0] == "shard":
            cases[-1]["shards"][int(w[1])] = dict(rows=int(w[3]), nrows=float(w[5]),
                                                  loss=float(w[7]), auc=float(w[9]))
        elif w[0] in ("label", "pred", "want"):
            cases[-1]["shards"][int(w[1])][w[0]] = np.array([float(x) for x in w[2:]],
                                                            np.float32)
        elif w[0] == "seq":
            seqs.append(line)
    return cases, seqs


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    assert os.path.exists(BIN), "build/shard_eval_tests missing: run make"
    r = subprocess.run([BIN, DATA, str(tmp_path_factory.mktemp("shard_eval"))],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    print(r.stderr[-4000:])
    return r, _parse(r.stdout)


def test_binary_passes_its_exact_checks(run):
    """validation changes no model word: train, train, validate, train leaves every shard's
    pull of every key bit-equal to the run without the validation step (flushed around it, and
    queued between the pipelined training steps), for both stores and both aggregations"""
    r, (cases, seqs) = run
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ALL PASSED" in r.stdout
    assert len(seqs) == 2 * 3 * 2 and all(" pulls equal " in s for s in seqs), seqs
    # 5 shapes x 2 schedules x (a2a sum, a2a ranks, split) + the after-flush cases
    assert len(cases) == 5 * 2 * 3 + 2 * 3


def test_predictions_match_single_context(run):
    _, (cases, _) = run
    assert cases
    seen_empty = 0
    for c in cases:
        N = int(c["N"])
        assert len(c["shards"]) == N, c
        for l, s in c["shards"].items():
            assert len(s["pred"]) == len(s["want"]) == len(s["label"]) == s["rows"], (c, l)
            seen_empty += s["rows"] == 0
            if c["store"] == "a2a":
                assert np.array_equal(s["pred"].view(np.uint32), s["want"].view(np.uint32)), (
                    c["store"], c["agg"], c["pipe"], N, c["shape"], l,
                    float(np.max(np.abs(s["pred"] - s["want"]), initial=0)))
            else:
                assert close(s["pred"], s["want"]), (
                    c["store"], c["pipe"], N, c["shape"], l,
                    float(np.max(np.abs(s["pred"] - s["want"]), initial=0)))
    assert seen_empty > 0


def test_progress_matches_own_predictions(run):
    _, (cases, _) = run
    assert cases
    for c in cases:
        for l, s in c["shards"].items():
            tag = (c["store"], c["agg"], c["pipe"], c["N"], c["shape"], l)
            assert s["nrows"] == s["rows"], tag
            if s["rows"] == 0:  # an idle shard adds nothing
                assert s["loss"] == 0 and s["auc"] == 0, (tag, s["loss"], s["auc"])
                continue
            assert s["auc"] == M.auc_times_n(s["label"], s["pred"]), tag
            S, tol = M.logloss_sum(s["label"], s["pred"])
            assert abs(s["loss"] - S) <= tol, (tag, s["loss"], S, tol)
