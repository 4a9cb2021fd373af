"""The two numbers every step reports, held to what the device's arithmetic allows
(tests/metric_exact.py): AUC * n exactly, the logloss within double rounding of the exact
sum — on every path that produces them.

* standalone dfx_auc / dfx_evaluate on two long-lived contexts (auc_sort = radix | merge) over
  the sizes at which metric.hip / sort.hip change path, visited large-small-large so workspaces
  and the last call's sortmeta are reused, with predictions that stress the key (signed zeros,
  subnormals, +-inf), the radix plan (one varying byte) and the ties (input order);
* the fused step: nrows, AUC and loss of dfx_progress against references computed from the
  device's OWN returned predictions (other tests pin those to the oracle), which isolates the
  forward's loss partials, the AUC snapshot, the lane and the finalizers;
* the owner-computes split and the sharded step through the loopback harness, per worker.

Every AUC comparison is `==`; every loss comparison uses the helper's tol."""
import math

import numpy as np
import pytest
import torch

from difacto_amd import data as D
from tests import metric_exact as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    from difacto_amd import hotpath
    return hotpath


@pytest.fixture(scope="module")
def ctxs(H):
    """radix and merge, alive over the whole module: every case runs on used workspaces"""
    cs = [H.Context(0, auc_sort=mode) for mode in ["radix", "merge"]]
    yield cs
    for c in cs:
        c.close()


def _check_loss(got, label, pred, what):
    S, tol = M.logloss_sum(label, pred)
    print(what, "loss", repr(got), "want", repr(S), "tol", tol)
    if math.isinf(S):  # exp overflows in double on both sides
        assert got == S, what
    else:
        assert abs(got - S) <= tol, (what, got, S, tol)


def _standalone(H, cs, label, pred, what):
    want = M.auc_times_n(label, pred)   # one reference for both modes
    for c, mode in zip(cs, ["radix", "merge"]):
        tl, tp = c.tensor(label, torch.float32), c.tensor(pred, torch.float32)
        got = H.auc(c, tl, tp)
        assert got == want, (what, mode, got, want)
        _check_loss(H.FMLoss(c, 0).evaluate(tl, tp), label, pred, (what, mode))


@pytest.mark.parametrize("name", M.PATTERNS)
def test_standalone_auc_exact_loss_to_rounding(H, ctxs, name):
    for n in M.SIZES:
        label, pred = M.standalone_case(name, n)
        _standalone(H, ctxs, label, pred, (name, n))


@pytest.mark.parametrize("name", ["correlated", "eighths"])
def test_standalone_labels_other_than_pm1(H, ctxs, name):
    """labels from {-1, -0.0, 0, 0.5, 2}: positive means label > 0 in the key's label, in the
    loss's y and in P"""
    for n in M.SIZES:
        label, pred = M.standalone_case(name, n, odd_labels=True)
        _standalone(H, ctxs, label, pred, (name, n, "odd labels"))


def test_standalone_degenerate(H, ctxs):
    """one class only: exactly 1.0 (not 1.0 * n); one positive ranked first, last and in the
    exact middle (P = 1, n = 3: a = 0.5 exactly, which is not flipped)"""
    rng = np.random.default_rng(3)
    for n in [100003, 1, 5, 12289, 12288]:
        pred = rng.standard_normal(n).astype(np.float32)
        for label in [np.ones(n, np.float32), -np.ones(n, np.float32), np.zeros(n, np.float32)]:
            assert M.auc_times_n(label, pred) == 1.0
            _standalone(H, ctxs, label, pred, ("one class", n, float(label[0])))
        if n >= 3:
            pred = np.arange(n, dtype=np.float32)
            for at in [0, n - 1, n // 2]:
                label = -np.ones(n, np.float32)
                label[at] = 1.0
                _standalone(H, ctxs, label, pred, ("one positive", n, at))
    three = np.array([0, 1, 2], np.float32)
    for label, want in [([1, -1, -1], 3.0), ([-1, -1, 1], 3.0), ([-1, 1, -1], 1.5)]:
        label = np.array(label, np.float32)
        assert M.auc_times_n(label, three) == want
        _standalone(H, ctxs, label, three, ("n = 3", want))


# ---------------------------------------------------------------- the fused step
def _long_rows(blk, lens, seed):
    """blk with rows of the given lengths appended (test_gpu_r5.py's idea: rows longer than a
    forward chunk — 32 nnz in the probe walk, 40 staged ids in the fat walk — and empty rows)"""
    rng = np.random.default_rng(seed)
    binary = blk.vals is None
    ids, offs, vals, labels = [blk.ids], [blk.offs], [blk.vals], [blk.labels]
    end = int(blk.offs[-1])
    for n in lens:
        ids.append(rng.integers(0, 1 << 40, n, dtype=np.uint64))
        end += n
        offs.append(np.array([end], np.uint64))
        if not binary:
            vals.append((1.0 - rng.random(n, dtype=np.float32)).astype(np.float32))
        labels.append(np.array([1.0 if n % 2 else -1.0], np.float32))
    return D.RowBlock(np.concatenate(offs).astype(np.uint64), np.concatenate(ids),
                      None if binary else np.concatenate(vals), np.concatenate(labels))


_FM = dict(V_threshold=0, l1=0, lr=.1, V_lr=.01)
FUSED = {  # name -> (updater kwargs, binary input, context kwargs)
    "lr_binary": (dict(V_dim=0, lr=.1, l1=.01), True, {}),            # the LR lanes
    "lr_valued": (dict(V_dim=0, lr=.1, l1=.01), False, {}),
    "v16_walk": (dict(V_dim=16, **_FM), True, {}),                    # k_fm_fwd_walk
    "v16_probe": (dict(V_dim=16, **_FM), True, dict(fat_fwd=0)),      # the probe walk
    "v5_odd": (dict(V_dim=5, **_FM), True, {}),
    "v128": (dict(V_dim=128, **_FM), True, {}),                       # 8 coordinates per lane
    "v200": (dict(V_dim=200, **_FM), True, {}),
}
KEY_SPACE = 1 << 14


def _fused_step(H, c, blk, job, push_cnt):
    """one step -> the device's own predictions"""
    pred = torch.zeros(blk.size, dtype=torch.float32, device=c.device)
    H.train_step(c, H.DeviceRowBlock(c, blk), job, push_cnt=push_cnt, pred=pred)
    return pred


def _check_progress(p, blocks, preds, what):
    """p: one read of dfx_progress over the steps (blocks, preds) since the last read"""
    assert p["nrows"] == sum(b.size for b in blocks), what
    want = 0.0
    for b, q in zip(blocks, preds):   # prog[2] += AUC * n, in step order
        want += M.auc_times_n(b.labels, q)
    print(what, "auc", repr(p["auc"]), "want", repr(want))
    assert p["auc"] == want, (what, p["auc"], want)
    # tol is linear in (S, n): the concatenated steps' tol is the sum of the steps'
    _check_loss(p["loss"], np.concatenate([b.labels for b in blocks]), np.concatenate(preds),
                what)


@pytest.mark.parametrize("name", list(FUSED))
def test_fused_step_metrics_from_device_predictions(H, name):
    kw, binary, ckw = FUSED[name]
    c = H.Context(0, max_keys=1 << 16, **kw, **ckw)
    sizes = [12289, 1, 30011, 255, 12288, 257]
    for step, B in enumerate(sizes + ["ragged"]):
        if B == "ragged":  # empty rows, rows past one and two forward chunks
            blk = _long_rows(D.synthetic(3001, 6, KEY_SPACE, binary=binary, ragged=True,
                                         seed=10 + step), [700, 0, 1300, 0, 3], seed=step)
        else:
            blk = D.synthetic(B, 12, KEY_SPACE, binary=binary, seed=10 + step)
        pred = _fused_step(H, c, blk, H.kTraining, step == 0)
        p = H.progress(c)
        q = pred.cpu().numpy()
        _check_progress(p, [blk], [q], (name, step, B))
        assert blk.size < 255 or step == 0 or len(np.unique(q)) > 1  # a trained model, not all 0
    c.close()


@pytest.mark.parametrize("mode", ["radix", "merge"])
@pytest.mark.parametrize("name", ["v16_walk", "lr_valued"])
def test_fused_accumulates_over_steps_without_a_read(H, name, mode):
    """block and tiled AUC paths alternating through both snapshot buffers and the accumulate
    branch of every finalizer, training and validation steps alternating; one read at the end"""
    kw, binary, ckw = FUSED[name]
    c = H.Context(0, max_keys=1 << 16, auc_sort=mode, **kw, **ckw)
    warm = D.synthetic(2000, 12, KEY_SPACE, binary=binary, seed=40)
    _fused_step(H, c, warm, H.kTraining, True)
    H.progress(c)  # (reset) so the steps below score a model that has been updated
    blocks, preds = [], []
    for step, B in enumerate([12289, 100, 12289, 1, 12289]):
        blk = D.synthetic(B, 12, KEY_SPACE, binary=binary, seed=50 + step)
        job = H.kTraining if step % 2 == 0 else H.kValidation
        preds.append(_fused_step(H, c, blk, job, False))
        blocks.append(blk)
    p = H.progress(c)
    _check_progress(p, blocks, [q.cpu().numpy() for q in preds], (name, mode))
    c.close()


# ---------------------------------------------------------------- the sharded paths
SHARDED = {
    "fm_v16": dict(V_dim=16, V_threshold=0, lr=0.1, V_lr=0.01, l1=0.0, seed=3),
    "fm_v5_odd": dict(V_dim=5, V_threshold=2, lr=0.05, l1=0.1, seed=11),
    "logit": dict(V_dim=0, lr=0.2, l1=0.05),
}


def _sharded(name, N, rows, split):
    """three steps of N loopback workers; each worker's progress against its own predictions"""
    from difacto_amd import dist as DI
    from difacto_amd import hotpath as H
    kw = SHARDED[name]
    ctxs = [H.Context(0, max_keys=1 << 16, push_agg="sum", **kw) for _ in range(N)]
    shards = [DI.Shard(c, N) for c in ctxs]
    comm = DI.LoopbackComm(N)
    for s in range(3):
        step = [D.synthetic(rows, 12, 6000, binary=(r % 2 == 0), seed=700 + 37 * s + r,
                            ragged=(s == 2)) for r in range(N)]
        dbs = [H.DeviceRowBlock(ctxs[r], step[r]) for r in range(N)]
        preds = [torch.zeros(rows, dtype=torch.float32, device=ctxs[r].device) for r in range(N)]
        if split:
            DI.split_step(shards, dbs, comm, H.kTraining, push_cnt=(s == 0), preds=preds)
        else:
            DI.sharded_step(shards, dbs, comm, H.kTraining, push_cnt=(s == 0), preds=preds)
        for r in range(N):
            _check_progress(H.progress(ctxs[r]), [step[r]], [preds[r].cpu().numpy()],
                            (name, N, rows, s, r))
    for c in ctxs:
        c.sync()
        c.close()


@pytest.mark.parametrize("rows", [400, 12289])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("name", list(SHARDED))
def test_split_step_worker_metrics(name, N, rows):
    """k_split_combine[_vec]'s partials over the `loss_part + lo / rpb` ranges,
    k_split_worker_finalize and the worker's AUC lane"""
    _sharded(name, N, rows, split=True)


@pytest.mark.parametrize("name", list(SHARDED))
def test_split_combine_in_row_slices_worker_metrics(name, monkeypatch):
    """dfx_split_combine_rows as the sliced host schedule calls it (split_host.cc): the batch
    combined in row ranges [0, 256), [256, 4352), [4352, B), each writing its blocks' partials
    at `loss_part + lo / rpb`; the last range runs the AUC and the worker's finalize"""
    import ctypes

    from difacto_amd import dist as DI

    def combine(self, dblk, parts, part_rows, slot=0, pred=None, pxv=None):
        lib = DI._lib.lib()
        PX = lib.dfx_split_pxv_floats(self.ctx.h)
        if pxv is None:
            pxv = torch.zeros(max(int(part_rows) * PX, 1), dtype=torch.float32,
                              device=self.ctx.device)
        b = dblk.as_batch()
        cuts = [0, 256, 4352, int(part_rows)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            DI.check(lib.dfx_split_combine_rows(self.ctx.h, slot, ctypes.byref(b), DI._p(parts),
                                                int(part_rows), self.nranks, DI._p(pxv),
                                                DI._p(pred), lo, hi - lo))
        return pxv

    monkeypatch.setattr(DI.Shard, "split_combine", combine)
    _sharded(name, 2, 12289, split=True)


@pytest.mark.parametrize("rows", [400, 12289])
@pytest.mark.parametrize("name", list(SHARDED))
def test_sharded_step_worker_metrics(name, rows):
    """the sharded step's forward over pulled records: its partials, sum_parts and the AUC lane
    (dist.hip dist_forward)"""
    _sharded(name, 2, rows, split=False)
