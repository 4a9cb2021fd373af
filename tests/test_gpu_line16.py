"""slot_layout=line vaux=f16 at V_dim 16: a key's entry, fp32 V and fp16 Vaux in one 128-byte line.

Every comparison is on bit patterns, against tests/line16_ref.Updater (pinned to the oracle with
the identity as rounding by tests/test_line16_ref.py) driven by backward_ref.fused_step.
"""
import copy

import numpy as np
import pytest
import torch

from difacto_amd import _lib
from difacto_amd import data as D
from oracle import oracle as O
from tests import backward_ref as R
from tests import line16_ref as L16
from tests.test_gpu_line_slots import (DFX_ERR_ARG, LAZY, H, _assert_store, _batch, _bits,  # noqa: F401
                                       _entry_eq, _record, _steps)

pytestmark = pytest.mark.gpu

CFG = dict(V_dim=16, V_threshold=0, l1=0, lr=.05, V_lr=.01)
LINE16 = dict(slot_layout="line", vaux="f16")


def _step(H, c, up, blk, push_cnt=False):
    want = R.fused_step(up, blk, push_cnt)
    pred = torch.zeros(blk.size, dtype=torch.float32, device=c.device)
    H.train_step(c, H.DeviceRowBlock(c, blk), H.kTraining, push_cnt=push_cnt, pred=pred)
    H.progress(c)
    assert np.array_equal(_bits(pred.cpu().numpy()), _bits(want))


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "valued"])
def test_fused_step_bit_equal(H, binary):
    """a count-push step and two training steps over one occurrence, the chunk gate and the hot-key
    pre-sums from both sides"""
    blk, _, uniq, _ = _batch(binary)
    c = H.Context(0, max_keys=1 << 12, **LINE16, **CFG)
    up, o = L16.Updater(**CFG), O.Updater(**CFG)
    _steps(H, c, up, binary, 3)
    c.close()
    assert up.rounded[0] > 0 and up.rounded[1] > 0, up.rounded      # rounded up, and down
    for step in range(3):       # the fp32 model after the same steps has another V
        R.fused_step(o, blk, step == 0)
    assert any(not np.array_equal(_bits(up.entry(k)[1][:16]), _bits(o.entry(k)[1][:16]))
               for k in uniq)


def test_range_edges(H):
    """row values scaled so that Vaux is stored as fp16 subnormals for some keys and saturates at
    65504 for others; V_lr_beta = 0 takes a tiny Vaux into eta"""
    cfg = dict(CFG, V_lr_beta=0, V_l2=0)
    b = R.planted_batch(1024, 8, (1, 128, 129), False, seed=12, zero_weights=False)
    scale = np.where(np.arange(b.size) % 8 == 0, 3e3, 1e-2).astype(np.float32)
    blk = D.RowBlock(b.offs, b.ids, b.vals * np.repeat(scale, 8), b.labels, b.weights)
    uniq = O.localize(blk.offs, blk.ids)[0]
    c = H.Context(0, max_keys=1 << 12, **LINE16, **cfg)
    up, st = L16.Updater(**cfg), H.Store(c)
    for step in range(3):
        _step(H, c, up, blk, step == 0)
        _assert_store(c, st, up, uniq, step)
    c.close()
    assert up.rounded[2] > 0 and up.rounded[3] > 0, up.rounded
    assert all(np.isfinite(up.entry(k)[1]).all() for k in uniq)


def test_lazy_v_bit_equal(H):
    cfg = dict(LAZY, V_dim=16)
    uniq = _batch(True)[2]
    c = H.Context(0, max_keys=1 << 12, **LINE16, **cfg)
    up = L16.Updater(**cfg)
    novee = hidden = 0
    for step in range(3):
        _steps(H, c, up, True, 1, flip=True, first=step)
        ent, (_, ol) = [up.entry(k) for k in uniq], up.get(uniq)
        novee += sum(e[1] is None for e in ent)
        hidden += sum(e[1] is not None and n == 1 for e, n in zip(ent, ol))
    assert novee > 0 and hidden > 0, (novee, hidden)
    c.close()


def test_rebuilds_and_store_push(H):
    """growth past load 0.5, then table_unclump on clustered keys (test_rebuilds_move_vaux's recipe),
    then one Update(kGradient) by dfx_store_push over keys with V and new keys"""
    c = H.Context(0, max_keys=64, **LINE16, **CFG)
    up, st = L16.Updater(**CFG), H.Store(c)
    cap0 = st.probe_stats()[2]
    rng = np.random.default_rng(5)
    seen = np.zeros(0, np.uint64)
    for step in range(4):
        B, k = 400, 8
        ids = rng.integers(0, 1500, B * k).astype(np.uint64)
        if step >= 2:
            ids = ids << np.uint64(40)      # keys that share their top bits: one home slot
        blk = D.RowBlock(np.arange(0, B * k + 1, k, dtype=np.uint64), ids, None,
                         np.where(rng.random(B) < .3, 1, -1).astype(np.float32))
        _step(H, c, up, blk, step == 0)     # (progress: the table grows / rehashes here)
        seen = np.union1d(seen, O.localize(blk.offs, blk.ids)[0])
        _assert_store(c, st, up, seen, step)
        _, mx, cap = st.probe_stats()
        assert step != 1 or (cap > cap0 and 2 * st.stats()["n_keys"] <= cap)    # it grew
        assert step < 2 or mx < 64 < len(seen)      # unclumped
    assert st.bytes()[1] == 0
    keys = np.union1d(seen[::3], np.arange(7, 60, 7, dtype=np.uint64))
    lens = up.get(keys)[1]
    assert (lens == 17).any() and (lens == 1).any()
    vals = (rng.standard_normal(int(lens.sum())) * .1).astype(np.float32)
    up.update(keys, up.kGradient, vals, lens)
    st.push(c.tensor(keys, torch.int64), up.kGradient, c.tensor(vals, torch.float32),
            c.tensor(lens, torch.int32))
    c.sync()
    _assert_store(c, st, up, keys, "push")
    c.close()


def test_model_files(H, tmp_path):
    blk, _, uniq, _ = _batch(False)
    c = H.Context(0, max_keys=1 << 12, **LINE16, **CFG)
    up = L16.Updater(**CFG)
    _steps(H, c, up, False, 3)
    files, dumps = set(), set()
    for dev in (False, True):       # the host and the device writers: one file and one text
        H.Store(c).save(str(tmp_path / ("m%d" % dev)), save_aux=True, device=dev)
        H.Store(c).dump(str(tmp_path / ("t%d" % dev)), dump_aux=True, need_reverse=True, device=dev)
        files.add((tmp_path / ("m%d" % dev)).read_bytes())
        dumps.add(tuple(sorted((tmp_path / ("t%d" % dev)).read_text().splitlines())))
    c.close()
    assert len(files) == 1 and len(dumps) == 1 and len(min(dumps)) > 1

    def same(st, ref):
        return [int(k) for k in uniq if not _entry_eq(_record(st.entry(k)), _record(ref.entry(k)))]
    for lay, dev in [(dict(slot_layout="split"), False), (dict(slot_layout="split"), True),
                     (LINE16, False), (LINE16, True)]:
        c = H.Context(0, max_keys=1 << 12, **lay, **CFG)
        st, ref = H.Store(c), copy.deepcopy(up)
        st.load(str(tmp_path / "m0"), device=dev)
        assert not same(st, ref), (lay, dev)        # fp32 in the file: exact in both layouts
        if lay is LINE16:       # one more step (Load sets new_w, leaves the seed: not compared)
            _step(H, c, ref, blk)
            assert not same(st, ref), (lay, dev)
        c.close()
    # a file of an fp32 run: Vaux narrows to the nearest fp16
    c, o = H.Context(0, max_keys=1 << 12, slot_layout="split", **CFG), O.Updater(**CFG)
    _steps(H, c, o, False, 3)
    H.Store(c).save(str(tmp_path / "s"), save_aux=True)
    c.close()
    exact = 0
    for dev in (False, True):
        c = H.Context(0, max_keys=1 << 12, **LINE16, **CFG)
        H.Store(c).load(str(tmp_path / "s"), device=dev)
        for k in uniq:
            (_, got), (_, want) = H.Store(c).entry(k), o.entry(k)
            exact += np.array_equal(want[16:], L16.nearest_f16(want[16:]))
            want[16:] = L16.nearest_f16(want[16:])
            assert np.array_equal(_bits(got), _bits(want)), (dev, int(k))
        c.close()
    assert exact < 2 * len(uniq)        # (some Vaux did narrow)


@pytest.mark.parametrize("kw", [dict(V_dim=16), dict(V_dim=16, slot_layout="fat"),
                                dict(V_dim=8, slot_layout="line"), dict(V_dim=32, slot_layout="line")],
                         ids=["auto", "fat", "line8", "line32"])
def test_vaux_f16_needs_line_at_16(H, kw):
    with pytest.raises(_lib.DfxError, match="slot_layout=line and V_dim=16"):
        H.Context(0, vaux="f16", **kw)


def test_single_context_one_line_per_slot(H):
    c = H.Context(0, max_keys=1 << 10, V_dim=16, **LINE16)
    lib = _lib.lib()
    assert lib.dfx_split_owner_forward(c.h, 0, None) == DFX_ERR_ARG
    assert lib.dfx_dist_owner_pull(c.h, 0, None) == DFX_ERR_ARG
    assert H.Store(c).bytes() == ((1 << 11) * 128, 0)
    c.close()
