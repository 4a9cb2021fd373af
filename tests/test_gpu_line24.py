"""slot_layout=line vrows=f16 at V_dim 24: a key's entry, fp16 V and fp16 Vaux in one 128-byte line.

Every comparison is on bit patterns, against tests/half_ref.Updater (held to the oracle at this
V_dim by the CPU case at the end) driven by backward_ref.fused_step.
"""
import numpy as np
import pytest
import torch

from difacto_amd import _lib
from difacto_amd import data as D
from oracle import oracle as O
from tests import backward_ref as R
from tests import half_ref as HR
from tests import penalty_ref as PR
from tests.test_gpu_line_slots import (DFX_ERR_ARG, H, _assert_store, _batch, _bits,  # noqa: F401
                                       _entry_eq, _record, _steps)

gpu = pytest.mark.gpu
L24 = dict(slot_layout="line", vrows="f16")


def cfg(shrk=1, thr=0):
    return dict(V_dim=24, V_threshold=thr, l1=1.0, l2=.01, l1_shrk=shrk, lr=.05, V_lr=.05,
                V_init_scale=.5)


def _trained(H, binary, shrk):
    """case 1's three steps -> the context and the yardstick after them"""
    c = H.Context(0, max_keys=1 << 12, **L24, **cfg(shrk))
    up = HR.Updater(**cfg(shrk))
    _steps(H, c, up, binary, 3)
    return c, up


def _same(st, ref, uniq):
    """the keys whose stored record (as a model file holds it: no fea_cnt, and no entry at all for
    SGDEntry::empty(), w == 0 without V) differs from the yardstick's"""
    def rec(e, filed):
        return None if e is None or (filed and e[1] is None and e[0][0] == 0) else _record(e)
    return [int(k) for k in uniq if not _entry_eq(rec(st.entry(k), False), rec(ref.entry(k), True))]


@gpu
@pytest.mark.parametrize("shrk", [0, 1])
@pytest.mark.parametrize("binary", [True, False], ids=["binary", "valued"])
def test_fused_step_bit_equal(H, binary, shrk):
    """1. a count-push step and two training steps over one occurrence, the chunk gate and the
    hot-key pre-sums from both sides: pred, every entry with V and Vaux, seed, new_w, n_keys"""
    c, up = _trained(H, binary, shrk)
    c.close()
    assert up.initv_in_step > 0
    assert min(up.rounded_v) > 0 and min(up.rounded[:2]) > 0, (up.rounded_v, up.rounded)


ROWS = (0, 1, 7, 8, 9, 40, 41, 81)     # nnz per row: the 8-nnz trip and the 40-id stage, each side


@gpu
@pytest.mark.parametrize("binary", [True, False], ids=["binary", "valued"])
def test_kernel_edges(H, binary):
    """2. rows off the trip and the stage, ids that share a home slot (probe chains), keys absent
    at the forward (step 0 has no count push: the backward inserts them), keys that gain V in a
    later step and keys that never do (V_threshold 3), a table that grows from 128 slots"""
    rng = np.random.default_rng(24)
    lens = np.tile(ROWS, 9)             # 72 rows: more than one block of 64 quads
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ids = rng.integers(0, 150, int(lens.sum())).astype(np.uint64)
    ids[::3] <<= np.uint64(40)          # a third of them share their top bits: one home slot
    vals = None if binary else rng.uniform(.5, 1.5, len(ids)).astype(np.float32)
    blk = D.RowBlock(offs, ids, vals, np.where(rng.random(len(lens)) < .4, 1, -1).astype(np.float32))
    uniq = O.localize(blk.offs, blk.ids)[0]
    kw = cfg(1, thr=3)
    c = H.Context(0, max_keys=64, **L24, **kw)
    up, st = HR.Updater(**kw), H.Store(c)
    cap0, nv = st.probe_stats()[2], []
    for step, push in enumerate((False, True, False, True, False)):
        want = R.fused_step(up, blk, push)
        pred = torch.zeros(blk.size, dtype=torch.float32, device=c.device)
        H.train_step(c, H.DeviceRowBlock(c, blk), H.kTraining, push_cnt=push, pred=pred)
        H.progress(c)                   # a sync point: the table grows here
        assert np.array_equal(_bits(pred.cpu().numpy()), _bits(want)), step
        _assert_store(c, st, up, uniq, step)
        nv.append(sum(up.entry(k)[1] is not None for k in uniq))
    assert st.probe_stats()[2] > cap0 and st.bytes()[1] == 0
    assert nv[0] == 0 < nv[1] < nv[-1] < len(uniq), nv
    c.close()


@gpu
def test_same_values_same_forward_and_w(H, tmp_path):
    """3. case 1's model through the host writer into a slot_layout=auto vrows=f32 context: one
    forward gives equal pred bits; p and XV*p have no read-back hook, so one more training step
    holds them through every key's {w, sqrt_g, z} (g_w is the sum of p x)"""
    blk, _, uniq, _ = _batch(False)
    c, _ = _trained(H, False, 1)
    H.Store(c).save(str(tmp_path / "m"), save_aux=True)
    c.close()
    out = []
    for kw in (L24, {}):
        c = H.Context(0, max_keys=1 << 12, **kw, **cfg(1))
        H.Store(c).load(str(tmp_path / "m"))
        preds = []
        for job in (H.kValidation, H.kTraining):
            pred = torch.zeros(blk.size, dtype=torch.float32, device=c.device)
            H.train_step(c, H.DeviceRowBlock(c, blk), job, pred=pred)
            preds.append(_bits(pred.cpu().numpy()))
        c.sync()
        out.append((preds, [_bits(H.Store(c).entry(k)[0][:3]) for k in uniq]))
        c.close()
    (pa, ea), (pb, eb) = out
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    assert len(set(pa[0].tolist())) > 100
    assert all(np.array_equal(a, b) for a, b in zip(ea, eb))


@gpu
def test_model_files(H, tmp_path):
    """4. line24 -> file -> slot_layout=split -> file -> line24 is unchanged (the device writers
    refuse); a file of an fp32 run loads narrowed to the nearest fp16"""
    blk, _, uniq, _ = _batch(False)
    c, up = _trained(H, False, 1)
    H.Store(c).save(str(tmp_path / "a"), save_aux=True)
    with pytest.raises(_lib.DfxError):
        H.Store(c).save(str(tmp_path / "x"), save_aux=True, device=True)
    c.close()
    for src, dst, lay in (("a", "b", dict(slot_layout="split")), ("b", None, L24)):
        c = H.Context(0, max_keys=1 << 12, **lay, **cfg(1))
        H.Store(c).load(str(tmp_path / src))
        assert not _same(H.Store(c), up, uniq), lay
        if dst:
            H.Store(c).save(str(tmp_path / dst), save_aux=True)
        c.close()
    f = H.Context(0, max_keys=1 << 12, **cfg(1))
    for step in range(2):
        H.train_step(f, H.DeviceRowBlock(f, blk), H.kTraining, push_cnt=step == 0)
    H.Store(f).save(str(tmp_path / "s"), save_aux=True)
    c = H.Context(0, max_keys=1 << 12, **L24, **cfg(1))
    H.Store(c).load(str(tmp_path / "s"))
    narrowed = 0
    for k in uniq:
        want = H.Store(f).entry(k)[1]
        if want is not None:
            narrowed += not np.array_equal(want, HR.nearest_f16(want))
            assert np.array_equal(_bits(H.Store(c).entry(k)[1]), _bits(HR.nearest_f16(want))), int(k)
    assert narrowed > 0
    f.close()
    c.close()


@gpu
def test_evaluate(H):
    """5. Store.evaluate on case 1's table: nnz_w exactly, the penalty within penalty_ref's bound"""
    uniq = _batch(False)[2]
    c, up = _trained(H, False, 1)
    kw = cfg(1)
    S, nnz, bound, _ = PR.penalty(PR.entries_of(up, uniq), kw["l1"], kw["l2"], 24)
    pen, got = H.Store(c).evaluate()
    c.close()
    assert got == nnz and abs(pen - S) <= bound, (pen, S, bound, got, nnz)


@gpu
@pytest.mark.parametrize("kw,text", [
    (dict(V_dim=24, slot_layout="line"), "4, 8 or 12"),
    (dict(V_dim=24, vrows="f16"), "V_dim=32 or 64"),
    (dict(V_dim=8, slot_layout="line", vrows="f16"), "V_dim=32 or 64.*V_dim 24 with slot_layout=line"),
    (dict(V_dim=16, slot_layout="line", vaux="f16", vrows="f16"), "V_dim=32 or 64"),
    (dict(V_dim=24, slot_layout="line", vaux="f16"), "slot_layout=line and V_dim=16"),
    (dict(V_dim=24, slot_layout="line", vrows="f16wide"), "vrows=f16wide needs V_dim=128"),
    (dict(V_dim=24, **L24, vaux="f16"), None), (dict(V_dim=24, **L24, loss="logit"), None),
], ids=["no-vrows", "auto", "line8", "line16", "vaux", "wide", "both", "logit"])
def test_refusals(H, kw, text):
    """6. every refused combination keeps its pinned text"""
    with pytest.raises(_lib.DfxError, match=text):
        H.Context(0, **kw)


@gpu
def test_single_context_one_line_per_slot(H):
    c = H.Context(0, max_keys=1 << 10, V_dim=24, **L24)
    lib = _lib.lib()
    assert lib.dfx_split_owner_forward(c.h, 0, None) == DFX_ERR_ARG
    assert lib.dfx_dist_owner_pull(c.h, 0, None) == DFX_ERR_ARG
    assert H.Store(c).bytes() == ((1 << 11) * 128, 0)
    c.close()


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "valued"])
def test_identity_is_the_oracle_at_24(binary):
    """7. (CPU) the yardstick at this V_dim, where lane 3's masking has no counterpart"""
    blk, _, uniq, _ = _batch(binary)
    up, o = HR.Updater(rounding=HR.identity, storage=HR.keep, **cfg()), O.Updater(**cfg())
    for step in range(3):
        pu, po = R.fused_step(up, blk, step == 0), R.fused_step(o, blk, step == 0)
        assert np.array_equal(_bits(pu), _bits(po)), step
        assert all(_entry_eq(up.entry(k), o.entry(k)) for k in uniq), step
        assert (up.seed, up.new_w, up.size()) == (o.seed, int(o.new_w), o.size()), step
    assert up.initv_in_step > 0
