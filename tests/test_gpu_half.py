"""vrows=f16 at V_dim 32 / 64: the split layout's pool rows as [V: d fp16 | Vaux: d fp16].

Every comparison is on bit patterns, against tests/half_ref.Updater (pinned to the oracle with the
identity as rounding and storage by tests/test_half_ref.py) driven by backward_ref.fused_step.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from difacto_amd import _lib
from difacto_amd import data as D
from oracle import oracle as O
from tests import backward_ref as R
from tests import half_ref as HR
from tests.test_gpu_line_slots import (DFX_ERR_ARG, H, _assert_store, _bits, _entry_eq,  # noqa: F401
                                       _record)

gpu = pytest.mark.gpu
HALF = dict(vrows="f16")
# chosen on half_ref alone (SEED too: test_reference_meets_the_conditions runs without a GPU):
# l1 keeps some w at 0, which l1_shrk hides; fea_cnt passes V_threshold for the ~16-occurrence keys
# in step 1's count push and for rarer ones later, so V comes by InitV inside steps 1 and 2 as well
SEED = 3
COUNTS = (130,) + (1,) * 60 + (2,) * 50 + (5,) * 20


def cfg(d):
    return dict(V_dim=d, V_threshold=20, l1=1.5, l1_shrk=1, lr=.05, V_lr=.05, V_init_scale=.5)


@functools.lru_cache(maxsize=None)
def batch(binary):
    """300 rows x 8 nnz over ~250 keys; key 0 has 130 occurrences (the chunk phase) -> the batch,
    the batch with its labels flipped (step 1 takes it: w goes back to 0 under V), the keys"""
    blk = R.planted_batch(300, 8, COUNTS, binary, seed=SEED)
    uniq, cnt, _ = O.localize(blk.offs, blk.ids)
    assert cnt.max() == 130 > 128
    return blk, D.RowBlock(blk.offs, blk.ids, blk.vals, -blk.labels, blk.weights), uniq


STEPS = (0, 1, 0)       # the batch of each step: as it is, flipped, as it is


@functools.lru_cache(maxsize=None)
def reference(d, binary):
    """three steps of half_ref, each with its count push -> per step (updater, predictions)"""
    up, out = HR.Updater(**cfg(d)), []
    for b in STEPS:
        pred = R.fused_step(up, batch(binary)[b], True)
        out.append((copy.deepcopy(up), pred))
    return out


CASES = [(32, True), (32, False), (64, True), (64, False)]
IDS = ["d32-binary", "d32-valued", "d64-binary", "d64-valued"]


@pytest.mark.parametrize("d,binary", CASES, ids=IDS)
def test_reference_meets_the_conditions(d, binary):
    """(CPU) the yardstick alone: both stores rounded both ways, V came by InitV inside a step, some
    w are hidden zeros — so that (a) cannot pass empty"""
    ref, uniq = reference(d, binary), batch(binary)[2]
    up = ref[-1][0]
    assert min(up.rounded_v) > 0 and min(up.rounded[:2]) > 0, (up.rounded_v, up.rounded)
    nv = [sum(u.entry(k)[1] is not None for k in uniq) for u, _ in ref]
    assert 0 < nv[0] < nv[1] < nv[2], nv
    assert up.initv_in_step > 0
    hidden = sum(e[1] is not None and e[0][0] == 0 for e in map(ref[1][0].entry, uniq))
    assert hidden > 0       # (what step 2 meets)


@gpu
@pytest.mark.parametrize("d,binary", CASES, ids=IDS)
def test_fused_steps_bit_equal(H, d, binary):
    """(a) three fused steps: predictions, every entry with its V and Vaux, counters and the seed
    bit for bit; the loss is the same rows' terms in double, summed by blocks: B 2^-52 relative"""
    (blk, neg, uniq), ref = batch(binary), reference(d, binary)
    c = H.Context(0, max_keys=1 << 10, **HALF, **cfg(d))
    assert H.localize_occ(c, blk.offs, blk.ids, blk.vals)["n_chunks"] == 2   # the hot key's
    st, dbs = H.Store(c), [H.DeviceRowBlock(c, blk), H.DeviceRowBlock(c, neg)]
    for step, (up, want) in enumerate(ref):
        pred = torch.zeros(blk.size, dtype=torch.float32, device=c.device)
        H.train_step(c, dbs[STEPS[step]], H.kTraining, push_cnt=True, pred=pred)
        loss = H.progress(c)["loss"]
        assert np.array_equal(_bits(pred.cpu().numpy()), _bits(want)), step
        y = np.where(blk.labels > 0, 1.0, -1.0) * (1 - 2 * STEPS[step])
        ref_loss = float(np.log(1.0 + np.exp(-y * want.astype(np.float64))).sum())
        assert abs(loss - ref_loss) <= blk.size * 2.0 ** -52 * ref_loss, (step, loss, ref_loss)
        _assert_store(c, st, up, uniq, step)
    assert st.bytes()[1] % (4 * d) == 0 and st.bytes()[1] // (4 * d) >= st.stats()["n_vrows"]
    c.close()


@gpu
def test_device_widen_is_f16_widen(H):
    """(b) the kernels' widening on all 65536 bit patterns, one launch"""
    c = H.Context(0, max_keys=64, **HALF, **cfg(32))
    got = H.Store(c).half_widen_table()
    c.close()
    h = np.arange(65536, dtype=np.uint32)
    e, m, s = (h >> 10) & 31, h & 1023, (h & 0x8000) << 16      # csrc/vaux16.h f16_widen
    sub = (m.astype(np.float32) * np.float32(2.0 ** -24)).view(np.uint32)
    want = np.where(e == 0, sub, (np.where(e == 31, 255, e + 112) << 23) | (m << 13)) | s
    assert np.array_equal(got, want.astype(np.uint32))
    fin = e < 31
    assert np.array_equal(got[fin], _bits(h[fin].astype(np.uint16).view(np.float16)))


def _load_both(H, d, path):
    ctxs = [H.Context(0, max_keys=1 << 10, **kw, **cfg(d)) for kw in (HALF, dict(vrows="f32"))]
    for c in ctxs:
        H.Store(c).load(path)
    return ctxs


@gpu
@pytest.mark.parametrize("d,binary", CASES, ids=IDS)
def test_same_values_same_forward(H, d, binary, tmp_path):
    """(c) a model whose values are all fp16 loaded into an f16 and an f32 context: one
    forward-only pass gives bit-equal predictions"""
    blk = batch(binary)[0]
    c = H.Context(0, max_keys=1 << 10, **HALF, **cfg(d))
    for b in STEPS:
        H.train_step(c, H.DeviceRowBlock(c, batch(binary)[b]), H.kTraining, push_cnt=True)
    H.Store(c).save(str(tmp_path / "m"), save_aux=True)
    c.close()
    preds = []
    for c in _load_both(H, d, str(tmp_path / "m")):
        pred = torch.zeros(blk.size, dtype=torch.float32, device=c.device)
        H.train_step(c, H.DeviceRowBlock(c, blk), H.kValidation, pred=pred)
        preds.append(_bits(pred.cpu().numpy()))
        c.close()
    assert np.array_equal(preds[0], preds[1]) and len(set(preds[0].tolist())) > 100


@gpu
@pytest.mark.parametrize("d", [32, 64])
def test_rebuild_grow_files_and_push(H, d, tmp_path):
    """(d) the table grows and the pool with it under the steps; a file such a table wrote
    reloads bit for bit, into an f32 context too; a file of fp32 rows loads narrowed to nearest;
    Store.push gives the fused step's model"""
    (blk, neg, uniq), ref = batch(False), reference(d, False)
    c = H.Context(0, max_keys=64, max_vrows=4, **HALF, **cfg(d))
    st, dbs = H.Store(c), [H.DeviceRowBlock(c, blk), H.DeviceRowBlock(c, neg)]
    cap0, pool0 = st.probe_stats()[2], st.bytes()[1]
    for step, (up, _) in enumerate(ref):
        H.train_step(c, dbs[STEPS[step]], H.kTraining, push_cnt=True)
        H.progress(c)
        _assert_store(c, st, up, uniq, step)
    assert st.probe_stats()[2] > cap0 and st.bytes()[1] > pool0    # rebuilt, and the pool moved
    up = ref[-1][0]
    st.save(str(tmp_path / "h"), save_aux=True)
    for cc in _load_both(H, d, str(tmp_path / "h")):
        for k in uniq:      # (SGDEntry::empty(): w == 0 without V is not in the file)
            got, want = H.Store(cc).entry(k), up.entry(k)
            if want[1] is None and want[0][0] == 0:
                assert got is None, int(k)
            else:
                assert _entry_eq(_record(got), _record(want)), int(k)
        cc.close()
    # Update(kGradient) by Store.push against the same update of the yardstick
    up = copy.deepcopy(up)
    lens = up.get(uniq)[1]
    vals = (np.random.default_rng(5).standard_normal(int(lens.sum())) * .1).astype(np.float32)
    up.update(uniq, up.kGradient, vals, lens)
    st.push(c.tensor(uniq, torch.int64), up.kGradient, c.tensor(vals, torch.float32),
            c.tensor(lens, torch.int32))
    c.sync()
    _assert_store(c, st, up, uniq, "push")
    c.close()
    # a file of an fp32 run narrows to the nearest fp16
    f = H.Context(0, max_keys=1 << 10, **cfg(d))
    for _ in range(2):
        H.train_step(f, H.DeviceRowBlock(f, blk), H.kTraining, push_cnt=True)
    H.Store(f).save(str(tmp_path / "s"), save_aux=True)
    c = H.Context(0, max_keys=1 << 10, **HALF, **cfg(d))
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
@pytest.mark.parametrize("kw", [dict(V_dim=16), dict(V_dim=128), dict(V_dim=8, slot_layout="fat"),
                                dict(V_dim=8, slot_layout="line"), dict(V_dim=32, loss="logit"),
                                dict(V_dim=16, slot_layout="line", vaux="f16")],
                         ids=["d16", "d128", "fat", "line", "logit", "vaux16"])
def test_vrows_f16_needs_32_or_64_split(H, kw):
    """(e) everything outside the allowed set"""
    with pytest.raises(_lib.DfxError, match="V_dim=32 or 64"):
        H.Context(0, vrows="f16", **kw)


@gpu
def test_single_context_only(H):
    """(e) the sharded stores refuse such a context; its pool rows are 4 d bytes"""
    c = H.Context(0, max_keys=1 << 10, max_vrows=100, V_dim=64, **HALF)
    lib = _lib.lib()
    assert lib.dfx_split_owner_forward(c.h, 0, None) == DFX_ERR_ARG
    assert lib.dfx_dist_owner_pull(c.h, 0, None) == DFX_ERR_ARG
    assert b"vrows=f16" in lib.dfx_last_error()
    assert H.Store(c).bytes() == ((1 << 11) * 32, 100 * 256)
    c.close()
