"""vrows=f16wide: V_dim 128 pool rows as [V: 128 fp16 | Vaux: 128 fp16], the spread forward
(k_fm_fwd_hw) and the two-pass backward's pass V (k_fm_bwd_hv) of csrc/fm_half.hip.

Every comparison is on bit patterns, against tests/half_ref.Updater (written over V_dim: nothing
in it fixes a width) driven by backward_ref.fused_step, as tests/test_gpu_half.py does at 32 / 64.
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
from tests.localizer_ref import reverse_bytes
from tests.test_gpu_line_slots import (DFX_ERR_ARG, H, _assert_store, _bits, _entry_eq,  # noqa: F401
                                       _record)

gpu = pytest.mark.gpu
WIDE = dict(vrows="f16wide", V_dim=128)
F, U64 = np.float32, np.uint64
LENS = [0, 17, 16, 1, 33, 48, 15]       # empty; on, one past and off the forward's 16-nnz trip


def cfg(shrk):
    """chosen on half_ref alone: step 1 leaves a dozen keys with V under w == 0, which l1_shrk hides
    from step 2 (the two runs then differ), and no prediction reaches the clip"""
    return dict(V_threshold=10, l1=1., l1_shrk=shrk, lr=.05, V_lr=.05, V_init_scale=.1)


@functools.lru_cache(maxsize=None)
def batches(binary):
    """48 ragged rows over ~300 keys: id 0 of the pool 140 times (two chunks: pass V reads
    partials), 40 ids ~9 times each (fea_cnt passes V_threshold in step 1's count push), the rest
    once or twice (never V: pass W's list is a strict subset); ids i << 40 share home slot 0.
    -> (the batch, it with flipped labels, it with every 9th id one never seen before)"""
    rng = np.random.default_rng(21)
    lens = np.array(LENS + rng.integers(5, 31, 41).tolist(), np.int64)
    nnz = int(lens.sum())
    pool = rng.integers(1, 1 << 55, 300).astype(U64)
    pool[1:9] = np.arange(1, 9, dtype=U64) << U64(40)
    pick = np.concatenate([np.zeros(140, np.int64), np.repeat(np.arange(1, 41), 9),
                           rng.integers(41, 300, nnz - 500)])
    ids = pool[pick[rng.permutation(nnz)]]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    vals = None if binary else (1.5 - rng.random(nnz, dtype=np.float32)).astype(F)
    w = (1.5 - rng.random(48)).astype(F)
    w[::7] = 0
    lab = np.where(rng.random(48) < .4, 1.0, -1.0).astype(F)
    new = ids.copy()
    new[::9] = rng.integers(1 << 55, 1 << 56, len(new[::9])).astype(U64)
    return tuple(D.RowBlock(offs, i, vals, y, w) for i, y in ((ids, lab), (ids, -lab), (new, lab)))


PUSH = (True, True, False)      # step 2 meets its new keys absent: the backward inserts them


@functools.lru_cache(maxsize=None)
def reference(binary, shrk):
    up, out = HR.Updater(V_dim=128, **cfg(shrk)), []
    for blk, push in zip(batches(binary), PUSH):
        pred = R.fused_step(up, blk, push)
        out.append((copy.deepcopy(up), pred, O.localize(blk.offs, blk.ids)[0]))
    return out


CASES = [(b, s) for b in (True, False) for s in (0, 1)]
IDS = ["%s-shrk%d" % ("binary" if b else "valued", s) for b, s in CASES]


@gpu
@pytest.mark.parametrize("binary,shrk", CASES, ids=IDS)
def test_fused_steps_bit_equal(H, binary, shrk):
    """(1) three fused steps in a table that grows from 64 slots and 4 pool rows: predictions,
    every entry with its V and Vaux halves, the counters and the seed, bit for bit"""
    ref, blks = reference(binary, shrk), batches(binary)
    nv = [sum(e[1] is not None for e in map(up.entry, uniq)) for up, _, uniq in ref]
    assert 0 < nv[0] < nv[1] < len(ref[1][2]) and ref[-1][0].initv_in_step > 0, nv
    assert min(ref[-1][0].rounded_v) > 0 and min(ref[-1][0].rounded[:2]) > 0
    c = H.Context(0, max_keys=64, max_vrows=4, **WIDE, **cfg(shrk))
    assert H.localize_occ(c, blks[0].offs, blks[0].ids, blks[0].vals)["n_chunks"] == 2
    st = H.Store(c)
    for step, (up, want, uniq) in enumerate(ref):
        pred = torch.zeros(48, dtype=torch.float32, device=c.device)
        H.train_step(c, H.DeviceRowBlock(c, blks[step]), H.kTraining, push_cnt=PUSH[step], pred=pred)
        H.progress(c)
        assert np.array_equal(_bits(pred.cpu().numpy()), _bits(want)), step
        _assert_store(c, st, up, uniq, step)
    assert st.probe_stats()[1] >= 7                 # the ids on one home slot: keys away from home
    assert st.bytes()[1] % 512 == 0 and st.bytes()[1] // 512 >= st.stats()["n_vrows"] == nv[2]
    c.close()


@gpu
@pytest.mark.parametrize("binary", [True, False], ids=["binary", "valued"])
def test_files_and_forward_against_f32(H, binary, tmp_path):
    """(2, 4) a file of a wide table holds the widened halves exactly and loads into an f32 and a
    wide context alike; over those values the two forwards give the same pred bit for bit, and a
    training step the same {w, sqrt_g, z} (functions of p alone).  The device writer and loader
    refuse the context"""
    ref, blks = reference(binary, 1), batches(binary)
    c = H.Context(0, max_keys=1 << 10, **WIDE, **cfg(1))
    for blk, push in zip(blks, PUSH):
        H.train_step(c, H.DeviceRowBlock(c, blk), H.kTraining, push_cnt=push)
    path = str(tmp_path / "m")
    H.Store(c).save(path, save_aux=True)
    for dev_io in (lambda: H.Store(c).save(path + "d", device=True),
                   lambda: H.Store(c).load(path, device=True)):
        with pytest.raises(_lib.DfxError, match="vrows=f16"):
            dev_io()
    c.close()
    up, _, uniq = ref[-1]
    out = []
    for kw in (WIDE, dict(V_dim=128, vrows="f32")):
        cc = H.Context(0, max_keys=1 << 10, **kw, **cfg(1))
        st = H.Store(cc)
        st.load(path)
        for k in uniq:      # (SGDEntry::empty(): w == 0 without V is not in the file)
            want = up.entry(k)
            if want[1] is not None or want[0][0] != 0:
                assert _entry_eq(_record(st.entry(k)), _record(want)), int(k)
        pred = torch.zeros(48, dtype=torch.float32, device=cc.device)
        H.train_step(cc, H.DeviceRowBlock(cc, blks[0]), H.kValidation, pred=pred)
        H.train_step(cc, H.DeviceRowBlock(cc, blks[1]), H.kTraining)
        out.append((_bits(pred.cpu().numpy()), [_bits(st.entry(k)[0][:3]) for k in ref[0][2]]))
        cc.close()
    assert np.array_equal(out[0][0], out[1][0]) and len(set(out[0][0].tolist())) > 40
    assert all(np.array_equal(a, b) for a, b in zip(out[0][1], out[1][1]))


@gpu
@pytest.mark.parametrize("kw", [dict(V_dim=32), dict(V_dim=64), dict(V_dim=16), dict(V_dim=256),
                                dict(V_dim=128, loss="logit"), dict(V_dim=8, slot_layout="fat"),
                                dict(V_dim=8, slot_layout="line"), dict(V_dim=128, bwd_two_pass=0),
                                dict(V_dim=16, slot_layout="line", vaux="f16")],
                         ids=["d32", "d64", "d16", "d256", "logit", "fat", "line", "onepass", "vaux16"])
def test_f16wide_needs_128_split(H, kw):
    """(3) everything outside the allowed set"""
    with pytest.raises(_lib.DfxError, match="vrows=f16wide needs V_dim=128"):
        H.Context(0, vrows="f16wide", **kw)


@gpu
def test_accepted_single_context_only(H):
    """(3) accepted at V_dim 128 with 512-byte pool rows; the sharded stores refuse it"""
    c = H.Context(0, max_keys=1 << 10, max_vrows=100, **WIDE)
    lib = _lib.lib()
    assert lib.dfx_split_owner_forward(c.h, 0, None) == DFX_ERR_ARG
    assert lib.dfx_dist_owner_pull(c.h, 0, None) == DFX_ERR_ARG
    assert H.Store(c).bytes() == ((1 << 11) * 32, 100 * 512)
    c.close()
