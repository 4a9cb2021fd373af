"""vrows=f16 off the 8-nnz grid and at fp16's edges: the paths of k_fm_fwd_h / k_fm_bwd_h
(csrc/fm_half.hip), vhalf_round (csrc/vhalf.h) and the half-row branches of the store that
tests/test_gpu_half.py's one batch shape (300 rows x 8 nnz, ordinary values) never runs.

Every comparison is on bit patterns against tests/half_ref.Updater driven by
backward_ref.fused_step, as in tests/test_gpu_half.py.  Every GPU case has a CPU twin (test_*_ref)
that asserts, on the yardstick alone, that the inputs reach the branch the case exists for.
"""
import copy
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from difacto_amd import data as D
from oracle import oracle as O
from tests import backward_ref as R
from tests import edge_ref as E
from tests import half_ref as HR
from tests import line16_ref as L16
from tests.localizer_ref import keys_of, reverse_bytes
from tests.test_gpu_half import CASES, HALF, IDS
from tests.test_gpu_line_slots import H, _assert_store, _bits, _entry_eq  # noqa: F401

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32, U64 = np.float32, np.uint32, np.uint64
ONES = (1 << 64) - 1
kHfNB, kHfIds = 8, 40       # csrc/fm_half.hip: nnz per trip, ids per staged chunk


def forward_ref(up, blk, max_index=ONES):
    """the yardstick's forward-only pass on a copy of `up` (Get default-constructs the keys it does
    not hold: w = 0, no V — they add nothing) -> the predictions"""
    up = copy.deepcopy(up)
    uniq, _, col = O.localize(blk.offs, blk.ids, max_index=max_index)
    vals, lens = up.get(uniq)
    wp, vp = O.get_pos(lens)
    return O.fm_predict(blk.offs, col, blk.vals, vals, wp, vp, up.V_dim)


def _pred(H, c, db, job, **kw):
    pred = torch.zeros(db.size, dtype=torch.float32, device=c.device)
    H.train_step(c, db, job, pred=pred, **kw)
    return pred.cpu().numpy()


def _flip(blk):
    return D.RowBlock(blk.offs, blk.ids, blk.vals, -blk.labels, blk.weights)


# ================================================================ 1, 2: ragged rows, folded ids
LONG = (80, 81, 88, 120)    # two and three staged chunks, ending on and off a trip boundary
RAGGED = ("plain", "fold251", "ones")
RAGGED_MAX_INDEX = dict(plain=ONES, fold251=251, ones=ONES)
STEPS = (0, 1, 0)           # the batch of each step: as it is, labels flipped, as it is


def ragged_cfg(d):
    return dict(V_dim=d, V_threshold=2, l1=.5, l1_shrk=1, lr=.05, V_lr=.05, V_init_scale=.5)


@functools.lru_cache(maxsize=None)
def ragged(binary, variant="plain"):
    """255 rows over 400 ids (id 0 among them): every length 0..49 twice, LONG, short rows of
    0..19, runs of empty rows at the head, inside and at the tail.  ones: some ids are 2^64 - 1
    (key 0, as id 0) -> (the batch, the batch with flipped labels, the keys, max_index)"""
    rng = np.random.default_rng(7)
    mid = 2 * list(range(50)) + list(LONG) + rng.integers(0, 20, 140).tolist()
    mid = [mid[i] for i in rng.permutation(len(mid))]
    lens = np.array([0, 0, 0] + mid[:100] + [0, 0, 0, 0] + mid[100:] + [0, 0, 0, 0], np.int64)
    # ids i and i + 251 fold onto one key at max_index = 251, and every residue occurs
    pool = (rng.integers(1, 1 << 55, 400) * 251 + np.arange(400) % 251).astype(U64)
    pool[0] = 0
    nnz = int(lens.sum())
    ids = pool[rng.integers(0, 400, nnz)]
    if variant == "ones":
        ids[rng.choice(nnz, 12, replace=False)] = U64(ONES)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    vals = None if binary else (1.5 - rng.random(nnz, dtype=np.float32)).astype(F)
    B = len(lens)
    w = (1.5 - rng.random(B)).astype(F)
    w[::7] = 0
    blk = D.RowBlock(offs, ids, vals, np.where(rng.random(B) < .4, 1.0, -1.0).astype(F), w)
    mi = RAGGED_MAX_INDEX[variant]
    return blk, _flip(blk), O.localize(blk.offs, blk.ids, max_index=mi)[0], mi


@functools.lru_cache(maxsize=None)
def ragged_reference(d, binary, variant):
    """three steps with the count push -> per step (updater, predictions), the final forward"""
    blk, neg, _, mi = ragged(binary, variant)
    up, out = HR.Updater(**ragged_cfg(d)), []
    for b in STEPS:
        pred = R.fused_step(up, (blk, neg)[b], True, max_index=mi)
        out.append((copy.deepcopy(up), pred))
    return out, forward_ref(up, blk, mi)


RAGGED_CASES = [(d, b, v) for v in RAGGED for d, b in CASES]
RAGGED_IDS = ["%s-%s" % (i, v) for v in RAGGED for i in IDS]


@pytest.mark.parametrize("d,binary,variant", RAGGED_CASES, ids=RAGGED_IDS)
def test_ragged_rows_ref(d, binary, variant):
    """(CPU) the batch reaches the forward's row-loop branches — empty rows (also first and last),
    nin < 8, a second trip, a restage on and off a trip boundary — and the yardstick's run has
    InitV inside a step, hidden zeros and both rounding directions.  fold251: every id folds and
    keys repeat inside rows.  ones: the all-ones id shares key 0 with id 0"""
    blk, _, uniq, mi = ragged(binary, variant)
    lens = np.diff(blk.offs.astype(np.int64))
    have = set(lens.tolist())
    assert set(range(50)) | set(LONG) <= have and 240 <= len(lens) <= 260
    assert all(n <= 19 or n in LONG or n < 50 for n in have)
    assert lens[:3].tolist() == [0, 0, 0] and lens[-4:].tolist() == [0] * 4        # o0 == o1
    assert any((lens[i:i + 4] == 0).all() for i in range(50, 200))
    assert {n % kHfNB for n in have} == set(range(kHfNB))                   # every nin < 8
    assert {80, 120} <= have and 80 % kHfIds == 0 and 120 % kHfIds == 0     # restage, chunk full
    assert {81, 88} <= have and {41, 47, 48, 49} <= have                    # ... and a partial one
    keys = keys_of(blk.ids, mi)
    assert np.array_equal(np.unique(keys), uniq)
    rep = sum(len(np.unique(keys[int(a):int(b)])) < int(b - a)
              for a, b in zip(blk.offs[:-1], blk.offs[1:]))
    assert rep > 10                                                         # keys repeat in rows
    if variant == "fold251":
        assert len(uniq) == 251 and (blk.ids >= 251).mean() > .99
    else:
        assert len(uniq) == 400
    if variant == "ones":
        n1, n0 = int((blk.ids == U64(ONES)).sum()), int((blk.ids == 0).sum())
        assert n1 == 12 and n0 > 0 and uniq[0] == 0
        assert O.localize(blk.offs, blk.ids)[1][0] == n0 + n1               # one slot for both
    ref, fwd = ragged_reference(d, binary, variant)
    up = ref[-1][0]
    assert up.initv_in_step > 0
    assert min(up.rounded_v) > 0 and min(up.rounded[:2]) > 0, (up.rounded_v, up.rounded)
    hidden = [sum(e[1] is not None and e[0][0] == 0 for e in map(u.entry, uniq)) for u, _ in ref]
    assert max(hidden[:2]) > 0, hidden          # (what a later step's Get hides)
    with_v = sum(up.entry(k)[1] is not None for k in uniq)
    print("nnz %d, keys with V %d of %d, hidden %s" % (blk.nnz, with_v, len(uniq), hidden))
    assert with_v > .85 * len(uniq)
    for _, pred in ref[1:]:
        assert len(set(_bits(pred).tolist())) > 200 and np.isfinite(pred).all()
        assert (pred[lens == 0] == 0).all()
    assert len(set(_bits(fwd).tolist())) > 200


@gpu
@pytest.mark.parametrize("d,binary,variant", RAGGED_CASES, ids=RAGGED_IDS)
def test_ragged_rows(H, d, binary, variant):
    """three fused steps over rows of 0..120 nnz, then one validation pass: predictions, every
    entry with V and Vaux, the counters and the seed bit for bit; the loss as
    test_fused_steps_bit_equal bounds it (an empty row's term is log 2)"""
    (blk, neg, uniq, mi), (ref, fwd) = ragged(binary, variant), ragged_reference(d, binary, variant)
    c = H.Context(0, max_keys=1 << 10, **HALF, **ragged_cfg(d))
    st, dbs = H.Store(c), [H.DeviceRowBlock(c, blk), H.DeviceRowBlock(c, neg)]
    for step, (up, want) in enumerate(ref):
        got = _pred(H, c, dbs[STEPS[step]], H.kTraining, push_cnt=True, max_index=mi)
        loss = H.progress(c)["loss"]
        assert np.array_equal(_bits(got), _bits(want)), step
        y = np.where(blk.labels > 0, 1.0, -1.0) * (1 - 2 * STEPS[step])
        ref_loss = float(np.log(1.0 + np.exp(-y * want.astype(np.float64))).sum())
        print("step %d loss %.17g yardstick %.17g" % (step, loss, ref_loss))
        assert abs(loss - ref_loss) <= blk.size * 2.0 ** -52 * ref_loss, (step, loss, ref_loss)
        _assert_store(c, st, up, uniq, step)
    n_keys = st.stats()["n_keys"]
    got = _pred(H, c, dbs[0], H.kValidation, max_index=mi)
    assert np.array_equal(_bits(got), _bits(fwd))
    H.progress(c)
    assert st.stats()["n_keys"] == n_keys
    c.close()


# ================================================================ 3: probe chains, absent keys
# Get find-or-inserts in every job type, as SGDUpdater::Get's model_[key] does (step.hip
# k_probe_keys, in count-push and non-training steps, before the forward).  So the forward meets a
# key the table does not hold only in a training step without the count push, where the backward
# inserts it afterwards; a validation pass over such keys finds them inserted, as empty entries.
N_CHAIN = 40        # trained keys on one home slot: distances 0..39, under kClusterProbe = 64
N_NEW = 10          # per batch: absent keys on that home slot, and as many with empty home slots


def chain_cfg(d):
    return dict(V_dim=d, V_threshold=0, l1=0, lr=.05, V_lr=.05, V_init_scale=.5)


@functools.lru_cache(maxsize=None)
def chain(binary):
    """ids i << 40: their keys are below 2^24, so they share home slot 0 of the ordered table at
    every capacity.  -> (the training batch over i < N_CHAIN, two batches that mix them with ids
    never seen before, the trained keys, per mixed batch (its new keys on that home slot, its new
    keys whose home slots are empty))"""
    rng = np.random.default_rng(13)
    tr_ids = np.arange(N_CHAIN, dtype=U64) << U64(40)

    def block(ids, B, k):
        vals = None if binary else (1.0 - rng.random(B * k, dtype=np.float32)).astype(F)
        return D.RowBlock(np.arange(0, B * k + 1, k, dtype=U64), ids, vals,
                          np.where(rng.random(B) < .4, 1.0, -1.0).astype(F),
                          (1.5 - rng.random(B)).astype(F))
    B, k = 60, 10
    out, new = [block(tr_ids[rng.integers(0, N_CHAIN, B * k)], B, k)], []
    kind = np.tile(np.array([0, 1, 0, 2, 0, 0, 1, 2, 0, 2]), B)     # per row: 5 trained, 2 + 3 new
    for n in range(2):
        near = np.arange(N_CHAIN + n * N_NEW, N_CHAIN + (n + 1) * N_NEW, dtype=U64) << U64(40)
        far = (np.arange(n * N_NEW, (n + 1) * N_NEW, dtype=U64) << U64(4)) | U64(0xF)
        pick = rng.integers(0, N_NEW, B * k)        # (the key's top hex digit is F)
        ids = np.where(kind == 0, tr_ids[rng.integers(0, N_CHAIN, B * k)],
                       np.where(kind == 1, near[pick], far[pick]))
        out.append(block(ids, B, k))
        new.append((reverse_bytes(near), reverse_bytes(far)))
    return out[0], out[1], out[2], reverse_bytes(tr_ids), new


@functools.lru_cache(maxsize=None)
def chain_reference(d, binary):
    """three steps with the count push on the trained keys, one step without it over the first
    mixed batch -> per step (updater, predictions); the forward over the second mixed batch"""
    train, mix1, mix2 = chain(binary)[:3]
    up, out = HR.Updater(**chain_cfg(d)), []
    for step in range(3):
        pred = R.fused_step(up, (train, _flip(train))[step % 2], True)
        out.append((copy.deepcopy(up), pred))
    pred = R.fused_step(up, mix1, False)
    out.append((copy.deepcopy(up), pred))
    return out, forward_ref(up, mix2)


def _homes(keys, logcap):
    return np.asarray(keys, U64) >> U64(64 - logcap)     # tbl_hash, ordered, range_mul = 1


@pytest.mark.parametrize("d,binary", CASES, ids=IDS)
def test_probe_chains_ref(d, binary):
    """(CPU) the trained keys share one home slot at every capacity from 128 slots up, so their
    probe distances are 0..N_CHAIN-1 (the forward's chain walk, for whole trips), and the chain
    stays under kClusterProbe with both batches' new keys on it; of each mixed batch's ids a third
    and more were never seen, inside rows with trained ones: some on the trained keys' home slot
    (the walk ends at an empty slot), the rest with home slots the chain does not reach (empty at
    once); keys the model does not hold add nothing to the yardstick's forward"""
    train, mix1, mix2, tr, new = chain(binary)
    every = np.concatenate([tr] + [k for pair in new for k in pair])
    assert len(np.unique(every)) == len(every) == N_CHAIN + 4 * N_NEW
    assert N_CHAIN - 1 >= kHfNB and N_CHAIN + 2 * N_NEW < 64 < (1 << 7) - 8
    for logcap in range(7, 25):
        assert not _homes(tr, logcap).any()
        for near, far in new:
            assert not _homes(near, logcap).any()
            assert (_homes(far, logcap) >= (1 << logcap) - (1 << logcap) // 16).all()
    assert np.array_equal(O.localize(train.offs, train.ids)[0], np.sort(tr))
    ref, fwd = chain_reference(d, binary)
    for blk, (near, far), up in zip((mix1, mix2), new, (ref[2][0], ref[3][0])):
        vk = keys_of(blk.ids).reshape(blk.size, -1)
        is_tr, is_near, is_far = (np.isin(vk, s) for s in (tr, near, far))
        assert (is_tr | is_near | is_far).all() and (~is_tr).mean() >= 1 / 3
        assert (is_tr.any(1) & is_near.any(1) & is_far.any(1)).all()        # mixed inside rows
        assert all(up.entry(k) is None for k in np.concatenate([near, far]))    # before the pass
        # the forward over the known nnz alone is the forward
        keep = is_tr.reshape(-1)
        offs = np.concatenate([[0], np.cumsum(is_tr.sum(1))]).astype(U64)
        only = D.RowBlock(offs, blk.ids[keep], None if binary else blk.vals[keep], blk.labels,
                          blk.weights)
        want = ref[3][1] if blk is mix1 else fwd
        assert np.array_equal(_bits(forward_ref(up, only)), _bits(want))
        assert len(set(_bits(want).tolist())) > 50
    assert ref[2][0].size() == N_CHAIN and ref[3][0].size() == N_CHAIN + 2 * N_NEW
    assert all(ref[2][0].entry(k)[1] is not None for k in tr)


@gpu
@pytest.mark.parametrize("d,binary", CASES, ids=IDS)
def test_probe_chains_and_absent_keys(H, d, binary):
    """three fused steps over keys that share a home slot, in a context that grows (max_keys=64,
    max_vrows=4): predictions and store bit for bit, the chains intact (no unclump ran).  Then a
    training step without the count push over trained and absent keys — the forward's key check
    leaves by both exits, the backward inserts — and a validation pass over trained and further
    absent keys: the yardstick's predictions, and Get's empty entries for the new keys"""
    (train, mix1, mix2, tr, new), (ref, fwd) = chain(binary), chain_reference(d, binary)
    c = H.Context(0, max_keys=64, max_vrows=4, **HALF, **chain_cfg(d))
    st, dbs = H.Store(c), [H.DeviceRowBlock(c, train), H.DeviceRowBlock(c, _flip(train))]
    pool0 = st.bytes()[1]
    uniq = np.sort(tr)
    for step, (up, want) in enumerate(ref[:3]):
        got = _pred(H, c, dbs[step % 2], H.kTraining, push_cnt=True)
        H.progress(c)
        assert np.array_equal(_bits(got), _bits(want)), step
        _assert_store(c, st, up, uniq, step)
        _, mx, cap = st.probe_stats()
        assert mx == N_CHAIN - 1 >= kHfNB, (step, mx, cap)      # one chain, never unclumped
    assert st.bytes()[1] > pool0 and st.stats()["n_vrows"] == N_CHAIN      # the pool grew
    up, want = ref[3]
    got = _pred(H, c, H.DeviceRowBlock(c, mix1), H.kTraining, push_cnt=False)
    H.progress(c)
    assert np.array_equal(_bits(got), _bits(want))
    uniq = np.sort(np.concatenate([tr, new[0][0], new[0][1]]))
    _assert_store(c, st, up, uniq, "absent")
    assert st.probe_stats()[1] == N_CHAIN + N_NEW - 1
    got = _pred(H, c, H.DeviceRowBlock(c, mix2), H.kValidation)
    H.progress(c)
    assert np.array_equal(_bits(got), _bits(fwd))
    up = copy.deepcopy(up)
    up.get(np.sort(np.concatenate(new[1])))            # Get's model_[key]: zero state, no V
    uniq = np.sort(np.concatenate([uniq, new[1][0], new[1][1]]))
    assert all(not up.entry(k)[0].any() and up.entry(k)[1] is None for k in np.concatenate(new[1]))
    _assert_store(c, st, up, uniq, "validation")        # nothing the model held has moved
    assert st.stats()["n_keys"] == N_CHAIN + 4 * N_NEW and st.stats()["n_vrows"] == N_CHAIN
    c.close()


# ================================================================ 4: range edges
EDGE = dict(V_threshold=0, l1=0, lr=.05, V_lr_beta=0, V_l2=0)
SMALL = dict(EDGE, V_lr=1e-5, V_init_scale=1e-5)
LARGE = dict(EDGE, V_lr=3e4, V_init_scale=.5)
TINY = F(2.0 ** -14)


@functools.lru_cache(maxsize=None)
def edge_batch():
    """test_gpu_line16.test_range_edges's scaled batch at 512 rows"""
    b = R.planted_batch(512, 8, (1, 128, 129), False, seed=12, zero_weights=False)
    scale = np.where(np.arange(b.size) % 8 == 0, 3e3, 1e-2).astype(F)
    blk = D.RowBlock(b.offs, b.ids, b.vals * np.repeat(scale, 8), b.labels, b.weights)
    return blk, O.localize(blk.offs, blk.ids)[0]


@functools.lru_cache(maxsize=None)
def edge_reference(d, large):
    blk, _ = edge_batch()
    up, out = HR.Updater(V_dim=d, **(LARGE if large else SMALL)), []
    for step in range(3):
        pred = R.fused_step(up, blk, step == 0)
        out.append((copy.deepcopy(up), pred))
    return out


def _rows(up, uniq):
    d = up.V_dim
    VV = np.stack([up.entry(k)[1] for k in uniq if up.entry(k)[1] is not None])
    return VV[:, :d], VV[:, d:]


@pytest.mark.parametrize("d", [32, 64])
def test_small_end_ref(d):
    """(CPU) the yardstick's stores hold V as fp16 subnormals of both signs and as -0, and Vaux as
    subnormals: the step kernels widen them (f16_widen, e == 0), vhalf_round floors magnitudes
    below 2^-14 (f16_floor, e < 113) and puts the sign back on them; the predictions stay finite
    and distinct"""
    uniq = edge_batch()[1]
    seen = np.zeros(4, np.int64)
    for up, pred in edge_reference(d, False):
        V, C = _rows(up, uniq)
        sub = (V != 0) & (np.abs(V) < TINY)
        seen += [sub.sum(), (sub & (V < 0)).sum(), (_bits(V) == 0x80000000).sum(),
                 ((C > 0) & (C < TINY)).sum()]
        assert np.isfinite(pred).all()
    print("subnormal V %d, negative %d, -0 %d, subnormal Vaux %d" % tuple(seen))
    assert (seen > 0).all(), seen
    assert up.rounded[2] > 0 and min(up.rounded_v) > 0 and min(up.rounded[:2]) > 0
    assert len(set(_bits(pred).tolist())) > 300


@pytest.mark.parametrize("d", [32, 64])
def test_large_end_ref(d):
    """(CPU) Vaux saturates at 65504 in the yardstick (vaux16_round's !(nc < 65504)), nothing
    stored is infinite"""
    uniq = edge_batch()[1]
    up = edge_reference(d, True)[-1][0]
    V, C = _rows(up, uniq)
    print("rounded", up.rounded, "Vaux at 65504:", int((C == 65504).sum()))
    assert up.rounded[2] > 0 and up.rounded[3] > 0 and (C == 65504).sum() > 100
    assert np.isfinite(V).all() and np.isfinite(C).all()


@gpu
@pytest.mark.parametrize("large", [False, True], ids=["small", "large"])
@pytest.mark.parametrize("d", [32, 64])
def test_range_edges(H, d, large):
    """three fused steps at either end of fp16's range (V_lr_beta = 0 takes a tiny Vaux into eta):
    predictions and store bit for bit, every stored value finite"""
    (blk, uniq), ref = edge_batch(), edge_reference(d, large)
    c = H.Context(0, max_keys=1 << 12, V_dim=d, **HALF, **(LARGE if large else SMALL))
    st, db = H.Store(c), H.DeviceRowBlock(c, blk)
    for step, (up, want) in enumerate(ref):
        got = _pred(H, c, db, H.kTraining, push_cnt=(step == 0))
        H.progress(c)
        assert np.array_equal(_bits(got), _bits(want)), step
        _assert_store(c, st, up, uniq, step)
    assert all(np.isfinite(st.entry(k)[1]).all() for k in uniq[::7])
    c.close()


# ---- V itself at +-65504 and in the subnormals: a model file, then Store.push(kGradient)
FILE_V = [65504, -65504, 7e4, -7e4, np.inf, -np.inf, 65503.9, -65503.9, 2.0 ** -14, -2.0 ** -14,
          2.0 ** -24, -2.0 ** -24, 2.0 ** -25, -2.0 ** -25, 0.0, -0.0]
PUSH = dict(V_threshold=0, l1=0, lr=.05, V_lr=64, V_lr_beta=1, V_l2=0, l1_shrk=0)
# (old V, gradient): nv = v - 64 g / (|g| + 1) with Vaux 0 before
PUSH_VG = [(65472, -3), (-65472, 3),                # across +-65504: 65472 +- 48
           (1024, 1), (-1024, -1),                  # 1024 - 32 = 992: an fp16, g != 0
           (2.0 ** -15, 1e-7), (-2.0 ** -15, -1e-7),    # inside the subnormals, between two fp16
           (2.0 ** -24, 3e-7), (-2.0 ** -24, -3e-7),    # through zero into them
           (2.0 ** -14, 2e-8), (-2.0 ** -14, -2e-8),    # from the smallest normal down
           (65504, -1e-3), (-65504, 1e-3),          # from the largest fp16 outwards
           (.5, .25), (-3, -7), (100, 0), (0, 1e-8)]


def _file_model(d):
    """eight keys whose V rows are FILE_V rotated (every value meets every lane and word half),
    Vaux the non-negative ones"""
    keys, _ = E._private_keys(8)
    vv = np.array(FILE_V, F)
    cc = vv[~np.signbit(vv)]
    return [(int(k), F(.5 + i), F(1 + i), F(-i), np.roll(np.resize(vv, d), i),
             np.roll(np.resize(cc, d), i)) for i, k in enumerate(keys)]


def _push_model(d):
    keys, _ = E._private_keys(8)
    v, g = np.array(PUSH_VG, np.float64).T
    out, grads = [], []
    for i, k in enumerate(keys):
        out.append((int(k), F(.5 + i), F(1 + i), F(-i), np.roll(np.resize(v.astype(F), d), i),
                    np.zeros(d, F)))
        grads.append(np.concatenate([[F(.01 * (i - 3))], np.roll(np.resize(g.astype(F), d), i)]))
    return out, np.concatenate(grads).astype(F)


def _loaded(model, cfg):
    """the yardstick after Load of a model file: the file's state, V and Vaux to the nearest fp16"""
    up = HR.Updater(**cfg)
    for k, w, sg, z, V, C in model:
        up.model[k] = [np.array([w, sg, z, 0], F), np.concatenate([HR.nearest_f16(V),
                                                                   HR.nearest_f16(C)])]
    return up


class _Recorded:
    """half_ref.round_half, keeping (nv, stored V) of every coordinate"""

    def __init__(self):
        self.nv, self.v = [], []

    def __call__(self, nv, nc, g, sg, j):
        v, c = HR.round_half(nv, nc, g, sg, j)
        self.nv.append(np.array(nv, F))
        self.v.append(v)
        return v, c


@functools.lru_cache(maxsize=None)
def push_reference(d):
    model, grads = _push_model(d)
    cfg, rec = dict(PUSH, V_dim=d), _Recorded()
    up = _loaded(model, cfg)
    up.rounding = rec
    keys = np.array([m[0] for m in model], U64)
    lens = up.get(keys)[1]
    up.update(keys, up.kGradient, grads, lens)
    up.rounding = HR.round_half
    return model, keys, grads, lens, up, np.concatenate(rec.nv), np.concatenate(rec.v)


@pytest.mark.parametrize("d", [32, 64])
def test_store_edges_ref(d):
    """(CPU) the file's V narrows to +-65504 from above, from inf and from 65503.9, keeps +-2^-14
    and +-2^-24, and takes +-2^-25 to +-0 (f16_nearest's saturation, floor and tie); the pushed
    gradients take nv across 65504 in both signs, exactly onto an fp16, and between two subnormal
    fp16 of both signs, where the stochastic round goes both ways"""
    near = _bits(HR.nearest_f16(np.array(FILE_V, F))).tolist()
    b = lambda x: int(_bits(F(x))[0])      # noqa: E731
    assert near == [b(65504), b(-65504)] * 4 + [b(2.0 ** -14), b(-2.0 ** -14), b(2.0 ** -24),
                                                 b(-2.0 ** -24), 0, 0x80000000, 0, 0x80000000]
    assert all(len(m[4]) == d and len(m[5]) == d for m in _file_model(d))
    model, keys, grads, lens, up, nv, v = push_reference(d)
    assert (lens == d + 1).all() and len(nv) == 8 * d
    old = np.concatenate([m[4] for m in model])
    assert ((nv > 65504) & (old < 65504) & (v == 65504)).any()
    assert ((nv < -65504) & (old > -65504) & (v == -65504)).any()
    assert ((nv == v) & (nv != old) & (np.abs(nv) > 1)).any()               # exactly an fp16
    for sign in (1, -1):
        sub = (sign * nv > 0) & (np.abs(nv) < TINY) & (np.abs(v) < TINY)
        assert (sub & (np.abs(v) > np.abs(nv))).any() and (sub & (np.abs(v) < np.abs(nv))).any()
        assert (sub & (np.signbit(v) == (sign < 0))).sum() == sub.sum()     # the sign goes back on
    assert ((np.sign(old) == -np.sign(nv)) & (old != 0) & (np.abs(nv) < TINY)).any()  # through zero
    assert np.isfinite(v).all()


@gpu
@pytest.mark.parametrize("d", [32, 64])
def test_store_edges(H, d, tmp_path):
    """a file of fp32 rows at fp16's edges loads narrowed to the nearest (the host loader: the
    device loader refuses a half table); then
    Store.push(kGradient) with planted gradients equals half_ref.Updater.update bit for bit"""
    model = _file_model(d)
    E.write_model(str(tmp_path / "edges"), d, model)
    c = H.Context(0, max_keys=64, **HALF, **dict(PUSH, V_dim=d))
    st = H.Store(c)
    st.load(str(tmp_path / "edges"))
    for k, w, sg, z, V, C in model:
        got = st.entry(k)
        assert np.array_equal(_bits(got[0][:3]), _bits([w, sg, z])), k
        want = np.concatenate([HR.nearest_f16(V), HR.nearest_f16(C)])
        assert np.array_equal(_bits(got[1]), _bits(want)), (k, got[1], want)
    c.close()
    model, keys, grads, lens, up, _, _ = push_reference(d)
    E.write_model(str(tmp_path / "push"), d, model)
    c = H.Context(0, max_keys=64, **HALF, **dict(PUSH, V_dim=d))
    st = H.Store(c)
    st.load(str(tmp_path / "push"))
    v, l = st.pull(c.tensor(keys, torch.int64))
    assert np.array_equal(l.cpu().numpy(), lens)
    st.push(c.tensor(keys, torch.int64), up.kGradient, c.tensor(grads, torch.float32),
            c.tensor(lens, torch.int32))
    c.sync()
    bad = [int(k) for k in keys if not _entry_eq(st.entry(k), up.entry(k))]
    assert not bad, bad
    v, _ = st.pull(c.tensor(keys, torch.int64))
    assert np.array_equal(_bits(v.cpu().numpy()), _bits(up.get(keys)[0]))
    c.close()


# ================================================================ 5: the narrowing functions
def _around(x, n=64):
    b = int(_bits(F(x))[0])
    a = np.arange(b - n, b + n + 1, dtype=np.int64).astype(U32)
    return np.concatenate([a, a | U32(0x80000000)])


@functools.lru_cache(maxsize=None)
def round_tuples():
    """-> (uint32[n, 4] tuples (bits of nv, of g, of sg, j), {class: slice})"""
    rng = np.random.default_rng(23)
    h = np.arange(0x7C00, dtype=U32)
    h = np.concatenate([h, h | U32(0x8000)])
    x = _bits(HR.widen(h))
    lo = np.arange(0x7BFF, dtype=U32)
    mid = _bits((HR.widen(lo).astype(np.float64) + HR.widen(lo + U32(1)).astype(np.float64)) / 2)
    nan = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001,
                    0x7FA00000, 0xFFBFFFFF, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC00001, 0xFFE00000], U32)
    sub = np.concatenate([np.arange(0, 4097), np.arange(0x7FF000, 0x801000),
                          1 << np.arange(23), (1 << np.arange(23)) * 3 // 2]).astype(U32)
    parts = dict(fp16=x, succ=x + U32(1), pred=np.where((x & U32(0x7FFFFFFF)) == 0, x, x - U32(1)),
                 mid=np.concatenate([mid, mid | U32(0x80000000)]),
                 edges=np.concatenate([_around(65504), _around(2.0 ** -14), _around(2.0 ** -24),
                                       _around(2.0 ** -25), _around(65520), sub,
                                       sub | U32(0x80000000)]),
                 nonfinite=nan, random=rng.integers(0, 1 << 32, 100000).astype(U32))
    nv = np.concatenate(list(parts.values()))
    n = len(nv)
    g = rng.integers(0, 1 << 32, n).astype(U32)
    sg = _bits(np.abs(rng.standard_normal(n)).astype(F) * F(3))
    j = rng.integers(0, 64, n).astype(U32)
    ends = np.cumsum([len(p) for p in parts.values()])
    cls = {k: slice(int(e - len(p)), int(e)) for (k, p), e in zip(parts.items(), ends)}
    return np.stack([nv, g, sg, j], 1).astype(U32), cls


@functools.lru_cache(maxsize=None)
def round_expected():
    """the numpy yardstick of the three functions -> uint32[n, 3] fp16 bit patterns:
    half_ref.round_v_bits, line16_ref.round_f16 (as the fp16 it widens from) and
    half_ref.nearest_f16 (a NaN reads as too large: +-65504, csrc/vaux16.h)"""
    t, _ = round_tuples()
    nv, g, sg = (t[:, i].copy().view(F) for i in range(3))
    j = t[:, 3].astype(np.int64)
    ax = np.abs(nv)
    with np.errstate(invalid="ignore", over="ignore"):
        a = HR.round_v_bits(nv, g, sg, j)
        b = L16.round_bits(ax, g, sg, j)
        assert np.array_equal(_bits(L16.f16_widen(b)), _bits(L16.round_f16(ax, g, sg, j)))
        near = HR.nearest_f16(np.where(np.isnan(nv), F(0), nv)).astype(np.float16).view(np.uint16)
    s = (t[:, 0] >> U32(16)) & U32(0x8000)
    c = np.where(np.isnan(nv), s | U32(0x7BFF), near.astype(U32))
    return np.stack([a, b, c], 1).astype(U32)


def test_round_tuples_ref():
    """(CPU) the tuples hold every class, and the yardstick does on them what the header says: an
    fp16 comes back unchanged from all three, sign included; a midpoint goes to the even
    neighbour; magnitudes below 2^-14 (f16_floor's e < 113) of both signs, -0, both saturating
    returns and NaN of both signs are there"""
    t, cls = round_tuples()
    want = round_expected()
    assert 3e5 <= len(t) <= 4e5 and set(cls) == {"fp16", "succ", "pred", "mid", "edges",
                                                 "nonfinite", "random"}
    h = np.arange(0x7C00, dtype=U32)
    h = np.concatenate([h, h | U32(0x8000)])
    f = want[cls["fp16"]]
    assert np.array_equal(f[:, 0], h) and np.array_equal(f[:, 1], h & U32(0x7FFF))
    assert np.array_equal(f[:, 2], h)
    m = want[cls["mid"]][:, 2] & U32(0x7FFF)
    lo = np.arange(0x7BFF, dtype=U32)
    even = np.where(lo & U32(1), lo + U32(1), lo)
    assert np.array_equal(m, np.concatenate([even, even]))
    s = want[cls["succ"]]       # just above an fp16: nearest is the floor, the hash may go one up
    assert np.array_equal(s[:0x7BFF, 2], h[:0x7BFF])
    assert set((s[:0x7BFF, 0] - h[:0x7BFF]).tolist()) == {0, 1}
    nv = t[:, 0].copy().view(F)
    small = (np.abs(nv) < TINY) & (nv != 0)
    assert (small & (nv > 0)).sum() > 5000 and (small & (nv < 0)).sum() > 5000
    assert (t[:, 0] == 0x80000000).any() and (want[t[:, 0] == 0x80000000] ==
                                               [0x8000, 0, 0x8000]).all()
    sat = ~(np.abs(nv) < 65504)
    assert (want[sat & ~np.signbit(nv)] == 0x7BFF).all() and (sat & ~np.signbit(nv)).sum() > 100
    assert (want[sat & np.signbit(nv)] == [0xFBFF, 0x7BFF, 0xFBFF]).all()
    assert (np.isnan(nv) & np.signbit(nv)).any() and (np.isnan(nv) & ~np.signbit(nv)).any()
    assert set(t[:, 3].tolist()) == set(range(64))


@gpu
def test_device_rounds_are_the_headers(H):
    """vhalf_round, vaux16_round and f16_nearest as fm_half.hip compiles them, one launch over
    ~3.6 10^5 tuples, against the numpy yardstick bit for bit"""
    t, cls = round_tuples()
    c = H.Context(0, max_keys=64, V_dim=32, **HALF)
    got = H.Store(c).half_round_table(t)
    c.close()
    want = round_expected()
    for name, sl in cls.items():
        bad = np.nonzero((got[sl] != want[sl]).any(1))[0]
        assert not len(bad), (name, len(bad), t[sl][bad[:4]], got[sl][bad[:4]], want[sl][bad[:4]])


def test_host_rounds_are_the_headers(tmp_path):
    """(CPU) the host compile of csrc/vhalf.h (tests/host/half_round_check.cc) on a few thousand of
    the tuples, every class among them, against the same yardstick"""
    t, cls = round_tuples()
    pick = np.concatenate([np.arange(sl.start, sl.stop)[::max(1, (sl.stop - sl.start) // 700)]
                           for sl in cls.values()])
    assert 3000 <= len(pick) <= 8000
    subprocess.check_call(["make", "-s", "build/half_round_check"], cwd=ROOT)
    t[pick].tofile(str(tmp_path / "in"))
    r = subprocess.run([os.path.join(ROOT, "build", "half_round_check"), str(tmp_path / "in")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = np.array([[int(x, 16) for x in ln.split()] for ln in r.stdout.splitlines()], U32)
    assert got.shape == (len(pick), 3)
    assert np.array_equal(got, round_expected()[pick])
