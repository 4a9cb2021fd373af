"""tests/penalty_ref.py on the CPU: the yardstick of Store.evaluate against the oracle's restatement
of SGDUpdater::Evaluate, and the planted model's power to tell a wrong kernel from a right one —
before tests/test_gpu_penalty.py hands either to a GPU."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import backward_ref as R
from tests import edge_ref as E
from tests import half_ref as HR
from tests import line16_ref as L16
from tests import penalty_ref as PR

F = np.float32


def _against_oracle(up, keys, l1, l2):
    """nnz equal; S within the error the issue grants the reference's accumulator: n_terms sums of
    relative error 2^-24 each (SGDUpdater::Evaluate adds into a float; oracle.cc's objv is a double
    and its l1 product a float one, so it sits well inside)"""
    ent = PR.entries_of(up, keys)
    S, nnz, bound, kinds = PR.penalty(ent, l1, l2, up.V_dim)
    want, want_nnz = up.penalty()
    assert nnz == want_nnz and isinstance(nnz, int)
    tol = PR.n_terms(ent) * 2.0 ** -24 * S
    assert bound <= tol          # the device is held to less than the reference's own error
    assert abs(S - want) <= tol, (S, want, tol)
    return S, kinds


def test_hand_case():
    """numbers small enough to add by hand: l1 = .5, l2 = .25, d = 2"""
    ent = [(F(2), None), (F(-3), np.array([1, -2], F)), (F(-0.0), np.array([4, 0], F)), (F(0), None)]
    S, nnz, bound, kinds = PR.penalty(ent, .5, .25, 2)
    #   l1 |w|: 1 + 1.5     l2/2 w^2: .5 + 1.125     l2/2 V^2: .125 + .5 + 2
    assert S == 6.75 and nnz == 2 + 2 * 2
    assert kinds == dict(w_v=1, w_nov=1, zero_v=1, zero_nov=1, neg_zero=1, subnormal=0, huge=0)
    assert 0 < bound < 1e-6
    assert PR.penalty([], .5, .25, 2)[:2] == (0.0, 0)
    # the parameters are the floats the context parsed: .1f is not .1
    assert PR.penalty([(F(1), None)], .1, 0, 0)[0] == float(F(.1))
    # a term float cannot hold, and the count of a subnormal
    S, nnz, _, kinds = PR.penalty([(F(3e19), None), (F(2.0 ** -149), None)], 0, .25, 0)
    assert S == .125 * float(F(3e19)) ** 2 and S > float(np.finfo(F).max) / 4 and nnz == 2
    assert kinds["huge"] == 1 and kinds["subnormal"] == 1


@pytest.mark.parametrize("d", [0, 5, 16])
def test_trained_and_loaded_models_match_oracle(d, tmp_path):
    """three fused steps of the lazy recipe (one count push, two training steps, the labels
    flipped in between), then the saved model loaded into a fresh updater"""
    cfg = dict(PR.LAZY_CFG, V_dim=d)
    blk, neg, uniq = PR.lazy_batches()
    up = O.Updater(**cfg)
    for step in range(3):
        R.fused_step(up, (blk, neg)[step % 2], push_cnt=(step == 0))
        S, kinds = _against_oracle(up, uniq, cfg["l1"], cfg["l2"])
        assert S > 0
    if d > 0:
        assert kinds["zero_v"] > 0 and kinds["w_nov"] + kinds["zero_nov"] > 0 and kinds["w_v"] > 0
    up.save(str(tmp_path / "m"), True)
    up2 = O.Updater(**cfg)
    up2.load(str(tmp_path / "m"))
    assert _against_oracle(up2, uniq, cfg["l1"], cfg["l2"])[0] == S


def test_lazy_recipe_on_the_gpu_tests_layouts():
    """what test_gpu_penalty's trained cases assert about the reference's state, at their V_dims
    (8: split, fat, line; 16: line16), here on the reference alone"""
    blk, neg, uniq = PR.lazy_batches()
    for up in (O.Updater(**dict(PR.LAZY_CFG, V_dim=8)), L16.Updater(**dict(PR.LAZY_CFG, V_dim=16))):
        for step in range(3):
            R.fused_step(up, (blk, neg)[step % 2], push_cnt=(step == 0))
        hidden, bare = PR.hidden_and_bare(up, uniq)
        assert hidden > 0 and bare > 0, (up.V_dim, hidden, bare)


@pytest.mark.parametrize("d", [0, 5, 16])
def test_plain_plant_matches_oracle(d, tmp_path):
    """the planted model without its |w| > 2^64 loads into the oracle: the builder, the writer and
    the yardstick agree with Evaluate on -0.0, subnormal, hidden-V and count-only entries"""
    planted = PR.plant(d, huge=False)
    E.write_model(str(tmp_path / "m"), d, planted)
    up = O.Updater(V_dim=d, l1=PR.L1, l2=PR.L2, V_l2=PR.V_L2)
    up.load(str(tmp_path / "m"))
    keys = [k for k, *_ in planted]
    S, kinds = _against_oracle(up, keys, PR.L1, PR.L2)
    ref = PR.penalty(PR.model_entries(planted), PR.L1, PR.L2, d)
    assert (S, kinds) == (ref[0], ref[3])
    assert kinds["neg_zero"] > 0 and kinds["subnormal"] > 0 and kinds["huge"] == 0


@pytest.mark.parametrize("huge", [True, False], ids=["huge", "plain"])
@pytest.mark.parametrize("i", range(len(PR.LAYOUTS)), ids=PR.layout_id)
def test_plant_discriminates(i, huge):
    """every class is planted, and each wrong kernel's sum lies more than 100 bounds from S: the
    condition under which test_gpu_penalty's planted cases can fail"""
    d = PR.LAYOUTS[i][0]
    planted = PR.plant(d, huge)
    S, nnz, bound, kinds = PR.penalty(PR.model_entries(planted), PR.L1, PR.L2, d)
    print("V_dim %d huge %d: S %.17g nnz %d bound %.3g %s" % (d, huge, S, nnz, bound, kinds))
    assert len({k for k, *_ in planted}) == len(planted) == PR.PLANT_KEYS
    with_v = ("w_v", "zero_v") if d == 0 else ()
    for name in PR.KINDS:
        assert (kinds[name] > 0) == (name not in with_v and (huge or name != "huge")), name
    # w * w overflows float, and the sum the float accumulator of Evaluate: no oracle for this plant
    assert (S > float(np.finfo(F).max)) == huge
    with np.errstate(over="ignore"):
        assert np.isinf(F(3e19) * F(3e19)) and np.isinf(F(-2.5e19) * F(-2.5e19))
    if d == 0:
        return
    assert PR.L2 != PR.V_L2
    for k, w, sg, z, V, C in planted:
        assert V is None or (not np.array_equal(V, C) and (C != L16.nearest_f16(C)).any())
    for name, wrong in PR.variants(planted).items():
        print("  %s: S' %.17g, |S' - S| = %.3g bounds" % (name, wrong, abs(wrong - S) / bound))
        assert abs(wrong - S) > 100 * bound, (name, wrong, S, bound)


@pytest.mark.parametrize("d", [32, 64])
def test_half_plant_discriminates(d):
    """the plain plant narrowed to fp16 (what a vrows=f16 table holds exactly): every class but
    huge, V and Vaux all fp16 numbers and still apart, and each wrong kernel — v_get reading the
    Vaux half among them — more than 100 bounds from S"""
    assert [(dd, kw) for dd, kw, _ in PR.HALF_LAYOUTS] == [(32, PR.HALF), (64, PR.HALF)]
    planted = PR.plant(d, False, narrow=HR.nearest_f16)
    S, nnz, bound, kinds = PR.penalty(PR.model_entries(planted), PR.L1, PR.L2, d)
    print("half V_dim %d: S %.17g nnz %d bound %.3g %s" % (d, S, nnz, bound, kinds))
    assert len({k for k, *_ in planted}) == len(planted) == PR.PLANT_KEYS
    for name in PR.KINDS:
        assert (kinds[name] > 0) == (name != "huge"), name
    for k, w, sg, z, V, C in planted:
        if V is not None:
            assert np.array_equal(V, HR.nearest_f16(V)) and np.array_equal(C, HR.nearest_f16(C))
            assert not np.array_equal(V, C) and V.shape == C.shape == (d,)
    for name, wrong in PR.variants(planted).items():
        print("  %s: S' %.17g, |S' - S| = %.3g bounds" % (name, wrong, abs(wrong - S) / bound))
        assert abs(wrong - S) > 100 * bound, (name, wrong, S, bound)


@pytest.mark.parametrize("d", [32, 64])
def test_lazy_recipe_on_half_rows(d):
    """what test_gpu_penalty's trained half-row cases assert about the yardstick's state"""
    blk, neg, uniq = PR.lazy_batches()
    up = HR.Updater(**dict(PR.LAZY_CFG, V_dim=d))
    for step in range(3):
        R.fused_step(up, (blk, neg)[step % 2], push_cnt=(step == 0))
    hidden, bare = PR.hidden_and_bare(up, uniq)
    kinds = PR.penalty(PR.entries_of(up, uniq), PR.LAZY_CFG["l1"], PR.LAZY_CFG["l2"], d)[3]
    assert hidden > 0 and bare > 0 and kinds["zero_v"] >= hidden and kinds["w_v"] > 0, kinds


def test_layouts_cover_every_es_and_line():
    """the table names what es_line derives, and holds every (es, line) a table can be allocated
    with, the issue's list of V_dims per layout included"""
    for d, kw, want in PR.LAYOUTS:
        assert PR.es_line(d, **kw) == want
    assert {w for _, _, w in PR.LAYOUTS} == PR.EVERY_ES_LINE
    # es_line over every V_dim and every kwarg a context takes produces nothing else
    seen = {PR.es_line(d, **kw) for d in range(0, 300)
            for kw in ({}, dict(slot_layout="split"), dict(slot_layout="fat"))}
    seen |= {PR.es_line(d, slot_layout="line") for d in (4, 8, 12)} | {PR.es_line(16, **PR.LINE16)}
    assert seen == PR.EVERY_ES_LINE
    have = {(d, kw.get("slot_layout", "auto"), kw.get("vaux")) for d, kw, _ in PR.LAYOUTS}
    assert have == {(0, "auto", None), (5, "auto", None), (16, "split", None), (200, "auto", None),
                    (4, "auto", None), (8, "auto", None), (16, "auto", None), (24, "auto", None),
                    (4, "line", None), (8, "line", None), (12, "line", None), (16, "line", "f16")}
