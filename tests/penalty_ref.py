"""Test infrastructure: the yardstick of Store.evaluate (csrc/store.hip k_penalty, which restates
SGDUpdater::Evaluate, sgd_updater.cc:15-32), in plain Python and numpy, and the builders of the
models tests/test_gpu_penalty.py plants.  tests/test_penalty_ref.py proves both on the CPU.

Evaluate, per stored entry e (l1, l2 the float32 parameters, dim = V_dim):

    if (e.w) ++nnz;
    objv += l1 * fabs(e.w) + .5 * l2 * e.w * e.w;
    if (e.V) { nnz += dim; for i < dim: objv += .5 * l2 * e.V[i] * e.V[i]; }     (sic: l2, not V_l2)

It looks at e.V, not at what Get shows: a V that l1_shrk hides because w == 0 is summed and counted.
"""
import math

import numpy as np

from tests.edge_ref import _private_keys

F = np.float32
U53, U24 = 2.0 ** -53, 2.0 ** -24
KINDS = ("w_v", "w_nov", "zero_v", "zero_nov", "neg_zero", "subnormal", "huge")


def penalty(entries, l1, l2, d):
    """entries: a list of (w: float32, V: float32[d] or None) -> (S, nnz, bound, kinds).

    Terms, in double from the float32 operands, in the order C++ evaluates them:
      l1 * |w|              one term per entry: 24 x 24 bits, exact in double
      ((.5 * l2) * w) * w   one term per entry: the first two products are exact (.5 * l2 is a
                            float, then 24 x 24 bits), the last is rounded once
      ((.5 * l2) * V[i]) * V[i]     d terms per entry with V, likewise
    S = math.fsum of all n terms (exact, then rounded once); nnz: +1 where w != 0 (-0.0 is not
    counted, a subnormal is), +d where V is not None.

    bound on |device - S|, derived, not measured.  All terms are >= 0.
      (1) The device adds its n double terms in some order (a thread's own terms one after the
          other, then wave shuffles, then atomics; the zeros of idle lanes add exactly): n - 1
          roundings at most on any path, so |fl(sum) - sum| <= n u / (1 - n u) * sum, u = 2^-53.
      (2) The last product of a term is rounded once, 2^-53 relative.  The device forms the same
          IEEE products as this file, but a yardstick must not lean on that: u * S.
      (3) l1 * fabs(w), store.hip:654: both operands are float and HIP's device fabs(float)
          returns float, so the product is a FLOAT product (v_mul_f32 of s, |v| in the gfx950
          code of k_penalty, widened afterwards), 2^-24 relative where it is normal and at most
          2^-150 absolute where it is subnormal (denormals are kept, float_denorm_mode_32 = 3).
          oracle.cc:534 (std::fabs(float)) forms the same float product; this yardstick forms the
          exact double one.  The model is the same either way; the bound takes
          2^-24 * sum of the l1 terms + 2^-150 per entry.
    kinds: how many entries are w != 0 with V, w != 0 without, w == 0 with V, w == 0 without,
    w == -0.0, subnormal w, |w| > 2^64 (w * w overflows float there, not the double terms)."""
    l1, l2 = F(l1), F(l2)
    assert l1 >= 0 and l2 >= 0
    half = np.float64(0.5) * np.float64(l2)
    terms, l1_terms, nnz = [], [], 0
    kinds = dict.fromkeys(KINDS, 0)
    for w, V in entries:
        w = F(w)
        wd = np.float64(w)
        l1_terms.append(float(np.float64(l1) * abs(wd)))
        terms.append(float(half * wd * wd))
        if w != 0:
            nnz += 1
        if V is not None:
            V = np.asarray(V)
            assert V.dtype == np.float32 and V.shape == (d,) and d > 0
            nnz += d
            Vd = V.astype(np.float64)
            terms.extend((half * Vd * Vd).tolist())
        kinds[("w" if w != 0 else "zero") + ("_v" if V is not None else "_nov")] += 1
        kinds["neg_zero"] += int(w == 0 and np.signbit(w))
        kinds["subnormal"] += int(0 < abs(wd) < 2.0 ** -126)
        kinds["huge"] += int(abs(wd) > 2.0 ** 64)
    n = len(terms) + len(l1_terms)
    S = math.fsum(terms + l1_terms)
    assert math.isfinite(S) and n * U53 < 0.5
    bound = n * U53 / (1 - n * U53) * S + U53 * S + U24 * math.fsum(l1_terms) \
        + len(entries) * 2.0 ** -150
    return S, nnz, bound, kinds


def n_terms(entries):
    return sum(2 + (0 if V is None else len(V)) for _, V in entries)


def entries_of(up, keys):
    """the (w, V) of every key an updater (oracle.Updater, line16_ref.Updater) holds"""
    d, out = up.V_dim, []
    for k in keys:
        e = up.entry(k)
        if e is not None:
            out.append((e[0][0], None if e[1] is None else e[1][:d].copy()))
    return out


# ---------------------------------------------------------------- the planted model
L1, L2, V_L2 = 0.5, 0.25, 0.01      # l2 != V_l2, Vaux != V: a kernel that mixes them up must miss
PLANT_KEYS = 336
# per 16 keys: (w, has V).  None: a random w of either sign
_CYCLE = [(None, True), (None, False), (0.0, True), (0.0, False), (None, True), ("count", False),
          (-0.0, False), (-0.0, True), (2.0 ** -140, False), (-2.0 ** -149, True), (None, True),
          ("huge+", False), ("huge-", True), (0.0, True), (None, False), (None, True)]


def plant(d, huge, seed=29, narrow=None):
    """-> model entries (key, w, sqrt_g, z, V | None, Vaux | None) for edge_ref.write_model, in a
    shuffled order (a file's order is the split layout's pool-row order; slots go by the hash).

    Every class of `kinds`; a count-only record (w = sqrt_g = z = 0, no V); w = 3e19 and -2.5e19,
    whose w * w overflows float.  huge: those two and V ~ 2^60 N(0, 1), so that the V terms weigh
    what the two w terms weigh (~1e38) and a wrong V term shows; the sum is past FLT_MAX, which
    Evaluate's float accumulator cannot hold, so the oracle is not consulted there.  not huge: the same plant without |w| > 2^64 and with
    V ~ N(0, 1) / 2 — sums of order 100, where the l1 terms show and the oracle can be asked.
    Vaux in [0.5, 100), not fp16 numbers: never V's values, and a vaux=f16 slot narrows them.
    narrow: applied to V and Vaux (half_ref.nearest_f16 for a vrows=f16 table, whose load is then
    exact; not with huge, whose V no fp16 holds)."""
    assert narrow is None or not huge
    rng = np.random.default_rng(seed + d)
    keys = _private_keys(PLANT_KEYS)[0]
    out = []
    for i, k in enumerate(keys):
        w, has_v = _CYCLE[i % len(_CYCLE)]
        sg, z = F(rng.random() + .5), F(rng.standard_normal())
        rw = F(rng.standard_normal() * .7) or F(.25)
        if w is None:
            w = rw
        elif w == "count":
            w, sg, z = F(0), F(0), F(0)
        elif w in ("huge+", "huge-"):
            w = (F(3e19) if w == "huge+" else F(-2.5e19)) if huge else rw
        V = C = None
        if has_v and d > 0:
            V = (rng.standard_normal(d) * (2.0 ** 60 if huge else .5)).astype(F)
            C = (rng.random(d) * 99.5 + .5).astype(F)
            if narrow is not None:
                V, C = narrow(V), narrow(C)
        out.append((int(k), F(w), sg, z, V, C))
    return [out[i] for i in rng.permutation(len(out))]


def model_entries(planted):
    return [(w, V) for _, w, _, _, V, _ in planted]


def variants(planted):
    """the planted model as four wrong kernels would sum it -> {name: S}: Vaux read in place of V;
    V_l2 in place of l2 on the V terms; the V terms dropped; a hidden V (w == 0) skipped.  Each is
    the yardstick itself on changed inputs."""
    d = max([len(V) for _, _, _, _, V, _ in planted if V is not None] or [0])
    S = lambda ent, l1=L1, l2=L2: penalty(ent, l1, l2, d)[0]   # noqa: E731
    w_only = [(w, None) for _, w, _, _, _, _ in planted]
    v_only = [(F(0), V) for _, _, _, _, V, _ in planted if V is not None]
    return {"vaux_for_v": S([(w, C) for _, w, _, _, _, C in planted]),
            "v_l2_for_l2": S(w_only) + S(v_only, 0.0, V_L2),
            "no_v_term": S(w_only),
            "hidden_v_skipped": S([(w, None if w == 0 else V) for _, w, _, _, V, _ in planted])}


# ---------------------------------------------------------------- the layouts
def es_line(d, slot_layout="auto", vaux=None):
    """(Table::es, Table::line) of a context: ctx.hip:359-360 with common.h fat_es / line_es"""
    if slot_layout == "line":
        if vaux == "f16":
            return (2 if d == 16 else 0), 2
        return {4: 1, 8: 2, 12: 2}.get(d, 0), 1
    if slot_layout == "split" or d < 4 or d % 4 or 32 + 4 * d > 128:
        return 0, 0
    return (1 if 32 + 4 * d <= 64 else 2), 0


LINE16 = dict(slot_layout="line", vaux="f16")
# (V_dim, context kwargs, (es, line))
LAYOUTS = [
    (0, {}, (0, 0)),
    (5, {}, (0, 0)),
    (16, dict(slot_layout="split"), (0, 0)),
    (200, {}, (0, 0)),
    (4, {}, (1, 0)),
    (8, {}, (1, 0)),
    (16, {}, (2, 0)),
    (24, {}, (2, 0)),
    (4, dict(slot_layout="line"), (1, 1)),
    (8, dict(slot_layout="line"), (2, 1)),
    (12, dict(slot_layout="line"), (2, 1)),
    (16, LINE16, (2, 2)),
]
# half rows (vrows=f16): the split layout's table, pool rows of [V | Vaux] fp16
HALF = dict(vrows="f16")
HALF_LAYOUTS = [(32, HALF, (0, 0)), (64, HALF, (0, 0))]
# what table_alloc can be handed: es 0 (split), fat_es's 1 and 2, line_es's 1 and 2, line16's 2
EVERY_ES_LINE = {(0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2)}


def layout_id(i):
    d, kw, _ = LAYOUTS[i]
    return "d%d-%s" % (d, "-".join(str(v) for _, v in sorted(kw.items())) or "auto")


# ---------------------------------------------------------------- the trained model
# test_gpu_line_slots.LAZY with l2 > 0: keys that never get V (fea_cnt <= V_threshold) and keys
# whose V Get hides when the flipped labels take w back to 0
LAZY_CFG = dict(V_threshold=10, l1=2.0, l1_shrk=1, lr=.05, V_lr=.01, l2=L2)


def lazy_batches():
    """test_gpu_line_slots._batch(True): -> (the batch, the batch with its labels flipped, keys)"""
    from difacto_amd import data as D
    from oracle import oracle as O
    from tests import backward_ref as R
    blk = R.planted_batch(1024, 8, (1, 128, 129, 896, 897), True, seed=11)
    neg = D.RowBlock(blk.offs, blk.ids, blk.vals, -blk.labels, blk.weights)
    return blk, neg, O.localize(blk.offs, blk.ids)[0]


def hidden_and_bare(up, keys):
    """-> (keys whose V Get hides, keys without V) in an updater's state"""
    ent, (_, lens) = [up.entry(k) for k in keys], up.get(keys)
    return (sum(e[1] is not None and n == 1 for e, n in zip(ent, lens)),
            sum(e[1] is None for e in ent))
