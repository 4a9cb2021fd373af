"""Test infrastructure: deterministic inputs that sit on the edges of the hot path's arithmetic,
for tests/test_gpu_loss_edges.py; tests/test_edge_ref.py proves on the CPU, from the oracle and
numpy alone, that each builder hits what it claims.

p_sweep     predictions handed straight to CalcGrad: every float exponent, the neighbourhoods of
            expf's four early-out cuts, of the subnormal turn, of 1 + e == 1, of the clip, and
            the specials.
clip_case   a batch and a planted model whose unclipped predictions sit on and around +-20, far
            beyond it, at +-FLT_MAX, +-inf and NaN.  Every planted number and every partial sum
            is exact in float, so any summation order gives the same bits and the plain oracle
            is the reference on the split and the sharded paths too.
ftrl_edges  planted (w, sqrt_g, z) and one gradient each whose new z is exactly +-l1, its
            neighbours on both sides, and 0.

Model entries are tuples (key, w, sqrt_g, z, V | None, Vaux | None), the form
tests/test_gpu_modelfile._write_model writes; write_model here is the same writer without that
module's GPU imports, so one file loads into oracle.Updater.load and into Store.load."""
import struct

import numpy as np

from difacto_amd import data as D
from tests.localizer_ref import reverse_bytes

F = np.float32
FLT_MAX = np.finfo(np.float32).max
# glibc expf's cuts (csrc/expf.h): overflow above OVER, underflow (0.0f) below UNDER
OVER = F(float.fromhex("0x1.62e42ep6"))
UNDER = F(float.fromhex("-0x1.9fe368p6"))
SUBN = F(-87.33655)      # expf(x) turns subnormal below this
ONE_PLUS = F(16.635532)  # 1 + expf(-x) stops changing above this
NAN_BITS = (0x7FC00000, 0xFFC00001, 0x7F800001)   # quiet, negative quiet with payload, signalling
SWEEP_ROWS = 1 << 18


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits1(x):
    """the bit pattern of one float"""
    return int(np.float32(x).view(np.uint32))


def write_model(path, d, entries):
    """SGDUpdater::Save's format with aux (test_gpu_modelfile._write_model)"""
    with open(path, "wb") as f:
        f.write(b"\x01")
        for key, w, sg, z, V, C in entries:
            f.write(struct.pack("<Qi", int(key), 1 + d if V is not None else 1))
            f.write(np.float32([w, sg, z]).tobytes())
            if V is not None:
                f.write(np.float32(V).tobytes() + np.float32(C).tobytes())


def _private_keys(n):
    """n model keys in ascending order, spread over the whole 64-bit range (so they spread over
    the table and over the owners of a sharded store), and the feature ids that map to them: the
    Localizer's rank of row i's key is i"""
    stride = np.uint64((1 << 64) // (n + 1))
    keys = np.arange(1, n + 1, dtype=np.uint64) * stride | np.uint64(5)
    return keys, reverse_bytes(keys)


# ---------------------------------------------------------------- p_sweep
def _near(x, n=64):
    """the bit patterns within n ulp of x on either side (same sign)"""
    b = bits1(x)
    return np.arange(b - n, b + n + 1, dtype=np.int64)


def sweep_values():
    """-> uint32 bit patterns of the sweep's predictions (unpadded)"""
    mant = np.array([0, 1, 2, 0x7FFFFF, 0x7FFFFE, 0x400000, 0x3FFFFF, 0x400001, 0x555555, 0x2AAAAA,
                     0x123456, 0x6DCBA9, 0x0000FF, 0x7FFF00, 0x100000, 0x31D2A7], np.int64)
    assert len(set(mant.tolist())) == 16
    out = []
    for sign in (0, 1 << 31):
        for e in range(255):                    # subnormals (e = 0) to the largest binade
            out.append(sign | (e << 23) | mant)
    for x in (0.0, OVER, -UNDER, 88.0, -SUBN, ONE_PLUS, 20.0):
        for s in (1, -1):
            if x == 0.0:                        # +-0 and the smallest subnormals beside them
                out.append(np.arange(0, 65, dtype=np.int64) | (0 if s > 0 else 1 << 31))
            else:
                out.append(_near(F(s) * F(x)))
    special = [1, 0x007FFFFF, 0x7F7FFFFF, 0x7F800000]      # denorm min / max, FLT_MAX, inf
    out.append(np.array(special + [v | 1 << 31 for v in special] + list(NAN_BITS), np.int64))
    return np.concatenate(out).astype(np.uint32)


def p_sweep():
    """-> (blk, pred, labels, rw): SWEEP_ROWS rows of one nnz, row i's key of rank i; blk is
    valued (x in [0.5, 1.5)) and carries rw as its row weights — the binary, unweighted run
    takes blk.vals = blk.weights = None.  The sweep's values are repeated to fill the block, so
    both label signs meet every value (the period is odd, the labels alternate)."""
    v = sweep_values()
    assert len(v) % 2 == 1 and 2 * len(v) <= SWEEP_ROWS
    B = SWEEP_ROWS
    pred = np.resize(v, B).view(np.float32)
    labels = np.where(np.arange(B) % 2 == 0, 1.0, -1.0).astype(np.float32)
    rng = np.random.default_rng(1618)
    rw = (rng.random(B, dtype=np.float32) + F(0.5)).astype(np.float32)
    x = (rng.random(B, dtype=np.float32) + F(0.5)).astype(np.float32)
    _, ids = _private_keys(B)
    blk = D.RowBlock(np.arange(B + 1, dtype=np.uint64), ids, x, labels, rw)
    return blk, pred, labels, rw


# ---------------------------------------------------------------- clip_case
ULP20 = 2.0 ** -19          # the spacing of floats in [16, 32)
# the unclipped predictions, both signs taken below: 20 and its neighbours to 4 ulp (k = 1 is
# nextafter), far beyond, and a value inside (no clip)
NEAR20 = [20.0 + k * ULP20 for k in range(-4, 5)]
CLASSES = ("below", "at", "above", "far", "fltmax", "inf", "nan", "inside")


def _class_of(t):
    """the class of a finite or infinite unclipped prediction"""
    a = abs(t)
    if np.isnan(t):
        return "nan"
    if np.isinf(t):
        return "inf"
    if a == float(FLT_MAX):
        return "fltmax"
    if a == 20.0:
        return "at"
    if a < 16.0:
        return "inside"
    if a < 20.0:
        return "below"
    return "above" if a < 21.0 else "far"


def clip_case(d, binary):
    """-> (blk, entries, targets): at most 512 rows of 1-3 nnz over private keys, the planted
    model, and targets = {"want": float64[B] the unclipped prediction of every row (NaN for the
    NaN group), "rows": {class: row indices}, "nan_grads": the NaN elements a CalcGrad of the
    whole batch holds in the Pull layout, "train": the rows outside the NaN group}.

    Rows, for every value t of NEAR20, 1e4 and 7.5 in both signs:
      one key without V               pred = w x                           (w x = t)
      two keys with V = (v, 0, ...)   pred = w_a x_a + w_b x_b + (v_a x_a)(v_b x_b), d > 0 only:
                                      the cross term is 2, w_a x_a = +-16 (8192 for 1e4)
    and  +-FLT_MAX (one key) and +-inf (w = +-0x1p127 twice), and the NaN group: +inf + -inf in
    the linear term (w = +-inf), and at d > 0 inf - inf in s (one key with V = (0x1p64, 0, ...):
    XV^2 and XXVV both overflow).  Valued blocks scale x by 2 or 0.5 and the planted numbers by
    the inverse, so every product is exact; rows whose w could not be scaled take x = 1."""
    ks = _private_keys(3 * 512)[0]
    # alternately from the lower and the upper half: a row's keys lie on different owners
    keys_it = iter(np.stack([ks[:768], ks[768:]], 1).ravel())
    entries, rows, want, labels = [], [], [], []
    ones = np.ones(max(d, 1), np.float32)[:d]

    def vrow(v):
        V = np.zeros(d, np.float32)
        V[0] = v
        return V, ones.copy()

    def key(w, v=None):
        k = next(keys_it)
        V, C = vrow(v) if v is not None else (None, None)
        entries.append((int(k), F(w), F(1.0), F(0.0), V, C))
        return k

    def one(t, scale=True):
        x = 1.0
        if not binary and scale and abs(t) < 1e30:
            x = 0.5 if len(rows) % 2 else 2.0
        rows.append([(key(t / x), x)])
        want.append(t)

    def two(t):
        sgn = 1.0 if t > 0 else -1.0
        wa = sgn * (8192.0 if abs(t) > 100 else 16.0)
        wb = t - 2.0 - wa
        xa, xb = (1.0, 1.0) if binary else (2.0, 0.5)
        rows.append([(key(wa / xa, 2.0 / xa), xa), (key(wb / xb, 1.0 / xb), xb)])
        want.append(t)

    for y in (1.0, -1.0):                       # every value under both labels
        for mag in NEAR20 + [1e4, 7.5]:
            for t in (mag, -mag):
                one(t)
                if d > 0:
                    two(t)
        for s in (1.0, -1.0):
            one(s * float(FLT_MAX), scale=False)
            rows.append([(key(s * 2.0 ** 127), 1.0), (key(s * 2.0 ** 127), 1.0)])
            want.append(s * np.inf)
        labels += [y] * (len(rows) - len(labels))
    n_train = len(rows)
    nan_grads = 0
    for s in (1.0, -1.0):                       # +inf + -inf in the linear term
        rows.append([(key(s * np.inf), 1.0), (key(-s * np.inf), 1.0), (key(3.0), 1.0)])
        want.append(np.nan)
        nan_grads += 3
    if d > 0:
        for w in (1.0, -2.0):                   # inf - inf in s
            x = 1.0 if binary else 0.5
            rows.append([(key(w / x, 2.0 ** 64 / x), x)])
            want.append(np.nan)
            nan_grads += 1 + d
    assert len(rows) <= 512
    offs = np.zeros(len(rows) + 1, np.uint64)
    offs[1:] = np.cumsum([len(r) for r in rows])
    ks = np.array([k for r in rows for k, _ in r], np.uint64)
    xs = np.array([x for r in rows for _, x in r], np.float32)
    labels += [1.0, -1.0] * ((len(rows) - n_train) // 2)
    blk = D.RowBlock(offs, reverse_bytes(ks), None if binary else xs, np.array(labels, np.float32))
    want = np.array(want, np.float64)
    cls = {c: [] for c in CLASSES}
    for i, t in enumerate(want):
        cls[_class_of(t)].append(i)
    targets = {"want": want, "rows": {c: np.array(r, np.int64) for c, r in cls.items()},
               "nan_grads": nan_grads, "train": np.arange(n_train)}
    return blk, entries, targets


def take_rows(blk, rows):
    """the block of the given rows, in that order"""
    o = blk.offs.astype(np.int64)
    idx = np.concatenate([np.arange(o[r], o[r + 1]) for r in rows]) if len(rows) else \
        np.zeros(0, np.int64)
    offs = np.zeros(len(rows) + 1, np.uint64)
    offs[1:] = np.cumsum([o[r + 1] - o[r] for r in rows])
    return D.RowBlock(offs, blk.ids[idx], None if blk.vals is None else blk.vals[idx],
                      blk.labels[rows], None if blk.weights is None else blk.weights[rows])


# ---------------------------------------------------------------- ftrl_edges
def _exact_pair(t):
    """(z, g) floats with w = 0 whose FTRL step gives z - g == t exactly"""
    t = F(t)
    for g in (F(0.5), F(0.25), F(2.0), F(-0.5), F(1.0)):
        z = F(t + g)
        if F(z - g) == t and np.float64(z) - np.float64(g) == np.float64(t):
            return z, g
    raise AssertionError(t)


def ftrl_edges(l1, lr, lr_beta=1.0, V_threshold=2):
    """-> (entries, counts, grads, names): model entries without V in ascending key order, the
    count each key is pushed before the gradient (Update(kFeaCount)), its w gradient, and what
    each entry is there for.  l2 = 0 is assumed (gw = g).

    w = 0 entries: z_new = z - g exactly, at 0, +-l1, and the floats next to +-l1 on both sides;
    the two outside leave zero (new_w + 1), drawing V when the planted count is V_threshold + 1
    and not at V_threshold.  Then w != 0 -> 0, w != 0 with g = 0, w = 0 with g = 0, counts at and
    past the threshold on keys with w != 0 (Update(kFeaCount)'s own InitV), and with lr_beta = 0
    the entries with sqrt_g = 0 and g = 0: eta = 0, w = (z -+ l1) / 0 = +-inf as the reference
    computes it, or 0 inside the band."""
    l1 = F(l1)
    keys = iter(_private_keys(64)[0])
    entries, counts, grads, names = [], [], [], []

    def add(name, w, sg, z, g, cnt=0.0):
        entries.append((int(next(keys)), F(w), F(sg), F(z), None, None))
        counts.append(F(cnt))
        grads.append(F(g))
        names.append(name)

    up, dn = F(np.inf), F(-np.inf)
    edge = [("zero", F(0)), ("at+l1", l1), ("at-l1", -l1),
            ("out+l1", np.nextafter(l1, up)), ("out-l1", np.nextafter(-l1, dn)),
            ("in+l1", np.nextafter(l1, dn)), ("in-l1", np.nextafter(-l1, up))]
    for cnt in (V_threshold, V_threshold + 1):
        for name, t in edge:
            z, g = _exact_pair(t)
            add("%s/cnt%d" % (name, cnt), 0.0, 0.75, z, g, cnt)
    add("w->0", 0.5, 1.0, 0.2 * float(l1), 0.1 * float(l1))
    add("w->0 neg", -0.5, 1.0, -0.2 * float(l1), -0.1 * float(l1))
    add("w,g=0", 0.5, 1.0, 3.0 * float(l1) + 1.0, 0.0)
    add("w=0,g=0", 0.0, 1.0, 0.5 * float(l1), 0.0)
    add("w=0,g=0,out", 0.0, 1.0, -3.0 * float(l1) - 1.0, 0.0)
    add("cnt at", 0.25, 1.0, 2.0 * float(l1) + 1.0, 0.125, V_threshold)
    add("cnt past", 0.25, 1.0, 2.0 * float(l1) + 1.0, 0.125, V_threshold + 1)
    if lr_beta == 0:
        add("eta0 +", 0.0, 0.0, 2.0 * float(l1) + 1.0, 0.0)
        add("eta0 -", 0.0, 0.0, -2.0 * float(l1) - 1.0, 0.0)
        add("eta0 in", 0.0, 0.0, 0.5 * float(l1), 0.0)
        add("eta0 w", 0.5, 0.0, 2.0 * float(l1) + 1.0, 0.0)
    return entries, np.array(counts, np.float32), np.array(grads, np.float32), names


# ---------------------------------------------------------------- the cases both test files run
CLIP_DIMS = (0, 1, 5, 16, 33, 200)
# the planted model's one training step: V_threshold = 0 with no counts pushed draws no V
CLIP_CFG = dict(V_threshold=0, l1=0.5, lr=.05, V_lr=.01)
# (l1, lr, lr_beta) of ftrl_edges: a dyadic and a non-dyadic band, and eta = 0
FTRL_CASES = ((1.0, .05, 1.0), (0.3, .1, 1.0), (1.0, .05, 0.0))
FTRL_VDIM, FTRL_VTHR = 4, 2
