"""tests/edge_ref.py's builders hit what they claim: shown from oracle.oracle and numpy alone, on
the CPU.  tests/test_gpu_loss_edges.py then holds the device to the oracle on the same inputs."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_ref as E

F = np.float32
FLT_MIN = np.finfo(np.float32).tiny


# ---------------------------------------------------------------- p_sweep
@pytest.fixture(scope="module")
def sweep():
    blk, pred, labels, rw = E.p_sweep()
    B = blk.size
    uniq, _, col = O.localize(blk.offs, blk.ids)
    assert len(uniq) == B and np.array_equal(col, np.arange(B, dtype=np.uint32))
    p = O.fm_calcgrad(blk.offs, col, None, labels, None, np.zeros(B, np.float32), None, None, B, 0,
                      pred)
    return blk, pred, labels, rw, p


def test_p_sweep_inputs(sweep):
    blk, pred, labels, rw, _ = sweep
    assert blk.size == E.SWEEP_ROWS == 1 << 18 and blk.nnz == blk.size
    assert np.array_equal(labels[:4], F([1, -1, 1, -1])) and set(labels) == {1.0, -1.0}
    have = set(E.bits(pred).tolist())
    inf = F(np.inf)
    for e in range(255):                        # every exponent, 16 mantissas, both signs
        for sign in (0, 1 << 31):
            assert sum(((b >> 23) & 0xFF) == e and (b >> 31) == (sign >> 31) for b in
                       (sign | (e << 23) | m for m in (0, 1, 0x7FFFFF, 0x555555))
                       if b in have) == 4
    for x in (E.OVER, -E.UNDER, F(88.0), -E.SUBN, E.ONE_PLUS, F(20.0)):
        for s in (F(1), F(-1)):
            c = E.bits1(s * x)
            assert all(c + k in have for k in range(-64, 65)), x
    assert all(k in have and (k | 1 << 31) in have for k in range(65))        # around +-0
    for b in (1, 0x007FFFFF, 0x7F7FFFFF, 0x7F800000):
        assert b in have and (b | 1 << 31) in have
    assert all(b in have for b in E.NAN_BITS)
    assert int(np.isnan(pred).sum()) == sum(int((E.bits(pred) == b).sum()) for b in E.NAN_BITS) > 0
    # every value meets both labels
    for x in (E.OVER, np.nextafter(E.OVER, inf), E.UNDER, np.nextafter(E.UNDER, -inf), F(20)):
        assert set(labels[pred == x]) == {1.0, -1.0}


def test_p_sweep_reaches_every_branch_of_p(sweep):
    """on the oracle's CalcGrad (glibc's expf): subnormal results of expf, subnormal quotients,
    p == -0.0 (a row TransTimes skips: the gradient stays +0.0), p == -+1, NaN on the NaN inputs
    alone; and both sides of the overflow and the underflow cut give different p"""
    _, pred, labels, _, p = sweep
    nan = np.isnan(pred)
    t = labels.astype(np.float64) * np.where(nan, 0, pred).astype(np.float64)
    assert np.array_equal(np.isnan(p), nan)
    ap = np.abs(p)
    assert ((ap > 0) & (ap < FLT_MIN)).any()                 # a subnormal quotient p
    assert ((t > 87.4) & (t <= float(E.OVER)) & (ap > 0) & (ap < FLT_MIN)).any()
    # y = +1 past the overflow cut: expf = inf, p = -1 / inf = -0.0; the row is skipped
    neg0 = (labels > 0) & (t > float(E.OVER)) & ~nan
    assert neg0.any() and not E.bits(p[neg0]).any()
    assert ((labels > 0) & (t == float(E.OVER)) & (p < 0)).any()     # at the cut: still finite
    # expf subnormal (t < -87.34) or zero (t < UNDER): 1 + e == 1, p == -y exactly
    for lo, hi in ((-np.inf, float(E.UNDER)), (float(E.UNDER), float(E.SUBN))):
        m = (t > lo) & (t < hi)
        assert (p[m & (labels > 0)] == -1).all() and (p[m & (labels < 0)] == 1).all()
        assert (m & (labels > 0)).any() and (m & (labels < 0)).any()
    assert (p == 1).any() and (p == -1).any()
    # around 16.635532 both 1 + e == 1 and 1 + e > 1 occur
    m = np.abs(t + float(E.ONE_PLUS)) < 1e-4
    assert (np.abs(p[m]) == 1).any() and (np.abs(p[m]) < 1).any()
    assert E.bits(p[pred == 0])[0] == E.bits1(-0.5)


# ---------------------------------------------------------------- clip_case
def _f64_pred(blk, entries, d):
    """the unclipped prediction of every row in float64 numpy, from the planted floats"""
    model = {k: (float(w), None if V is None else V.astype(np.float64))
             for k, w, _, _, V, _ in entries}
    keys = E.reverse_bytes(blk.ids)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(blk.size):
            lin, xv, xxvv = 0.0, np.zeros(d), np.zeros(d)
            for j in range(int(blk.offs[r]), int(blk.offs[r + 1])):
                w, V = model[int(keys[j])]
                x = 1.0 if blk.vals is None else float(blk.vals[j])
                lin += w * x
                if V is not None:
                    xv += V * x
                    xxvv += V * V * x * x
            out.append(lin + .5 * float((xv * xv - xxvv).sum()))
    return np.array(out)


def _oracle_pred(tmp_path, blk, entries, d, train_rows=None):
    path = str(tmp_path / "model")
    E.write_model(path, d, entries)
    up = O.Updater(V_dim=d, **E.CLIP_CFG)
    up.load(path)
    assert up.size() == len(entries)
    _, _, pred = up.train_step(blk.offs, blk.ids, blk.vals, blk.labels, train=False,
                               want_pred=True)
    if train_rows is not None:
        tb = E.take_rows(blk, train_rows)
        up.train_step(tb.offs, tb.ids, tb.vals, tb.labels)
    return pred, up


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("d", E.CLIP_DIMS)
def test_clip_case_hits(tmp_path, d, binary):
    blk, entries, tg = E.clip_case(d, binary)
    want, rows = tg["want"], tg["rows"]
    assert blk.size <= 512 and set(np.diff(blk.offs.astype(np.int64))) <= {1, 2, 3}
    assert (blk.vals is None) == binary
    keys = E.reverse_bytes(blk.ids)
    assert len(set(keys.tolist())) == blk.nnz == len(entries)        # private keys
    assert all(len(rows[c]) > 0 for c in E.CLASSES)
    fin = np.isfinite(want)
    # the planted values are what the builder says, exactly: float64 from the planted floats
    f64 = _f64_pred(blk, entries, d)
    assert np.array_equal(f64[fin], want[fin])
    assert np.array_equal(f64[fin].astype(np.float32).astype(np.float64), want[fin])
    w32 = want.astype(np.float32)
    for k in range(1, 5):
        for s in (1, -1):
            assert F(s * (20 + k * E.ULP20)) in w32 and F(s * (20 - k * E.ULP20)) in w32
    inf = F(np.inf)
    for v in (np.nextafter(F(20), inf), np.nextafter(F(20), F(0)), F(20), F(1e4), E.FLT_MAX, inf):
        assert v in w32 and -v in w32
    for c in ("below", "at", "above", "far", "fltmax", "inf"):      # both signs, both labels
        assert {(np.sign(want[r]), blk.labels[r]) for r in rows[c]} == \
            {(1, 1), (1, -1), (-1, 1), (-1, -1)}, c
    # the oracle clips exactly the rows above 20 in magnitude, and only at V_dim > 0
    opred, up = _oracle_pred(tmp_path, blk, entries, d, tg["train"])
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(opred), nan) and np.array_equal(np.flatnonzero(nan), rows["nan"])
    assert np.array_equal(tg["train"], np.flatnonzero(~nan))
    clipped = ~nan & (E.bits(opred) != E.bits(w32))
    if d > 0:
        assert np.array_equal(clipped, ~nan & (np.abs(want) > 20))
        assert (np.abs(opred[clipped]) == 20).all()
        assert (np.abs(opred[rows["at"]]) == 20).all()
        assert (np.abs(opred[rows["below"]]) < 20).all()
    else:
        assert not clipped.any()
        assert F(1e4) in opred and -E.FLT_MAX in opred and inf in opred
        t = blk.labels * opred
        assert (t[~nan] > E.OVER).any() and ((t[~nan] > 0) & (t[~nan] <= E.OVER)).any()
        assert (t[~nan] < E.UNDER).any()
    # the training step on the rows outside the NaN group leaves no NaN in the model (the GPU
    # test compares its entries bit for bit)
    for k, *_ in entries:
        st, V = up.entry(k)
        assert not np.isnan(st).any() and (V is None or not np.isnan(V).any())


@pytest.mark.parametrize("d", [5, 16])
def test_clip_case_any_summation_order(d):
    """every partial sum is exact: float32 sums in nnz order and in reverse give the same bits"""
    blk, entries, tg = E.clip_case(d, False)
    model = {k: (w, V) for k, w, _, _, V, _ in entries}
    keys = E.reverse_bytes(blk.ids)
    for r in tg["train"]:
        js = list(range(int(blk.offs[r]), int(blk.offs[r + 1])))
        res = []
        for order in (js, js[::-1]):
            lin, xv, xxvv = F(0), np.zeros(d, F), np.zeros(d, F)
            with np.errstate(over="ignore"):
                for j in order:
                    w, V = model[int(keys[j])]
                    lin = F(lin + F(w * blk.vals[j]))
                    if V is not None:
                        xv = xv + V * blk.vals[j]
                        xxvv = xxvv + (V * V) * F(blk.vals[j] * blk.vals[j])
            res.append(np.concatenate([[lin], xv, xxvv]).astype(F))
        assert np.array_equal(E.bits(res[0]), E.bits(res[1])), r
        # and each is the exact value: float64 agrees
        assert np.isinf(res[0][0]) or float(res[0][0]) + float(res[0][1]) ** 2 / 2 - \
            float(res[0][1 + d]) / 2 == tg["want"][r]


# ---------------------------------------------------------------- ftrl_edges
@pytest.mark.parametrize("l1_shrk", [0, 1])
@pytest.mark.parametrize("l1,lr,lr_beta", E.FTRL_CASES)
def test_ftrl_edges_hits(tmp_path, l1, lr, lr_beta, l1_shrk):
    d, thr = E.FTRL_VDIM, E.FTRL_VTHR
    entries, counts, grads, names = E.ftrl_edges(l1, lr, lr_beta, thr)
    keys = np.array([e[0] for e in entries], np.uint64)
    assert (np.diff(keys.astype(np.float64)) > 0).all()
    path = str(tmp_path / "m")
    E.write_model(path, d, entries)
    up = O.Updater(V_dim=d, V_threshold=thr, l1=l1, lr=lr, lr_beta=lr_beta, l1_shrk=l1_shrk,
                   V_lr=.01, seed=3)
    up.load(path)
    up.update(keys, O.Updater.kFeaCount, counts)
    by = dict(zip(names, keys))
    assert up.entry(by["cnt past"])[1] is not None and up.entry(by["cnt at"])[1] is None
    _, lens = up.get(keys)
    g = []
    for gw, n in zip(grads, lens):
        g += [gw] + [F(0.25)] * (n - 1)
    seed0, nw0 = up.seed, up.new_w
    up.update(keys, O.Updater.kGradient, np.array(g, F), lens)
    L1 = F(l1)
    inf = F(np.inf)
    want_z = {"zero": F(0), "at+l1": L1, "at-l1": -L1, "out+l1": np.nextafter(L1, inf),
              "out-l1": np.nextafter(-L1, -inf), "in+l1": np.nextafter(L1, -inf),
              "in-l1": np.nextafter(-L1, inf)}
    dnw = 0
    for cnt in (thr, thr + 1):
        for name, z in want_z.items():
            st, V = up.entry(by["%s/cnt%d" % (name, cnt)])
            assert E.bits1(st[2]) == E.bits1(z), (name, st, z)
            out = name.startswith("out")
            assert (st[0] != 0) == out, (name, st)      # inclusive band: +-l1 itself gives w = 0
            assert (V is not None) == (out and cnt == thr + 1), (name, cnt)
            dnw += out
    assert up.entry(by["w->0"])[0][0] == 0 and up.entry(by["w->0 neg"])[0][0] == 0
    assert up.entry(by["w,g=0"])[0][0] > 0 and up.entry(by["w=0,g=0"])[0][0] == 0
    assert up.entry(by["w=0,g=0,out"])[0][0] < 0
    dnw += -2 + 1
    if lr_beta == 0:
        assert up.entry(by["eta0 +"])[0][0] == inf and up.entry(by["eta0 -"])[0][0] == -inf
        assert up.entry(by["eta0 in"])[0][0] == 0 and up.entry(by["eta0 w"])[0][0] == inf
        dnw += 2
    assert up.new_w - nw0 == dnw
    for k in keys:                                     # bit-comparable on any machine
        st, V = up.entry(k)
        assert not np.isnan(st).any() and (V is None or not np.isnan(V).any())
    assert up.seed != seed0                            # the two keys past the threshold drew V
