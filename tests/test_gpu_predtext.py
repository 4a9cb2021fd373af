"""dfx_format_pred and the two-slot dfx_predtext (csrc/predtext.hip, csrc/fmtg.h) against the
driver's own fprintf("%g\\t%g\\n", label, pred_prob ? 1.0 / (1.0 + std::exp(-pred)) : pred),
which build/fmtg_check rows runs on the host (numpy's exp is not glibc's expf, so nothing here
computes a probability): the text byte for byte, the printed doubles bit for bit.

One reference of 262 401 rows is made once; every size is a prefix of it (or a range, for the
two-slot test).  Sizes: the issue's 0, 1, 63, 64, 65, 255, 256, 257, 4097, 70 001, the tile of
256 rows again at 511 / 512 / 513, and both sides of the one-block scan's round of 1024 tiles
(262 143, 262 144, 262 145, and 262 401 = one tile and a row past it).

With labels from {0, 1, -1, 0.5, 3} the longest row is 17 bytes ("0.5\\t-1.23457e-05\\n"), so the
issue's "rows of 20 and more" cannot occur with them; test_long_rows adds labels from the edge
list as well, where rows reach the format's 26 bytes beside rows of 4."""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

CHECK = os.path.join(ROOT, "build", "fmtg_check")
N_REF = 262401
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4097, 70001, 262143, 262144, 262145,
         N_REF]


def _edge_floats(tmp):
    p = str(tmp / "edges.f32")
    subprocess.run([CHECK, "edgelist", p], check=True, timeout=60)
    return np.fromfile(p, np.float32)


def _host_rows(tmp, name, label, pred):
    """-> {prob: (text bytes, line starts [n + 1], float64 values)} by the host"""
    pairs = np.stack([label, pred], axis=1).astype(np.float32)
    src, out = str(tmp / (name + ".in")), str(tmp / name)
    pairs.tofile(src)
    subprocess.run([CHECK, "rows", src, out], check=True, timeout=300)
    ref = {}
    for prob in (0, 1):
        text = open("%s.p%d" % (out, prob), "rb").read()
        nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
        assert len(nl) == len(label)
        starts = np.concatenate([[0], nl + 1])
        ref[prob] = (text, starts, np.fromfile("%s.v%d" % (out, prob), np.float64))
    return ref


def _in_domain(x):
    a = np.abs(x.astype(np.float64))
    return np.isfinite(a) & ((a == 0) | ((a >= 1e-12) & (a < 1e12)))


@pytest.fixture(scope="module")
def ctx():
    from difacto_amd import hotpath as H
    c = H.Context(0, V_dim=0, max_keys=1 << 10)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    """(label, pred, {prob: (text, starts, values)}): every row inside the guaranteed domain
    under both pred_prob settings"""
    tmp = tmp_path_factory.mktemp("predtext")
    rng = np.random.RandomState(11)
    edges = _edge_floats(tmp)
    # raw predictions must be in the domain, and so must their probabilities: 1 / (1 + e^27.6)
    # is 1e-12, so nothing below -27
    edges = edges[_in_domain(edges) & (edges >= -27)]
    edges = np.concatenate([edges, -edges[(edges > 0) & (edges <= 27)], [1e6, 20, -20]])
    pred = rng.randn(N_REF).astype(np.float32) * rng.choice([1e-3, 1, 4], N_REF).astype(np.float32)
    pick = rng.rand(N_REF)
    pred[pick < .25] = rng.choice(edges, int((pick < .25).sum())).astype(np.float32)
    pred[(pick >= .25) & (pick < .45)] = 0  # "0\t0\n": rows of 4 bytes under pred_prob=0
    label = rng.choice(np.float32([0, 1, -1, .5, 3]), N_REF)
    label[(pick >= .25) & (pick < .45)] = rng.choice(np.float32([0, 1, 3]),
                                                     int(((pick >= .25) & (pick < .45)).sum()))
    r = _host_rows(tmp, "ref", label, pred)
    lens = np.diff(r[0][1])
    assert lens.min() == 4 and 15 <= lens.max() <= 17, (lens.min(), lens.max())
    return label, pred, r


@pytest.mark.parametrize("prob", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_text_and_values_equal_the_hosts(ctx, ref, n, prob):
    from difacto_amd import hotpath as H
    label, pred, r = ref
    text, starts, values = r[prob]
    got, flagged, vals = H.format_pred(ctx, label[:n], pred[:n], pred_prob=bool(prob), values=True)
    assert flagged == 0
    want = text[:starts[n]]
    assert len(got) == len(want)
    assert got == want
    assert np.array_equal(vals.view(np.int64), values[:n].view(np.int64))


@pytest.mark.parametrize("prob", [0, 1])
def test_long_rows(ctx, tmp_path, prob):
    """labels from the edge list too: rows from 4 to 26 bytes side by side, 5000 of them at
    every phase of the 16-byte pieces"""
    from difacto_amd import hotpath as H
    rng = np.random.RandomState(5)
    edges = _edge_floats(tmp_path)
    edges = edges[_in_domain(edges) & (edges >= -27)]
    edges = np.concatenate([edges, -edges[(edges > 0) & (edges <= 27)], np.float32([-1.2345678e-5])])
    n = 5000
    label = rng.choice(np.concatenate([edges, np.zeros(len(edges), np.float32)]), n)
    pred = rng.choice(np.concatenate([edges, np.zeros(len(edges), np.float32)]), n)
    for i in range(0, n, 250):  # "-1.23457e-05\t-1.23457e-05\n" beside "0\t0\n"
        label[i] = pred[i] = -1.2345678e-5
        label[i + 1] = pred[i + 1] = 0
    text, starts, values = _host_rows(tmp_path, "long", label, pred)[prob]
    lens = np.diff(starts)
    # (under pred_prob the 4-byte rows are "0\t1\n", the probability of 1e6, and the longest
    # value is a small probability such as 2.06115e-09)
    assert lens.min() == 4 and (lens.max() == 26 if prob == 0 else lens.max() >= 20), (
        lens.min(), lens.max())
    got, flagged, vals = H.format_pred(ctx, label, pred, pred_prob=bool(prob), values=True)
    assert flagged == 0 and got == text
    assert np.array_equal(vals.view(np.int64), values.view(np.int64))


@pytest.mark.parametrize("shift", [0, 3])
def test_capacity_one_byte_short(ctx, ref, shift):
    """cap_bytes one below the text's size, guard bytes behind (and, shift=3, a text buffer off
    the 16-byte grid): the status says so, the text is cut at the capacity, the guard is whole"""
    from difacto_amd import hotpath as H
    label, pred, r = ref
    n = 4097
    text, starts, _ = r[1]
    need = int(starts[n])
    cap = need - 1
    buf = torch.full((shift + cap + 64,), 0xA5, dtype=torch.uint8, device=ctx.device)
    lt, pt = ctx.tensor(label[:n], torch.float32), ctx.tensor(pred[:n], torch.float32)
    stat = H.format_pred_raw(ctx, lt, pt, True, buf[shift:], cap)
    assert stat == [cap, 0, -1, need]
    host = buf.cpu().numpy()
    assert host[shift:shift + cap].tobytes() == text[:cap]
    assert np.all(host[:shift] == 0xA5) and np.all(host[shift + cap:] == 0xA5)
    # and with room: the whole text, the guard still whole
    buf.fill_(0xA5)
    stat = H.format_pred_raw(ctx, lt, pt, True, buf[shift:], need)
    assert stat == [need, 0, -1, need]
    host = buf.cpu().numpy()
    assert host[shift:shift + need].tobytes() == text[:need]
    assert np.all(host[shift + need:] == 0xA5)


def test_flagged_rows(ctx, tmp_path):
    """a NaN, an infinity and 1e-30 as raw predictions: counted, the first one reported, every
    other row's text in place"""
    from difacto_amd import hotpath as H
    rng = np.random.RandomState(3)
    n = 1000
    label = rng.choice(np.float32([0, 1, -1, .5, 3]), n)
    pred = rng.randn(n).astype(np.float32)
    bad = {700: np.nan, 300: np.inf, 500: 1e-30}
    for i, v in bad.items():
        pred[i] = v
    text, starts, _ = _host_rows(tmp_path, "flag", label, pred)[0]
    want = b"".join(text[starts[i]:starts[i + 1]] for i in range(n) if i not in bad)
    lt, pt = ctx.tensor(label, torch.float32), ctx.tensor(pred, torch.float32)
    buf = torch.zeros(H.PRED_ROW_BYTES * n, dtype=torch.uint8, device=ctx.device)
    stat = H.format_pred_raw(ctx, lt, pt, False, buf, buf.numel())
    assert stat == [len(want), 3, 300, len(want)]
    assert buf[:len(want)].cpu().numpy().tobytes() == want
    got, flagged = H.format_pred(ctx, label, pred, pred_prob=False)
    assert flagged == 3 and got == want
    # as probabilities 1e-30 is 0.5 and the infinity is 1: one row is left to the host
    got, flagged = H.format_pred(ctx, label, pred, pred_prob=True)
    assert flagged == 1


def test_rejected_arguments(ctx):
    from difacto_amd import _lib
    from difacto_amd import hotpath as H
    one = torch.zeros(4, dtype=torch.float32, device=ctx.device)
    buf = torch.zeros(128, dtype=torch.uint8, device=ctx.device)
    with pytest.raises(_lib.DfxError):
        H.format_pred_raw(ctx, one, one, True, buf, -1)
    stat = torch.zeros(4, dtype=torch.int64, device=ctx.device)
    L = _lib.lib()
    assert L.dfx_format_pred(ctx.h, H._p(one), H._p(one), -1, 1, H._p(buf), 128, H._p(stat),
                             None) == 1
    assert L.dfx_format_pred(ctx.h, None, H._p(one), 4, 1, H._p(buf), 128, H._p(stat), None) == 1
    assert L.dfx_format_pred(ctx.h, H._p(one), H._p(one), 4, 1, H._p(buf), 128, None, None) == 1


def test_two_slots(ctx, ref):
    """five batches of different sizes through the two slots, submitted ahead as the driver's
    writer does: every take returns its own batch's text, labels and predictions"""
    from difacto_amd import _lib
    from difacto_amd import hotpath as H
    label, pred, r = ref
    text, starts, _ = r[1]
    sizes = [1000, 37, 5000, 256, 70001]
    at = np.concatenate([[0], np.cumsum(sizes)])
    lt, pt = ctx.tensor(label[:at[-1]], torch.float32), ctx.tensor(pred[:at[-1]], torch.float32)
    pw = H.PredText(ctx, rows_hint=100)
    taken = []

    def submit(k):
        pw.submit(k % 2, lt[at[k]:at[k + 1]], pt[at[k]:at[k + 1]], True)

    def take(k):
        o = pw.take(k % 2)
        assert o["rows"] == sizes[k] and o["flagged"] == 0 and o["first_flagged"] == -1
        assert o["text"] == text[starts[at[k]]:starts[at[k + 1]]], k
        assert np.array_equal(o["label"], label[at[k]:at[k + 1]])
        assert np.array_equal(o["pred"], pred[at[k]:at[k + 1]])
        taken.append(k)

    submit(0)
    with pytest.raises(_lib.DfxError):
        submit(0)  # the slot is pending
    with pytest.raises(_lib.DfxError):
        pw.take(1)  # nothing was submitted to it
    for k in range(1, 5):
        submit(k)
        take(k - 1)
    take(4)
    assert taken == [0, 1, 2, 3, 4]
    pw.close()
