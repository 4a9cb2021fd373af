"""tests/line16_ref.Updater with the identity as rounding is oracle.Updater, bit for bit: that pins
the restated UpdateW / UpdateV / InitV, so the half-precision yardstick adds only its rounding."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import backward_ref as R
from tests import line16_ref as L16
from tests.test_gpu_line_slots import LAZY, _batch, _entry_eq

CFG = dict(V_dim=16, V_threshold=0, l1=0, lr=.05, V_lr=.01)


@pytest.mark.parametrize("cfg,binary,flip", [(CFG, True, False), (CFG, False, False),
                                             (dict(LAZY, V_dim=16), True, True)],
                         ids=["binary", "valued", "lazy"])
def test_identity_rounding_is_the_oracle(cfg, binary, flip):
    blk, neg, uniq, _ = _batch(binary)
    up, o = L16.Updater(rounding=L16.identity, **cfg), O.Updater(**cfg)
    for step in range(3):
        b = (blk, neg)[step % 2 if flip else 0]
        pu, po = R.fused_step(up, b, step == 0), R.fused_step(o, b, step == 0)
        assert np.array_equal(pu.view(np.uint32), po.view(np.uint32)), step
        assert all(_entry_eq(up.entry(k), o.entry(k)) for k in uniq), step
        assert (up.seed, up.new_w, up.size()) == (o.seed, int(o.new_w), o.size()), step


def test_rounding_keeps_fp16_values_and_saturates():
    h = np.arange(0x7C00, dtype=np.uint32)          # every finite fp16 >= 0
    x = h.astype(np.uint16).view(np.float16).astype(np.float32)
    assert np.array_equal(L16.f16_widen(h), x)
    assert np.array_equal(L16.round_bits(x, x, x, h % 16), h)       # f = 0: stored as it is
    big = np.array([65504, 65520, 1e9, np.inf], np.float32)
    assert (L16.round_bits(big, big, big, 0) == 0x7BFF).all()
    # between two neighbours: one of them, and both over a few operands (2^-20: subnormal)
    for lo in (np.float32(2.0 ** -20), np.float32(1.0)):
        hi = np.nextafter(np.float16(lo), np.float16(2)).astype(np.float32)
        got = L16.round_f16(np.full(64, (lo + hi) / 2, np.float32), np.arange(64), 1, 0)
        assert set(got.tolist()) == {float(lo), float(hi)}
