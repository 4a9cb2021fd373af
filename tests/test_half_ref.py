"""tests/half_ref.Updater with the identity as rounding and storage is oracle.Updater, bit for bit:
that pins the restated update, so the vrows=f16 yardstick adds only its narrowing; and the signed
round is unbiased over its hash."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import backward_ref as R
from tests import half_ref as HR
from tests.test_gpu_half import batch, cfg
from tests.test_gpu_line_slots import _entry_eq


@pytest.mark.parametrize("binary", [True, False], ids=["binary", "valued"])
def test_identity_is_the_oracle(binary):
    blk, _, uniq = batch(binary)
    up, o = HR.Updater(rounding=HR.identity, storage=HR.keep, **cfg(32)), O.Updater(**cfg(32))
    for step in range(3):
        pu, po = R.fused_step(up, blk, True), R.fused_step(o, blk, True)
        assert np.array_equal(pu.view(np.uint32), po.view(np.uint32)), step
        assert all(_entry_eq(up.entry(k), o.entry(k)) for k in uniq), step
        assert (up.seed, up.new_w, up.size()) == (o.seed, int(o.new_w), o.size()), step
    assert up.initv_in_step > 0


def test_signed_round_keeps_fp16_values_and_is_unbiased():
    h = np.arange(0x7C00, dtype=np.uint32)
    h = np.concatenate([h, h | 0x8000])             # every finite fp16, both signs
    x = h.astype(np.uint16).view(np.float16).astype(np.float32)
    assert np.array_equal(HR.widen(h).view(np.uint32), x.view(np.uint32))
    assert np.array_equal(HR.round_v_bits(x, x, x, h % 64), h)      # stored unchanged
    big = np.array([-65504, -65520, -1e9, -np.inf, 7e4], np.float32)
    assert HR.round_v_bits(big, big, big, 0).tolist() == [0xFBFF] * 4 + [0x7BFF]
    # one coordinate, N distinct gradients: nv = -(1.5 + 2458 / 8192 ulp) rounds away from zero with
    # probability f = 2458 / 8192 exactly (r is uniform on 13 bits), so the mean of the stored values
    # sits within 4 binomial standard errors of nv: (hi - lo) sqrt(f (1 - f) / N)
    N, f = 20000, 2458 / 8192
    lo, hi = np.float32(-1.5), np.float32(-1.5 - 2.0 ** -10)
    nv = (np.float32(1.5).view(np.uint32) + np.uint32(2458) | np.uint32(0x80000000)).view(np.float32)
    g = (np.arange(N) + 1).astype(np.float32) * np.float32(1e-3)
    got = HR.widen(HR.round_v_bits(np.full(N, nv), g, np.float32(.7), 5)).astype(np.float64)
    assert set(got.tolist()) == {float(lo), float(hi)}
    assert abs(float(nv) - (float(lo) + f * (float(hi) - float(lo)))) < 1e-12
    se = abs(float(hi) - float(lo)) * np.sqrt(f * (1 - f) / N)
    assert abs(got.mean() - float(nv)) <= 4 * se, (got.mean(), float(nv), se)
