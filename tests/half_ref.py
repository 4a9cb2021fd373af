"""Plain numpy float32 restatement of SGDUpdater with half-precision V rows: the yardstick of
vrows=f16 (V_dim 32 / 64; run on the CPU; test infrastructure).

tests/line16_ref.Updater restated UpdateW, UpdateV and InitV with a narrowed Vaux; here V narrows
too.  Updater below keeps its interface (oracle.Updater's), so tests/backward_ref.fused_step drives
it, and its forward is the oracle's on the widened values it holds.  What is new: csrc/vhalf.h's
signed round of the updated V (round_v_bits), and InitV's draw stored as the nearest fp16.  Both
are arguments: with `identity` as rounding and as storage the class must equal oracle.Updater bit
for bit (tests/test_half_ref.py).  eta and the new V come from the widened old values and the
unrounded accumulator; only the two stores narrow."""
import numpy as np

from tests import line16_ref as L16
from tests.line16_ref import f32, u32


def identity(nv, nc, g, sg, j):
    return nv, nc


def keep(x):
    return x


def widen(h):
    """fp16 bit patterns, sign and all -> float32, exactly (finite patterns)"""
    h = np.asarray(h, u32)
    m = L16.f16_widen(h & u32(0x7FFF))
    return (m.view(u32) | ((h & u32(0x8000)) << u32(16))).view(f32)


def round_v_bits(nv, g, sg, j):
    """vhalf_round (csrc/vhalf.h) -> the stored fp16 bit patterns"""
    nv, g = np.atleast_1d(np.asarray(nv, f32)), np.atleast_1d(np.asarray(g, f32))
    sg = np.broadcast_to(np.asarray(sg, f32), nv.shape).copy()
    j = np.broadcast_to(np.asarray(j, np.int64), nv.shape).astype(u32) | u32(0x10000)
    b = nv.view(u32)
    s, ax = (b >> u32(16)) & u32(0x8000), (b & u32(0x7FFFFFFF)).view(f32)
    sat = ~(ax < f32(65504))
    lo, fr = L16.f16_floor(np.where(sat, f32(0), ax))
    h = L16._k(b)
    for w in (g.view(u32), sg.view(u32), j):
        h = L16._rotl(h ^ L16._k(w), 13) * u32(5) + u32(0xE6546B64)
    h ^= h >> u32(16)
    h *= u32(0x85EBCA6B)
    h ^= h >> u32(13)
    h *= u32(0xC2B2AE35)
    h ^= h >> u32(16)
    up = fr > (h >> u32(19)).astype(f32)
    return (s | np.where(sat, u32(0x7BFF), lo + up.astype(u32))).astype(u32)


def round_half(nv, nc, g, sg, j):
    return widen(round_v_bits(nv, g, sg, j)), L16.round_f16(nc, g, sg, j)


def nearest_f16(x):
    """f16_nearest: ties to even, saturating at +-65504 — InitV's store, a model file's load"""
    return np.clip(np.asarray(x, f32), f32(-65504), f32(65504)).astype(np.float16).astype(f32)


class Updater(L16.Updater):
    def __init__(self, rounding=round_half, storage=nearest_f16, **kw):
        super().__init__(rounding=rounding, **kw)
        self.storage = storage
        self.rounded_v = [0, 0]     # V coordinates stored above / below the unrounded value
        self.initv_in_step = 0      # InitV draws made by Update(kGradient)'s transitions
        self._typ = None

    def update(self, keys, typ, vals, lens=None):
        self._typ = typ
        super().update(keys, typ, vals, lens)

    def _init_v(self, e):
        super()._init_v(e)
        self.initv_in_step += self._typ == self.kGradient
        e[1][:self.V_dim] = self.storage(e[1][:self.V_dim])

    def _update_v(self, gV, e):
        d = self.V_dim
        V, c = e[1][:d], e[1][d:]
        with np.errstate(over="ignore", invalid="ignore"):
            g = np.asarray(gV, f32) + self.V_l2 * V
            nc = np.sqrt(c * c + g * g)
            nv = V - (self.V_lr / (nc + self.V_lr_beta)) * g
        V[:], c[:] = self.rounding(nv, nc, g, e[0][1], np.arange(d))
        with np.errstate(invalid="ignore"):
            self.rounded_v[0] += int((V > nv).sum())
            self.rounded_v[1] += int((V < nv).sum())
            self.rounded[0] += int((c > nc).sum())
            self.rounded[1] += int((c < nc).sum())
        self.rounded[2] += int(((c > 0) & (c < f32(2.0 ** -14))).sum())    # (line16_ref's counts)
        self.rounded[3] += int((c == f32(65504)).sum())
