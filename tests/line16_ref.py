"""Plain numpy float32 restatement of SGDUpdater (sgd_updater.cc:60-152) with a narrowed Vaux: the
yardstick of slot_layout=line vaux=f16 (run on the CPU; test infrastructure).

Updater below has oracle.Updater's interface, so tests/backward_ref.fused_step drives it through
one IterateData step (O.localize, O.fm_predict, backward_ref.backward for the sums, chunked keys
included).  What is restated here: UpdateW and UpdateV (:105-142), the count push's and the
transition's InitV (:64-75, :118-121, :144-152, rand_r by O.rand_r_seq), and the rounding of
csrc/vaux16.h in integer and float32 numpy operations.  The rounding is an argument: with
`identity` the class must equal oracle.Updater bit for bit (tests/test_line16_ref.py), so only
`round_f16` is new.  eta and the V update use the unrounded accumulator; only the store narrows."""
import numpy as np

from oracle import oracle as O

f32, u32 = np.float32, np.uint32


def identity(nc, g, sg, j):
    return nc


def f16_widen(h):
    """fp16 bit patterns (finite, >= 0) -> float32, exactly"""
    h = np.asarray(h, u32)
    e, m = (h >> u32(10)) & u32(31), h & u32(1023)
    sub = m.astype(f32) * f32(2.0 ** -24)
    nrm = (((e + u32(112)) << u32(23)) | (m << u32(13))).view(f32)
    return np.where(e == 0, sub, nrm).astype(f32)


def f16_floor(x):
    """0 <= x < 65504 -> (lo: the largest fp16 <= x, as bits; fr = 8192 (x - lo) / (hi - lo))"""
    x = np.asarray(x, f32)
    b = x.view(u32)
    e = (b >> u32(23)).astype(np.int64)
    nrm = e >= 113
    lo_n = ((np.maximum(e - 112, 0) << 10) | ((b >> u32(13)) & u32(1023))).astype(u32)
    fr_n = (b & u32(0x1FFF)).astype(f32)
    t = np.where(nrm, f32(0), x) * f32(16777216)          # x 2^24 < 1024 below 2^-14
    lo_s = t.astype(u32)
    fr_s = (t - lo_s.astype(f32)) * f32(8192)
    return np.where(nrm, lo_n, lo_s).astype(u32), np.where(nrm, fr_n, fr_s).astype(f32)


def _rotl(x, r):
    return (x << u32(r)) | (x >> u32(32 - r))


def _k(x):
    return _rotl(x * u32(0xCC9E2D51), 15) * u32(0x1B873593)


def round_bits(nc, g, sg, j):
    """vaux16_round (csrc/vaux16.h) -> the stored fp16 bit patterns"""
    nc, g = np.atleast_1d(np.asarray(nc, f32)), np.atleast_1d(np.asarray(g, f32))
    sg = np.broadcast_to(np.asarray(sg, f32), nc.shape).copy()
    j = np.broadcast_to(np.asarray(j, np.int64), nc.shape).astype(u32)
    sat = ~(nc < f32(65504))
    lo, fr = f16_floor(np.where(sat, f32(0), nc))
    h = _k(nc.view(u32))
    for w in (g.view(u32), sg.view(u32), j):
        h = _rotl(h ^ _k(w), 13) * u32(5) + u32(0xE6546B64)
    h ^= h >> u32(16)
    h *= u32(0x85EBCA6B)
    h ^= h >> u32(13)
    h *= u32(0xC2B2AE35)
    h ^= h >> u32(16)
    up = fr > (h >> u32(19)).astype(f32)
    return np.where(sat, u32(0x7BFF), lo + up.astype(u32)).astype(u32)


def round_f16(nc, g, sg, j):
    return f16_widen(round_bits(nc, g, sg, j))


def nearest_f16(x):
    """what a model file's fp32 Vaux becomes in a line16 slot: nearest, ties to even, saturating"""
    return np.minimum(np.asarray(x, f32), f32(65504)).astype(np.float16).astype(f32)


class Updater:
    kFeaCount, kWeight, kGradient = 1, 2, 3

    def __init__(self, rounding=round_f16, **kw):
        p = dict(l1=1, l2=0, V_l2=.01, lr=.01, lr_beta=1, V_lr=.01, V_lr_beta=1, V_init_scale=.01,
                 V_threshold=10, V_dim=0, l1_shrk=1, seed=0)
        assert set(kw) <= set(p), kw
        p.update(kw)
        self.rounding = rounding
        self.V_dim, self.V_threshold = int(p["V_dim"]), int(p["V_threshold"])
        self.l1_shrk, self.seed, self.new_w = bool(int(p["l1_shrk"])), int(p["seed"]), 0
        for k in ("l1", "l2", "V_l2", "lr", "lr_beta", "V_lr", "V_lr_beta", "V_init_scale"):
            setattr(self, k, f32(p[k]))
        self.model = {}     # key -> [state f32[4] = w, sqrt_g, z, fea_cnt; V f32[2 d] or None]
        self.rounded = [0, 0, 0, 0]     # Vaux coordinates stored: above nc, below nc, < 2^-14, 65504

    def size(self):
        return len(self.model)

    def _e(self, key):
        return self.model.setdefault(int(key), [np.zeros(4, f32), None])

    def entry(self, key):
        e = self.model.get(int(key))
        return None if e is None else (e[0].copy(), None if e[1] is None else e[1].copy())

    def _live(self, e):
        return e[1] is not None and not (self.l1_shrk and e[0][0] == 0)

    def get(self, keys):
        vals, lens = [], []
        for k in keys:
            e = self._e(k)
            vals.append(e[0][:1])
            if self._live(e):
                vals.append(e[1][:self.V_dim])
            lens.append(1 + self.V_dim if self._live(e) else 1)
        return (np.concatenate(vals).astype(f32) if vals else np.zeros(0, f32),
                np.array(lens, np.int32) if self.V_dim > 0 else None)

    def _init_v(self, e):
        d = self.V_dim
        r, self.seed = O.rand_r_seq(self.seed, d)
        q = np.array(r, np.int64).astype(f32) / f32(2147483648)
        V = ((q.astype(np.float64) - 0.5) * np.float64(self.V_init_scale)).astype(f32)
        e[1] = np.concatenate([V, np.zeros(d, f32)])

    def _update_w(self, gw, e):
        s = e[0]
        sg, w = s[1], s[0]
        gw = f32(gw) + w * self.l2
        s[1] = np.sqrt(sg * sg + gw * gw)
        s[2] = s[2] - (gw - (s[1] - sg) / self.lr * w)
        z, l1 = s[2], self.l1
        if -l1 <= z <= l1:
            s[0] = 0
        else:
            s[0] = (z - l1 if z > 0 else z + l1) / ((self.lr_beta + s[1]) / self.lr)
        if w == 0 and s[0] != 0:
            self.new_w += 1
            if self.V_dim > 0 and e[1] is None and s[3] > f32(self.V_threshold):
                self._init_v(e)
        elif w != 0 and s[0] == 0:
            self.new_w -= 1

    def _update_v(self, gV, e):
        d = self.V_dim
        V, c = e[1][:d], e[1][d:]
        with np.errstate(over="ignore", invalid="ignore"):
            g = np.asarray(gV, f32) + self.V_l2 * V
            nc = np.sqrt(c * c + g * g)
            V -= (self.V_lr / (nc + self.V_lr_beta)) * g
        c[:] = self.rounding(nc, g, e[0][1], np.arange(d))
        with np.errstate(invalid="ignore"):
            self.rounded[0] += int((c > nc).sum())
            self.rounded[1] += int((c < nc).sum())
        self.rounded[2] += int(((c > 0) & (c < f32(2.0 ** -14))).sum())
        self.rounded[3] += int((c == f32(65504)).sum())

    def update(self, keys, typ, vals, lens=None):
        vals = np.asarray(vals, f32)
        if typ == self.kFeaCount:
            for k, v in zip(keys, vals):
                e = self._e(k)
                e[0][3] += v
                if (self.V_dim > 0 and e[1] is None and e[0][0] != 0
                        and e[0][3] > f32(self.V_threshold)):
                    self._init_v(e)
            return
        assert typ == self.kGradient
        p = 0
        for i, k in enumerate(keys):
            e = self._e(k)
            self._update_w(vals[p], e)
            p += 1
            if lens is not None and lens[i] > 1:
                assert lens[i] == self.V_dim + 1 and e[1] is not None
                self._update_v(vals[p:p + self.V_dim], e)
                p += self.V_dim
        assert p == len(vals)
