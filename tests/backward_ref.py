"""Plain numpy restatement of FMLoss::CalcGrad (fm_loss.h:148-203) in the DEVICE's documented
summation order (run on the CPU; test infrastructure).  Every float32 term is formed as the
reference forms it (oracle.cc CalcGrad); what is restated is only how a key's terms are summed:

* a key of <= kChunkOcc occurrences: sequentially in float32 in occurrence order, i.e. ascending
  (row, nnz) — the reference's own order (spmv.h:139-171, spmm.h:127-159; csrc/fm.hip k_fm_bwd
  lines 949-977 and 1006-1146, k_fm_bwd_w 1317-, k_fm_bwd_v 1506-);
* a key of more: per chunk of kChunkOcc occurrences a sequential double sum from 0.0 of the
  float32 terms (csrc/fm.hip chunk_one 1547-1634), the chunks combined by their count
  (fewer than kHotChunks: in chunk order, fm.hip 978-1005 / 1306-1316 / 1489-1505; else
  k_chunk_hotgroup's groups of kHotGroup chunks, fm.hip 1658-1679, and hotsum_key's R slices,
  fm.hip 1686-1722), rounded to float once.

Pinned on the CPU by tests/test_backward_ref.py: equal to the oracle bit for bit where no key is
chunked, within the recursive-summation bound of math.fsum where keys are, and its plans by hand.
Bit equality of a device result with this file pins membership (every term counted once) and the
single rounding; it does not pin the order of the double additions, which reaches the rounded
float only in rare cases."""
import ctypes
import ctypes.util

import numpy as np

from oracle import oracle as O

kChunkOcc = 128   # csrc/internal.h:408
kHotChunks = 8    # csrc/internal.h:411 (hot_chunks_read, :412-414)
kHotGroup = 32    # csrc/fm.hip:1657

f32 = np.float32

_libm = None


def expf(x):
    """the host libm's expf (glibc: the yardstick DESIGN.md names; csrc/expf.h restates it), one
    call per element"""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.expf.restype = ctypes.c_float
        _libm.expf.argtypes = [ctypes.c_float]
    x = np.asarray(x, f32)
    return np.array([_libm.expf(float(v)) for v in x.ravel()], f32).reshape(x.shape)


def row_p(labels, pred, rweight=None):
    """p = -y / (1 + expf(y pred)) [* row weight], every operation in float32 (oracle.cc
    CalcGrad :268-272, fm_loss.h:155-165)"""
    y = np.where(np.asarray(labels, f32) > 0, f32(1), f32(-1)).astype(f32)
    e = expf(y * np.asarray(pred, f32))
    with np.errstate(over="ignore"):
        p = (-y) / (f32(1) + e)
    if rweight is not None:
        p = p * np.asarray(rweight, f32)
    return p.astype(f32)


# ---- the float32 terms (shared with tests/exact_sums.py) ---------------------------------
def xv_rows(offs, col, x, W, vp, d):
    """X V per row in float32 in the reference's (row, nnz) order (fm_loss.h:81-83, oracle.cc
    CalcGrad :304-313): keys without V (vp == -1) are skipped"""
    offs = np.asarray(offs, np.int64)
    B = len(offs) - 1
    XV = np.zeros((B, d), f32)
    lens = np.diff(offs)
    ar = np.arange(d)
    for j in range(int(lens.max()) if B else 0):
        rows = np.nonzero(lens > j)[0]
        q = offs[rows] + j
        v = vp[col[q]]
        ok = v >= 0
        r2, q2, v2 = rows[ok], q[ok], v[ok]
        XV[r2] = XV[r2] + W[v2[:, None] + ar] * x[q2][:, None]
    return XV


def w_terms(p, row, x):
    """per nnz the float32 terms of g_w and XXp: p x and p (x x) (oracle.cc CalcGrad :282, :294)"""
    pr = p[row]
    return (pr * x).astype(f32), (pr * (x * x).astype(f32)).astype(f32)


def v_terms(XVp, row, x):
    """per nnz the float32 terms of g_V: (XV p)[row] x (oracle.cc CalcGrad :314, :325)"""
    return (XVp[row] * x[:, None]).astype(f32)


# ---- the plan of a long key ----------------------------------------------------------------
def n_chunks(length):
    """ceil(len / kChunkOcc) chunks when len > kChunkOcc, else none (csrc/localize.hip:273)"""
    return (length + kChunkOcc - 1) // kChunkOcc if length > kChunkOcc else 0


def n_groups(length):
    """group totals of a hot key (>= kHotChunks chunks), else none (fm.hip:1668, :1688)"""
    nc = n_chunks(length)
    return (nc + kHotGroup - 1) // kHotGroup if nc >= kHotChunks else 0


def n_slices(d):
    """R of hotsum_key (fm.hip:1689): 64 / (d + 2) interleaved slices, one when d + 2 > 64"""
    P = d + 2
    return 64 // P if P <= 64 else 1


def combine(parts, d):
    """parts f64[nc, P]: a long key's chunk partials in chunk order -> f64[P], in the device's
    order of double additions"""
    nc, P = parts.shape
    if nc < kHotChunks:                       # fm.hip:988-999: in chunk order
        s = np.zeros(P)
        for c in range(nc):
            s = s + parts[c]
        return s
    groups = []                               # level 1, hotgroup_one (fm.hip:1669-1678)
    for g0 in range(0, nc, kHotGroup):
        s = np.zeros(P)
        for c in range(g0, min(g0 + kHotGroup, nc)):
            s = s + parts[c]
        groups.append(s)
    ng, R = len(groups), n_slices(d)
    if R > 1:                                 # level 2, hotsum_key (fm.hip:1698-1717)
        tot = np.zeros(P)
        for r in range(R):
            s = np.zeros(P)
            for g in range(r, ng, R):
                s = s + groups[g]
            tot = tot + s
        return tot
    s = np.zeros(P)                           # R == 1 (fm.hip:1699-1706, :1720)
    for g in range(ng):
        s = s + groups[g]
    return s


# ---- the backward --------------------------------------------------------------------------
def backward(offs, col, val, label, rweight, W, wp, vp, U, d, pred, debug=False, XVp=None,
             p=None):
    """-> grad f32 in the layout of W (O.fm_calcgrad's arguments and result; grad starts at
    zero).  debug: -> (grad, dict) with the sorted terms and the long keys' double sums before
    their rounding.  XVp f32[B, d], p f32[B]: the rows' XV * p and p as given (the owner-computes
    split's backward reads them from the workers' combined rows, tests/split_ref.py) instead of
    this batch's own forward; pred, label and rweight are then unused."""
    offs = np.asarray(offs, np.int64)
    col = np.asarray(col, np.int64)
    W = np.asarray(W, f32)
    B, nnz = len(offs) - 1, len(col)
    x = np.ones(nnz, f32) if val is None else np.asarray(val, f32)
    wp = np.arange(U, dtype=np.int64) if wp is None else np.asarray(wp, np.int64)
    vp = np.full(U, -1, np.int64) if (vp is None or d == 0) else np.asarray(vp, np.int64)
    p = row_p(label, pred, rweight) if p is None else np.asarray(p, f32)
    row = np.repeat(np.arange(B), np.diff(offs))
    order = np.argsort(col, kind="stable")    # occurrence order: ascending (row, nnz) per key
    cnt = np.bincount(col, minlength=U).astype(np.int64)
    seg = np.concatenate([[0], np.cumsum(cnt)])
    px, pxx = w_terms(p, row, x)
    px, pxx, nz = px[order], pxx[order], (p[row] != 0)[order]
    hasv = vp >= 0
    T = None
    if d > 0:
        with np.errstate(invalid="ignore", over="ignore"):
            if XVp is None:
                XVp = (xv_rows(offs, col, x, W, vp, d) * p[:, None]).astype(f32)
            XVp = np.asarray(XVp, f32)
            T = v_terms(XVp, row[order], x[order])
    ar = np.arange(d)
    Vk = np.zeros((U, d), f32)
    if d > 0:
        Vk[hasv] = W[vp[hasv][:, None] + ar]
    long_ = cnt > kChunkOcc
    gw = np.zeros(U, f32)
    xxp = np.zeros(U, f32)
    gV = np.zeros((U, d), f32)
    g0 = np.zeros((U, d), f32)

    # keys of <= kChunkOcc occurrences: sequential float32 sums; g_w and XXp skip p == 0
    short = np.nonzero(~long_)[0]
    for j in range(int(cnt[short].max()) if len(short) else 0):
        k = short[cnt[short] > j]
        i = seg[k] + j
        gw[k] = np.where(nz[i], gw[k] + px[i], gw[k])
        xxp[k] = np.where(nz[i], xxp[k] + pxx[i], xxp[k])
    if d > 0:
        sv = short[hasv[short]]
        gV[sv] = g0[sv] - Vk[sv] * xxp[sv][:, None]
        for j in range(int(cnt[sv].max()) if len(sv) else 0):
            k = sv[cnt[sv] > j]
            gV[k] = gV[k] + T[seg[k] + j]

    # keys of more: chunks in double, combined by count, rounded once
    dbg = {"long": np.nonzero(long_)[0], "sums": {}}
    lk = dbg["long"]
    if len(lk):
        nck = np.array([n_chunks(int(c)) for c in cnt[lk]], np.int64)
        ckey = np.repeat(np.arange(len(lk)), nck)
        cfirst = np.cumsum(nck) - nck
        cidx = np.arange(len(ckey)) - cfirst[ckey]
        cs0 = seg[lk][ckey] + cidx * kChunkOcc
        clen = np.minimum(cs0 + kChunkOcc, seg[lk + 1][ckey]) - cs0
        cv = hasv[lk][ckey]
        part = np.zeros((len(ckey), d + 2))
        for j in range(kChunkOcc):            # chunk_one: occurrence order, from 0.0
            c = np.nonzero(clen > j)[0]
            i = cs0[c] + j
            part[c, 0] = np.where(nz[i], part[c, 0] + px[i].astype(np.float64), part[c, 0])
            part[c, 1] = np.where(nz[i], part[c, 1] + pxx[i].astype(np.float64), part[c, 1])
            if d > 0:
                c2 = c[cv[c]]
                part[c2, 2:] = part[c2, 2:] + T[cs0[c2] + j].astype(np.float64)
        for n, u in enumerate(lk):
            S = combine(part[cfirst[n]:cfirst[n] + nck[n]], d)
            dbg["sums"][int(u)] = S
            gw[u] = f32(S[0])
            xxp[u] = f32(S[1])
            if hasv[u]:
                base = (g0[u] - Vk[u] * xxp[u]).astype(f32)
                gV[u] = (base.astype(np.float64) + S[2:]).astype(f32)

    out = np.zeros(len(W), f32)
    hw = wp >= 0
    out[wp[hw]] = gw[hw]
    if d > 0:
        out[vp[hasv][:, None] + ar] = gV[hasv]
    if debug:
        dbg.update(seg=seg, cnt=cnt, px=px, pxx=pxx, nz=nz, T=T, hasv=hasv, p=p)
        return out, dbg
    return out


# ---- batches with keys at chosen occurrence counts -----------------------------------------
# every boundary of the summation paths: 8 | 9 (chunk_one's and the walks' trips), 127 | 128 | 129
# (kChunkOcc), 256 | 257 (2 | 3 chunks), 896 | 897 (7 | 8 chunks: kHotChunks), 1024 | 1025, 4096 |
# 4097 (32 | 33 chunks: kHotGroup).  Key order is chunk-table order: two hot keys (897, 1024)
# open the table, 480 two-chunk keys push it past 1024 chunks (k_chunk_hotsum's tile, kHotNT),
# and the hot key of 4097 starts in the second tile.
PLANTED = (897, 1024, 1, 8, 9, 127, 128, 129, 256, 257, 896, 1025, 4096) + \
    tuple(129 + (i % 7) for i in range(480)) + (4097,)


def owner_base(o, owners):
    """the first key of owner o's range of `owners` (floor(key * owners / 2^64) == o, csrc/split.hip
    split_owner): ceil(o 2^64 / owners)"""
    return -(-(int(o) << 64) // int(owners))


def planted_key(i, owners=1):
    """the Localizer key (ReverseBytes of the id) of planted key i: ascending in i; owners > 1:
    in owner (i % owners)'s key range, ascending in i within each owner"""
    return np.uint64(((i + 1) << 24) + owner_base(i % owners, owners))


def planted_batch(rows, per_row, counts, binary, seed, zero_weights=True, owners=1):
    """rows x per_row nnz; planted key i (planted_key(i)) occurs exactly counts[i] times, the
    other slots hold background keys of ~16 occurrences each; slots are shuffled, so a key's
    occurrences spread over the rows and repeat inside rows.  Row weights in (0.5, 1.5] with
    every seventh 0.0 (both sides of p != 0).  owners > 1: planted key i and background key b lie
    in the key ranges of owners i % owners and b % owners (planted_key)."""
    from difacto_amd import data as D
    from tests.localizer_ref import reverse_bytes
    rng = np.random.default_rng(seed)
    n = rows * per_row
    planted = np.repeat(np.arange(len(counts), dtype=np.uint64), counts)
    assert len(planted) <= n
    nbg = max((n - len(planted)) // 16, 1)
    bg = rng.integers(0, nbg, n - len(planted)).astype(np.uint64)
    keys = np.concatenate([(planted + np.uint64(1)) << np.uint64(24),
                           (bg << np.uint64(1)) + np.uint64(1)])   # odd: never a planted key
    if owners > 1:
        base = np.array([owner_base(o, owners) for o in range(owners)], np.uint64)
        who = np.concatenate([planted, bg]) % np.uint64(owners)
        keys = keys + base[who.astype(np.int64)]
    keys = keys[rng.permutation(n)]
    offs = (np.arange(rows + 1) * per_row).astype(np.uint64)
    vals = None if binary else (1.0 - rng.random(n, dtype=np.float32)).astype(f32)
    labels = np.where(rng.random(rows) < 0.3, 1.0, -1.0).astype(f32)
    w = (1.5 - rng.random(rows)).astype(f32)
    if zero_weights:
        w[::7] = 0
    return D.RowBlock(offs, reverse_bytes(keys), vals, labels, w)


def fused_step(up, blk, push_cnt, max_index=(1 << 64) - 1):
    """One training minibatch on an oracle.Updater in SGDLearner::IterateData's order (oracle.cc
    orc_train_step :638-677) with the gradients of backward() above: the count push, Get, GetPos,
    Predict, CalcGrad, Update(kGradient).  The oracle's own UpdateW / UpdateV / InitV do the
    update, so only the sums are restated.  -> the predictions"""
    d = up.V_dim
    uniq, cnt, col = O.localize(blk.offs, blk.ids, max_index=max_index)
    if push_cnt and d > 0:
        up.update(uniq, O.Updater.kFeaCount, cnt)
    vals, lens = up.get(uniq)
    wp, vp = O.get_pos(lens) if d > 0 else (None, None)
    pred = O.fm_predict(blk.offs, col, blk.vals, vals, wp, vp, d)
    grad = backward(blk.offs, col, blk.vals, blk.labels, blk.weights, vals, wp, vp, len(uniq), d,
                    pred)
    up.update(uniq, O.Updater.kGradient, grad, lens)
    return pred
