"""The device reshuffler (difacto_amd/csrc/reshuffle.hip) in plain numpy: the permutation and
the epoch key restated from difacto_amd/csrc/reshuffle.h, and the batches a reshuffled epoch
must hand out.  A reference for the tests; nothing here touches a GPU."""
import numpy as np

M64 = (1 << 64) - 1
ROUNDS = 4  # kRsRounds


def _splitmix64(state):
    """-> (new state, output), rs_splitmix64"""
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def _fmix32(h):
    """rs_fmix32 over a uint32 array (products wrap mod 2^32)"""
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def epoch_key(shuffle_seed, epoch, lst):
    """rs_epoch_key"""
    _, a = _splitmix64(int(shuffle_seed) & M64)
    _, b = _splitmix64(a ^ (int(epoch) & M64))
    _, k = _splitmix64(b ^ (int(lst) & M64))
    return k


def net(N, key):
    """rs_make -> (round keys, half bits)"""
    s, ks = int(key) & M64, []
    for _ in range(ROUNDS):
        s, z = _splitmix64(s)
        ks.append(np.uint32(z & 0xFFFFFFFF))
    b = 0
    if N > 1:
        b = 2
        while b < 32 and (1 << b) < N:
            b += 2
    return ks, b // 2


def perm(N, key):
    """-> uint32[N]: output position j takes input row perm[j] (rs_perm for every j)"""
    ks, h = net(N, key)
    x = np.arange(N, dtype=np.uint32)
    if h == 0:
        return x
    m, hh = np.uint32((1 << h) - 1), np.uint32(h)
    todo = np.arange(N)
    with np.errstate(over="ignore"):
        while todo.size:
            v = x[todo]
            L, R = v >> hh, v & m
            for k in ks:
                L, R = R, L ^ (_fmix32(R ^ k) & m)
            v = (L << hh) | R
            x[todo] = v
            todo = todo[v >= N]
    return x


def _arr(b, name):
    return b.get(name) if isinstance(b, dict) else getattr(b, name)


def reshuffle(batches, batch_rows, key):
    """batches: the list's batches in order, each with offs / ids / vals / labels / weights
    (dicts or RowBlocks; vals and weights may be None).  -> the reshuffled epoch's batches as
    dicts of arrays: the list's N rows in the order perm(N, key), cut every batch_rows rows,
    offsets rebased; vals iff some source batch has them (binary sources read as ones), and the
    same for weights."""
    srcs = []
    for b in batches:
        offs = np.asarray(_arr(b, "offs"), np.uint64)
        srcs.append((offs, _arr(b, "ids"), _arr(b, "vals"), _arr(b, "labels"),
                     _arr(b, "weights")))
    valued = any(s[2] is not None for s in srcs)
    weighted = any(s[4] is not None for s in srcs)
    sizes = np.array([len(s[0]) - 1 for s in srcs], np.int64)
    prefix = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(prefix[-1])
    p = perm(N, key).astype(np.int64)
    which = np.searchsorted(prefix, p, side="right") - 1
    out = []
    for k0 in range(0, N, batch_rows):
        rows = range(k0, min(k0 + batch_rows, N))
        ids, vals, labels, weights, offs = [], [], [], [], [0]
        for j in rows:
            offs_s, ids_s, vals_s, labels_s, weights_s = srcs[which[j]]
            r = int(p[j] - prefix[which[j]])
            a, e = int(offs_s[r]), int(offs_s[r + 1])
            ids.append(np.asarray(ids_s[a:e], np.uint64) if e > a else np.zeros(0, np.uint64))
            if valued:
                vals.append(np.ones(e - a, np.float32) if vals_s is None
                            else np.asarray(vals_s[a:e], np.float32))
            labels.append(labels_s[r])
            weights.append(np.float32(1) if weights_s is None else weights_s[r])
            offs.append(offs[-1] + e - a)
        out.append({"offs": np.array(offs, np.uint64),
                    "ids": np.concatenate(ids) if ids else np.zeros(0, np.uint64),
                    "vals": (np.concatenate(vals) if vals else np.zeros(0, np.float32))
                    if valued else None,
                    "labels": np.array(labels, np.float32),
                    "weights": np.array(weights, np.float32) if weighted else None})
    return out
