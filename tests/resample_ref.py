"""The per-epoch negative down-sample of the device reshuffler (dfx_reshuffle_begin_epoch_sampled)
in plain numpy: rs_draw and rs_dropped restated from difacto_amd/csrc/reshuffle.h, and the
batches a sampled epoch must hand out (the permuted order of tests/reshuffle_ref.py, filtered by
the draw on the SOURCE row, cut every batch_rows kept rows).  A reference for the tests; nothing
here touches a GPU."""
import numpy as np

from tests import reshuffle_ref as R

M64 = R.M64


def draw(key, rows):
    """rs_draw for an array of source rows -> float32 in [0, 1), multiples of 2^-24"""
    rows = np.asarray(rows, np.uint64)
    with np.errstate(over="ignore"):
        s = np.uint64(int(key) & M64) ^ (np.uint64(0xA0761D6478BD642F) * (rows + np.uint64(1)))
        z = s + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def dropped(key, rows, labels, neg_sampling):
    """rs_dropped -> bool array: the reader's inequality in fp32, drawn only below 1"""
    ns = np.float32(neg_sampling)
    labels = np.asarray(labels, np.float32)
    if not ns < np.float32(1):
        return np.zeros(len(labels), bool)
    return (labels <= np.float32(0)) & (draw(key, rows) > np.float32(1) - ns)


def _labels(batches):
    labs = [np.asarray(R._arr(b, "labels"), np.float32) for b in batches]
    return np.concatenate(labs) if labs else np.zeros(0, np.float32)


def kept_rows(batches, key, neg_sampling):
    """-> the source rows of the sampled epoch in output order (int64[K])"""
    labels = _labels(batches)
    N = len(labels)
    p = R.perm(N, key).astype(np.int64)
    return p[~dropped(key, p, labels[p], neg_sampling)]


def resample(batches, batch_rows, key, neg_sampling):
    """the sampled epoch's batches, as reshuffle_ref.reshuffle's dicts: the list's rows in the
    order perm(N, key) without the dropped ones, cut every min(batch_rows, N) rows; vals and
    weights as the whole list has them"""
    srcs = []
    for b in batches:
        srcs.append((np.asarray(R._arr(b, "offs"), np.uint64), R._arr(b, "ids"), R._arr(b, "vals"),
                     R._arr(b, "labels"), R._arr(b, "weights")))
    valued = any(s[2] is not None for s in srcs)
    weighted = any(s[4] is not None for s in srcs)
    sizes = np.array([len(s[0]) - 1 for s in srcs], np.int64)
    prefix = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(prefix[-1])
    keep = kept_rows(batches, key, neg_sampling)
    which = np.searchsorted(prefix, keep, side="right") - 1
    step = max(min(batch_rows, N), 1)
    out = []
    for k0 in range(0, len(keep), step):
        ids, vals, labels, weights, offs = [], [], [], [], [0]
        for c in range(k0, min(k0 + step, len(keep))):
            offs_s, ids_s, vals_s, labels_s, weights_s = srcs[which[c]]
            r = int(keep[c] - prefix[which[c]])
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
