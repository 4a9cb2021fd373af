"""Test infrastructure: the two progress metrics restated in float64 with the device's own
arithmetic, so the device can be held to them exactly (AUC) or to double rounding (logloss).

auc_times_n    BinClassMetric::AUC * n as metric.hip computes it: a stable sort by the
               orderable key of pred + 0.0f (ties in input order), the area an exact integer,
               then k_auc_final's / k_auc_block's operations in their order — one division, the
               flip below 0.5, one multiplication.  IEEE double division and multiplication are
               correctly rounded on both sides, so the comparison with the device is `==`.

logloss_sum    Loss::Evaluate's sum, log(1.0 + exp(-y * pred)) per row in double, summed
               exactly (math.fsum), with the bound `tol` on what the device's own double
               evaluation of the same terms in another order can differ by.

tol = 2^-53 * ((D + 4) * S + 6 * n):
  u = 2^-53 is the rounding unit, 1 ulp <= 2 u relative.  One term is t = log(x), x = 1.0 + e,
  e = exp(-y * pred); -y * pred is exact in double (a float times +-1).  exp is within 1 ulp
  on the device and within 1 ulp here, so the two e differ by at most 4 u e; the addition
  rounds once on each side, 2 u x; together the two x differ by at most 6 u x, and through
  log (derivative 1 / x) the terms by 6 u.  log is within 1 ulp on each side: 4 u t.  Per term
  u (6 + 4 t) at most, over n rows u (6 n + 4 S).
  A sum of non-negative terms whose longest chain of additions has D links is within D u S of
  the exact sum (each addition rounds a partial sum that is at most S; the second-order
  terms are 1e-14 of this bound at D = 256).

D = 256, read from the kernels: the additions on the longest path from a row's term to
ds->prog[1].
  rows a lane loops over     1 in k_eval_part, k_fm_fwd, k_fm_fwd_probe, k_split_combine[_vec].
                             k_fm_fwd_walk's groups loop over rows on a resident grid of g
                             blocks of 256 / G rows, G = V_dim / 4 in {2, 4}: ceil(B * G / (256
                             g)) rows.  __launch_bounds__(256, 4) makes at least 4 blocks per
                             CU resident, so g >= 8 on anything with two CUs: at the largest
                             batch tested (B = 10^5, G = 4) at most 196 (2 on a 256-CU part)
  6                          the wave's __shfl_xor steps
  4                          waves per block (256 threads), summed in order by thread 0
  partials per thread        step_finalize_body (256 threads): nparts / 256, nparts = one per
                             block = ceil(B * G / 256), G <= 64 lanes per row: 98 at B = 10^5;
                             at most 4 for the walk's resident grid.  k_sum_parts /
                             k_split_worker_finalize (1024 threads): nparts / 1024 = 4 at the
                             largest standalone n (4096 * 240 + 1 rows, 256 per block)
  6 + 16                     the finalizer's __shfl_xor steps and its waves (4 of 256 threads,
                             16 of 1024)
  1 per step                 prog[1] += the step's sum; tests accumulate at most 16 steps
                             between two reads
The walk: 196 + 6 + 4 + 1 + 6 + 4 + 16 = 233.  Every other forward: 1 + 6 + 4 + 98 + 6 + 16 +
16 = 147.  Both are below 256, which is the one bound used everywhere."""
import math

import numpy as np

D_LINKS = 256


def auc_times_n(label, pred):
    """AUC * n exactly as the device computes it (1.0 when all labels are of one class)."""
    label = np.asarray(label, np.float32)
    key = np.asarray(pred).astype(np.float32) + np.float32(0)
    n = len(key)
    order = np.argsort(key, kind="stable")
    pos = (label[order] > 0).astype(np.int64)
    P = int(pos.sum())
    if P in (0, n):
        return 1.0
    below = np.cumsum(pos) - pos           # positives ranked strictly before each item
    area = int(below[pos == 0].sum())      # an exact integer
    a = float(area) / (float(P) * (float(n) - float(P)))
    return ((1 - a) if a < 0.5 else a) * float(n)


def logloss_terms(label, pred):
    """the rows' terms of Loss::Evaluate in double, as the kernels write them"""
    y = np.where(np.asarray(label, np.float32) > 0, 1.0, -1.0)
    with np.errstate(over="ignore"):
        return np.log(1.0 + np.exp(-y * np.asarray(pred).astype(np.float64)))


def logloss_sum(label, pred):
    """-> (S, tol): the exact sum of the float64 terms, and the bound on |device - S|"""
    t = logloss_terms(label, pred)
    S = math.fsum(t)
    tol = 2.0 ** -53 * ((D_LINKS + 4) * S + 6 * len(t))
    return S, tol


# ---- the standalone cases' inputs, shared by test_metric_exact.py (their references' own
# properties, on the CPU) and test_gpu_metric_exact.py (the device against them)
# Each size is the smallest that reaches a boundary of metric.hip / sort.hip; the order mixes
# large and small so a long-lived context reuses its workspaces and the last call's sortmeta.
SIZES = [
    4096 * 240 + 1,   # first radix fallback inside merge mode (241 runs > kMaxMergeRuns)
    1, 12289,         # 12289: 4 runs, the last of 1 item; the first tiled counting pass
    64, 4096 * 239 + 1,  # 240 runs with a 1-item tail: 120 pairs = kMaxPairs
    2, 63, 16385,     # 16385: 5 runs, an odd pair count
    65, 767, 4096 * 240,  # 4096 * 240: the last merge size
    768, 28673,       # 768: one wave's 12 x 64 items in k_auc_block; 28673: 8 runs, 4 / 2 / 1
    769, 12287, 100003, 12288,  # 12288: the one-block limit
    2048 * 9 - 1, 3, 2048 * 9 + 1, 2048 * 9,  # the counting pass's tile edge
]

PATTERNS = ["correlated", "anti", "eighths", "equal", "saturated", "signed_zero", "inf",
            "subnormal", "low_byte", "exp_byte"]
# patterns whose terms are standard-normal sized: tol must stay below their smallest term
NORMAL_PATTERNS = ("correlated", "anti")


def labels_pm1(rng, n):
    return np.where(rng.random(n) < 0.3, 1.0, -1.0).astype(np.float32)


def labels_odd(rng, n):
    """labels other than +-1: positive means label > 0, so -0.0 and 0 are negatives"""
    return rng.choice(np.array([-1, -0.0, 0, 0.5, 2], np.float32), size=n)


def make_pred(name, rng, n, label):
    """float32 predictions of one pattern (no NaN: the reference's sort is undefined there)"""
    y = np.where(label > 0, 1.0, -1.0)
    if name == "correlated":   # distinct normals, area > 0.5
        return (rng.standard_normal(n) + 0.5 * y).astype(np.float32)
    if name == "anti":         # area < 0.5: the 1 - a branch
        return (rng.standard_normal(n) - 0.8 * y).astype(np.float32)
    if name == "eighths":      # heavy ties
        return (np.round(rng.standard_normal(n) * 8) / 8).astype(np.float32)
    if name == "equal":        # one run of ties: every radix digit constant
        return np.full(n, 0.75, np.float32)
    if name == "saturated":    # a model clipped at +-20
        return np.where(rng.random(n) < 0.5 + 0.2 * y, 20.0, -20.0).astype(np.float32)
    if name == "signed_zero":  # -0 == +0 for operator<
        p = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        p[rng.random(n) < 0.3] = -1.5
        return p
    if name == "inf":
        p = (rng.standard_normal(n) + 0.5 * y).astype(np.float32)
        r = rng.random(n)
        p[r < 0.1] = np.inf
        p[r > 0.9] = -np.inf
        return p
    if name == "subnormal":    # a flushing key add would tie these with 0
        vals = np.array([1e-45, -1e-45, 1e-40, -1e-40, 3e-39, 0.0, -0.0], np.float32)
        return rng.choice(vals, size=n)
    if name == "low_byte":     # keys differ in their lowest byte only: one active radix pass
        bits = np.uint32(0x3F800000) | rng.integers(0, 256, n).astype(np.uint32)
        return bits.view(np.float32)
    if name == "exp_byte":     # keys differ in their top byte only (sign and 7 exponent bits)
        bits = (rng.integers(0, 256, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00400000)
        return bits.view(np.float32)
    raise ValueError(name)


def standalone_case(name, n, odd_labels=False):
    """(label, pred) of one (pattern, size): seeded by both, the same on the CPU and the GPU"""
    rng = np.random.default_rng([PATTERNS.index(name), n, int(odd_labels)])
    label = labels_odd(rng, n) if odd_labels else labels_pm1(rng, n)
    return label, make_pred(name, rng, n, label)
