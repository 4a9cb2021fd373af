"""Replay from the device batch cache with and without the kept Localizer outputs at the C3 shape
(12 batches of 100 k rows x 39 binary ids, uniform over 2^24 keys, V_dim = 16): after a recording
epoch with append_loc, epochs of the 12 cached batches alternate plain / loc / loc / plain three
times; prints M ex/s per epoch (host clock around the steps and the progress join).
    python tools/cache_loc_replay.py"""
import os
import sys
import time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from difacto_amd import data as D, hotpath as H
N = 12
cfg = dict(V_dim=16, V_threshold=0, l1=0, lr=.1, V_lr=.01, max_keys=1 << 25)
ctx = H.Context(0, **cfg)
bc = H.BatchCache(ctx, 8 << 30)
bc.begin(0)
for i in range(N):
    d = H.DeviceRowBlock(ctx, D.synthetic(100000, 39, 1 << 24, seed=100 + i))
    assert bc.append(d)
    H.train_step(ctx, d, H.kTraining, push_cnt=True)
    assert bc.append_loc()
assert bc.seal() == N
H.progress(ctx)
print("cache", bc.stats(), "loc", bc.stats_loc(), flush=True)
batches = [bc.get(0, i) for i in range(N)]
locs = [bc.get_loc(0, i) for i in range(N)]
print("U", [l.U for l in locs[:3]], "nnz", locs[0].nnz, "n_chunks", locs[0].n_chunks)
def epoch(use):
    t = time.perf_counter()
    for i in range(N):
        H.train_step(ctx, batches[i], H.kTraining, loc=locs[i] if use else None)
    p = H.progress(ctx)
    return N * 100000 / (time.perf_counter() - t) / 1e6, p["loss"]
for w in range(2):
    epoch(False); epoch(True)
for rep in range(3):
    for use in (False, True, True, False):
        r, loss = epoch(use)
        print("loc" if use else "plain", "%.1f M ex/s" % r, "loss %.6f" % (loss / (N * 100000)), flush=True)
bc.close()
ctx.close()
