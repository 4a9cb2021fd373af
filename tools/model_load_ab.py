"""The model file's host loader (dfx_store_load_part) against the device loader
(dfx_store_load_dev), A B B A on one box, the files in one directory and in the page cache
(each was just written, and every load reads it again):

  load    the aux=1 file of tools/model_write_ab.py's C3-shaped model (uniform keys over
          2^KEY_BITS, V_dim 16) into a fresh context
  reload  that model as two parts (the keys of rank 0 and 1 of 2) into rank 1 of 3: both files
          read, the keys the rank owns kept - what each of M ranks pays in an N -> M reload

and, from the device loader's own clocks, the seconds in fread and the seconds the host waited
for the device.  After every load the store's counters are compared with the first load's.
Prints as it goes; nothing is asserted about the times.
    python tools/model_load_ab.py [--key-bits 24] [--dir /tmp]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from model_write_ab import H, build  # noqa: E402


def fresh():
    return H.Context(0, V_dim=16, max_keys=1 << 10, max_vrows=1 << 10)


def abba(name, key_bits, files, rank, nranks):
    first, same, secs = None, True, {"host": [], "device": []}
    for who in ("host", "device", "device", "host"):
        ctx = fresh()
        s = H.Store(ctx)
        read = wait = 0.0
        t = time.perf_counter()
        for p in files:
            r = s.load(p, device=who == "device", rank=rank, nranks=nranks)
            if r:
                assert not r["host_loaded"], r
                read, wait = read + r["read_s"], wait + r["wait_s"]
        dt = time.perf_counter() - t
        secs[who].append(dt)
        st = s.stats()
        got = (st["n_keys"], st["n_vrows"], st["new_w"], s.capacity())
        line = "%s %-6s %8.3f s  %d keys, %d V rows, %d slots" % (name, who, dt, got[0], got[1],
                                                                 got[3])
        if who == "device":
            line += "  fread %.3f s (%.0f %%), waited %.3f s for the device" % (
                read, 100 * read / dt, wait)
        print(line, flush=True)
        first = first or got
        same = same and got == first
        ctx.close()
    print("%s: the four stores' counters are %s" % (name, "equal" if same else "DIFFERENT"))
    h, d = sum(secs["host"]) / 2, sum(secs["device"]) / 2
    print("%s: host %.3f s, device %.3f s (means of two), host / device = %.2f" % (name, h, d,
                                                                                  h / d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-bits", type=int, default=24)
    ap.add_argument("--dir", default="/tmp")
    a = ap.parse_args()
    whole = os.path.join(a.dir, "model_load_ab_whole")
    parts = [os.path.join(a.dir, "model_load_ab_part-%d" % r) for r in range(2)]
    ctx = build(a.key_bits)
    H.Store(ctx).save(whole, True, device=True)
    ctx.close()
    for r, p in enumerate(parts):  # (the parts a 2-shard run would save: the owner rule's)
        ctx = fresh()
        H.Store(ctx).load(whole, device=True, rank=r, nranks=2)
        H.Store(ctx).save(p, True, device=True)
        ctx.close()
    print("## load: %d bytes; reload: %s bytes" % (
        os.path.getsize(whole), " + ".join(str(os.path.getsize(p)) for p in parts)), flush=True)
    abba("load", a.key_bits, [whole], 0, 1)
    abba("reload", a.key_bits, parts, 1, 3)
    for p in [whole] + parts:
        os.unlink(p)


if __name__ == "__main__":
    main()
