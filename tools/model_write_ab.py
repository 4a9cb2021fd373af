"""The model files' host writers (dfx_store_save, dfx_store_dump) against the device writers
(dfx_store_save_dev, dfx_store_dump_dev), A B B A on one box, both writing to one directory:

  save  aux=1 of a C3-shaped model (uniform keys over 2^KEY_BITS, V_dim 16, fused steps on
        device-generated batches as bench.py makes them)
  dump  aux=0 of a model over 2^DUMP_BITS keys (the host's stream insertions stay within a minute)

and, from the device writers' own clocks, the seconds the host waited for a chunk (the kernels
and the copies it could not hide) against the seconds it spent writing (fwrite).  Every file of
a pair is compared byte for byte.  Prints as it goes; nothing is asserted about the times.
    python tools/model_write_ab.py [--key-bits 24] [--dump-bits 20] [--dir /tmp]"""
import argparse
import ctypes
import filecmp
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from bench import DevBatch  # noqa: E402
from difacto_amd import hotpath as H  # noqa: E402


def build(key_bits, batch=1 << 18, nnz=39):
    """fused steps until about four draws per key have been made -> the context"""
    ctx = H.Context(0, V_dim=16, V_threshold=0, l1=0, lr=.1, V_lr=.01, max_keys=1 << key_bits,
                    max_vrows=1 << key_bits)
    batch = min(batch, max(1 << key_bits >> 2, 1024))
    ctx.reserve(batch, batch * nnz)
    lib = H._lib.lib()
    steps = max(4, (4 << key_bits) // (batch * nnz))
    for i in range(steps):
        b = DevBatch(torch, ctx.device, batch, nnz, key_bits, seed=500 + i)
        torch.cuda.synchronize()
        bb = b.as_batch()
        H.check(lib.dfx_train_step(ctx.h, ctypes.byref(bb), H.kTraining, 1,
                                   ctypes.c_uint64(H.MAX_INDEX), None))
        ctx.sync()
    H.progress(ctx)
    return ctx


def abba(name, ctx, write, directory):
    s = H.Store(ctx)
    st = s.stats()
    print("## %s: %d keys, %d V rows, %d table slots" % (name, st["n_keys"], st["n_vrows"],
                                                         s.capacity()), flush=True)
    first, same, secs = None, True, {"host": [], "device": []}
    for i, who in enumerate(("host", "device", "device", "host")):
        p = os.path.join(directory, "model_write_ab_%s_%d" % (name, i))
        t = time.perf_counter()
        r = write(s, p, who == "device")
        dt = time.perf_counter() - t
        secs[who].append(dt)
        line = "%s %-6s %8.3f s  %d bytes" % (name, who, dt, os.path.getsize(p))
        if r:
            line += "  entries %d chunks %d host_chunks %d  waited %.3f s, writing %.3f s" % (
                r["entries"], r["chunks"], r["host_chunks"], r["wait_s"], r["write_s"])
        print(line, flush=True)
        if first is None:
            first = p
        else:  # (compared and removed at once: two files on the disk at most)
            same = filecmp.cmp(first, p, shallow=False) and same
            os.unlink(p)
    os.unlink(first)
    print("%s: the four files are %s" % (name, "identical" if same else "DIFFERENT"))
    h, d = sum(secs["host"]) / 2, sum(secs["device"]) / 2
    print("%s: host %.3f s, device %.3f s (means of two), host / device = %.2f" % (name, h, d,
                                                                                  h / d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-bits", type=int, default=24)
    ap.add_argument("--dump-bits", type=int, default=20)
    ap.add_argument("--dir", default="/tmp")
    a = ap.parse_args()
    ctx = build(a.key_bits)
    abba("save", ctx, lambda s, p, dev: s.save(p, True, device=dev), a.dir)
    ctx.close()
    ctx = build(a.dump_bits)
    abba("dump", ctx, lambda s, p, dev: s.dump(p, False, False, device=dev), a.dir)
    ctx.close()


if __name__ == "__main__":
    main()
