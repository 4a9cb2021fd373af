"""Python mirror of DiFacto's plugin interfaces for the hot path, over libdifacto_amd.so.

Names, argument meaning and error behaviour follow the reference's C++ interfaces so the
parity tests read like its gtests:

    Localizer.compact          src/data/localizer.h:41-51
    FMLoss.predict/calc_grad   src/loss/fm_loss.h:56-203 (LogitLoss == FMLoss with V_dim 0)
    Loss.evaluate, auc         include/difacto/loss.h:57-66, src/loss/bin_class_metric.h:35-57
    Store.pull/push            include/difacto/store.h:44-75 over SGDUpdater::Get/Update
    Store.save/load/dump       src/sgd/sgd_updater.h:84-139
    train_step                 SGDLearner::IterateData's per-batch executor (fused)

Device buffers are torch tensors (torch is the allocator and stream provider only); u64
keys travel as int64 tensors holding the same bits, u32 as int32.  Every call goes through
the C-ABI; a failing status raises DfxError (the reference would LOG(FATAL)).
"""
import ctypes
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import check

kFeaCount, kWeight, kGradient = 1, 2, 3
kTraining, kValidation, kPrediction = 3, 4, 5
MAX_INDEX = (1 << 64) - 1


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _kwstr(kwargs):
    return ",".join("%s=%s" % (k, v) for k, v in kwargs.items()).encode()


class Context:
    """One device context: a stream, the device model store and a scratch workspace.

    kwargs are the reference .conf keys (lr, V_dim, V_lr, l1, l2, V_threshold, ...) plus
    max_keys / max_vrows for the device hash table.  Like the reference's Loss objects a
    context is not thread-safe.
    """

    def __init__(self, device=0, **kwargs):
        self.device = torch.device("cuda", device)
        self.kwargs = dict(kwargs)
        h = ctypes.c_void_p()
        # strict: a misspelt or retired kwarg raises instead of running the default
        check(_lib.lib().dfx_ctx_create(device, _kwstr(dict(kwargs, strict=1)), ctypes.byref(h)))
        self.h = h
        self.V_dim = _lib.lib().dfx_ctx_vdim(h)
        self.use_current_stream()

    def use_current_stream(self):
        s = torch.cuda.current_stream(self.device)
        check(_lib.lib().dfx_ctx_set_stream(self.h, ctypes.c_void_p(s.cuda_stream)))

    def set_input_stream(self, stream):
        """batches of train_step are produced on this torch stream (None: the context's)"""
        check(_lib.lib().dfx_ctx_set_input_stream(
            self.h, None if stream is None else ctypes.c_void_p(stream.cuda_stream)))

    def close(self):
        if getattr(self, "h", None):
            for bc in list(getattr(self, "_caches", ())):  # they join this context
                bc.close()
            _lib.lib().dfx_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(_lib.lib().dfx_sync(self.h))

    def reserve(self, max_rows, max_nnz):
        check(_lib.lib().dfx_reserve(self.h, int(max_rows), int(max_nnz)))

    # ---- helpers -------------------------------------------------------------------------
    def tensor(self, a, dtype):
        """host numpy array -> device tensor of ``dtype`` (u64 -> int64 bits, u32 -> int32)."""
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        elif a.dtype == np.uint32:
            a = a.view(np.int32)
        return torch.from_numpy(a.copy()).to(self.device, dtype=dtype)


class DeviceRowBlock:
    """dmlc::RowBlock<feaid_t> resident on the device (BatchReader output)."""

    def __init__(self, ctx, blk):
        self.size = blk.size
        self.nnz = blk.nnz
        self.offs = ctx.tensor(blk.offs, torch.int64)
        self.ids = ctx.tensor(blk.ids, torch.int64)
        self.vals = ctx.tensor(blk.vals, torch.float32)
        self.labels = ctx.tensor(blk.labels, torch.float32)
        self.weights = ctx.tensor(blk.weights, torch.float32)

    def as_batch(self):
        return _lib.Batch(self.size, self.nnz, _p(self.offs), _p(self.ids), _p(self.vals),
                          _p(self.labels), _p(self.weights))


def u64(t):
    """device int64 tensor holding u64 bits -> numpy uint64"""
    return t.cpu().numpy().view(np.uint64)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


class Localizer:
    """Localizer (src/data/localizer.h:16-95): uint64 ids -> sorted unique reversed keys,
    float counts and a u32-remapped CSR.  Compact returns (col, uniq, cnt) device tensors; the
    compacted block's offsets/values/labels are the input's."""

    def __init__(self, ctx, max_index=MAX_INDEX):
        self.ctx = ctx
        self.max_index = max_index

    def compact(self, dblk, want_cnt=True):
        ctx = self.ctx
        nnz = dblk.nnz
        uniq = torch.empty(max(nnz, 1), dtype=torch.int64, device=ctx.device)
        cnt = torch.empty(max(nnz, 1), dtype=torch.float32, device=ctx.device) if want_cnt else None
        col = torch.empty(max(nnz, 1), dtype=torch.int32, device=ctx.device)
        n = ctypes.c_int64(0)
        check(_lib.lib().dfx_localize(ctx.h, dblk.size, nnz, _p(dblk.offs), _p(dblk.ids),
                                      ctypes.c_uint64(self.max_index), _p(uniq), _p(cnt),
                                      _p(col), ctypes.byref(n)))
        U = n.value
        return col[:nnz], uniq[:U], (cnt[:U] if want_cnt else None)


LOC_STATS = ("U", "n_chunks", "n_init", "used", "hint0", "hint1", "hint2", "hint3", "lb_over",
             "lb_map_steps", "deferred", "pk_valid", "wbits", "ntiles", "rt", "q_lds")


def localize_occ(ctx, offs, ids, vals=None, max_index=MAX_INDEX, keys_ready=False):
    """dfx_localize_occ: what the fused step's Localizer lane (and the split owner, keys_ready)
    leaves for the forward / backward, as host numpy arrays: uniq[U], segstart[U + 1],
    occ_row[nnz], occ_x[nnz] (uint32 bit patterns; None for binary data), n_chunks, choff[U]
    and chunk_seg[n_chunks] (None without chunks), and the stats by name (LOC_STATS) plus
    ``mapped``: this batch was placed by the hot-key map.  With lb_gather=2 the occurrences'
    rows and values are resolved through the {row, value}-by-position array, as the backward
    reads them."""
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    B, nnz = max(len(offs) - 1, 0), len(ids)
    dev = ctx.device

    def buf(n, dt):
        return torch.empty(max(int(n), 1), dtype=dt, device=dev)

    d_offs = ctx.tensor(offs, torch.int64) if len(offs) else None
    d_ids = ctx.tensor(ids, torch.int64) if nnz else None
    d_vals = ctx.tensor(np.ascontiguousarray(vals, dtype=np.float32), torch.float32) \
        if vals is not None and nnz else None
    valued = vals is not None
    uniq, seg = buf(nnz, torch.int64), buf(nnz + 1, torch.int32)
    occ_row, choff = buf(nnz, torch.int32), buf(nnz, torch.int32)
    occ_x = buf(nnz, torch.int32) if valued else None
    rowof = buf(2 * nnz, torch.int32) if valued else None
    cseg = buf(nnz // 128 + nnz // 129 + 2, torch.int32)
    stats = (ctypes.c_int64 * len(LOC_STATS))()
    torch.cuda.current_stream(dev).synchronize()  # the inputs, for the context's own stream
    check(_lib.lib().dfx_localize_occ(ctx.h, B, nnz, _p(d_offs), _p(d_ids), _p(d_vals),
                                      ctypes.c_uint64(max_index), int(bool(keys_ready)),
                                      _p(uniq), _p(seg), _p(occ_row), _p(occ_x), _p(choff),
                                      _p(cseg), _p(rowof), stats))
    st = dict(zip(LOC_STATS, (int(v) for v in stats)))
    prev = getattr(ctx, "_lb_map_steps", 0)
    st["mapped"] = st["lb_map_steps"] - prev
    ctx._lb_map_steps = st["lb_map_steps"]
    U, nch = st["U"], st["n_chunks"]
    out = {"U": U, "n_chunks": nch, "stats": st,
           "uniq": u64(uniq[:U]), "segstart": u32(seg[:U + 1])}
    rows = u32(occ_row[:nnz])
    xs = u32(occ_x[:nnz]) if valued else None
    if st["deferred"]:
        rv = u32(rowof[:2 * nnz]).reshape(nnz, 2)
        rows, xs = rv[rows, 0].copy(), rv[rows, 1].copy()
    out["occ_row"], out["occ_x"] = rows, xs
    out["choff"] = u32(choff[:U]) if nch > 0 else None
    out["chunk_seg"] = u32(cseg[:nch]) if nch > 0 else None
    return out


class FMLoss:
    """FMLoss (src/loss/fm_loss.h); V_dim == 0 is LogitLoss (src/loss/logit_loss.h)."""

    def __init__(self, ctx, V_dim=0):
        self.ctx = ctx
        self.V_dim = int(V_dim)

    def predict(self, dblk, col, weights, w_pos, V_pos, pred, n_cols):
        """pred += forward(X, weights) — accumulates like the reference."""
        check(_lib.lib().dfx_fm_predict(self.ctx.h, dblk.size, dblk.nnz, _p(dblk.offs), _p(col),
                                        _p(dblk.vals), _p(weights), _p(w_pos), _p(V_pos),
                                        int(n_cols), self.V_dim, _p(pred)))

    def calc_grad(self, dblk, col, weights, w_pos, V_pos, pred, grad, n_cols):
        """grad += backward(X, weights, pred) — grad must be pre-zeroed like the reference."""
        check(_lib.lib().dfx_fm_calcgrad(self.ctx.h, dblk.size, dblk.nnz, _p(dblk.offs), _p(col),
                                         _p(dblk.vals), _p(dblk.labels), _p(dblk.weights),
                                         _p(weights), _p(w_pos), _p(V_pos), int(n_cols),
                                         self.V_dim, _p(pred), _p(grad)))

    def evaluate(self, label, pred):
        out = ctypes.c_double(0)
        check(_lib.lib().dfx_evaluate(self.ctx.h, pred.numel(), _p(label), _p(pred),
                                      ctypes.byref(out)))
        return out.value


def auc(ctx, label, pred):
    """BinClassMetric::AUC, returned as AUC * n like the reference."""
    out = ctypes.c_double(0)
    check(_lib.lib().dfx_auc(ctx.h, pred.numel(), _p(label), _p(pred), ctypes.byref(out)))
    return out.value


def get_pos(ctx, lens):
    n = lens.numel()
    w = torch.empty(max(n, 1), dtype=torch.int32, device=ctx.device)
    v = torch.empty(max(n, 1), dtype=torch.int32, device=ctx.device)
    check(_lib.lib().dfx_get_pos(ctx.h, n, _p(lens), _p(w), _p(v)))
    return w[:n], v[:n]


class Store:
    """The device model store: Store push/pull over the SGDUpdater (FTRL w, AdaGrad V,
    V_threshold lazy InitV)."""

    def __init__(self, ctx):
        self.ctx = ctx

    def pull(self, keys):
        ctx = self.ctx
        n = keys.numel()
        d = ctx.V_dim
        vals = torch.empty(max(n * (1 + d), 1), dtype=torch.float32, device=ctx.device)
        lens = torch.empty(max(n, 1), dtype=torch.int32, device=ctx.device) if d > 0 else None
        nv = ctypes.c_int64(0)
        check(_lib.lib().dfx_store_pull(ctx.h, _p(keys), n, _p(vals), _p(lens), ctypes.byref(nv)))
        return vals[:nv.value], (lens[:n] if d > 0 else None)

    def push(self, keys, val_type, vals, lens=None):
        check(_lib.lib().dfx_store_push(self.ctx.h, _p(keys), keys.numel(), int(val_type),
                                        _p(vals), vals.numel(), _p(lens)))

    def save(self, path, save_aux=True, device=False, chunk_slots=0):
        """SGDUpdater::Save's file.  device: packed on the device (dfx_store_save_dev), the same
        bytes -> its stats (model_write_stats)"""
        if device:
            st, tm = (ctypes.c_int64 * 4)(), (ctypes.c_double * 2)()
            check(_lib.lib().dfx_store_save_dev(self.ctx.h, str(path).encode(), int(save_aux),
                                                int(chunk_slots), st, tm))
            return model_write_stats(st, tm)
        check(_lib.lib().dfx_store_save(self.ctx.h, str(path).encode(), int(save_aux)))

    def load(self, path):
        check(_lib.lib().dfx_store_load(self.ctx.h, str(path).encode()))

    def dump(self, path, dump_aux=False, need_reverse=False, device=False, chunk_slots=0):
        """SGDUpdater::Dump's text.  device: formatted on the device (dfx_store_dump_dev), the
        same bytes -> its stats; host_chunks counts the chunks the host loop wrote in the
        device's place (an entry with a float outside csrc/fmtg.h's domain)"""
        if device:
            st, tm = (ctypes.c_int64 * 4)(), (ctypes.c_double * 2)()
            check(_lib.lib().dfx_store_dump_dev(self.ctx.h, str(path).encode(), int(dump_aux),
                                                int(need_reverse), int(chunk_slots), st, tm))
            return model_write_stats(st, tm)
        check(_lib.lib().dfx_store_dump(self.ctx.h, str(path).encode(), int(dump_aux),
                                        int(need_reverse)))

    def capacity(self):
        """the table's slots (the range of model_pack / model_format and of chunk_slots)"""
        cap = ctypes.c_int64(0)
        check(_lib.lib().dfx_store_probe_stats(self.ctx.h, None, None, ctypes.byref(cap)))
        return cap.value

    def stats(self):
        nk, nv, nw = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_double(0)
        seed = ctypes.c_uint32(0)
        check(_lib.lib().dfx_store_stats(self.ctx.h, ctypes.byref(nk), ctypes.byref(nv),
                                         ctypes.byref(nw), ctypes.byref(seed)))
        return {"n_keys": nk.value, "n_vrows": nv.value, "new_w": nw.value, "seed": seed.value}

    def evaluate(self):
        pen, nnz = ctypes.c_double(0), ctypes.c_int64(0)
        check(_lib.lib().dfx_store_evaluate(self.ctx.h, ctypes.byref(pen), ctypes.byref(nnz)))
        return pen.value, nnz.value

    def probe_stats(self):
        """-> (mean probe distance, longest probe distance, table capacity)"""
        m, mx, cap = ctypes.c_double(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(_lib.lib().dfx_store_probe_stats(self.ctx.h, ctypes.byref(m), ctypes.byref(mx),
                                               ctypes.byref(cap)))
        return m.value, mx.value, cap.value

    def reserve(self, n_keys, n_vrows):
        check(_lib.lib().dfx_store_reserve(self.ctx.h, int(n_keys), int(n_vrows)))

    def entry(self, key):
        d = self.ctx.V_dim
        st = (ctypes.c_float * 4)()
        V = (ctypes.c_float * max(2 * d, 1))()
        hv, found = ctypes.c_int(0), ctypes.c_int(0)
        check(_lib.lib().dfx_store_entry(self.ctx.h, ctypes.c_uint64(int(key)), st, V,
                                         ctypes.byref(hv), ctypes.byref(found)))
        if not found.value:
            return None
        return (np.array(st, np.float32),
                np.array(V, np.float32)[:2 * d].copy() if hv.value else None)


def train_step(ctx, dblk, job_type=kTraining, push_cnt=False, max_index=MAX_INDEX, pred=None,
               loc=None):
    """One fused minibatch (localize -> [feacnt] -> pull -> predict -> eval -> AUC ->
    calcgrad -> push).  Progress accumulates on the device; read it with progress().
    loc: the batch's Localizer outputs from BatchCache.get_loc (dfx_train_step_loc: the step
    reads them from the cache and runs no Localizer); None, or one that holds none: as without."""
    b = dblk.as_batch()
    if loc is None:
        check(_lib.lib().dfx_train_step(ctx.h, ctypes.byref(b), int(job_type),
                                        int(bool(push_cnt)), ctypes.c_uint64(max_index),
                                        _p(pred)))
        return
    check(_lib.lib().dfx_train_step_loc(ctx.h, ctypes.byref(b), ctypes.byref(loc.l),
                                        int(job_type), int(bool(push_cnt)),
                                        ctypes.c_uint64(max_index), _p(pred)))


class CachedLoc:
    """The Localizer outputs a BatchCache keeps with a batch (dfx_loc; its pointers point into
    the cache).  held: False when the batch has none (train_step(loc=) then runs the
    Localizer); arrays() downloads them."""

    def __init__(self, ctx, l):
        self.ctx = ctx
        self.l = l
        self.held = bool(l.uniq)
        self.U, self.n_chunks, self.form = l.U, l.n_chunks, l.form
        self.size, self.nnz, self.max_index = l.size, l.nnz, l.max_index

    def pointers(self):
        """the device addresses of the kept arrays (None: NULL)"""
        l = self.l
        return {"uniq": l.uniq, "segstart": l.segstart, "occ_row": l.occ_row, "occ_x": l.occ_x,
                "rowof": l.rowof, "choff": l.choff, "chunk_seg": l.chunk_seg,
                "totals": l.totals}

    def _download(self, ptr, n, dtype):
        out = np.empty(n, dtype)
        if n:
            check(_lib.lib().dfx_memcpy(self.ctx.h, ctypes.c_void_p(out.ctypes.data),
                                        ctypes.c_void_p(ptr), out.nbytes, 1))
        return out

    def arrays(self):
        """-> what localize_occ returns for the batch, from the cache: U, n_chunks, uniq[U],
        segstart[U + 1], occ_row[nnz] and occ_x[nnz] (uint32 bit patterns, None for binary data;
        the rowof form resolved through its {row, value}-by-position array as the backward reads
        it), choff[U] and chunk_seg[n_chunks] (None without chunks); plus form and totals, the
        record's four device words.  None when the batch holds no outputs."""
        if not self.held:
            return None
        l = self.l
        U, nch, nnz = l.U, l.n_chunks, l.nnz if l.size > 0 else 0
        out = {"U": U, "n_chunks": nch, "form": l.form,
               "uniq": self._download(l.uniq, U, np.uint64),
               "segstart": self._download(l.segstart, U + 1, np.uint32),
               "totals": self._download(l.totals, 4, np.uint32)}
        rows = self._download(l.occ_row, nnz, np.uint32)
        xs = self._download(l.occ_x, nnz, np.uint32) if l.form == 1 else None
        if l.form == 2:
            rv = self._download(l.rowof, 2 * nnz, np.uint32).reshape(nnz, 2)
            rows, xs = rv[rows, 0].copy(), rv[rows, 1].copy()
        out["occ_row"], out["occ_x"] = rows, xs
        out["choff"] = self._download(l.choff, U, np.uint32) if nch > 0 else None
        out["chunk_seg"] = self._download(l.chunk_seg, nch, np.uint32) if nch > 0 else None
        return out


class CachedBatch:
    """A batch held by a BatchCache: as_batch() like DeviceRowBlock (its pointers point into
    the cache and stay valid until the cache is closed); arrays() downloads it."""

    def __init__(self, ctx, b):
        self.ctx = ctx
        self.b = b
        self.size = b.size
        self.nnz = b.nnz

    def as_batch(self):
        b = self.b
        return _lib.Batch(b.size, b.nnz, b.offset, b.index, b.value, b.label, b.weight)

    def pointers(self):
        """the device addresses of offset, index, value, label, weight (None: NULL)"""
        b = self.b
        return {"offs": b.offset, "ids": b.index, "vals": b.value, "labels": b.label,
                "weights": b.weight}

    def _download(self, ptr, n, dtype):
        if ptr is None:
            return None
        out = np.empty(n, dtype)
        if n:
            check(_lib.lib().dfx_memcpy(self.ctx.h, ctypes.c_void_p(out.ctypes.data),
                                        ctypes.c_void_p(ptr), out.nbytes, 1))
        return out

    def arrays(self):
        """-> dict of host numpy arrays (None where the cached pointer is NULL); joins the
        context stream, behind which the cache's copies ran when no input stream is set"""
        b = self.b
        return {"offs": self._download(b.offset, b.size + 1, np.uint64),
                "ids": self._download(b.index, b.nnz, np.uint64),
                "vals": self._download(b.value, b.nnz, np.float32),
                "labels": self._download(b.label, b.size, np.float32),
                "weights": self._download(b.weight, b.size, np.float32)}


class BatchCache:
    """The device batch cache (dfx_batchcache_*, include/difacto_amd.h): lists of formed
    batches kept in device memory and replayed through train_step.  A list that does not fit
    budget_bytes is dropped (append returns False, seal -1), never an error."""

    def __init__(self, ctx, budget_bytes, block_bytes=0):
        self.ctx = ctx
        h = ctypes.c_void_p()
        check(_lib.lib().dfx_batchcache_create(ctx.h, int(budget_bytes), int(block_bytes),
                                               ctypes.byref(h)))
        self.h = h
        if not hasattr(ctx, "_caches"):
            ctx._caches = weakref.WeakSet()  # Context.close closes its caches first
        ctx._caches.add(self)

    def begin(self, list_id):
        check(_lib.lib().dfx_batchcache_begin(self.h, int(list_id)))

    def append(self, dblk):
        """copies dblk (anything with as_batch()) into the open list -> kept"""
        b = dblk.as_batch()
        kept = ctypes.c_int(0)
        check(_lib.lib().dfx_batchcache_append(self.h, ctypes.byref(b), ctypes.byref(kept)))
        return bool(kept.value)

    def seal(self):
        n = ctypes.c_int64(0)
        check(_lib.lib().dfx_batchcache_seal(self.h, ctypes.byref(n)))
        return n.value

    def count(self, list_id):
        n = ctypes.c_int64(0)
        check(_lib.lib().dfx_batchcache_count(self.h, int(list_id), ctypes.byref(n)))
        return n.value

    def get(self, list_id, i):
        b = _lib.Batch()
        check(_lib.lib().dfx_batchcache_get(self.h, int(list_id), int(i), ctypes.byref(b)))
        return CachedBatch(self.ctx, b)

    def stats(self):
        out = (ctypes.c_int64 * 4)()
        check(_lib.lib().dfx_batchcache_stats(self.h, out))
        return dict(zip(("sealed", "dropped", "batches", "bytes"), list(out)))

    def append_loc(self):
        """after the train_step (on this cache's context) that consumed the batch last
        appended: keeps that step's Localizer outputs with it -> kept (False: they did not fit
        the budget; the batch stays cached without them, the list is not dropped)"""
        kept = ctypes.c_int(0)
        check(_lib.lib().dfx_batchcache_append_loc(self.h, ctypes.byref(kept)))
        return bool(kept.value)

    def get_loc(self, list_id, i):
        """-> CachedLoc of batch i of a sealed list, for train_step(loc=)"""
        l = _lib.Loc()
        check(_lib.lib().dfx_batchcache_get_loc(self.h, int(list_id), int(i), ctypes.byref(l)))
        return CachedLoc(self.ctx, l)

    def stats_loc(self):
        """-> (batches holding Localizer outputs, the bytes those take, steps served from them)"""
        out = (ctypes.c_int64 * 3)()
        check(_lib.lib().dfx_batchcache_stats_loc(self.h, out))
        return tuple(out)

    def close(self):
        if getattr(self, "h", None):
            for rs in list(getattr(self, "_reshufflers", ())):  # they read this cache
                rs.close()
            h, self.h = self.h, None
            check(_lib.lib().dfx_batchcache_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Reshuffler:
    """A fresh shuffle of a sealed list of a BatchCache per epoch (dfx_reshuffle_*,
    include/difacto_amd.h): begin_epoch(key) -> the epoch's batch count, then next() /
    train_step / consumed() per batch.  kept: False when the ring and the scratch did not fit
    the cache's budget (every other call then raises: replay the list as recorded)."""

    def __init__(self, bc, list_id, batch_rows, nring=2):
        self.bc, self.ctx = bc, bc.ctx
        h, kept = ctypes.c_void_p(), ctypes.c_int(0)
        check(_lib.lib().dfx_reshuffle_create(bc.h, int(list_id), int(batch_rows), int(nring),
                                              ctypes.byref(h), ctypes.byref(kept)))
        self.h = h if kept.value else None
        self.kept = bool(kept.value)
        if self.kept:
            if not hasattr(bc, "_reshufflers"):
                bc._reshufflers = weakref.WeakSet()  # BatchCache.close closes them first
            bc._reshufflers.add(self)

    def begin_epoch(self, key):
        """-> the number of batches of the epoch keyed by ``key`` (any 64 bits); -1: the ring
        had to grow and no longer fits the budget"""
        n = ctypes.c_int64(0)
        check(_lib.lib().dfx_reshuffle_begin_epoch(self.h, ctypes.c_uint64(int(key)),
                                                   ctypes.byref(n)))
        return n.value

    def begin_epoch_sampled(self, key, neg_sampling):
        """the epoch keyed by ``key`` without the negative rows rs_dropped names (a fresh
        down-sample per key) -> (its batch count, its rows); (-1, 0): the compacted arrays or the
        ring do not fit the budget"""
        n, rows = ctypes.c_int64(0), ctypes.c_int64(0)
        check(_lib.lib().dfx_reshuffle_begin_epoch_sampled(
            self.h, ctypes.c_uint64(int(key)), ctypes.c_float(neg_sampling), ctypes.byref(n),
            ctypes.byref(rows)))
        return n.value, rows.value

    def next(self):
        """-> the next batch (a CachedBatch whose pointers point into the ring), None past the
        last one"""
        b, has = _lib.Batch(), ctypes.c_int(0)
        check(_lib.lib().dfx_reshuffle_next(self.h, ctypes.byref(b), ctypes.byref(has)))
        return CachedBatch(self.ctx, b) if has.value else None

    def consumed(self):
        """after the train_step that took the batch next() handed out"""
        check(_lib.lib().dfx_reshuffle_consumed(self.h))

    def stats(self):
        out = (ctypes.c_int64 * 4)()
        check(_lib.lib().dfx_reshuffle_stats(self.h, out))
        return dict(zip(("rows", "batches", "ring_bytes", "scratch_bytes"), list(out)))

    def close(self):
        if getattr(self, "h", None):
            h, self.h = self.h, None
            check(_lib.lib().dfx_reshuffle_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def parse_criteo(ctx, data, is_train=True):
    """Criteo text (whole lines, bytes) parsed on the device (dfx_parse_criteo, replacing
    criteo_parser.h:40-92) -> (RowBlock, needs_host).  needs_host: the chunk holds a form the
    device leaves to the host parser (include/difacto_amd.h lists them); the block is then
    None.  is_train=False is criteo_test (no label column)."""
    from .data import RowBlock
    data = bytes(data)
    max_rows = data.count(b"\n") + 1
    max_nnz = 39 * max_rows
    dev = ctx.device
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev) if data else None
    offs = torch.empty(max_rows + 1, dtype=torch.int64, device=dev)
    ids = torch.empty(max_nnz, dtype=torch.int64, device=dev)
    labels = torch.empty(max_rows, dtype=torch.float32, device=dev)
    stat_dev = torch.empty(4, dtype=torch.int64, device=dev)
    check(_lib.lib().dfx_parse_criteo(ctx.h, _p(text), len(data), int(bool(is_train)), max_rows,
                                      max_nnz, _p(offs), _p(ids), _p(labels), _p(stat_dev)))
    stat = (ctypes.c_int64 * 4)()
    check(_lib.lib().dfx_parse_criteo_wait(ctx.h, _p(stat_dev), stat))
    rows, nnz, needs_host = stat[0], stat[1], bool(stat[2])
    if needs_host:
        return None, True
    return RowBlock(u64(offs[:rows + 1]), u64(ids[:nnz]), None, labels[:rows].cpu().numpy()), False


def parse_libsvm(ctx, data):
    """libsvm text (whole lines, bytes) parsed on the device (dfx_parse_libsvm, replacing the
    host reader's ParseLibSVM) -> (offs, ids, vals, labels, rowflag, stat): numpy arrays (uint64
    offsets and ids, float32 values and labels, uint8 row flags: 1 iff the row holds a value
    whose bits are not 1.0f's) and stat = {rows, nnz, needs_host}.  needs_host: the chunk holds
    a form the device leaves to the host parser (include/difacto_amd.h lists them); the arrays
    are then None."""
    data = bytes(data)
    max_rows = data.count(b"\n") + 1
    max_nnz = data.count(b" ") + data.count(b"\t") + 1  # a feature follows a blank
    dev = ctx.device
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev) if data else None
    offs = torch.empty(max_rows + 1, dtype=torch.int64, device=dev)
    ids = torch.empty(max_nnz, dtype=torch.int64, device=dev)
    vals = torch.empty(max_nnz, dtype=torch.float32, device=dev)
    labels = torch.empty(max_rows, dtype=torch.float32, device=dev)
    rowflag = torch.empty(max_rows, dtype=torch.uint8, device=dev)
    stat_dev = torch.empty(4, dtype=torch.int64, device=dev)
    check(_lib.lib().dfx_parse_libsvm(ctx.h, _p(text), len(data), max_rows, max_nnz, _p(offs),
                                      _p(ids), _p(vals), _p(labels), _p(rowflag), _p(stat_dev)))
    st = (ctypes.c_int64 * 4)()
    check(_lib.lib().dfx_parse_criteo_wait(ctx.h, _p(stat_dev), st))
    rows, nnz = st[0], st[1]
    stat = {"rows": rows, "nnz": nnz, "needs_host": bool(st[2])}
    if stat["needs_host"]:
        return None, None, None, None, None, stat
    return (u64(offs[:rows + 1]), u64(ids[:nnz]), vals[:nnz].cpu().numpy(),
            labels[:rows].cpu().numpy(), rowflag[:rows].cpu().numpy(), stat)


def parse_adfea(ctx, data):
    """adfea text (whole lines, bytes) parsed on the device (dfx_parse_adfea, replacing the host
    reader's ParseAdfea) -> (offs, ids, labels, stat): numpy arrays (uint64 offsets and ids
    (idx << 12) | (gid & 4095), float32 labels) and stat = {rows, nnz, needs_host}.  needs_host:
    the chunk holds a form the device leaves to the host parser (include/difacto_amd.h lists
    them); the arrays are then None."""
    data = bytes(data)
    max_rows = data.count(b"\n") + 1
    max_nnz = data.count(b" ") + data.count(b"\t") + 1  # a feature follows a blank
    dev = ctx.device
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev) if data else None
    offs = torch.empty(max_rows + 1, dtype=torch.int64, device=dev)
    ids = torch.empty(max_nnz, dtype=torch.int64, device=dev)
    labels = torch.empty(max_rows, dtype=torch.float32, device=dev)
    stat_dev = torch.empty(4, dtype=torch.int64, device=dev)
    check(_lib.lib().dfx_parse_adfea(ctx.h, _p(text), len(data), max_rows, max_nnz, _p(offs),
                                     _p(ids), _p(labels), _p(stat_dev)))
    st = (ctypes.c_int64 * 4)()
    check(_lib.lib().dfx_parse_criteo_wait(ctx.h, _p(stat_dev), st))
    rows, nnz = st[0], st[1]
    stat = {"rows": rows, "nnz": nnz, "needs_host": bool(st[2])}
    if stat["needs_host"]:
        return None, None, None, stat
    return u64(offs[:rows + 1]), u64(ids[:nnz]), labels[:rows].cpu().numpy(), stat


def gather_rows_valued(ctx, src, rows=None, begin=0, n=None, dst=None, r0=0):
    """dfx_gather_rows_valued (the host reader's GatherRows with values and row flags) on device
    tensors.  src / dst: dicts of offs, ids (int64 holding the uint64 bits), vals (float32 or
    None), labels (float32), rowflag (uint8 or None); rows: an int32 device tensor holding the
    uint32 row list, or None for the range [begin, begin + n).  Appends at row r0 of dst (the
    caller sizes it) and joins the input stream."""
    if rows is not None:
        n = rows.numel()
    check(_lib.lib().dfx_gather_rows_valued(
        ctx.h, _p(src["offs"]), _p(src["ids"]), _p(src.get("vals")), _p(src["labels"]),
        _p(src.get("rowflag")), _p(rows), int(begin), int(n), _p(dst["offs"]), _p(dst["ids"]),
        _p(dst.get("vals")), _p(dst["labels"]), _p(dst.get("rowflag")), int(r0)))
    stat_dev = torch.zeros(4, dtype=torch.int64, device=ctx.device)
    st = (ctypes.c_int64 * 4)()
    check(_lib.lib().dfx_parse_criteo_wait(ctx.h, _p(stat_dev), st))


def model_write_stats(st, tm):
    """the four counts and the two host times of dfx_store_save_dev / _dump_dev"""
    return {"entries": st[0], "bytes": st[1], "chunks": st[2], "host_chunks": st[3],
            "wait_s": tm[0], "write_s": tm[1]}


def _model_chunk(ctx, text, slot0, nslots, aux, need_reverse, out, cap_bytes):
    stat_dev = torch.empty(4, dtype=torch.int64, device=ctx.device)
    L = _lib.lib()
    if text:
        check(L.dfx_model_format(ctx.h, int(slot0), int(nslots), int(bool(aux)),
                                 int(bool(need_reverse)), _p(out), int(cap_bytes), _p(stat_dev)))
    else:
        check(L.dfx_model_pack(ctx.h, int(slot0), int(nslots), int(bool(aux)), _p(out),
                               int(cap_bytes), _p(stat_dev)))
    ctx.sync()
    return [int(x) for x in stat_dev.cpu().tolist()]


def model_pack(ctx, slot0, nslots, save_aux, out, cap_bytes):
    """dfx_model_pack: SGDUpdater::Save's records of table slots [slot0, slot0 + nslots) into
    the uint8 device tensor out, no byte at or past cap_bytes -> [bytes needed, bytes written,
    entries, 0]; joins the context stream"""
    return _model_chunk(ctx, False, slot0, nslots, save_aux, False, out, cap_bytes)


def model_format(ctx, slot0, nslots, dump_aux, need_reverse, out, cap_bytes):
    """dfx_model_format: SGDUpdater::Dump's lines of those slots -> [bytes needed, bytes
    written, entries, entries the device did not format (then the text is not to be used)]"""
    return _model_chunk(ctx, True, slot0, nslots, dump_aux, need_reverse, out, cap_bytes)


PRED_ROW_BYTES = 26  # a formatted prediction row at most (csrc/fmtg.h kMaxRow)


def format_pred_raw(ctx, label, pred, pred_prob, text, cap_bytes, values=None):
    """dfx_format_pred on device tensors (float32 label / pred, uint8 text, float64 values or
    None) -> [bytes written, rows flagged, first flagged row or -1, bytes the text needs];
    joins the context stream."""
    n = label.numel()
    stat_dev = torch.empty(4, dtype=torch.int64, device=ctx.device)
    check(_lib.lib().dfx_format_pred(ctx.h, _p(label), _p(pred), n, int(bool(pred_prob)),
                                     _p(text), int(cap_bytes), _p(stat_dev), _p(values)))
    ctx.sync()
    return [int(x) for x in stat_dev.cpu().tolist()]


def format_pred(ctx, label, pred, pred_prob=True, values=False):
    """SavePred's lines (sgd_learner.h:72-83), "label\\tvalue\\n" with both fields as %g and
    value = 1 / (1 + exp(-pred)) under pred_prob, formatted on the device (dfx_format_pred)
    -> (text bytes, rows flagged[, the float64 values]).  A flagged row (a field outside
    1e-12 <= |x| < 1e12 and not 0) is missing from the text: have the host write those."""
    label = ctx.tensor(np.asarray(label, np.float32), torch.float32)
    pred = ctx.tensor(np.asarray(pred, np.float32), torch.float32)
    n = label.numel()
    assert pred.numel() == n
    cap = PRED_ROW_BYTES * n
    text = torch.empty(max(cap, 1), dtype=torch.uint8, device=ctx.device)
    vals = torch.empty(max(n, 1), dtype=torch.float64, device=ctx.device) if values else None
    stat = format_pred_raw(ctx, label, pred, pred_prob, text, cap, vals)
    out = bytes(text[:stat[0]].cpu().numpy().tobytes())
    if values:
        return out, stat[1], vals[:n].cpu().numpy()
    return out, stat[1]


class PredText:
    """Two slots of device-formatted prediction text with pinned copies (dfx_predtext_*):
    submit(slot, label, pred) behind the step that wrote pred, take(slot) while the next step
    runs."""

    def __init__(self, ctx, rows_hint=0):
        self.ctx = ctx
        h = ctypes.c_void_p()
        check(_lib.lib().dfx_predtext_create(ctx.h, int(rows_hint), ctypes.byref(h)))
        self.h = h

    def submit(self, slot, label, pred, pred_prob=True):
        """label, pred: float32 device tensors of one length"""
        assert label.numel() == pred.numel()
        check(_lib.lib().dfx_predtext_submit(self.h, int(slot), _p(label), _p(pred),
                                             label.numel(), int(bool(pred_prob))))

    def take(self, slot):
        """-> dict(text=bytes, rows, flagged, first_flagged, label, pred): copies of the slot"""
        o = _lib.PredTextOut()
        check(_lib.lib().dfx_predtext_take(self.h, int(slot), ctypes.byref(o)))

        def arr(p, n):
            if not n:
                return np.zeros(0, np.float32)
            return np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_float)),
                                         shape=(n,)).copy()
        return dict(text=ctypes.string_at(o.text, o.bytes) if o.bytes else b"", rows=o.rows,
                    flagged=o.flagged, first_flagged=o.first_flagged, label=arr(o.label, o.rows),
                    pred=arr(o.pred, o.rows))

    def close(self):
        if getattr(self, "h", None):
            h, self.h = self.h, None
            check(_lib.lib().dfx_predtext_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# main-stream phases of dfx_train_step (the Localizer runs on its own lane; "localize" is
# the part of it the main stream waits for)
PHASES = ("localize", "probe_pull", "feacnt", "forward", "eval_auc", "backward_update", "initv")


def prof_enable(ctx, max_steps, phases=None):
    """time the next max_steps dfx_train_step calls: every phase and the lanes, or only the
    named phases (e.g. ("backward_update",): fewer events, less added latency)"""
    if phases is None:
        check(_lib.lib().dfx_prof_enable(ctx.h, int(max_steps)))
        return
    mask = 0
    for p in phases:
        m = PHASES.index(p)
        mask |= 3 << m
    check(_lib.lib().dfx_prof_enable_marks(ctx.h, int(max_steps), mask))


def prof_read(ctx):
    """-> ({phase: summed ms}, recorded steps, mean U per step)"""
    ms = (ctypes.c_double * 7)()
    n = ctypes.c_int(0)
    mu = ctypes.c_double(0)
    check(_lib.lib().dfx_prof_read(ctx.h, ms, ctypes.byref(n), ctypes.byref(mu)))
    return dict(zip(PHASES, list(ms))), n.value, mu.value


def prof_counts(ctx):
    """per step since the last call (or prof_read): mean unique keys, keys with live V and
    their occurrences; and the batches the bucket Localizer placed by its hot-key map; resets"""
    out = (ctypes.c_double * 4)()
    check(_lib.lib().dfx_prof_counts(ctx.h, out))
    r = dict(zip(("U", "U_V", "occ_V"), list(out)))
    r["lb_map_steps"] = int(out[3])
    return r


def prof_host(ctx):
    """host seconds dfx_train_step calls waited (capacity guard) since the last call, waits"""
    out = (ctypes.c_double * 2)()
    if not hasattr(_lib.lib(), "dfx_prof_host"):  # an older library under A/B (DFX_LIB_PATH)
        return {"wait_s": 0.0, "waits": 0}
    check(_lib.lib().dfx_prof_host(ctx.h, out))
    return {"wait_s": out[0], "waits": int(out[1])}


def prof_lanes(ctx):
    """after prof_read: mean ms per batch of the Localizer lane, its start / end relative to
    the main stream reaching the batch, and the AUC lane"""
    out = (ctypes.c_double * 4)()
    check(_lib.lib().dfx_prof_lanes(ctx.h, out))
    return dict(zip(("loc_ms", "loc_start_rel_ms", "loc_end_rel_ms", "auc_ms"), list(out)))


def progress(ctx, reset=True):
    p = _lib.Progress()
    check(_lib.lib().dfx_progress_read(ctx.h, ctypes.byref(p), int(reset)))
    return {"nrows": p.nrows, "loss": p.loss, "auc": p.auc, "penalty": p.penalty,
            "nnz_w": p.nnz_w}
