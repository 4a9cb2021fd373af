"""Plain numpy reference of what the Localizer hands to the fused step (run on the CPU):
Localizer::Compact (src/data/localizer.cc:11-107) without col — sorted unique keys, segment
starts, per occurrence in stable (key, position) order its row and value — and the chunk plan
of the long segments (csrc/localize.hip chunk_plan).  Integers and bit patterns only: every
comparison against it is exact.  Pinned by tests/test_localizer_ref.py."""
import numpy as np

MAX_INDEX = (1 << 64) - 1
kChunkOcc = 128  # csrc/internal.h: occurrences per chunk of a long segment


def reverse_bytes(x):
    """ReverseBytes (include/difacto/base.h:39-51) of a uint64 array: the bytes reversed, then
    the two nibbles of every byte swapped (the 16 hex digits in reverse order)"""
    x = np.ascontiguousarray(x, dtype=np.uint64).byteswap()
    lo, hi = np.uint64(0x0F0F0F0F0F0F0F0F), np.uint64(0xF0F0F0F0F0F0F0F0)
    return ((x & lo) << np.uint64(4)) | ((x & hi) >> np.uint64(4))


def keys_of(ids, max_index=MAX_INDEX, keys_ready=False):
    """ReverseBytes(id % max_index) (localizer.cc:24); uint64 `%` by 2^64 - 1 sends the all-ones
    id to 0 and keeps every other id (csrc/locbucket.hip lb_key)"""
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    if keys_ready:
        return ids.copy()
    return reverse_bytes(ids % np.uint64(max_index))


def chunk_plan(lens):
    """per segment ceil(len / kChunkOcc) chunks when len > kChunkOcc, else none ->
    (n_chunks, choff = their exclusive prefix sum, chunk_seg = the segment of every chunk)"""
    lens = np.asarray(lens, dtype=np.int64)
    ch = np.where(lens > kChunkOcc, (lens + kChunkOcc - 1) // kChunkOcc, 0)
    choff = (np.cumsum(ch) - ch).astype(np.uint32)
    chunk_seg = np.repeat(np.arange(len(lens), dtype=np.uint32), ch)
    return int(ch.sum()), choff, chunk_seg


def localize(offs, ids, vals=None, max_index=MAX_INDEX, keys_ready=False):
    """-> dict(U, uniq u64[U], cnt i64[U], segstart u32[U + 1], occ_row u32[nnz],
    occ_x u32[nnz] (the values' bit patterns) or None, n_chunks, choff u32[U], chunk_seg)"""
    offs = np.ascontiguousarray(offs, dtype=np.uint64).astype(np.int64)
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    nnz = len(ids)
    B = max(len(offs) - 1, 0)
    assert B == 0 or (offs[0] == 0 and offs[-1] == nnz)
    keys = keys_of(ids, max_index, keys_ready)
    order = np.argsort(keys, kind="stable")
    row_of_position = np.repeat(np.arange(B, dtype=np.uint32), np.diff(offs)) if B else \
        np.zeros(0, np.uint32)
    uniq, cnt = np.unique(keys, return_counts=True)
    segstart = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    n_chunks, choff, chunk_seg = chunk_plan(cnt)
    occ_x = None
    if vals is not None:
        occ_x = np.ascontiguousarray(vals, dtype=np.float32).view(np.uint32)[order]
    return dict(U=len(uniq), uniq=uniq, cnt=cnt.astype(np.int64), segstart=segstart,
                occ_row=row_of_position[order], occ_x=occ_x, n_chunks=n_chunks, choff=choff,
                chunk_seg=chunk_seg)
