// Device batch cache: formed batches kept in HBM so that every epoch after the first replays
// them through dfx_train_step with no reader, no PCIe traffic and no parse.  A reader lives for
// one part of one epoch and seeds its shuffle and its down-sampling afresh (reader.h), so part p
// yields the same batches in every epoch: the copies ARE the later epochs' input.
//
// A list (one per job kind and part) is recorded with begin / append / seal and handed out with
// get.  The arrays of a list live in device blocks of block_bytes that belong to that list alone
// and never move, each array on a 256-byte boundary like an allocation of its own (the step's
// kernels read them with vector loads).  The copies are plain device-to-device hipMemcpyAsync on
// the context's input stream, i.e. behind the producer of the source batch and before that
// stream reuses the source buffers; a replayed batch is ready by the same stream order
// (dfx_train_step's Localizer lane waits for the input stream).  A list that does not fit the
// budget is dropped, never the run.
//
// Optionally (dfx_batchcache_append_loc) a batch's Localizer outputs are kept next to it — they
// depend on the batch and max_index alone — and dfx_train_step_loc (step.hip) replays them with
// no Localizer: uniq[U], segstart[U + 1], occ_row[nnz], occ_x[nnz] or rowof[2 nnz], choff[U] and
// chunk_seg[n_chunks] when the plan holds chunks, and the totals record {U, n_chunks, gate, 0}.
// Exact sizes, so ~16 B/nnz where U ~ nnz (the C3 shape) beside the batch's 8 B/nnz, about three
// times the cache, and ~4 B/nnz on skewed data.  One k_loc_pack launch on the Localizer lane's
// stream copies them, behind the lane and before that stream reuses the parity's buffers.
#include <map>
#include <vector>

#include "internal.h"

namespace {
constexpr int64_t kAlign = 256;
constexpr int64_t kDefaultBlock = (int64_t)64 << 20;
enum ListState { kOpen = 0, kSealed = 1, kDropped = 2 };

struct Alloc {
  void* p = nullptr;
  int64_t bytes = 0;
};

struct List {
  int state = kOpen;
  std::vector<Alloc> allocs;
  std::vector<dfx_batch> batches;
  // per batch, the Localizer outputs kept with it (uniq == NULL: none); what they hold and take;
  // the batch append_loc was last called for; the lane stream the packs were queued on
  std::vector<dfx_loc> locs;
  int64_t n_loc = 0, loc_bytes = 0, loc_tried = -1;
  hipStream_t loc_stream = nullptr;
  bool loc_pending = false;  // packs queued and not joined by the host since
  char* cur = nullptr;   // the unused tail of the list's last block
  int64_t cur_left = 0;
  hipStream_t copy_stream = nullptr;  // the stream its copies were queued on
  bool copied = false;
  bool streams_differ = false;  // copies went to more than one stream (a feeder was rebuilt)
};

inline int64_t round_up(int64_t n) { return (n + kAlign - 1) / kAlign * kAlign; }
}  // namespace

struct dfx_batchcache {
  dfx_ctx* ctx = nullptr;
  int64_t budget = 0, block_bytes = 0, allocated = 0;
  std::map<int64_t, List> lists;
  int64_t open = -1;
  int64_t n_sealed = 0, n_dropped = 0, n_batches = 0;
  int held = 0;  // live reshufflers over lists of this cache (reshuffle.hip)
  // kept Localizer outputs (sealed lists): batches, bytes; steps dfx_train_step_loc served
  int64_t n_loc = 0, loc_bytes = 0, served = 0;
  uint64_t loc_seq = 0;               // the context step whose outputs append_loc took last
  unsigned int* host_rec = nullptr;   // pinned: {U, n_chunks, gate, 0} of the lane just asked
  hipEvent_t ev_rec = nullptr;        // ... written (the lane's stream)
};

using namespace dfx;

namespace {
inline hipStream_t copy_stream(dfx_batchcache* bc) {
  const Context& c = bc->ctx->c;
  return c.has_in_stream ? c.in_stream : c.stream;
}

// one device allocation within the budget -> 1; over the budget or out of device memory -> 0
// (the HIP error cleared); another HIP failure -> -1 with the error set
int alloc_within_budget(dfx_batchcache* bc, List* l, int64_t bytes, void** out) {
  const int rc = batchcache_take(bc, bytes, out);
  if (rc == 1) l->allocs.push_back(Alloc{*out, bytes});
  return rc;
}

// room for an array of `bytes` (> 0) on a 256-byte boundary: the tail of the list's block, a new
// block, or an allocation of its own when it is larger than a block; returns as above
int place(dfx_batchcache* bc, List* l, int64_t bytes, void** out) {
  const int64_t need = round_up(bytes);
  if (need > bc->block_bytes) return alloc_within_budget(bc, l, need, out);
  if (need > l->cur_left) {
    void* blk = nullptr;
    const int rc = alloc_within_budget(bc, l, bc->block_bytes, &blk);
    if (rc != 1) return rc;
    l->cur = static_cast<char*>(blk);
    l->cur_left = bc->block_bytes;
  }
  *out = l->cur;
  l->cur += need;
  l->cur_left -= need;
  return 1;
}

// frees a list's blocks once the copies into them have run
void release(dfx_batchcache* bc, List* l) {
  if (l->copied) {
    // a stream that took earlier copies may be gone (a rebuilt feeder joins and destroys its
    // own): then the device is joined instead
    if (l->streams_differ || l->copy_stream != copy_stream(bc))
      (void)hipDeviceSynchronize();
    else
      (void)hipStreamSynchronize(l->copy_stream);
  }
  // the packs of kept Localizer outputs write into the blocks from the lane's stream (a lane
  // stream that was replaced since was joined when it was, dfx_ctx_set_lane_stream)
  if (l->loc_pending && l->loc_stream == bc->ctx->c.loc_stream)
    (void)hipStreamSynchronize(l->loc_stream);
  l->loc_pending = false;
  l->locs.clear();
  l->locs.shrink_to_fit();
  l->n_loc = 0;
  l->loc_bytes = 0;
  for (const Alloc& a : l->allocs) {
    (void)hipFree(a.p);
    bc->allocated -= a.bytes;
  }
  l->allocs.clear();
  l->allocs.shrink_to_fit();
  l->batches.clear();
  l->batches.shrink_to_fit();
  l->cur = nullptr;
  l->cur_left = 0;
  l->copied = false;
}
}  // namespace

// ---- the cache's side of a reshuffler (internal.h) --------------------------------------------
namespace dfx {
dfx_ctx* batchcache_ctx(dfx_batchcache* bc) { return bc->ctx; }

int batchcache_take(dfx_batchcache* bc, int64_t bytes, void** out) {
  if (bytes > bc->budget - bc->allocated) return 0;
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, (size_t)bytes);
  if (e == hipErrorOutOfMemory) {
    (void)hipGetLastError();
    return 0;
  }
  if (e != hipSuccess) {
    set_error(std::string("batchcache: hipMalloc: ") + hipGetErrorString(e));
    return -1;
  }
  bc->allocated += bytes;
  *out = p;
  return 1;
}

void batchcache_give(dfx_batchcache* bc, void* p, int64_t bytes) {
  (void)hipFree(p);
  bc->allocated -= bytes;
}

void batchcache_hold(dfx_batchcache* bc, int delta) { bc->held += delta; }

int batchcache_sealed(dfx_batchcache* bc, int64_t list, const dfx_batch** batches, int64_t* n) {
  const auto it = bc->lists.find(list);
  DFX_CHECK_ARG(it != bc->lists.end(), "reshuffle_create: no such list");
  List& l = it->second;
  DFX_CHECK_ARG(l.state != kOpen, "reshuffle_create: the list is still open (seal it)");
  DFX_CHECK_ARG(l.state == kSealed, "reshuffle_create: the list was dropped (over budget)");
  // the reshuffler reads the list on the input stream of now: copies queued elsewhere are joined
  if (l.copied && (l.streams_differ || l.copy_stream != copy_stream(bc))) {
    DFX_HIP(hipDeviceSynchronize());
    l.streams_differ = false;
    l.copy_stream = copy_stream(bc);
  }
  *batches = l.batches.data();
  *n = (int64_t)l.batches.size();
  return DFX_OK;
}
}  // namespace dfx

// ---- the Localizer's outputs kept with a batch (dfx_batchcache_append_loc) -------------------
namespace dfx {
// the lane's sizes for the host, after the lane's last kernel: {U, n_chunks, the plan's gate}
// into the pinned record (one thread; the kernel's end makes them visible to the waiting host)
__global__ void k_loc_report(const DevState* __restrict__ ds, unsigned int* __restrict__ rec) {
  rec[0] = ds->u_count;
  rec[1] = ds->totals[1];
  rec[2] = ds->n_init;
  rec[3] = 0u;
}

// One launch copies every kept array of a batch: a by-value table of {source, destination,
// bytes} (bytes a multiple of 4; both ends 16-byte aligned: workspace buffers and 256-byte cache
// slots), moved as 16-byte vectors by a grid-stride loop, the at most three trailing words of an
// array by the grid's first threads.  Plain loads and stores.  Thread 0 also writes the batch's
// totals record {U, n_chunks, gate, 0} from the lane's device state.  Six to eight separate async
// copies would cost the lane's queue microseconds each (profiles/r6/waitbench.txt).
constexpr int kPackMax = 8, kPackNT = 256, kPackGridMax = 2048;
struct PackTab {
  const void* src[kPackMax];
  void* dst[kPackMax];
  int64_t bytes[kPackMax];
  int n;
  const DevState* ds;
  uint4* totals;
};
__global__ __launch_bounds__(kPackNT) void k_loc_pack(PackTab t) {
  const int64_t tid = (int64_t)blockIdx.x * kPackNT + threadIdx.x;
  const int64_t nthr = (int64_t)gridDim.x * kPackNT;
  for (int a = 0; a < t.n; ++a) {
    const uint4* __restrict__ s = static_cast<const uint4*>(t.src[a]);
    uint4* __restrict__ d = static_cast<uint4*>(t.dst[a]);
    const int64_t nv = t.bytes[a] >> 4;
    for (int64_t i = tid; i < nv; i += nthr) d[i] = s[i];
    const int64_t w = nv * 4 + tid;  // a trailing word
    if (w < (t.bytes[a] >> 2))
      static_cast<uint32_t*>(t.dst[a])[w] = static_cast<const uint32_t*>(t.src[a])[w];
  }
  if (tid == 0) *t.totals = make_uint4(t.ds->u_count, t.ds->totals[1], t.ds->n_init, 0u);
}
}  // namespace dfx

extern "C" int dfx_batchcache_create(dfx_ctx* ctx, int64_t budget_bytes, int64_t block_bytes,
                                     dfx_batchcache** out) {
  DFX_CHECK_ARG(ctx && out, "batchcache_create: null argument");
  DFX_CHECK_ARG(budget_bytes >= 0 && block_bytes >= 0, "batchcache_create: negative size");
  dfx_batchcache* bc = new dfx_batchcache();
  bc->ctx = ctx;
  bc->budget = budget_bytes;
  bc->block_bytes = round_up(block_bytes > 0 ? block_bytes : kDefaultBlock);
  *out = bc;
  return DFX_OK;
}

extern "C" int dfx_batchcache_destroy(dfx_batchcache* bc) {
  if (!bc) return DFX_OK;
  DFX_CHECK_ARG(bc->held == 0,
                "batchcache_destroy: a reshuffler of this cache is alive (destroy it first)");
  // batches handed out by get may still be read by queued steps, and copies may be queued
  const int rc = dfx_sync(bc->ctx);
  (void)hipSetDevice(bc->ctx->c.device);
  (void)hipDeviceSynchronize();
  for (auto& kv : bc->lists)
    for (const Alloc& a : kv.second.allocs) (void)hipFree(a.p);
  if (bc->host_rec) (void)hipHostFree(bc->host_rec);
  if (bc->ev_rec) (void)hipEventDestroy(bc->ev_rec);
  delete bc;
  return rc;
}

extern "C" int dfx_batchcache_begin(dfx_batchcache* bc, int64_t list) {
  DFX_CHECK_ARG(bc, "batchcache_begin: null cache");
  DFX_CHECK_ARG(list >= 0, "batchcache_begin: the list id must be >= 0");
  DFX_CHECK_ARG(bc->open < 0, "batchcache_begin: a list is already open (seal it first)");
  DFX_CHECK_ARG(bc->lists.find(list) == bc->lists.end(),
                "batchcache_begin: this list was already recorded (sealed or dropped)");
  bc->lists[list] = List();
  bc->open = list;
  return DFX_OK;
}

extern "C" int dfx_batchcache_append(dfx_batchcache* bc, const dfx_batch* src, int* kept) {
  DFX_CHECK_ARG(bc && src && kept, "batchcache_append: null argument");
  DFX_CHECK_ARG(bc->open >= 0, "batchcache_append: no open list (begin one first)");
  DFX_CHECK_ARG(src->size >= 0 && src->nnz >= 0, "batchcache_append: negative size");
  DFX_CHECK_ARG(src->size == 0 || (src->offset && src->label),
                "batchcache_append: a batch with rows needs offset and label");
  DFX_CHECK_ARG(src->nnz == 0 || src->index, "batchcache_append: a batch with nnz needs index");
  List& l = bc->lists[bc->open];
  *kept = 0;
  if (l.state == kDropped) return DFX_OK;
  DFX_HIP(hipSetDevice(bc->ctx->c.device));
  const int64_t B = src->size, nnz = src->nnz;
  // {source, bytes} of offset, index, value, label, weight; a NULL source stays NULL, a source
  // of no elements keeps a pointer of its own (binary and valued batches take other kernels)
  const void* from[5] = {src->offset, src->index, src->value, src->label, src->weight};
  const int64_t bytes[5] = {(B + 1) * 8, nnz * 8, nnz * 4, B * 4, B * 4};
  void* to[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  for (int a = 0; a < 5; ++a) {
    if (!from[a]) continue;
    const int rc = place(bc, &l, bytes[a] > 0 ? bytes[a] : 1, &to[a]);
    if (rc < 0) return DFX_ERR_HIP;
    if (rc == 0) {  // over the budget: the list is dropped, the run goes on
      release(bc, &l);
      l.state = kDropped;
      bc->n_dropped += 1;
      return DFX_OK;
    }
  }
  const hipStream_t st = copy_stream(bc);
  for (int a = 0; a < 5; ++a)
    if (to[a] && bytes[a] > 0)
      DFX_HIP(hipMemcpyAsync(to[a], from[a], (size_t)bytes[a], hipMemcpyDeviceToDevice, st));
  if (l.copied && l.copy_stream != st) l.streams_differ = true;
  l.copy_stream = st;
  l.copied = true;
  dfx_batch b{};
  b.size = B;
  b.nnz = nnz;
  b.offset = static_cast<const uint64_t*>(to[0]);
  b.index = static_cast<const uint64_t*>(to[1]);
  b.value = static_cast<const float*>(to[2]);
  b.label = static_cast<const float*>(to[3]);
  b.weight = static_cast<const float*>(to[4]);
  l.batches.push_back(b);
  l.locs.push_back(dfx_loc{});
  *kept = 1;
  return DFX_OK;
}

extern "C" int dfx_batchcache_seal(dfx_batchcache* bc, int64_t* n_batches) {
  DFX_CHECK_ARG(bc && n_batches, "batchcache_seal: null argument");
  DFX_CHECK_ARG(bc->open >= 0, "batchcache_seal: no open list");
  List& l = bc->lists[bc->open];
  bc->open = -1;
  if (l.state == kDropped) {
    *n_batches = -1;
    return DFX_OK;
  }
  l.state = kSealed;
  l.cur = nullptr;  // the block's tail stays unused: a block belongs to one list
  l.cur_left = 0;
  bc->n_sealed += 1;
  bc->n_batches += (int64_t)l.batches.size();
  bc->n_loc += l.n_loc;
  bc->loc_bytes += l.loc_bytes;
  *n_batches = (int64_t)l.batches.size();
  return DFX_OK;
}

extern "C" int dfx_batchcache_count(dfx_batchcache* bc, int64_t list, int64_t* n_batches) {
  DFX_CHECK_ARG(bc && n_batches, "batchcache_count: null argument");
  const auto it = bc->lists.find(list);
  if (it == bc->lists.end()) {
    *n_batches = -2;
  } else if (it->second.state == kDropped) {
    *n_batches = -1;
  } else {
    DFX_CHECK_ARG(it->second.state == kSealed, "batchcache_count: the list is still open");
    *n_batches = (int64_t)it->second.batches.size();
  }
  return DFX_OK;
}

extern "C" int dfx_batchcache_get(dfx_batchcache* bc, int64_t list, int64_t i, dfx_batch* out) {
  DFX_CHECK_ARG(bc && out, "batchcache_get: null argument");
  const auto it = bc->lists.find(list);
  DFX_CHECK_ARG(it != bc->lists.end(), "batchcache_get: no such list");
  DFX_CHECK_ARG(it->second.state != kOpen, "batchcache_get: the list is still open (seal it)");
  DFX_CHECK_ARG(it->second.state == kSealed, "batchcache_get: the list was dropped (over budget)");
  DFX_CHECK_ARG(i >= 0 && i < (int64_t)it->second.batches.size(),
                "batchcache_get: batch index out of range");
  *out = it->second.batches[(size_t)i];
  return DFX_OK;
}

extern "C" int dfx_batchcache_stats(dfx_batchcache* bc, int64_t* out) {
  DFX_CHECK_ARG(bc && out, "batchcache_stats: null argument");
  out[0] = bc->n_sealed;
  out[1] = bc->n_dropped;
  out[2] = bc->n_batches;
  out[3] = bc->allocated;
  return DFX_OK;
}

extern "C" int dfx_batchcache_append_loc(dfx_batchcache* bc, int* kept) {
  DFX_CHECK_ARG(bc && kept, "batchcache_append_loc: null argument");
  DFX_CHECK_ARG(bc->open >= 0, "batchcache_append_loc: no open list (begin one first)");
  List& l = bc->lists[bc->open];
  *kept = 0;
  if (l.state == kDropped) return DFX_OK;  // nothing to keep them with
  DFX_CHECK_ARG(!l.batches.empty(), "batchcache_append_loc: nothing appended since begin");
  const int64_t at = (int64_t)l.batches.size() - 1;
  DFX_CHECK_ARG(l.loc_tried != at, "batchcache_append_loc: called twice for one batch");
  Context& c = bc->ctx->c;
  const Context::LastLoc ll = c.last_loc;
  DFX_CHECK_ARG(ll.ran && c.loc_stream,
                "batchcache_append_loc: the context's last step ran no Localizer (no "
                "dfx_train_step yet, or a replayed one)");
  DFX_CHECK_ARG(ll.seq != bc->loc_seq,
                "batchcache_append_loc: that step's outputs were already kept (step the batch "
                "last appended first)");
  const dfx_batch& b = l.batches[(size_t)at];
  DFX_CHECK_ARG(ll.B == b.size && ll.nnz == b.nnz,
                "batchcache_append_loc: the context's last step was of a batch of another B or "
                "nnz than the batch last appended");
  DFX_CHECK_ARG((ll.form != 0) == (b.value != nullptr),
                "batchcache_append_loc: the context's last step was valued and the batch last "
                "appended is not (or the reverse)");
  l.loc_tried = at;
  bc->loc_seq = ll.seq;
  DFX_HIP(hipSetDevice(c.device));
  if (!bc->host_rec) {
    DFX_HIP(hipHostMalloc(reinterpret_cast<void**>(&bc->host_rec), 4 * sizeof(unsigned int),
                          hipHostMallocDefault));
    DFX_HIP(hipEventCreateWithFlags(&bc->ev_rec, hipEventDisableTiming));
  }
  // the lane's sizes: written behind the lane's last kernel, awaited on the lane's stream alone
  // (the lane itself waited for the step two back on the main stream, no more)
  const hipStream_t st = c.loc_stream;
  const DevState* ds = c.bds[ll.k];
  const Workspace& w = c.bws[ll.k];
  hipLaunchKernelGGL(k_loc_report, dim3(1), dim3(1), 0, st, ds, bc->host_rec);
  DFX_HIP(hipGetLastError());
  DFX_HIP(hipEventRecord(bc->ev_rec, st));
  DFX_HIP(hipEventSynchronize(bc->ev_rec));
  const volatile unsigned int* hr = bc->host_rec;
  const int64_t B = b.size, nnz = b.nnz;
  const int64_t U = hr[0], nch = hr[1];
  if (U > (nnz > 0 ? nnz : 0) || nch > max_chunks(nnz)) {
    set_error("batchcache_append_loc: the lane reports U / n_chunks out of range");
    return DFX_ERR_CHECK;
  }
  const bool occ = B > 0 && nnz > 0;  // (an empty batch: the lane wrote U = 0 and segstart[0])
  // {source, bytes} of uniq, segstart, occ_row, occ_x | rowof, choff, chunk_seg; then the totals
  const void* from[kPackMax] = {w.uniq.p, w.segstart.p, w.occ_row.p,
                                ll.form == 2 ? static_cast<const void*>(ll.rowof) : w.occ_x.p,
                                w.flags.p, w.rowtmp.p};
  const int64_t bytes[kPackMax] = {U * 8, (U + 1) * 4, occ ? nnz * 4 : 0,
                                   !occ || ll.form == 0 ? 0 : (ll.form == 2 ? nnz * 8 : nnz * 4),
                                   nch > 0 ? U * 4 : 0, nch > 0 ? nch * 4 : 0};
  const bool want[6] = {true, true, true, ll.form != 0, nch > 0, nch > 0};
  void* to[7] = {};
  // all or nothing: what a refused set already took is given back (nothing was copied there)
  const size_t allocs0 = l.allocs.size();
  char* const cur0 = l.cur;
  const int64_t left0 = l.cur_left;
  int rc = 1;
  for (int a = 0; a < 7 && rc == 1; ++a) {
    if (a < 6 && !want[a]) continue;
    const int64_t n = a < 6 ? bytes[a] : (int64_t)sizeof(uint4);
    rc = place(bc, &l, n > 0 ? n : 1, &to[a]);
  }
  if (rc != 1) {
    while (l.allocs.size() > allocs0) {
      (void)hipFree(l.allocs.back().p);
      bc->allocated -= l.allocs.back().bytes;
      l.allocs.pop_back();
    }
    l.cur = cur0;
    l.cur_left = left0;
    return rc < 0 ? DFX_ERR_HIP : DFX_OK;  // over the budget: the batch stays, without outputs
  }
  PackTab t{};
  int64_t vecs = 0;
  for (int a = 0; a < 6; ++a) {
    if (!to[a] || bytes[a] <= 0) continue;
    t.src[t.n] = from[a];
    t.dst[t.n] = to[a];
    t.bytes[t.n] = bytes[a];
    ++t.n;
    vecs += bytes[a] / 16 + 1;
  }
  t.ds = ds;
  t.totals = static_cast<uint4*>(to[6]);
  // ~4 vectors a thread; a small batch gets one block
  int64_t grid = (vecs + kPackNT * 4 - 1) / (kPackNT * 4);
  grid = grid < 1 ? 1 : (grid > kPackGridMax ? kPackGridMax : grid);
  hipLaunchKernelGGL(k_loc_pack, dim3((unsigned)grid), dim3(kPackNT), 0, st, t);
  DFX_HIP(hipGetLastError());
  l.loc_stream = st;
  l.loc_pending = true;
  dfx_loc o{};
  o.uniq = static_cast<const uint64_t*>(to[0]);
  o.segstart = static_cast<const uint32_t*>(to[1]);
  o.occ_row = static_cast<const uint32_t*>(to[2]);
  o.occ_x = ll.form == 1 ? static_cast<const float*>(to[3]) : nullptr;
  o.rowof = ll.form == 2 ? static_cast<const uint32_t*>(to[3]) : nullptr;
  o.choff = static_cast<const uint32_t*>(to[4]);
  o.chunk_seg = static_cast<const uint32_t*>(to[5]);
  o.totals = static_cast<const uint32_t*>(to[6]);
  o.U = U;
  o.n_chunks = nch;
  o.size = B;
  o.nnz = nnz;
  o.max_index = ll.max_index;
  o.form = ll.form;
  o.served = &bc->served;
  l.locs[(size_t)at] = o;
  l.n_loc += 1;
  // (what the arrays take of the blocks; a fresh block's unused tail counts with the batches)
  for (int a = 0; a < 7; ++a)
    if (to[a]) l.loc_bytes += round_up(a < 6 ? (bytes[a] > 0 ? bytes[a] : 1) : (int64_t)sizeof(uint4));
  *kept = 1;
  return DFX_OK;
}

extern "C" int dfx_batchcache_get_loc(dfx_batchcache* bc, int64_t list, int64_t i, dfx_loc* out) {
  DFX_CHECK_ARG(bc && out, "batchcache_get_loc: null argument");
  const auto it = bc->lists.find(list);
  DFX_CHECK_ARG(it != bc->lists.end(), "batchcache_get_loc: no such list");
  List& l = it->second;
  DFX_CHECK_ARG(l.state != kOpen, "batchcache_get_loc: the list is still open (seal it)");
  DFX_CHECK_ARG(l.state == kSealed, "batchcache_get_loc: the list was dropped (over budget)");
  DFX_CHECK_ARG(i >= 0 && i < (int64_t)l.locs.size(), "batchcache_get_loc: batch index out of range");
  // the packs ran on the lane's stream: joined once, so that any stream may read the arrays (a
  // replayed step needs no join: its lane is queued behind them)
  if (l.loc_pending) {
    if (l.loc_stream == bc->ctx->c.loc_stream) DFX_HIP(hipStreamSynchronize(l.loc_stream));
    l.loc_pending = false;
  }
  *out = l.locs[(size_t)i];
  return DFX_OK;
}

extern "C" int dfx_batchcache_stats_loc(dfx_batchcache* bc, int64_t* out) {
  DFX_CHECK_ARG(bc && out, "batchcache_stats_loc: null argument");
  out[0] = bc->n_loc;
  out[1] = bc->loc_bytes;
  out[2] = bc->served;
  return DFX_OK;
}
