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
  l->allocs.push_back(Alloc{p, bytes});
  bc->allocated += bytes;
  *out = p;
  return 1;
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
  // batches handed out by get may still be read by queued steps, and copies may be queued
  const int rc = dfx_sync(bc->ctx);
  (void)hipSetDevice(bc->ctx->c.device);
  (void)hipDeviceSynchronize();
  for (auto& kv : bc->lists)
    for (const Alloc& a : kv.second.allocs) (void)hipFree(a.p);
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
