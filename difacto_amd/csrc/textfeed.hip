// The text feed: raw text to device batches beside the step (the producer half of
// sgd_learner.cc:289-314).  Pinned text slots, a loader stream, one parsed chunk per slot, a
// shuffle buffer and a ring of device batches; the parsers (dfx_parse_criteo, textparse.hip;
// dfx_parse_libsvm, libsvmparse.hip; dfx_parse_adfea, adfeaparse.hip) and the row gather
// (textparse.hip) do the device work.
//
// The format is fixed at dfx_textfeed_create and every later call takes its behaviour from it,
// through two properties.  Sized (libsvm, adfea): a row has any number of features, so every CSR
// has an nnz capacity of its own: a slot's is the caller's bound for its chunk, the shuffle
// buffer's and a ring entry's grow on demand and keep their contents.  A Criteo feed's rows hold
// at most 39 ids, so rows alone size every array.  Valued (libsvm): every CSR also holds values
// and row flags.  Criteo and adfea feeds are binary: no value arrays, no row flags.
#include <algorithm>
#include <vector>

#include "textscan.h"

using namespace dfx;

namespace {
// what a feed's format means for its arrays (the head comment)
struct FeedFmt {
  bool sized = false;   // an nnz capacity of its own (DFX_TEXT_LIBSVM, DFX_TEXT_ADFEA)
  bool valued = false;  // values and row flags (DFX_TEXT_LIBSVM)
};
struct DevCsr {
  uint64_t *off = nullptr, *idx = nullptr;
  float *lab = nullptr, *val = nullptr;  // val, flag: a valued CSR only
  uint8_t* flag = nullptr;
  int64_t cap = 0, nnz_cap = 0;  // rows, features
  // room for rows / nnz; growth is x1.25 (at least 16 rows; sized: 64 features, else 39 ids for
  // every row of the new capacity).  With st the first keep_rows rows and keep_nnz features are
  // kept: copied on st, in order behind whatever st holds that reads or writes the old arrays,
  // and joined before they are freed.
  int reserve(int64_t rows, int64_t nnz, FeedFmt fmt, hipStream_t st = nullptr,
              int64_t keep_rows = 0, int64_t keep_nnz = 0) {
    const bool valued = fmt.valued;
    if (off && rows <= cap && nnz <= nnz_cap) return DFX_OK;
    const int64_t nr = off && rows <= cap ? cap : std::max<int64_t>(rows + rows / 4, 16);
    const int64_t nn = !fmt.sized              ? nr * kCols
                       : off && nnz <= nnz_cap ? nnz_cap
                                               : std::max<int64_t>(nnz + nnz / 4, 64);
    DevCsr n;
    DFX_HIP(hipMalloc(&n.off, (size_t)(nr + 1) * 8));
    DFX_HIP(hipMalloc(&n.idx, (size_t)nn * 8));
    DFX_HIP(hipMalloc(&n.lab, (size_t)nr * 4));
    if (valued) {
      DFX_HIP(hipMalloc(&n.val, (size_t)nn * 4));
      DFX_HIP(hipMalloc(&n.flag, (size_t)nr));
    }
    n.cap = nr;
    n.nnz_cap = nn;
    if (st && off && (keep_rows || keep_nnz)) {
      const hipMemcpyKind k = hipMemcpyDeviceToDevice;
      DFX_HIP(hipMemcpyAsync(n.off, off, (size_t)(keep_rows + 1) * 8, k, st));
      if (keep_rows) DFX_HIP(hipMemcpyAsync(n.lab, lab, (size_t)keep_rows * 4, k, st));
      if (keep_rows && valued) DFX_HIP(hipMemcpyAsync(n.flag, flag, (size_t)keep_rows, k, st));
      if (keep_nnz) DFX_HIP(hipMemcpyAsync(n.idx, idx, (size_t)keep_nnz * 8, k, st));
      if (keep_nnz && valued) DFX_HIP(hipMemcpyAsync(n.val, val, (size_t)keep_nnz * 4, k, st));
    }
    if (st) DFX_HIP(hipStreamSynchronize(st));
    release();
    *this = n;
    return DFX_OK;
  }
  void release() {
    for (void* p : {(void*)off, (void*)idx, (void*)lab, (void*)val, (void*)flag})
      if (p) (void)hipFree(p);
    *this = DevCsr();
  }
};
}  // namespace

// Two streams: the gathers run on `stream`, the context's input stream, which a step waits
// for; uploads, parses and the copies back run on `up_stream`, so a later chunk's upload does
// not sit between a batch's gathers and its step.  Events order the two: a gather waits for
// its source chunk's `parsed`, a parse into a slot for the slot's last gather (`gathered`).
struct dfx_textfeed {
  dfx_ctx* ctx = nullptr;
  hipStream_t stream = nullptr, up_stream = nullptr;
  DevBuf tp[6];  // the parser's scratch on up_stream
  struct Slot {
    char *h_text = nullptr, *d_text = nullptr;
    int64_t text_cap = 0;
    DevCsr csr;
    uint64_t* h_off = nullptr;  // pinned mirrors of the parsed offsets / labels / row flags
    float* h_lab = nullptr;
    uint8_t* h_flag = nullptr;  // a valued feed only
    int64_t mirror_cap = 0;
    int64_t *d_stat = nullptr, *h_stat = nullptr;
    int64_t rows = 0, nnz = 0;
    hipEvent_t parsed = nullptr, consumed = nullptr, gathered = nullptr;
  };
  struct Ring {
    DevCsr csr;
    uint32_t *h_rows = nullptr, *d_rows = nullptr;  // the batch's row lists, appended
    int64_t used = 0;
    int64_t nnz = 0;  // features gathered into the batch so far (the callers of a sized feed)
    hipEvent_t consumed = nullptr;
  };
  std::vector<Slot> slot;
  std::vector<Ring> ring;
  DevCsr shuf;
  int64_t shuf_nnz = 0;  // features in the shuffle buffer, as Ring::nnz
  int64_t batch_rows = 0;
  int cur = -1;
  int format = DFX_TEXT_CRITEO;
  FeedFmt fmt;
};

extern "C" int dfx_textfeed_destroy(dfx_textfeed* f) {
  if (!f) return DFX_OK;
  if (f->stream) (void)hipStreamSynchronize(f->stream);
  if (f->up_stream) (void)hipStreamSynchronize(f->up_stream);
  (void)hipDeviceSynchronize();
  for (DevBuf& b : f->tp) b.release();
  for (auto& s : f->slot) {
    for (void* p : {(void*)s.h_text, (void*)s.h_off, (void*)s.h_lab, (void*)s.h_stat,
                    (void*)s.h_flag})
      if (p) (void)hipHostFree(p);
    for (void* p : {(void*)s.d_text, (void*)s.d_stat})
      if (p) (void)hipFree(p);
    s.csr.release();
    for (hipEvent_t e : {s.parsed, s.consumed, s.gathered})
      if (e) (void)hipEventDestroy(e);
  }
  for (auto& r : f->ring) {
    r.csr.release();
    if (r.h_rows) (void)hipHostFree(r.h_rows);
    if (r.d_rows) (void)hipFree(r.d_rows);
    if (r.consumed) (void)hipEventDestroy(r.consumed);
  }
  f->shuf.release();
  if (f->ctx) (void)dfx_ctx_set_input_stream(f->ctx, nullptr);
  if (f->stream) (void)hipStreamDestroy(f->stream);
  if (f->up_stream) (void)hipStreamDestroy(f->up_stream);
  delete f;
  return DFX_OK;
}

extern "C" int dfx_textfeed_create(dfx_ctx* ctx, int nslots, int nring, int64_t batch_rows,
                                   int64_t shuf_rows, int format, dfx_textfeed** out) {
  DFX_CHECK_ARG(ctx && out && nslots >= 2 && nslots <= 8 && nring >= 2 && nring <= 8 &&
                    batch_rows > 0 && batch_rows < (1ll << 31) && shuf_rows >= 0 &&
                    (format == DFX_TEXT_CRITEO || format == DFX_TEXT_LIBSVM ||
                     format == DFX_TEXT_ADFEA),
                "textfeed_create: bad argument");
  DFX_HIP(hipSetDevice(ctx->c.device));
  dfx_textfeed* f = new dfx_textfeed();
  f->ctx = ctx;
  f->format = format;
  f->fmt.sized = format != DFX_TEXT_CRITEO;
  f->fmt.valued = format == DFX_TEXT_LIBSVM;
  f->batch_rows = batch_rows;
  f->slot.resize((size_t)nslots);
  f->ring.resize((size_t)nring);
  auto fail = [&](const char* what) {
    set_error(std::string("textfeed_create: ") + what);
    dfx_textfeed_destroy(f);
    return DFX_ERR_HIP;
  };
  if (hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess ||
      hipStreamCreateWithFlags(&f->up_stream, hipStreamNonBlocking) != hipSuccess)
    return fail("stream");
  for (auto& s : f->slot) {
    if (hipEventCreateWithFlags(&s.parsed, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s.gathered, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s.consumed, hipEventDisableTiming) != hipSuccess)
      return fail("event");
    if (hipMalloc(&s.d_stat, 4 * sizeof(int64_t)) != hipSuccess ||
        hipHostMalloc(&s.h_stat, 4 * sizeof(int64_t), hipHostMallocDefault) != hipSuccess)
      return fail("counters");
  }
  for (auto& r : f->ring) {
    if (hipEventCreateWithFlags(&r.consumed, hipEventDisableTiming) != hipSuccess)
      return fail("event");
    if (r.csr.reserve(batch_rows, batch_rows * kCols, f->fmt) != DFX_OK)
      return fail("device batch");
    if (hipHostMalloc(&r.h_rows, (size_t)batch_rows * 4, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&r.d_rows, (size_t)batch_rows * 4) != hipSuccess)
      return fail("row lists");
  }
  if (shuf_rows > 0 && f->shuf.reserve(shuf_rows, shuf_rows * kCols, f->fmt) != DFX_OK)
    return fail("shuffle buffer");
  int rc = dfx_ctx_set_input_stream(ctx, f->stream);
  if (rc != DFX_OK) {
    dfx_textfeed_destroy(f);
    return rc;
  }
  *out = f;
  return DFX_OK;
}

#define DFX_FEED_SLOT(f, s, what) \
  DFX_CHECK_ARG((f) && (s) >= 0 && (s) < (int)(f)->slot.size(), what ": bad slot")
// what only a valued feed has: its values, a batch handed out with them
#define DFX_FEED_VALUED(f, asked, what)                                                    \
  do {                                                                                     \
    DFX_CHECK_ARG(!(asked) || (f)->format != DFX_TEXT_CRITEO,                              \
                  what ": a Criteo feed has no values");                                   \
    DFX_CHECK_ARG(!(asked) || (f)->fmt.valued, what ": an adfea feed has no values");      \
  } while (0)
// what only a sized feed takes: the features a gather appends
#define DFX_FEED_SIZED(f, asked, what) \
  DFX_CHECK_ARG(!(asked) || (f)->fmt.sized, what ": a Criteo feed has no values")

extern "C" int dfx_textfeed_text(dfx_textfeed* f, int slot, int64_t bytes, char** pinned) {
  DFX_FEED_SLOT(f, slot, "textfeed_text");
  DFX_CHECK_ARG(pinned && bytes >= 0 && bytes < (1ll << 31), "textfeed_text: bad argument");
  DFX_HIP(hipSetDevice(f->ctx->c.device));
  auto& s = f->slot[slot];
  if (bytes > s.text_cap || !s.h_text) {
    if (s.h_text) DFX_HIP(hipHostFree(s.h_text));
    if (s.d_text) DFX_HIP(hipFree(s.d_text));
    s.h_text = s.d_text = nullptr;
    s.text_cap = 0;
    const int64_t cap = std::max<int64_t>(bytes + bytes / 8, 4096);
    DFX_HIP(hipHostMalloc(&s.h_text, (size_t)cap, hipHostMallocDefault));
    DFX_HIP(hipMalloc(&s.d_text, (size_t)cap));
    s.text_cap = cap;
  }
  *pinned = s.h_text;
  return DFX_OK;
}

// room for a chunk in the slot's CSR and in its pinned mirrors, which follow the CSR's rows
static int feed_slot(dfx_textfeed* f, dfx_textfeed::Slot& s, int64_t rows, int64_t nnz) {
  DFX_TRY(s.csr.reserve(rows, nnz, f->fmt));
  if (s.csr.cap > s.mirror_cap || !s.h_off) {
    for (void* p : {(void*)s.h_off, (void*)s.h_lab, (void*)s.h_flag})
      if (p) DFX_HIP(hipHostFree(p));
    s.h_off = nullptr;
    s.h_lab = nullptr;
    s.h_flag = nullptr;
    s.mirror_cap = 0;
    DFX_HIP(hipHostMalloc(&s.h_off, (size_t)(s.csr.cap + 1) * 8, hipHostMallocDefault));
    DFX_HIP(hipHostMalloc(&s.h_lab, (size_t)s.csr.cap * 4, hipHostMallocDefault));
    if (f->fmt.valued)
      DFX_HIP(hipHostMalloc(&s.h_flag, (size_t)s.csr.cap, hipHostMallocDefault));
    s.mirror_cap = s.csr.cap;
  }
  return DFX_OK;
}

extern "C" int dfx_textfeed_submit(dfx_textfeed* f, int slot, int64_t nbytes, int is_train,
                                   int64_t max_rows, int64_t max_nnz) {
  DFX_FEED_SLOT(f, slot, "textfeed_submit");
  auto& s = f->slot[slot];
  DFX_CHECK_ARG(nbytes >= 0 && nbytes <= s.text_cap && max_rows >= 0 && max_nnz >= 0,
                "textfeed_submit: more bytes than dfx_textfeed_text reserved");
  DFX_HIP(hipSetDevice(f->ctx->c.device));
  if (!f->fmt.sized) max_nnz = max_rows * kCols;
  DFX_TRY(feed_slot(f, s, max_rows, max_nnz));
  hipStream_t up = f->up_stream;
  // the gathers that read the slot's previous chunk, and a step that took it as its batch,
  // must be past the device
  DFX_HIP(hipStreamWaitEvent(up, s.gathered, 0));
  DFX_HIP(hipStreamWaitEvent(up, s.consumed, 0));
  if (nbytes)
    DFX_HIP(hipMemcpyAsync(s.d_text, s.h_text, (size_t)nbytes, hipMemcpyHostToDevice, up));
  const TpScratch ws{&f->tp[0], &f->tp[1], &f->tp[2], &f->tp[3], &f->tp[4], &f->tp[5]};
  if (f->format == DFX_TEXT_LIBSVM)
    DFX_TRY(parse_libsvm_on(ws, up, s.d_text, nbytes, max_rows, max_nnz, s.csr.off, s.csr.idx,
                            s.csr.val, s.csr.lab, s.csr.flag, s.d_stat));
  else if (f->format == DFX_TEXT_ADFEA)
    DFX_TRY(parse_adfea_on(ws, up, s.d_text, nbytes, max_rows, max_nnz, s.csr.off, s.csr.idx,
                           s.csr.lab, s.d_stat));
  else
    DFX_TRY(parse_criteo_on(ws, up, s.d_text, nbytes, is_train, max_rows, max_nnz, s.csr.off,
                            s.csr.idx, s.csr.lab, s.d_stat));
  // offsets, labels and row flags (12 or 13 bytes a row) for the batch planner, the counts
  DFX_HIP(hipMemcpyAsync(s.h_off, s.csr.off, (size_t)(max_rows + 1) * 8, hipMemcpyDeviceToHost,
                         up));
  if (max_rows)
    DFX_HIP(hipMemcpyAsync(s.h_lab, s.csr.lab, (size_t)max_rows * 4, hipMemcpyDeviceToHost, up));
  if (max_rows && f->fmt.valued)
    DFX_HIP(hipMemcpyAsync(s.h_flag, s.csr.flag, (size_t)max_rows, hipMemcpyDeviceToHost, up));
  DFX_HIP(hipMemcpyAsync(s.h_stat, s.d_stat, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, up));
  DFX_HIP(hipEventRecord(s.parsed, up));
  return DFX_OK;
}

extern "C" int dfx_textfeed_wait(dfx_textfeed* f, int slot, int64_t* stat,
                                 const uint64_t** offset_host, const float** label_host,
                                 const uint8_t** rowflag_host) {
  DFX_FEED_SLOT(f, slot, "textfeed_wait");
  DFX_CHECK_ARG(stat, "textfeed_wait: null argument");
  auto& s = f->slot[slot];
  DFX_HIP(hipEventSynchronize(s.parsed));
  for (int i = 0; i < 4; ++i) stat[i] = s.h_stat[i];
  s.rows = stat[0];
  s.nnz = stat[1];
  if (offset_host) *offset_host = s.h_off;
  if (label_host) *label_host = s.h_lab;
  if (rowflag_host) *rowflag_host = s.h_flag;
  return capacity_status(stat);
}

extern "C" int dfx_textfeed_upload(dfx_textfeed* f, int slot, int64_t rows, int64_t nnz,
                                   const uint64_t* offset, const uint64_t* index,
                                   const float* value, const float* label,
                                   const uint8_t** rowflag_host) {
  DFX_FEED_SLOT(f, slot, "textfeed_upload");
  DFX_FEED_VALUED(f, value, "textfeed_upload");
  DFX_CHECK_ARG(rows >= 0 && nnz >= 0 && offset && (index || !nnz) && (label || !rows) &&
                    (value || !nnz || !f->fmt.valued) && (f->fmt.sized || nnz <= rows * kCols) &&
                    offset[0] == 0 && (int64_t)offset[rows] == nnz,
                "textfeed_upload: bad argument");
  auto& s = f->slot[slot];
  DFX_HIP(hipSetDevice(f->ctx->c.device));
  hipStream_t up = f->up_stream;
  if (rows > s.csr.cap || nnz > s.csr.nnz_cap || !s.h_off) {
    DFX_HIP(hipStreamSynchronize(up));
    DFX_TRY(feed_slot(f, s, rows, f->fmt.sized ? nnz : rows * kCols));
  }
  // after the slot's own parse (dfx_textfeed_wait joined it); the gathers wait for `parsed`
  std::copy(offset, offset + rows + 1, s.h_off);
  if (rows) std::copy(label, label + rows, s.h_lab);
  // the row flags: a value that is not 1.0f
  for (int64_t r = 0; r < rows && f->fmt.valued; ++r) {
    uint8_t fl = 0;
    for (uint64_t k = offset[r]; k < offset[r + 1] && !fl; ++k) fl = value[k] != 1.f;
    s.h_flag[r] = fl;
  }
  DFX_HIP(hipMemcpyAsync(s.csr.off, s.h_off, (size_t)(rows + 1) * 8, hipMemcpyHostToDevice, up));
  if (nnz) DFX_HIP(hipMemcpyAsync(s.csr.idx, index, (size_t)nnz * 8, hipMemcpyHostToDevice, up));
  if (nnz && f->fmt.valued)
    DFX_HIP(hipMemcpyAsync(s.csr.val, value, (size_t)nnz * 4, hipMemcpyHostToDevice, up));
  if (rows)
    DFX_HIP(hipMemcpyAsync(s.csr.lab, s.h_lab, (size_t)rows * 4, hipMemcpyHostToDevice, up));
  if (rows && f->fmt.valued)
    DFX_HIP(hipMemcpyAsync(s.csr.flag, s.h_flag, (size_t)rows, hipMemcpyHostToDevice, up));
  // the caller's arrays are pageable: staged before the calls return
  DFX_HIP(hipEventRecord(s.parsed, up));
  s.rows = rows;
  s.nnz = nnz;
  if (rowflag_host) *rowflag_host = s.h_flag;
  return DFX_OK;
}

extern "C" int dfx_textfeed_batch_begin(dfx_textfeed* f) {
  DFX_CHECK_ARG(f, "textfeed_batch_begin: null argument");
  f->cur = (f->cur + 1) % (int)f->ring.size();
  auto& r = f->ring[f->cur];
  // the step that consumed this ring entry a round ago must be past the device (its row lists
  // are pinned host memory the gathers' copies read)
  DFX_HIP(hipEventSynchronize(r.consumed));
  r.used = 0;
  return DFX_OK;
}

extern "C" int dfx_textfeed_gather(dfx_textfeed* f, int src, int to_batch, const uint32_t* rows,
                                   int64_t begin, int64_t n, int64_t r0, int64_t nnz) {
  DFX_CHECK_ARG(f && src >= -1 && src < (int)f->slot.size() && n >= 0 && r0 >= 0 && begin >= 0 &&
                    nnz >= 0,
                "textfeed_gather: bad argument");
  DFX_CHECK_ARG(!to_batch || f->cur >= 0, "textfeed_gather: no batch begun");
  DFX_CHECK_ARG(src >= 0 || to_batch, "textfeed_gather: the shuffle buffer onto itself");
  DFX_FEED_SIZED(f, nnz, "textfeed_gather");
  if (n == 0) return DFX_OK;
  DFX_HIP(hipSetDevice(f->ctx->c.device));
  const DevCsr& S = src >= 0 ? f->slot[src].csr : f->shuf;
  DevCsr& D = to_batch ? f->ring[f->cur].csr : f->shuf;
  int64_t& used = to_batch ? f->ring[f->cur].nnz : f->shuf_nnz;
  DFX_CHECK_ARG(r0 + n <= D.cap, "textfeed_gather: more rows than the destination holds");
  if (r0 == 0) used = 0;
  // a sized destination grows by the caller's nnz; the copies of a growth run on the gathers'
  // stream: behind the gathers that filled the old arrays and, for the shuffle buffer, behind
  // the gathers that read them.  A Criteo destination holds 39 ids a row from the start: nnz
  // is 0 and this returns at once, nothing queued.
  DFX_TRY(D.reserve(D.cap, used + nnz, f->fmt, f->stream, r0, used));
  used += nnz;
  const uint32_t* rows_dev = nullptr;
  if (rows) {
    DFX_CHECK_ARG(to_batch, "textfeed_gather: row lists go to the batch");
    auto& r = f->ring[f->cur];
    DFX_CHECK_ARG(r.used + n <= f->batch_rows, "textfeed_gather: row lists past the batch size");
    std::copy(rows, rows + n, r.h_rows + r.used);
    DFX_HIP(hipMemcpyAsync(r.d_rows + r.used, r.h_rows + r.used, (size_t)n * 4,
                           hipMemcpyHostToDevice, f->stream));
    rows_dev = r.d_rows + r.used;
    r.used += n;
  }
  if (src >= 0) DFX_HIP(hipStreamWaitEvent(f->stream, f->slot[src].parsed, 0));
  // a sized feed: the valued gather, with no value and flag arrays on either side when binary
  if (f->fmt.sized)
    DFX_TRY(gather_rows_on<true>(&f->ctx->c, f->stream, S.off, S.idx, S.lab, rows_dev, begin, n,
                                 D.off, D.idx, D.lab, r0, S.val, D.val, S.flag, D.flag));
  else
    DFX_TRY(gather_rows_on<false>(&f->ctx->c, f->stream, S.off, S.idx, S.lab, rows_dev, begin, n,
                                  D.off, D.idx, D.lab, r0));
  if (src >= 0) DFX_HIP(hipEventRecord(f->slot[src].gathered, f->stream));
  return DFX_OK;
}

static void feed_batch(const DevCsr& c, int64_t rows, int64_t nnz, int valued, dfx_batch* out) {
  *out = dfx_batch{};
  out->size = rows;
  out->nnz = nnz;
  out->offset = c.off;
  out->index = c.idx;
  out->value = valued ? c.val : nullptr;
  out->label = c.lab;
}

extern "C" int dfx_textfeed_batch_end(dfx_textfeed* f, int64_t rows, int64_t nnz, int valued,
                                      dfx_batch* out) {
  DFX_CHECK_ARG(f && out && rows >= 0 && nnz >= 0, "textfeed_batch_end: bad argument");
  DFX_FEED_VALUED(f, valued, "textfeed_batch_end");
  DFX_CHECK_ARG(f->cur >= 0, "textfeed_batch_end: no batch begun");
  feed_batch(f->ring[f->cur].csr, rows, nnz, valued, out);
  return DFX_OK;
}

extern "C" int dfx_textfeed_consumed(dfx_textfeed* f) { return dfx_textfeed_consumed_back(f, 0); }

// Late marking (as dfx_feeder_consumed_back): a store that defers a step queues the last reader
// of a batch calls after it was handed out.  An event wait sees only the last record made
// before the wait is issued, so the entry begun `back` begins ago is marked here, by the call
// that follows the one that queued its last reader, and before dfx_textfeed_batch_begin comes
// round to it (the caller's ring is deeper than its deferral).  The readers run on the context
// stream (the sharded stores' fwd_bwd / combine), so that is where the event goes.
extern "C" int dfx_textfeed_consumed_back(dfx_textfeed* f, int back) {
  const int n = f ? (int)f->ring.size() : 0;
  DFX_CHECK_ARG(f && f->cur >= 0, "textfeed_consumed: no batch begun");
  DFX_CHECK_ARG(back >= 0 && back < n, "textfeed_consumed_back: back outside the ring");
  DFX_HIP(hipEventRecord(f->ring[(f->cur - back + n) % n].consumed, f->ctx->c.stream));
  return DFX_OK;
}

extern "C" int dfx_textfeed_counts(dfx_textfeed* f, int* nslots, int* nring, int* cur) {
  DFX_CHECK_ARG(f, "textfeed_counts: null argument");
  if (nslots) *nslots = (int)f->slot.size();
  if (nring) *nring = (int)f->ring.size();
  if (cur) *cur = f->cur;
  return DFX_OK;
}

extern "C" int dfx_textfeed_slot_batch(dfx_textfeed* f, int slot, int valued, dfx_batch* out) {
  DFX_FEED_SLOT(f, slot, "textfeed_slot_batch");
  DFX_CHECK_ARG(out, "textfeed_slot_batch: null argument");
  DFX_FEED_VALUED(f, valued, "textfeed_slot_batch");
  const auto& s = f->slot[slot];
  // the step waits for the input stream, the input stream for the chunk's parse
  DFX_HIP(hipStreamWaitEvent(f->stream, s.parsed, 0));
  feed_batch(s.csr, s.rows, s.nnz, valued, out);
  return DFX_OK;
}

extern "C" int dfx_textfeed_slot_consumed(dfx_textfeed* f, int slot) {
  DFX_FEED_SLOT(f, slot, "textfeed_slot_consumed");
  DFX_HIP(hipEventRecord(f->slot[slot].consumed, f->ctx->c.stream));
  return DFX_OK;
}
