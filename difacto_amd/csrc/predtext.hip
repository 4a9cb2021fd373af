// Prediction rows as text on the device: SavePred's "label\tvalue\n" lines
// (src/sgd/sgd_learner.h:72-83) formatted by csrc/fmtg.h, one lane per row, and packed into one
// contiguous text by the plain multi-launch scan of csrc/textscan.h (tile totals, one block over
// the totals, the apply folded into the write pass) - nothing spins, looks back or waits on
// another block, and every per-row loop is bounded by the record's 32 bytes.
//
//   k_pt_format   a row -> its 32-byte record (the text, zero filled, byte 31 the length; a
//                 flagged row has length 0 and is counted), the double it printed, and the
//                 tile's byte total
//   k_scan_totals the tiles' exclusive offsets and the text's size
//   k_pt_write    a tile's records laid end to end in LDS at the destination's 16-byte phase,
//                 stored as 16-byte pieces; only the tile's two ragged ends go by bytes; no byte
//                 at or past the capacity
//
// dfx_predtext: two slots of that with pinned copies, so the host writes batch t's text while
// the step of batch t + 1 runs.
#include <algorithm>

#include "fmtg.h"
#include "textscan.h"

namespace {

using dfx_fmtg::kMaxRow;
using dfx_fmtg::kRecBytes;

constexpr int64_t kPtMaxRows = (int64_t)1 << 26;  // 32 bytes a row in 32-bit offsets
// LDS of the write pass: a tile's text behind up to 15 bytes of phase, in 16-byte pieces
constexpr int kPtStage16 = (15 + kNT * kMaxRow + 15) / 16;

static __constant__ const uint64_t kPtExp2fTab[32] = DFX_EXP2F_TAB;

__global__ void k_pt_init(long long* stat) {
  stat[0] = 0;
  stat[1] = 0;
  stat[2] = -1;  // as unsigned: above every row (atomicMin)
  stat[3] = 0;
}

__global__ __launch_bounds__(kNT) void k_pt_format(const float* __restrict__ label,
                                                   const float* __restrict__ pred, uint32_t n,
                                                   int pred_prob, uint4* __restrict__ rec,
                                                   uint32_t* __restrict__ tot,
                                                   unsigned long long* stat,
                                                   double* __restrict__ value_out) {
  __shared__ uint4 srec[kNT * 2];
  __shared__ uint32_t lds[2 * kNT];
  const uint32_t t = threadIdx.x, i = blockIdx.x * kNT + t;
  uint32_t len = 0;
  if (i < n) {
    srec[2 * t] = make_uint4(0, 0, 0, 0);
    srec[2 * t + 1] = make_uint4(0, 0, 0, 0);
    const double v =
        dfx_fmtg::pred_value(pred[i], pred_prob, [](int k) { return kPtExp2fTab[k]; });
    if (value_out) value_out[i] = v;
    char* r = reinterpret_cast<char*>(&srec[2 * t]);
    const int L = dfx_fmtg::fmt_row(label[i], v, r);
    if (L < 0) {
      atomicAdd(&stat[1], 1ull);
      atomicMin(&stat[2], (unsigned long long)i);
    } else {
      len = (uint32_t)L;
    }
    r[kRecBytes - 1] = (char)len;
    rec[2 * (size_t)i] = srec[2 * t];
    rec[2 * (size_t)i + 1] = srec[2 * t + 1];
  }
  uint32_t incl, excl, total;
  block_scan<AddOp, kNT>(len, lds, &incl, &excl, &total);
  if (t == 0) tot[blockIdx.x] = total;
}

__global__ __launch_bounds__(kNT) void k_pt_write(const uint4* __restrict__ rec, uint32_t n,
                                                  const uint32_t* __restrict__ tot,
                                                  const uint32_t* __restrict__ total_dev,
                                                  char* __restrict__ text, uint64_t cap,
                                                  long long* __restrict__ stat) {
  __shared__ uint4 srec[kNT * 2];
  __shared__ uint4 stage16[kPtStage16];
  __shared__ uint32_t lds[2 * kNT];
  const uint32_t t = threadIdx.x, i = blockIdx.x * kNT + t;
  const char* mine = reinterpret_cast<const char*>(&srec[2 * t]);
  uint32_t len = 0;
  if (i < n) {
    srec[2 * t] = rec[2 * (size_t)i];
    srec[2 * t + 1] = rec[2 * (size_t)i + 1];
    len = (uint8_t)mine[kRecBytes - 1];
    if (len > (uint32_t)kMaxRow) len = kMaxRow;  // (k_pt_format writes no longer row)
  }
  uint32_t incl, excl, btotal;
  block_scan<AddOp, kNT>(len, lds, &incl, &excl, &btotal);
  const uint64_t base = tot[blockIdx.x];  // the tile's first byte in the text
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(text + base) & 15u);
  char* stage = reinterpret_cast<char*>(stage16);
  for (uint32_t j = 0; j < (uint32_t)kRecBytes; ++j)
    if (j < len) stage[mis + excl + j] = mine[j];
  __syncthreads();
  // stage[mis, end) is text[base, base + btotal); piece p is stage[16 p, 16 p + 16), aligned in
  // the text too
  const uint32_t end = mis + btotal, np = (end + 15u) / 16u;  // np <= kPtStage16 < 2 kNT
  for (uint32_t p = t; p < np; p += kNT) {
    const uint32_t s0 = 16u * p;
    const int64_t g0 = (int64_t)base - (int64_t)mis + (int64_t)s0;
    if (s0 >= mis && s0 + 16u <= end && (uint64_t)(g0 + 16) <= cap) {
      *reinterpret_cast<uint4*>(text + g0) = stage16[p];
    } else {
      for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t s = s0 + j;
        if (s >= mis && s < end && (uint64_t)(g0 + (int64_t)j) < cap) text[g0 + (int64_t)j] = stage[s];
      }
    }
  }
  if (blockIdx.x == 0 && t == 0) {
    const uint64_t need = *total_dev;
    stat[3] = (long long)need;
    stat[0] = (long long)(need < cap ? need : cap);
  }
}

int format_pred_on(Context* c, hipStream_t st, const float* label, const float* pred, int64_t n,
                   int pred_prob, char* text, int64_t cap, int64_t* stat_dev, double* value_out) {
  DFX_CHECK_ARG(stat_dev, "format_pred: null stat_dev");
  DFX_CHECK_ARG(n >= 0 && n <= kPtMaxRows, "format_pred: n outside [0, 2^26]");
  DFX_CHECK_ARG(cap >= 0, "format_pred: cap_bytes < 0");
  DFX_CHECK_ARG(n == 0 || (label && pred && text), "format_pred: null label, pred or text");
  const unsigned nb = blocks_for((uint64_t)n, kNT);
  if (n > 0) {
    DFX_TRY(c->pt_rec.ensure((size_t)n * kRecBytes));
    DFX_TRY(c->pt_tot.ensure(((size_t)nb + 1) * sizeof(uint32_t)));
  }
  long long* stat = reinterpret_cast<long long*>(stat_dev);
  hipLaunchKernelGGL(k_pt_init, dim3(1), dim3(1), 0, st, stat);
  if (n > 0) {
    uint4* rec = c->pt_rec.as<uint4>();
    uint32_t* tot = c->pt_tot.as<uint32_t>();
    hipLaunchKernelGGL(k_pt_format, dim3(nb), dim3(kNT), 0, st, label, pred, (uint32_t)n,
                       pred_prob ? 1 : 0, rec, tot, reinterpret_cast<unsigned long long*>(stat),
                       value_out);
    hipLaunchKernelGGL((k_scan_totals<AddOp>), dim3(1), dim3(1024), 0, st, tot,
                       (const uint32_t*)nullptr, (uint32_t)n, (uint32_t)kNT, tot + nb);
    hipLaunchKernelGGL(k_pt_write, dim3(nb), dim3(kNT), 0, st, (const uint4*)rec, (uint32_t)n,
                       (const uint32_t*)tot, (const uint32_t*)(tot + nb), text, (uint64_t)cap,
                       stat);
  }
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

}  // namespace

extern "C" int dfx_format_pred(dfx_ctx* ctx, const float* label_dev, const float* pred_dev,
                               int64_t n, int pred_prob, char* text_dev, int64_t cap_bytes,
                               int64_t* stat_dev, double* value_out) {
  DFX_CHECK_ARG(ctx, "null ctx");
  DFX_HIP(hipSetDevice(ctx->c.device));
  return format_pred_on(&ctx->c, ctx->c.stream, label_dev, pred_dev, n, pred_prob, text_dev,
                        cap_bytes, stat_dev, value_out);
}

// ---- the two-slot object --------------------------------------------------------------------
struct dfx_predtext {
  dfx_ctx* ctx = nullptr;
  struct Slot {
    char* text_dev = nullptr;
    char* text_host = nullptr;   // pinned
    float* lp_host = nullptr;    // pinned: cap_rows labels, then cap_rows predictions
    int64_t* stat_dev = nullptr;
    int64_t* stat_host = nullptr;  // pinned
    hipEvent_t ev = nullptr;
    int64_t cap_rows = 0, n = 0;
    bool pending = false;
  } s[2];
};

namespace {

void pt_slot_free(dfx_predtext::Slot& s) {
  if (s.text_dev) (void)hipFree(s.text_dev);
  if (s.text_host) (void)hipHostFree(s.text_host);
  if (s.lp_host) (void)hipHostFree(s.lp_host);
  s.text_dev = s.text_host = nullptr;
  s.lp_host = nullptr;
  s.cap_rows = 0;
}

// the slot's three row-sized buffers for at least `rows` rows (the slot is not pending: nothing
// queued reads them)
int pt_slot_reserve(dfx_predtext::Slot& s, int64_t rows) {
  if (rows <= s.cap_rows) return DFX_OK;
  pt_slot_free(s);
  const size_t tb = (size_t)rows * kMaxRow;
  DFX_HIP(hipMalloc(reinterpret_cast<void**>(&s.text_dev), tb));
  DFX_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.text_host), tb, hipHostMallocDefault));
  DFX_HIP(hipHostMalloc(reinterpret_cast<void**>(&s.lp_host), (size_t)rows * 8,
                        hipHostMallocDefault));
  s.cap_rows = rows;
  return DFX_OK;
}

void pt_release(dfx_predtext* pt) {
  for (auto& s : pt->s) {
    pt_slot_free(s);
    if (s.stat_dev) (void)hipFree(s.stat_dev);
    if (s.stat_host) (void)hipHostFree(s.stat_host);
    if (s.ev) (void)hipEventDestroy(s.ev);
  }
  delete pt;
}

}  // namespace

extern "C" int dfx_predtext_create(dfx_ctx* ctx, int64_t rows_hint, dfx_predtext** out) {
  DFX_CHECK_ARG(ctx && out, "predtext_create: null argument");
  DFX_CHECK_ARG(rows_hint >= 0 && rows_hint <= kPtMaxRows, "predtext_create: rows_hint");
  DFX_HIP(hipSetDevice(ctx->c.device));
  *out = nullptr;
  dfx_predtext* pt = new dfx_predtext;
  pt->ctx = ctx;
  auto fail = [&](int rc) {
    pt_release(pt);
    return rc;
  };
  for (auto& s : pt->s) {
    if (hipMalloc(reinterpret_cast<void**>(&s.stat_dev), 4 * sizeof(int64_t)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&s.stat_host), 4 * sizeof(int64_t),
                      hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&s.ev, hipEventDisableTiming) != hipSuccess) {
      set_error("predtext_create: a slot's status words or event");
      return fail(DFX_ERR_HIP);
    }
    const int rc = pt_slot_reserve(s, std::max<int64_t>(rows_hint, 1));
    if (rc != DFX_OK) return fail(rc);
  }
  *out = pt;
  return DFX_OK;
}

extern "C" int dfx_predtext_submit(dfx_predtext* pt, int slot, const float* label_dev,
                                   const float* pred_dev, int64_t n, int pred_prob) {
  DFX_CHECK_ARG(pt, "predtext_submit: null object");
  DFX_CHECK_ARG(slot == 0 || slot == 1, "predtext_submit: slot outside 0..1");
  dfx_predtext::Slot& s = pt->s[slot];
  DFX_CHECK_ARG(!s.pending, "predtext_submit: the slot is pending (take it first)");
  DFX_CHECK_ARG(n >= 0 && n <= kPtMaxRows, "predtext_submit: n outside [0, 2^26]");
  DFX_CHECK_ARG(n == 0 || (label_dev && pred_dev), "predtext_submit: null label or pred");
  Context* c = &pt->ctx->c;
  DFX_HIP(hipSetDevice(c->device));
  DFX_TRY(pt_slot_reserve(s, n));
  const hipStream_t st = c->stream;
  DFX_TRY(format_pred_on(c, st, label_dev, pred_dev, n, pred_prob, s.text_dev, n * kMaxRow,
                         s.stat_dev, nullptr));
  DFX_HIP(hipMemcpyAsync(s.stat_host, s.stat_dev, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (n > 0) {
    DFX_HIP(hipMemcpyAsync(s.text_host, s.text_dev, (size_t)n * kMaxRow, hipMemcpyDeviceToHost,
                           st));
    DFX_HIP(hipMemcpyAsync(s.lp_host, label_dev, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    DFX_HIP(hipMemcpyAsync(s.lp_host + s.cap_rows, pred_dev, (size_t)n * 4,
                           hipMemcpyDeviceToHost, st));
  }
  DFX_HIP(hipEventRecord(s.ev, st));
  s.n = n;
  s.pending = true;
  return DFX_OK;
}

extern "C" int dfx_predtext_take(dfx_predtext* pt, int slot, dfx_predtext_out* out) {
  DFX_CHECK_ARG(pt && out, "predtext_take: null argument");
  DFX_CHECK_ARG(slot == 0 || slot == 1, "predtext_take: slot outside 0..1");
  dfx_predtext::Slot& s = pt->s[slot];
  DFX_CHECK_ARG(s.pending, "predtext_take: nothing was submitted to the slot");
  DFX_HIP(hipEventSynchronize(s.ev));
  s.pending = false;
  out->text = s.text_host;
  out->bytes = s.stat_host[0];
  out->rows = s.n;
  out->flagged = s.stat_host[1];
  out->first_flagged = s.stat_host[2];
  out->label = s.lp_host;
  out->pred = s.lp_host + s.cap_rows;
  return DFX_OK;
}

extern "C" int dfx_predtext_destroy(dfx_predtext* pt) {
  if (!pt) return DFX_OK;
  (void)hipSetDevice(pt->ctx->c.device);
  (void)hipStreamSynchronize(pt->ctx->c.stream);
  pt_release(pt);
  return DFX_OK;
}
