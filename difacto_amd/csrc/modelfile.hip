// The two model files written from the device: SGDUpdater::Save's records and ::Dump's lines
// (src/sgd/sgd_updater.h:84-139, as csrc/store.hip's host writers lay them down and
// csrc/modeltext.h restates them), byte for byte.
//
// The table is walked in slot order, the host writers' order, in chunks of slots.  A chunk is a
// length pass, the plain multi-launch scan of csrc/textscan.h (tile totals, one block over the
// totals) and a write pass - nothing spins, looks back or waits on another block.  Both files
// are the concatenation of small pieces in slot order - a record's dwords, a line's fields with
// their separators - so a tile of kNT slots numbers its pieces through an LDS scan and hands
// piece q to thread q mod kNT, whichever slot it belongs to (a binary search in the tile's
// offsets): free and empty slots cost nothing, and a record's V rows or a line's fields are
// spread over the lanes, not walked by one.
//
//   k_mp_len     binary: a slot -> its record's bytes (0: free, or SGDEntry::empty()); tile totals
//   k_mp_write   a tile's records as dwords at their offsets (every record is a multiple of 4
//                bytes and the staging buffer is dword aligned); consecutive lanes, consecutive
//                dwords
//   k_mt_len     text: a tile's fields formatted for their lengths (csrc/fmtg.h through
//                csrc/modeltext.h); a field fmt_g refuses flags its entry; tile totals
//   k_mt_write   the fields again, kNT at a time, laid end to end in LDS at the destination's
//                16-byte phase and stored as 16-byte pieces (csrc/predtext.hip's write)
//
// V and Vaux are read through row_V / row_C, so fat slots and the split pool are one path.  No
// pass writes a byte at or past the capacity; the need is reported.  Offsets inside a chunk are
// 32-bit: the entry points refuse a chunk whose worst case does not fit.
//
// dfx_store_save_dev / dfx_store_dump_dev: two staging buffers with pinned mirrors, kept with
// the context; chunk t + 1's kernels and chunk t's copy run while the host writes chunk t - 1
// with one fwrite.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <string>
#include <vector>

#include "modeltext.h"
#include "textscan.h"

namespace {

namespace mt = dfx_modeltext;

constexpr int64_t kMfBudget = (int64_t)64 << 20;  // bytes of one staging buffer, at most
constexpr uint64_t kMfMaxChunkBytes = 0xFFFFFFFFull;
// LDS of the text write: kNT fields and their separators behind up to 15 bytes of phase
constexpr int kMtStage16 = (15 + kNT * (mt::kMaxKey + 1) + 15) / 16;

// stat: [0] bytes the chunk needs, [1] bytes written, [2] entries, [3] entries flagged
__global__ void k_mf_init(unsigned long long* stat) {
  stat[0] = 0;
  stat[1] = 0;
  stat[2] = 0;
  stat[3] = 0;
}

struct MfSlot {
  bool live;   // the files hold this entry
  bool has_v;
};
__device__ inline MfSlot mf_slot(const Table& T, int64_t s) {
  const Entry* e = ent_at(T, s);
  MfSlot r;
  r.has_v = e->vrow >= 0;
  r.live = e->key != kEmptyKey && !mt::entry_empty(e->w, r.has_v);
  return r;
}

// the slot of the tile that piece x belongs to: the r with off[r] <= x < off[r + 1]
// (off[0 .. kNT]: the exclusive scan of the slots' piece counts; x < off[kNT])
__device__ inline uint32_t mf_owner(const uint32_t* off, uint32_t x) {
  uint32_t lo = 0, hi = kNT - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid + 1] > x) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// ---- binary ---------------------------------------------------------------------------------
__device__ inline uint32_t mp_bytes(const Table& T, int64_t slot0, uint32_t i, uint32_t n,
                                    int aux) {
  if (i >= n) return 0;
  const MfSlot s = mf_slot(T, slot0 + i);
  return s.live ? (uint32_t)mt::record_bytes(s.has_v, T.d, aux) : 0u;
}

__global__ __launch_bounds__(kNT) void k_mp_len(Table T, int64_t slot0, uint32_t n, int aux,
                                                uint32_t* __restrict__ tot,
                                                unsigned long long* stat) {
  __shared__ uint32_t lds[2 * kNT];
  const uint32_t len = mp_bytes(T, slot0, blockIdx.x * kNT + threadIdx.x, n, aux);
  uint32_t incl, excl, total;
  block_scan<AddOp, kNT>(len, lds, &incl, &excl, &total);
  const int live = __syncthreads_count(len != 0);
  if (threadIdx.x == 0) {
    tot[blockIdx.x] = total;
    if (live) atomicAdd(&stat[2], (unsigned long long)live);
  }
}

__global__ __launch_bounds__(kNT) void k_mp_write(Table T, int64_t slot0, uint32_t n, int aux,
                                                  const uint32_t* __restrict__ tot,
                                                  const uint32_t* __restrict__ total_dev,
                                                  char* __restrict__ out, uint64_t cap,
                                                  unsigned long long* stat) {
  __shared__ uint32_t lds[2 * kNT];
  __shared__ uint32_t soff[kNT + 1];
  const uint32_t t = threadIdx.x;
  const uint32_t len = mp_bytes(T, slot0, blockIdx.x * kNT + t, n, aux);
  uint32_t incl, excl, btotal;
  block_scan<AddOp, kNT>(len, lds, &incl, &excl, &btotal);
  soff[t] = excl;
  if (t == 0) soff[kNT] = btotal;
  __syncthreads();
  const uint64_t base = tot[blockIdx.x];
  const int d = T.d, head = mt::record_head_dwords(aux);
  for (uint32_t q = t; q < btotal / 4u; q += kNT) {
    const uint32_t r = mf_owner(soff, 4u * q);
    const int j = (int)(q - soff[r] / 4u);  // the dword of its record
    const int64_t slot = slot0 + (int64_t)blockIdx.x * kNT + r;
    const Entry* e = ent_at(T, slot);
    uint32_t v;
    if (j < head) {
      const unsigned long long key = e->key;
      v = j == 0   ? (uint32_t)key
          : j == 1 ? (uint32_t)(key >> 32)
          : j == 2 ? (uint32_t)(e->vrow >= 0 ? 1 + d : 1)
          : j == 3 ? __float_as_uint(e->w)
          : j == 4 ? __float_as_uint(e->sqrt_g)
                   : __float_as_uint(e->z);
    } else {
      const int k = j - head;
      v = __float_as_uint(k < d ? row_V(T, e->vrow)[k] : row_C(T, e->vrow)[k - d]);
    }
    const uint64_t g = base + 4ull * q;
    if (g + 4u <= cap) {
      *reinterpret_cast<uint32_t*>(out + g) = v;
    } else {
      for (uint32_t b = 0; b < 4u; ++b)
        if (g + b < cap) out[g + b] = (char)(v >> (8u * b));
    }
  }
  if (blockIdx.x == 0 && t == 0) {
    const uint64_t need = *total_dev;
    stat[0] = need;
    stat[1] = need < cap ? need : cap;
  }
}

// ---- text -----------------------------------------------------------------------------------
// field j of slot's line and its separator into out -> the bytes, or -1: needs the host
__device__ inline int mt_field(const Table& T, int64_t slot, int j, int aux, int rev, char* out) {
  const Entry* e = ent_at(T, slot);
  const int d = T.d;
  const bool has_v = e->vrow >= 0;
  const int nf = mt::line_fields(has_v, d, aux);
  int k;
  const mt::Field what = mt::field_of(j, d, aux, &k);
  uint64_t u = 0;
  float f = 0.f;
  switch (what) {
    case mt::kKey: u = mt::printed_key(e->key, rev); break;
    case mt::kSize: u = (uint64_t)(has_v ? 1 + d : 1); break;
    case mt::kW: f = e->w; break;
    case mt::kSqrtG: f = e->sqrt_g; break;
    case mt::kZ: f = e->z; break;
    case mt::kV: f = row_V(T, e->vrow)[k]; break;
    default: f = row_C(T, e->vrow)[k]; break;
  }
  return mt::fmt_field(what, u, f, j == nf - 1, out);
}

// the tile's exclusive field offsets into sfoff[0 .. kNT] -> its field count
__device__ inline uint32_t mt_tile_fields(const Table& T, int64_t slot0, uint32_t n, int aux,
                                          uint32_t* lds, uint32_t* sfoff, uint32_t* mine) {
  const uint32_t t = threadIdx.x, i = blockIdx.x * kNT + t;
  uint32_t nf = 0;
  if (i < n) {
    const MfSlot s = mf_slot(T, slot0 + i);
    if (s.live) nf = (uint32_t)mt::line_fields(s.has_v, T.d, aux);
  }
  uint32_t incl, excl, F;
  block_scan<AddOp, kNT>(nf, lds, &incl, &excl, &F);
  sfoff[t] = excl;
  if (t == 0) sfoff[kNT] = F;
  __syncthreads();
  *mine = nf;
  return F;
}

__global__ __launch_bounds__(kNT) void k_mt_len(Table T, int64_t slot0, uint32_t n, int aux,
                                                int rev, uint32_t* __restrict__ tot,
                                                unsigned long long* stat) {
  __shared__ uint32_t lds[2 * kNT];
  __shared__ uint32_t sfoff[kNT + 1];
  __shared__ uint32_t sbad[kNT];
  __shared__ char sfield[kNT][mt::kFieldBytes];
  const uint32_t t = threadIdx.x;
  uint32_t nf;
  sbad[t] = 0;
  const uint32_t F = mt_tile_fields(T, slot0, n, aux, lds, sfoff, &nf);
  uint32_t bytes = 0;
  for (uint32_t q = t; q < F; q += kNT) {
    const uint32_t r = mf_owner(sfoff, q);
    const int L = mt_field(T, slot0 + (int64_t)blockIdx.x * kNT + r, (int)(q - sfoff[r]), aux,
                           rev, sfield[t]);
    if (L < 0) sbad[r] = 1u;  // (racing writers store the same value)
    else bytes += (uint32_t)L;
  }
  uint32_t incl, excl, total;
  block_scan<AddOp, kNT>(bytes, lds, &incl, &excl, &total);  // (its barriers order sbad)
  const int live = __syncthreads_count(nf != 0);
  const int bad = __syncthreads_count(sbad[t] != 0);
  if (t == 0) {
    tot[blockIdx.x] = total;
    if (live) atomicAdd(&stat[2], (unsigned long long)live);
    if (bad) atomicAdd(&stat[3], (unsigned long long)bad);
  }
}

__global__ __launch_bounds__(kNT) void k_mt_write(Table T, int64_t slot0, uint32_t n, int aux,
                                                  int rev, const uint32_t* __restrict__ tot,
                                                  const uint32_t* __restrict__ total_dev,
                                                  char* __restrict__ text, uint64_t cap,
                                                  unsigned long long* stat) {
  __shared__ uint32_t lds[2 * kNT];
  __shared__ uint32_t sfoff[kNT + 1];
  __shared__ char sfield[kNT][mt::kFieldBytes];
  __shared__ uint4 stage16[kMtStage16];
  const uint32_t t = threadIdx.x;
  uint32_t nf;
  const uint32_t F = mt_tile_fields(T, slot0, n, aux, lds, sfoff, &nf);
  char* stage = reinterpret_cast<char*>(stage16);
  uint64_t base = tot[blockIdx.x];  // the first byte of the round's fields in the text
  for (uint32_t q0 = 0; q0 < F; q0 += kNT) {
    const uint32_t q = q0 + t;
    uint32_t len = 0;
    if (q < F) {
      const uint32_t r = mf_owner(sfoff, q);
      const int L = mt_field(T, slot0 + (int64_t)blockIdx.x * kNT + r, (int)(q - sfoff[r]), aux,
                             rev, sfield[t]);
      if (L > 0) len = (uint32_t)L;  // (a refused field: the chunk is flagged, its text unused)
    }
    uint32_t incl, excl, rtotal;
    block_scan<AddOp, kNT>(len, lds, &incl, &excl, &rtotal);
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(text + base) & 15u);
    for (uint32_t j = 0; j < len; ++j) stage[mis + excl + j] = sfield[t][j];
    __syncthreads();
    // stage[mis, end) is text[base, base + rtotal); piece p is stage[16 p, 16 p + 16), aligned
    // in the text too
    const uint32_t end = mis + rtotal, np = (end + 15u) / 16u;  // np <= kMtStage16
    for (uint32_t p = t; p < np; p += kNT) {
      const uint32_t s0 = 16u * p;
      const int64_t g0 = (int64_t)base - (int64_t)mis + (int64_t)s0;
      if (s0 >= mis && s0 + 16u <= end && (uint64_t)(g0 + 16) <= cap) {
        *reinterpret_cast<uint4*>(text + g0) = stage16[p];
      } else {
        for (uint32_t j = 0; j < 16u; ++j) {
          const uint32_t s = s0 + j;
          if (s >= mis && s < end && (uint64_t)(g0 + (int64_t)j) < cap)
            text[g0 + (int64_t)j] = stage[s];
        }
      }
    }
    __syncthreads();  // the next round writes the stage again
    base += rtotal;
  }
  if (blockIdx.x == 0 && t == 0) {
    const uint64_t need = *total_dev;
    stat[0] = need;
    stat[1] = need < cap ? need : cap;
  }
}

// ---- one chunk ------------------------------------------------------------------------------
int64_t mf_worst(int d, int aux, bool text) {
  return text ? mt::worst_line_bytes(d, aux) : (int64_t)mt::record_bytes(true, d, aux);
}

// slots [slot0, slot0 + n) of the context's table into out[0, cap) on the context stream; text:
// Dump's lines, else Save's records
int mf_chunk(Context* c, int64_t slot0, int64_t n, bool text, int aux, int rev, char* out,
             int64_t cap, int64_t* stat_dev) {
  const unsigned nb = blocks_for((uint64_t)n, kNT);
  const hipStream_t st = c->stream;
  unsigned long long* stat = reinterpret_cast<unsigned long long*>(stat_dev);
  hipLaunchKernelGGL(k_mf_init, dim3(1), dim3(1), 0, st, stat);
  if (n > 0) {
    DFX_TRY(c->mf_tot.ensure(((size_t)nb + 1) * sizeof(uint32_t)));
    uint32_t* tot = c->mf_tot.as<uint32_t>();
    const uint32_t n32 = (uint32_t)n;
    if (text)
      hipLaunchKernelGGL(k_mt_len, dim3(nb), dim3(kNT), 0, st, c->T, slot0, n32, aux, rev, tot,
                         stat);
    else
      hipLaunchKernelGGL(k_mp_len, dim3(nb), dim3(kNT), 0, st, c->T, slot0, n32, aux, tot, stat);
    hipLaunchKernelGGL((k_scan_totals<AddOp>), dim3(1), dim3(1024), 0, st, tot,
                       (const uint32_t*)nullptr, n32, (uint32_t)kNT, tot + nb);
    if (text)
      hipLaunchKernelGGL(k_mt_write, dim3(nb), dim3(kNT), 0, st, c->T, slot0, n32, aux, rev,
                         (const uint32_t*)tot, (const uint32_t*)(tot + nb), out, (uint64_t)cap,
                         stat);
    else
      hipLaunchKernelGGL(k_mp_write, dim3(nb), dim3(kNT), 0, st, c->T, slot0, n32, aux,
                         (const uint32_t*)tot, (const uint32_t*)(tot + nb), out, (uint64_t)cap,
                         stat);
  }
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

int mf_chunk_checked(dfx_ctx* ctx, int64_t slot0, int64_t n, bool text, int aux, int rev,
                     char* out, int64_t cap, int64_t* stat_dev) {
  DFX_CHECK_ARG(ctx, "null ctx");
  Context* c = &ctx->c;
  DFX_CHECK_ARG(stat_dev, "model chunk: null stat_dev");
  DFX_CHECK_ARG(slot0 >= 0 && n >= 0 && slot0 <= c->cap && n <= c->cap - slot0,
                "model chunk: slots outside the table");
  DFX_CHECK_ARG(cap >= 0 && (cap == 0 || out), "model chunk: cap_bytes < 0 or a null buffer");
  DFX_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3u) == 0,
                "model chunk: out_dev not dword aligned");
  DFX_CHECK_ARG((uint64_t)n * (uint64_t)mf_worst(c->T.d, aux, text) <= kMfMaxChunkBytes,
                "model chunk: nslots times the longest record or line passes 32-bit offsets");
  DFX_HIP(hipSetDevice(c->device));
  return mf_chunk(c, slot0, n, text, aux ? 1 : 0, rev ? 1 : 0, out, cap, stat_dev);
}

// ---- the whole file -------------------------------------------------------------------------
// the staging set lives in the context (internal.h MfStaging): made by the first call, grown
// when a call needs larger buffers, freed with the context.  The stream is idle when a call
// returns, so nothing queued reads it between calls.
void mf_staging_free_buffers(MfStaging& S) {
  for (int k = 0; k < 2; ++k) {
    if (S.dev[k]) (void)hipFree(S.dev[k]);
    if (S.host[k]) (void)hipHostFree(S.host[k]);
    S.dev[k] = S.host[k] = nullptr;
  }
  S.cap_bytes = 0;
}

int mf_staging_reserve(MfStaging& S, int64_t cap_bytes) {
  if (!S.stat_dev) {
    DFX_HIP(hipMalloc(reinterpret_cast<void**>(&S.stat_dev), 8 * sizeof(int64_t)));
    DFX_HIP(hipHostMalloc(reinterpret_cast<void**>(&S.stat_host), 8 * sizeof(int64_t),
                          hipHostMallocDefault));
    for (int k = 0; k < 2; ++k)
      DFX_HIP(hipEventCreateWithFlags(&S.ev[k], hipEventDisableTiming));
  }
  if (cap_bytes <= S.cap_bytes) return DFX_OK;
  mf_staging_free_buffers(S);
  for (int k = 0; k < 2; ++k) {
    DFX_HIP(hipMalloc(reinterpret_cast<void**>(&S.dev[k]), (size_t)cap_bytes));
    DFX_HIP(hipHostMalloc(reinterpret_cast<void**>(&S.host[k]), (size_t)cap_bytes,
                          hipHostMallocDefault));
  }
  S.cap_bytes = cap_bytes;
  return DFX_OK;
}

struct MfFile {  // closes the file on every way out
  FILE* f = nullptr;
  ~MfFile() {
    if (f) fclose(f);
  }
};

double mf_now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

int mf_write_file(dfx_ctx* ctx, const char* path, bool text, int aux, int rev,
                  int64_t chunk_slots, int64_t* stats, double* times) {
  DFX_CHECK_ARG(ctx && path, "null argument");
  DFX_CHECK_ARG(chunk_slots >= 0, "model file: chunk_slots < 0");
  Context* c = &ctx->c;
  DFX_HIP(hipSetDevice(c->device));
  aux = aux ? 1 : 0;
  rev = rev ? 1 : 0;
  const int64_t worst = mf_worst(c->T.d, aux, text);
  // the staging budget bounds a chunk, asked for or not: device and pinned memory stay
  // constant whatever the table's size
  const int64_t fit = std::max<int64_t>(kMfBudget / worst, 1);
  const int64_t per = std::min(chunk_slots > 0 ? std::min(chunk_slots, fit) : fit,
                               std::max<int64_t>(c->cap, 1));
  const int64_t cap_bytes = per * worst;
  const int64_t nchunks = (c->cap + per - 1) / per;
  MfFile F;
  F.f = fopen(path, "wb");
  if (!F.f) { set_error(std::string("cannot open ") + path); return DFX_ERR_IO; }
  if (!text) {
    const bool b = aux != 0;
    fwrite(&b, sizeof(bool), 1, F.f);
  }
  MfStaging& S = c->mf_stage;
  DFX_TRY(mf_staging_reserve(S, cap_bytes));
  const hipStream_t st = c->stream;
  int64_t entries = 0, bytes = sizeof(bool) * (text ? 0 : 1), host_chunks = 0;
  double wait_s = 0, write_s = 0;
  std::vector<float> pool;  // the split layout's V pool, once a chunk needs the host
  std::string host_text;

  // chunk t's kernels and its four status words, then the event of its slot
  auto submit = [&](int64_t t) -> int {
    const int k = (int)(t & 1);
    const int64_t s0 = t * per, n = std::min(per, c->cap - s0);
    DFX_TRY(mf_chunk(c, s0, n, text, aux, rev, S.dev[k], cap_bytes, S.stat_dev + 4 * k));
    DFX_HIP(hipMemcpyAsync(S.stat_host + 4 * k, S.stat_dev + 4 * k, 4 * sizeof(int64_t),
                           hipMemcpyDeviceToHost, st));
    DFX_HIP(hipEventRecord(S.ev[k], st));
    return DFX_OK;
  };
  // what chunk t left: the bytes to copy down (0 for one the host writes)
  struct Done { int64_t bytes = 0; bool host = false; };
  Done done[2];
  auto put = [&](int64_t t) -> int {  // chunk t into the file; its copy has finished
    const int k = (int)(t & 1);
    const double t0 = mf_now();
    const char* p = S.host[k];
    size_t nb = (size_t)done[k].bytes;
    if (done[k].host) {
      const int64_t s0 = t * per, n = std::min(per, c->cap - s0);
      DFX_TRY(store_dump_range(c, s0, n, aux, rev, &pool, &host_text));
      p = host_text.data();
      nb = host_text.size();
      ++host_chunks;
    }
    if (nb && fwrite(p, 1, nb, F.f) != nb) {
      set_error(std::string("short write to ") + path);
      return DFX_ERR_IO;
    }
    bytes += (int64_t)nb;
    write_s += mf_now() - t0;
    return DFX_OK;
  };

  if (nchunks > 0) DFX_TRY(submit(0));
  for (int64_t t = 0; t < nchunks; ++t) {
    const int k = (int)(t & 1);
    const double t0 = mf_now();
    DFX_HIP(hipEventSynchronize(S.ev[k]));  // (in stream order behind chunk t - 1's copy)
    wait_s += mf_now() - t0;
    const int64_t* hs = S.stat_host + 4 * k;
    if (hs[0] > cap_bytes) {
      set_error("model file: a chunk needs more than its staging buffer");
      return DFX_ERR_CAPACITY;
    }
    entries += hs[2];
    done[k].host = hs[3] != 0;
    done[k].bytes = done[k].host ? 0 : hs[0];
    if (done[k].bytes)
      DFX_HIP(hipMemcpyAsync(S.host[k], S.dev[k], (size_t)done[k].bytes, hipMemcpyDeviceToHost,
                             st));
    if (t + 1 < nchunks) DFX_TRY(submit(t + 1));
    if (t > 0) DFX_TRY(put(t - 1));
  }
  if (nchunks > 0) {
    const double t0 = mf_now();
    DFX_HIP(hipStreamSynchronize(st));
    wait_s += mf_now() - t0;
    DFX_TRY(put(nchunks - 1));
  }
  const double t0 = mf_now();
  const int rc = fclose(F.f);
  F.f = nullptr;
  write_s += mf_now() - t0;
  if (rc != 0) { set_error(std::string("cannot close ") + path); return DFX_ERR_IO; }
  if (times) {
    times[0] = wait_s;
    times[1] = write_s;
  }
  if (stats) {
    stats[0] = entries;
    stats[1] = bytes;
    stats[2] = nchunks;
    stats[3] = host_chunks;
  }
  return DFX_OK;
}

}  // namespace

extern "C" {

int dfx_model_pack(dfx_ctx* ctx, int64_t slot0, int64_t nslots, int save_aux, char* out_dev,
                   int64_t cap_bytes, int64_t* stat_dev) {
  return mf_chunk_checked(ctx, slot0, nslots, false, save_aux, 0, out_dev, cap_bytes, stat_dev);
}

int dfx_model_format(dfx_ctx* ctx, int64_t slot0, int64_t nslots, int dump_aux, int need_reverse,
                     char* out_dev, int64_t cap_bytes, int64_t* stat_dev) {
  return mf_chunk_checked(ctx, slot0, nslots, true, dump_aux, need_reverse, out_dev, cap_bytes,
                          stat_dev);
}

// (a failed call may leave work queued that reads the context's staging set: join it)
static int mf_write_joined(dfx_ctx* ctx, const char* path, bool text, int aux, int rev,
                           int64_t chunk_slots, int64_t* stats, double* times) {
  const int rc = mf_write_file(ctx, path, text, aux, rev, chunk_slots, stats, times);
  if (rc != DFX_OK && ctx) (void)hipStreamSynchronize(ctx->c.stream);
  return rc;
}

int dfx_store_save_dev(dfx_ctx* ctx, const char* path, int save_aux, int64_t chunk_slots,
                       int64_t* stats, double* times) {
  return mf_write_joined(ctx, path, false, save_aux, 0, chunk_slots, stats, times);
}

int dfx_store_dump_dev(dfx_ctx* ctx, const char* path, int dump_aux, int need_reverse,
                       int64_t chunk_slots, int64_t* stats, double* times) {
  return mf_write_joined(ctx, path, true, dump_aux, need_reverse, chunk_slots, stats, times);
}

}  // extern "C"
