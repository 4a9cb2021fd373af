// The scan helpers of the device text parsers (textparse.hip: Criteo, the row gather;
// libsvmparse.hip: libsvm; adfeaparse.hip: adfea): a block scan, the plain multi-launch scan
// (tile totals, a scan of the totals, apply - no look-back, nothing spins) and the launch
// helpers.  These sit in an unnamed namespace: each .hip file that uses them gets kernels of its
// own.  In front of them: what the text feed (textfeed.hip) calls of the three parsers and the
// gather.
#pragma once
#include "internal.h"

namespace dfx {
constexpr int kCols = 39;  // criteo feature columns (13 integer + 26 categorical)

// a parser's scratch: the context's own set (dfx_parse_criteo / _libsvm / _adfea, on the input
// stream) or a text feed's (textfeed.hip; its parses run on a stream of their own).  The libsvm
// and adfea parsers use tiles and stat only.
struct TpScratch {
  DevBuf *tiles, *cells, *lines, *pair, *tot, *stat;
};
// the parsers and the row gather on a stream of the caller's choice (textparse.hip,
// libsvmparse.hip, adfeaparse.hip); capacity_status: DFX_ERR_CAPACITY when the stat a parser
// left says overflow
int parse_criteo_on(const TpScratch& ws, hipStream_t st, const char* text, int64_t nbytes,
                    int is_train, int64_t max_rows, int64_t max_nnz, uint64_t* offset,
                    uint64_t* index, float* label, int64_t* stat_dev);
int parse_libsvm_on(const TpScratch& ws, hipStream_t st, const char* text, int64_t nbytes,
                    int64_t max_rows, int64_t max_nnz, uint64_t* offset, uint64_t* index,
                    float* value, float* label, uint8_t* rowflag, int64_t* stat_dev);
int parse_adfea_on(const TpScratch& ws, hipStream_t st, const char* text, int64_t nbytes,
                   int64_t max_rows, int64_t max_nnz, uint64_t* offset, uint64_t* index,
                   float* label, int64_t* stat_dev);
int capacity_status(const int64_t* stat);
template <bool kValued>
int gather_rows_on(Context* c, hipStream_t st, const uint64_t* src_offset,
                   const uint64_t* src_index, const float* src_label, const uint32_t* rows_dev,
                   int64_t begin, int64_t n, uint64_t* dst_offset, uint64_t* dst_index,
                   float* dst_label, int64_t r0, const float* src_value = nullptr,
                   float* dst_value = nullptr, const uint8_t* src_flag = nullptr,
                   uint8_t* dst_flag = nullptr);
inline TpScratch context_scratch(Context* c) {
  return TpScratch{&c->tp_tiles, &c->tp_cells, &c->tp_lines,
                   &c->tp_pair,  &c->tp_tot,   &c->tp_stat};
}
}  // namespace dfx

namespace {

using namespace dfx;

constexpr int kNT = 256;               // threads of the tile kernels
constexpr int kTpBytes = 16;           // text bytes per thread
constexpr int kTpTile = kNT * kTpBytes;
constexpr int kWavesPerBlock = kNT / 64;

struct MaxOp {
  using T = uint32_t;
  __device__ static T id() { return 0; }
  __device__ static T f(T a, T b) { return a > b ? a : b; }
};
struct AddOp {
  using T = uint32_t;
  __device__ static T id() { return 0; }
  __device__ static T f(T a, T b) { return a + b; }
};
struct Add2Op {
  using T = uint2;
  __device__ static T id() { return make_uint2(0, 0); }
  __device__ static T f(const T& a, const T& b) { return make_uint2(a.x + b.x, a.y + b.y); }
};

// inclusive / exclusive scan of one value per thread over a block of NT threads (Hillis-Steele
// through lds[2 * NT]); every thread also gets the block's total
template <class Op, int NT>
__device__ inline void block_scan(typename Op::T v, typename Op::T* lds, typename Op::T* incl,
                                  typename Op::T* excl, typename Op::T* total) {
  using T = typename Op::T;
  const int t = threadIdx.x;
  int cur = 0;
  lds[t] = v;
  __syncthreads();
  for (int d = 1; d < NT; d <<= 1) {
    T x = lds[cur * NT + t];
    if (t >= d) x = Op::f(lds[cur * NT + t - d], x);
    cur ^= 1;
    lds[cur * NT + t] = x;
    __syncthreads();
  }
  *incl = lds[cur * NT + t];
  *excl = t ? lds[cur * NT + t - 1] : Op::id();
  *total = lds[cur * NT + NT - 1];
  __syncthreads();
}

// ---- the plain multi-launch scan: tile totals, a scan of the totals, apply ------------------
// n = min(*n_dev, n_cap) when the length is only known on the device
__device__ inline uint32_t scan_len(const uint32_t* n_dev, uint32_t n_cap) {
  if (!n_dev) return n_cap;
  const uint32_t n = *n_dev;
  return n < n_cap ? n : n_cap;
}

template <class Op, class Load>
__global__ __launch_bounds__(kNT) void k_scan_reduce(Load load, const uint32_t* n_dev,
                                                     uint32_t n_cap, typename Op::T* tot) {
  using T = typename Op::T;
  __shared__ T lds[2 * kNT];
  const uint32_t n = scan_len(n_dev, n_cap);
  if ((uint64_t)blockIdx.x * kNT >= n) return;
  const uint32_t i = blockIdx.x * kNT + threadIdx.x;
  T incl, excl, total;
  block_scan<Op, kNT>(i < n ? load(i) : Op::id(), lds, &incl, &excl, &total);
  if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// exclusive scan, in place, of the ceil(n / tile) tile totals by one block; the grand total
// goes to *total_out
template <class Op>
__global__ __launch_bounds__(1024) void k_scan_totals(typename Op::T* tot, const uint32_t* n_dev,
                                                      uint32_t n_cap, uint32_t tile,
                                                      typename Op::T* total_out) {
  using T = typename Op::T;
  __shared__ T lds[2 * 1024];
  const uint32_t n = scan_len(n_dev, n_cap);
  const uint32_t nt = n / tile + (n % tile ? 1 : 0);
  T carry = Op::id();
  for (uint32_t base = 0; base < nt; base += 1024) {
    const uint32_t i = base + threadIdx.x;
    T incl, excl, total;
    block_scan<Op, 1024>(i < nt ? tot[i] : Op::id(), lds, &incl, &excl, &total);
    if (i < nt) tot[i] = Op::f(carry, excl);
    carry = Op::f(carry, total);
  }
  if (total_out && threadIdx.x == 0) *total_out = carry;
}

template <class Op, class Load, bool kInclusive>
__global__ __launch_bounds__(kNT) void k_scan_apply(Load load, const uint32_t* n_dev,
                                                    uint32_t n_cap, const typename Op::T* tot,
                                                    typename Op::T* out) {
  using T = typename Op::T;
  __shared__ T lds[2 * kNT];
  const uint32_t n = scan_len(n_dev, n_cap);
  if ((uint64_t)blockIdx.x * kNT >= n) return;
  const uint32_t i = blockIdx.x * kNT + threadIdx.x;
  T incl, excl, total;
  block_scan<Op, kNT>(i < n ? load(i) : Op::id(), lds, &incl, &excl, &total);
  if (i < n) out[i] = Op::f(tot[blockIdx.x], kInclusive ? incl : excl);
}

template <class T>
struct PtrLoad {
  const T* p;
  __device__ T operator()(uint32_t i) const { return p[i]; }
};

inline hipStream_t input_stream(Context* c) { return c->has_in_stream ? c->in_stream : c->stream; }
inline unsigned blocks_for(uint64_t n, uint64_t per) { return (unsigned)((n + per - 1) / per); }

}  // namespace
