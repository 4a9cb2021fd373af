// InitV (sgd_updater.cc:144-152), every path of it.  The reference draws a new key's V from one
// sequential rand_r stream, in the order its Update meets the keys; here each key that asks for
// V gets its rank r in that order and starts its row 3 * V_dim * r LCG steps past the seed,
// which reproduces the sequential draws bit for bit (common.h lcg_jump).  Three orders exist:
//   the fused step     key order, one launch: k_initv_onepass ranks its 8192-key tiles by a
//                      decoupled look-back and ends the step in its last block
//   the ranked pair    key order over all owners of a sharded model (one owner for the store
//                      calls and the fused step's count push): k_initv_rank_count, the owners'
//                      counts all-gathered by the caller, k_initv_rank_draw
//   push_agg=ranks     (pushing rank, key) order on one server: a list of the flagged keys, a
//                      stable sort by rank, k_initv_byrank_draw
// All place a key with initv_place and draw the placed keys with initv_draw.
//
// Two hand-offs between blocks of one launch go through initv_arrive's word: the request count
// that the fused step's last block advances the seed by, and the sum of the count kernel's
// tiles.  The value rides in the word the election reads, so the elected block has it from its
// own atomic's result: no fence (a device-scope release per block writes back its XCD's L2, full
// of the backward's dirty model lines — measured −2.7 % at C3), no second atomic.
//
// ds->seed and ds->n_vrows are read by every drawing block and then overwritten by the elected
// block of the same launch (initv_advance).  Those stores cannot reach the loads: a block loads
// both before its first barrier and either uses the values for its draws — so they have
// returned, a wave waits for a load before the first use — or has no key and never looks at
// them; only after its draws does it arrive at the word, and the elected block stores only
// after its own arrival returned a count that includes every other block's.  A load that has
// returned does not change its value.  Nothing is published by those stores within the launch,
// which is why this needs no fence; the next launch sees them across the kernel boundary.
#include <algorithm>

#include "lookback.h"

namespace dfx {

constexpr int kIvNT = 256;  // threads of every InitV block
static_assert(kIvNT == kFinNT, "the fused InitV's blocks run the step's finalize");

// One key's place: its V row (the own-th new row of this owner in the split layout, its slot
// with fat slots) written to its entry, and the rand_r state at its first draw, 3 * d * all steps
// past the seed (all: its rank over every owner's draws of this Update).  seed and nv0 are the
// store's as of the kernel's start.  A full pool: kErrPoolFull, no row, 0xFFFFFFFF returned.
__device__ inline uint32_t initv_place(const Table& T, uint32_t seed, uint64_t nv0, uint32_t own,
                                       uint64_t all, uint32_t slot, int* err, uint32_t* state) {
  *state = lcg_advance(seed, 3ull * (uint64_t)T.d * all);
  const int64_t vr = initv_row(T, nv0, own, slot);
  if (vr >= T.vcap) {
    atomicOr(err, kErrPoolFull);
    return 0xFFFFFFFFu;
  }
  ent_at(T, slot)->vrow = (int32_t)vr;
  return (uint32_t)vr;
}

// (A[j], C[j]) = the LCG jump to coordinate j of a row (initv_draw_list)
__device__ inline void initv_jumps(int d, uint32_t* A, uint32_t* C) {
  for (int j = threadIdx.x; j < d && j < kIvMaxD; j += kIvNT) lcg_jump(3ull * (uint64_t)j, &A[j], &C[j]);
}

// The block's n placed keys drawn (st, vrow: initv_place's, in LDS; the caller's barriers around
// it): a coordinate per thread, or a whole row per thread where V is wider than kIvMaxD
__device__ inline void initv_draw(const Table& T, uint32_t n, const uint32_t* st,
                                  const uint32_t* vrow, float scale, const uint32_t* A,
                                  const uint32_t* C) {
  const int d = T.d;
  if (d <= kIvMaxD) {
    initv_draw_list<kIvNT>(n, st, vrow, d, scale, A, C, [&](uint32_t r) { return row_V(T, r); },
                           [&](uint32_t r) { return row_C(T, r); });
    return;
  }
  for (uint32_t i = threadIdx.x; i < n; i += kIvNT) {
    if (vrow[i] == 0xFFFFFFFFu) continue;
    uint32_t s = st[i];
    float* V = row_V(T, vrow[i]);
    float* Cg = row_C(T, vrow[i]);
    for (int k = 0; k < d; ++k) {
      V[k] = initv_value(rand_r_dev(&s), scale);
      Cg[k] = 0.f;
    }
  }
}

// The block arrives at *word (blocks arrived << 32 | the sum of what they carried) with v
// (block-uniform): one returning add.  True in every thread of the last of nblocks to arrive,
// with *sum = the sum over all of them, taken from that add's result; it zeroes the word for
// the next launch.
__device__ inline bool initv_arrive(unsigned long long* word, uint32_t v, uint32_t nblocks,
                                    uint32_t* sum) {
  __shared__ unsigned long long s_old;
  __syncthreads();
  if (threadIdx.x == 0) {
    s_old = atomicAdd(word, (1ull << 32) | v);
    if ((uint32_t)(s_old >> 32) == nblocks - 1)
      __hip_atomic_store(word, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  *sum = (uint32_t)s_old + v;
  return (uint32_t)(s_old >> 32) == nblocks - 1;
}

// ---- the fused step's InitV in one launch -------------------------------------------------------
// Block b counts a tile's kIvTile flags, publishes the count and finds its prefix by the
// block-wide decoupled look-back over the lower tiles' tagged words (lookback.h), then draws its
// keys.  The step's last work follows in this launch (step_finalize_body: the seed and n_vrows
// advanced by the request count, the progress, the capacity guard's counts) — by block 0 when
// the gate is closed, else by the last block to arrive at ds->iv_done, to which the block of the
// last tile carries the count (its prefix + its own).
// 8192-key tiles (a thread's 32 flags as one bit mask), the requested keys listed kIvList at a
// time: 4096-key tiles took 850 tickets at C3, ~9 us of serialised atomics.
constexpr int kIvItems = 32, kIvTile = kIvNT * kIvItems, kIvList = 4096;

// -> the request count of the step if this block took the last tile, else 0
__device__ uint32_t initv_onepass_body(const uint32_t* flags, const uint32_t* slot, const Table& T,
                                       float scale, DevState* ds, unsigned long long* status,
                                       int64_t n, uint32_t need);

__global__ __launch_bounds__(kIvNT) void k_initv_onepass(const uint32_t* flags,
                                                         const uint32_t* slot, Table T,
                                                         float scale, DevState* ds,
                                                         const DevState* nds,
                                                         const uint32_t* gate,
                                                         unsigned long long* status, FinArgs fin) {
  __shared__ double s_red[kFinNT / kWave];
  const int64_t n = (int64_t)nds->u_count;
  const uint32_t need = (uint32_t)((n + kIvTile - 1) / kIvTile);
  if (*gate == 0u || need == 0) {  // nothing to draw: block 0 finalizes
    if (blockIdx.x == 0) step_finalize_body<kFinNT>(fin, 0u, s_red);
    return;
  }
  if (blockIdx.x >= need) return;
  const uint32_t part = initv_onepass_body(flags, slot, T, scale, ds, status, n, need);
  uint32_t total;
  if (initv_arrive(&ds->iv_done, part, need, &total)) step_finalize_body<kFinNT>(fin, total, s_red);
}

__device__ uint32_t initv_onepass_body(const uint32_t* flags, const uint32_t* slot, const Table& T,
                                       float scale, DevState* ds, unsigned long long* status,
                                       int64_t n, uint32_t need) {
  __shared__ uint32_t lds[kIvNT / kWave + 1];
  __shared__ uint32_t s_lb[3 * kIvNT / kWave];
  const uint32_t seed = ds->seed;  // (before the first barrier: the header's last paragraph)
  const uint64_t nv0 = ds->n_vrows;
  // tile by ticket, in the order blocks start: a block only waits on running ones.  Block index
  // order is not start order across XCDs, and the AUC lane's look-back sort can run beside this
  // kernel, so tile = block index could wait on a block that cannot be placed.  The
  // block that draws the last ticket zeroes the counter for the next launch (k_step_finalize
  // zeroes it too).  Only as many blocks as the batch has tiles draw one: the grid is sized for
  // the nnz bound, and each ticket is a returning atomic on one word, ~11 ns apiece serialised
  // (DESIGN.md (d)); the blocks past the count leave at once, and the tickets still go to running
  // blocks in start order.
  __shared__ uint32_t s_tile;
  if (threadIdx.x == 0) {
    s_tile = atomicAdd(&ds->iv_ticket, 1u);
    if (s_tile == need - 1)
      __hip_atomic_store(&ds->iv_ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const int64_t tile = s_tile;
  const int64_t base = tile * kIvTile;
  const uint32_t tag = ds->iv_epoch & 0x3FFFFFFFu;
  // this thread's kIvItems consecutive flags (0 / 1) as bits
  const int64_t i0 = base + (int64_t)threadIdx.x * kIvItems;
  uint32_t mask = 0;
  if (i0 + kIvItems <= n && ((uintptr_t)flags & 15u) == 0) {
    const uint4* f4 = reinterpret_cast<const uint4*>(flags + i0);
#pragma unroll
    for (int q = 0; q < kIvItems / 4; ++q) {
      const uint4 v = f4[q];
      mask |= ((v.x ? 1u : 0u) | (v.y ? 2u : 0u) | (v.z ? 4u : 0u) | (v.w ? 8u : 0u)) << (4 * q);
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < kIvItems; ++k)
      if (i0 + k < n && flags[i0 + k]) mask |= 1u << k;
  }
  const uint32_t cnt = (uint32_t)__popc(mask);
  uint32_t tot;
  const uint32_t ex = block_excl_scan<kIvNT>(cnt, lds, &tot);
  const uint32_t pre = block_lookback<kIvNT>(status, tile, tag, tot, &ds->err, s_lb);
  const uint32_t part = base + kIvTile >= n ? pre + tot : 0u;  // the last tile: the step's count
  if (tot == 0) return part;  // block-uniform
  // the block's requested keys, kIvList at a time, each with its V row and the LCG state at its
  // first draw, then every (key, coordinate) drawn by its own thread: coordinate j's state is
  // 3·j steps on (A_j·state + C_j), the same rand_r values as one thread walking the row — a
  // row's d draws were one lane's d · 3 dependent LCG steps (C5: ~0.1 ms of the step with ~1.5 k
  // requests per 4096-key tile)
  __shared__ uint32_t s_st[kIvList], s_vr[kIvList];
  __shared__ uint32_t s_A[kIvMaxD], s_C[kIvMaxD];
  initv_jumps(T.d, s_A, s_C);
  for (uint32_t q0 = 0; q0 < tot; q0 += kIvList) {
    if (ex < q0 + kIvList && ex + cnt > q0) {
      uint32_t idx = ex;
      for (uint32_t m = mask; m; m &= m - 1, ++idx) {
        if (idx < q0) continue;
        if (idx >= q0 + kIvList) break;
        const int64_t u = i0 + (__ffs(m) - 1);
        const uint32_t e = pre + idx;
        s_vr[idx - q0] = initv_place(T, seed, nv0, e, e, slot[u], &ds->err, &s_st[idx - q0]);
      }
    }
    __syncthreads();
    initv_draw(T, tot - q0 < (uint32_t)kIvList ? tot - q0 : (uint32_t)kIvList, s_st, s_vr, scale,
               s_A, s_C);
    __syncthreads();
  }
  return part;
}

// ---- the ranked pair ----------------------------------------------------------------------------
//   count: per tile of kIvrTile flags its count (ts[tile], for the draw kernel: a kernel boundary
//          orders it); every block arrives with the sum of its tiles, and the last to arrive has
//          this owner's F — the request count the owners all-gather — from its own add
//   draw:  per tile its exclusive prefix from ts, per chunk of kIvNT flags a block scan, then the
//          listed keys drawn at their rank over all owners (off + e); the last block advances
//          the shared seed by every owner's draws and the V pool by F
// The flags are read raw (0 / 1), never scanned in place.  nuniq == null: the count is `bound`.
constexpr int kIvrTile = 4096, kIvrGrid = 256;

__device__ inline int64_t ivr_n(const uint32_t* nuniq, int64_t bound) {
  const int64_t n = nuniq ? (int64_t)*nuniq : bound;
  return n < bound ? n : bound;
}

__global__ __launch_bounds__(kIvNT) void k_initv_rank_count(const uint32_t* flags, int64_t bound,
                                                            const uint32_t* nuniq,
                                                            const uint32_t* gate, uint32_t* ts,
                                                            uint32_t* ftotal, int64_t* count_out,
                                                            unsigned long long* ticket) {
  __shared__ uint32_t lds[kIvNT / kWave + 1];
  if (gate && *gate == 0u) {  // no key flagged this step (the steady state): F = 0
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      *ftotal = 0u;
      *count_out = 0;
    }
    return;
  }
  const int64_t n = ivr_n(nuniq, bound);
  const int64_t ntiles = (n + kIvrTile - 1) / kIvrTile;
  uint32_t mine = 0;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * kIvrTile;
    uint32_t f = 0;
    for (int i = threadIdx.x; i < kIvrTile; i += kIvNT) {
      const int64_t u = b0 + i;
      f += (u < n && flags[u]) ? 1u : 0u;
    }
    uint32_t tot;
    (void)block_excl_scan<kIvNT>(f, lds, &tot);
    if (threadIdx.x == 0) ts[tile] = tot;
    mine += tot;
  }
  uint32_t F;
  if (!initv_arrive(ticket, mine, gridDim.x, &F) || threadIdx.x != 0) return;
  *ftotal = F;
  *count_out = (int64_t)F;
}

__global__ __launch_bounds__(kIvNT) void k_initv_rank_draw(
    const uint32_t* flags, int64_t bound, const uint32_t* nuniq, const uint32_t* ftotal,
    const uint32_t* ts, const uint32_t* segslot, const int64_t* Fall, int rank, int nranks,
    Table T, float scale, DevState* ds, uint32_t* fcount, unsigned long long* ticket,
    unsigned long long* cap_host) {
  __shared__ uint32_t lds[kIvNT / kWave + 1];
  __shared__ uint32_t s_st[kIvNT], s_vr[kIvNT], s_A[kIvMaxD], s_C[kIvMaxD];
  int64_t tot = 0, off = 0;
  for (int h = 0; h < nranks; ++h) {
    tot += Fall[h];
    if (h < rank) off += Fall[h];
  }
  if (tot == 0) {  // no owner draws: nothing advances (the gate's reset only)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (fcount) *fcount = 0u;
      if (cap_host) {  // the capacity guard's counts (pinned host words)
        cap_host[0] = ds->n_keys;
        cap_host[1] = ds->n_vrows;
      }
    }
    return;
  }
  const uint32_t F = *ftotal;
  if (F > 0) {
    const uint32_t seed = ds->seed;  // (before the first barrier: the header's last paragraph)
    const uint64_t nv0 = ds->n_vrows;
    initv_jumps(T.d, s_A, s_C);
    const int64_t n = ivr_n(nuniq, bound);
    const int64_t ntiles = (n + kIvrTile - 1) / kIvrTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      uint32_t pre = 0;  // the tile's exclusive prefix: the counts of the tiles before it
      for (int64_t i = threadIdx.x; i < tile; i += kIvNT) pre += ts[i];
      uint32_t base;
      (void)block_excl_scan<kIvNT>(pre, lds, &base);
      if (ts[tile] == 0u) continue;
      const int64_t b0 = tile * kIvrTile;
      for (int c0 = 0; c0 < kIvrTile; c0 += kIvNT) {
        const int64_t u = b0 + c0 + threadIdx.x;
        const bool f = u < n && flags[u] != 0u;
        uint32_t cnt;
        const uint32_t at = block_excl_scan<kIvNT>(f ? 1u : 0u, lds, &cnt);
        if (f)
          s_vr[at] = initv_place(T, seed, nv0, base + at, (uint64_t)off + base + at, segslot[u],
                                 &ds->err, &s_st[at]);
        __syncthreads();
        initv_draw(T, cnt, s_st, s_vr, scale, s_A, s_C);
        base += cnt;
        __syncthreads();
      }
    }
  }
  // the last block: every owner's draws advance the shared seed, this owner's F the pool.  It
  // consumes nothing that another block of this launch wrote — F and Fall come from earlier
  // launches, and ds->seed / n_vrows / n_keys are written here alone — so the word only elects
  uint32_t none;
  if (!initv_arrive(ticket, 0u, gridDim.x, &none) || threadIdx.x != 0) return;
  if (fcount) *fcount = 0u;
  initv_advance(ds, T.d, (uint64_t)tot, F, T.vcap);
  if (cap_host) {
    cap_host[0] = ds->n_keys;
    cap_host[1] = ds->n_vrows;
  }
}

int initv_rank_count(const Lane& L, const uint32_t* flags, int64_t bound, const uint32_t* nuniq,
                     uint32_t* ftotal, const uint32_t* gate, int64_t* count_dev) {
  const int64_t ntiles = std::max<int64_t>(1, (bound + kIvrTile - 1) / kIvrTile);
  DFX_TRY(L.ws->tiles.ensure(sizeof(uint32_t) * (ntiles + 1)));
  const dim3 g((unsigned)std::min<int64_t>(ntiles, kIvrGrid));
  hipLaunchKernelGGL(k_initv_rank_count, g, dim3(kIvNT), 0, L.stream, flags, bound, nuniq, gate,
                     L.ws->tiles.as<uint32_t>(), ftotal, count_dev, &L.ds->ivr_ticket[0]);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

int initv_rank_draw(Context* c, const Lane& L, const uint32_t* flags, const uint32_t* ftotal,
                    const uint32_t* nuniq, int64_t bound, const uint32_t* segslot,
                    const int64_t* counts_all, int rank, int nranks, uint32_t* fcount,
                    unsigned long long* cap_host) {
  const int64_t ntiles = std::max<int64_t>(1, (bound + kIvrTile - 1) / kIvrTile);
  DFX_TRY(L.ws->tiles.ensure(sizeof(uint32_t) * (ntiles + 1)));
  const dim3 g((unsigned)std::min<int64_t>(ntiles, kIvrGrid));
  hipLaunchKernelGGL(k_initv_rank_draw, g, dim3(kIvNT), 0, L.stream, flags, bound, nuniq, ftotal,
                     L.ws->tiles.as<uint32_t>(), segslot, counts_all, rank, nranks, c->T,
                     c->P.V_init_scale, c->ds, fcount, &L.ds->ivr_ticket[1], cap_host);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

int run_initv(Context* c, int64_t n_bound, const uint32_t* flags, const uint32_t* slot,
              const DevState* nds, const FinArgs* fin) {
  if (c->P.V_dim <= 0 || n_bound <= 0) return DFX_OK;
  if (fin) {  // the fused step
    const int64_t ntiles = (n_bound + kIvTile - 1) / kIvTile;
    Workspace& ws = c->ws;
    void* before = ws.ivstat.p;
    DFX_TRY(ws.ivstat.ensure((size_t)ntiles * 8));
    if (ws.ivstat.p != before)  // fresh words read as unpublished (tag 0, flag 0)
      DFX_HIP(hipMemsetAsync(ws.ivstat.p, 0, ws.ivstat.bytes, c->stream));
    hipLaunchKernelGGL(k_initv_onepass, dim3((unsigned)ntiles), dim3(kIvNT), 0, c->stream, flags,
                       slot, c->T, c->P.V_init_scale, c->ds, nds, &c->ds->n_init,
                       ws.ivstat.as<unsigned long long>(), *fin);
    DFX_HIP(hipGetLastError());
    return DFX_OK;
  }
  // one owner: its count is every owner's (DevState::iv_count, read back by the draw)
  const Lane L = main_lane(c);
  const uint32_t* nuniq = nds ? &nds->u_count : nullptr;
  uint32_t* ftotal = &c->ds->totals[0];
  int64_t* count = reinterpret_cast<int64_t*>(&c->ds->iv_count);
  DFX_TRY(initv_rank_count(L, flags, n_bound, nuniq, ftotal, nullptr, count));
  return initv_rank_draw(c, L, flags, ftotal, nuniq, n_bound, slot, count, 0, 1, nullptr);
}

// ---- push_agg=ranks: the draws in (pushing rank, key) order --------------------------------------
// flagged keys (key order; excl: the exclusive scan of their flags) -> rank keys, segment
// payloads for the stable sort by rank that follows (it reads the first *ftotal of them).
// Strided over a capped grid.
__global__ void k_initv_byrank_list(const uint32_t* excl, const uint32_t* ftotal,
                                    const uint32_t* frank, const uint32_t* nuniq, int64_t bound,
                                    uint32_t* rk, uint32_t* rv) {
  const uint32_t F = *ftotal;
  if (F == 0) return;  // no InitV this step (the steady state)
  const int64_t n = ivr_n(nuniq, bound);
  for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n;
       u += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t e = excl[u];
    const uint32_t nx = (u + 1 < n) ? excl[u + 1] : F;
    if (nx != e) {
      rk[e] = frank[u];
      rv[e] = (uint32_t)u;
    }
  }
}

// the q-th segment of the sorted list is the q-th draw
__global__ __launch_bounds__(kIvNT) void k_initv_byrank_draw(const uint32_t* rv0,
                                                             const uint32_t* rv1,
                                                             const uint32_t* ftotal,
                                                             const uint32_t* segslot, Table T,
                                                             float scale, DevState* ds,
                                                             const unsigned int* sortmeta) {
  __shared__ uint32_t s_st[kIvNT], s_vr[kIvNT], s_A[kIvMaxD], s_C[kIvMaxD];
  const int64_t F = (int64_t)*ftotal;
  if (F == 0) return;
  const uint32_t* rv = sortmeta[31] ? rv1 : rv0;
  const uint32_t seed = ds->seed;
  const uint64_t nv0 = ds->n_vrows;
  initv_jumps(T.d, s_A, s_C);
  for (int64_t q0 = (int64_t)blockIdx.x * kIvNT; q0 < F; q0 += (int64_t)gridDim.x * kIvNT) {
    const int64_t q = q0 + threadIdx.x;
    if (q < F)
      s_vr[threadIdx.x] = initv_place(T, seed, nv0, (uint32_t)q, (uint64_t)q, segslot[rv[q]],
                                      &ds->err, &s_st[threadIdx.x]);
    __syncthreads();
    initv_draw(T, (uint32_t)std::min<int64_t>(F - q0, kIvNT), s_st, s_vr, scale, s_A, s_C);
    __syncthreads();
  }
}

__global__ void k_initv_byrank_finalize(const uint32_t* ftotal, Table T, DevState* ds,
                                        uint32_t* fcount) {
  *fcount = 0u;  // the flag count of the next Update of this slot
  initv_advance(ds, T.d, *ftotal, *ftotal, T.vcap);
}

int initv_by_rank(Context* c, const Lane& OL, int64_t R, int nranks, const uint32_t* segslot) {
  Workspace& ws = *OL.ws;
  uint32_t* flags = ws.oflags.as<uint32_t>();
  uint32_t* nuniq = &OL.ds->totals[1];
  uint32_t* ftotal = &OL.ds->totals[2];
  uint32_t* fcount = &OL.ds->totals[3];
  // gated on the device by the flag count: the scan, the sort and the draws exit at once
  // when no key asked for V (the steady state)
  DFX_TRY(scan_u32(OL, flags, R, ftotal, nuniq, fcount));
  uint32_t* rk0 = ws.vals0.as<uint32_t>();
  uint32_t* rv0 = ws.vals1.as<uint32_t>();
  uint32_t* rk1 = reinterpret_cast<uint32_t*>(ws.keys0.as<uint64_t>());
  uint32_t* rv1 = reinterpret_cast<uint32_t*>(ws.keys1.as<uint64_t>());
  const dim3 igrid((unsigned)std::min<int64_t>((R + kIvNT - 1) / kIvNT, 1024));
  hipLaunchKernelGGL(k_initv_byrank_list, igrid, dim3(kIvNT), 0, OL.stream, flags, ftotal,
                     ws.ofrank.as<uint32_t>(), nuniq, R, rk0, rv0);
  int bits = 0;
  while ((1 << bits) < nranks) ++bits;
  // stable by rank, over the *ftotal flagged keys
  DFX_TRY(radix_sort_pairs<uint32_t>(OL, rk0, rv0, rk1, rv1, R, 0, bits > 0 ? 8 : 0, nullptr,
                                     OL.ds->sortmeta, ftotal));
  hipLaunchKernelGGL(k_initv_byrank_draw, igrid, dim3(kIvNT), 0, OL.stream, rv0, rv1, ftotal,
                     segslot, c->T, c->P.V_init_scale, c->ds, OL.ds->sortmeta);
  hipLaunchKernelGGL(k_initv_byrank_finalize, dim3(1), dim3(1), 0, OL.stream, ftotal, c->T, c->ds,
                     fcount);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

}  // namespace dfx
