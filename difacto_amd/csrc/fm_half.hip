// The fused step over half rows (kwarg vrows=f16, V_dim 32 / 64): k_fm_bwd_h, k_fm_fwd_h and their
// launchers.  A half table is the split layout — 32-byte entries, vrow = a pool row — whose pool
// row is [V: d fp16 | Vaux: d fp16], 4 d bytes: one 128-byte line at d = 32, two adjacent ones at
// d = 64, where fp32 rows take two and four.  Both kernels give a key G = d / 8 lanes, lane l the
// coordinates 8l..8l+7, which are one 16-byte piece of V and one of Vaux: a lane's whole share of a
// row is two loads, widened in registers (f16_widen, the integer path: the conversion instruction
// quiets signalling NaN patterns, so it is not f16_widen on all 65536), and the arithmetic is fp32
// throughout.  Built without packed fp32 arithmetic, as fm_line.hip is (Makefile).  V_dim 128
// (kwarg vrows=f16wide) has the same rows and kernels of another shape, further down.
#include <algorithm>

#include "fm_bwd_sums.h"
#include "fm_fwd_out.h"

namespace dfx {

// ---- the fused backward -------------------------------------------------------------------------
// Two dependent trips per key, as in the split layout (the row's address is the entry's vrow), each
// issued once by the group:
//   the entry    lane l loads half l % 2 — {w, vrow, sqrt_g, z} / {fea_cnt, pad, key} — so the
//                group's requests are the two halves of one 32-byte entry, and the halves reach
//                every lane from lanes 0 and 1: by quad_perm moves in the VALU at G = 4 (the group
//                is a DPP quad, fm_line.hip's k_fm_bwd_line16), by shuffles at G = 8.  k_fm_bwd has
//                every lane load both halves (2 G requests per key where this has G); "lane 0 loads"
//                would leave the broadcast four shuffles longer and the other lanes idle in the trip
//   the row      lane l loads V piece l and Vaux piece l: at d = 32 the eight pieces of one line
//                from four lanes, at d = 64 sixteen pieces of two adjacent lines from eight
// beside the first UNR occurrences' p and XV*p.  The key check, find-or-insert, dead / flags / slot
// and the block's counts are k_fm_bwd_line's; the sums are bwd_key_sums<G, 8> (k_fm_bwd's bwd_cpl = 8
// lane layout: every coordinate's terms and their order are one lane's own, so the sums are those
// of a vrows=f32 table that holds the same values, bit for bit; a chunked key reads its partials).
// FTRL, then AdaGrad per coordinate from the widened old values (adagrad_update), then the two
// stochastic rounds (vhalf.h) — and one 16-byte store of V, one of Vaux per lane, the hot entry
// half from lane 0.
template <int CTRL>
__device__ __forceinline__ float4 quad_perm4(float4 v) {
  auto mv = [](float x) {
    const int i = __float_as_int(x);
    return __int_as_float(__builtin_amdgcn_update_dpp(i, i, CTRL, 0xF, 0xF, false));
  };
  return make_float4(mv(v.x), mv(v.y), mv(v.z), mv(v.w));
}

template <int G>
__device__ __forceinline__ void half_entry_load(const Table& T, int64_t s, int l, int gb, bool nt,
                                                float4* h0, float4* h1) {
  const float4 eh = ld4(reinterpret_cast<const float*>(ent_at(T, s)) + 4 * (l & 1), nt);
  if constexpr (G == 4) {
    *h0 = quad_perm4<0x00>(eh);  // quad_perm:[0,0,0,0]
    *h1 = quad_perm4<0x55>(eh);  // quad_perm:[1,1,1,1]
  } else {
    *h0 = make_float4(__shfl(eh.x, gb, kWave), __shfl(eh.y, gb, kWave), __shfl(eh.z, gb, kWave),
                      __shfl(eh.w, gb, kWave));
    *h1 = make_float4(__shfl(eh.x, gb + 1, kWave), __shfl(eh.y, gb + 1, kWave),
                      __shfl(eh.z, gb + 1, kWave), __shfl(eh.w, gb + 1, kWave));
  }
}

template <int G>
__global__ __launch_bounds__(kFmNT) void k_fm_bwd_h(BwdArgs a) {
  constexpr int CPL = 8, UNR = 2, SPB = kFmNT / G, d = 8 * G;
  const int g = threadIdx.x / G;
  const int l = threadIdx.x % G;
  const int gb = (int)(threadIdx.x % kWave) - l;
  const int64_t u = (int64_t)blockIdx.x * SPB + g;
  const int64_t nseg = a.nseg_host >= 0 ? a.nseg_host : (int64_t)a.ds->u_count;
  int dnew = 0, ninit = 0, nins = 0;
  unsigned nlive = 0, nlocc = 0;
  if (u < nseg) {
    const bool ntb = (a.nt & kNtBwdTable) != 0, nto = (a.nt & kNtBwdOcc) != 0;
    const uint32_t s0 = ldnt(a.segstart + u, nto), s1 = ldnt(a.segstart + u + 1, nto);
    const uint32_t cidx = a.segcol ? a.segcol[u] : (uint32_t)u;
    const bool valued = a.occ_x != nullptr;
    const int64_t xs = a.xs > d ? a.xs : d;
    const uint32_t len = s1 - s0;
    // ---- trip 1: the key's entry (its home slot, or the slot the Get pass found) and the first
    // UNR occurrences of its segment, mutually independent
    uint64_t key = 0;
    uint32_t sl = a.insert_keys ? 0u : a.slot[cidx];
    bool dead = !a.insert_keys && sl == kNoSlot;
    if (a.insert_keys) {
      key = ldnt(a.uniq + cidx, nto);
      sl = (uint32_t)tbl_hash(key, a.T);
    }
    float4 h0, h1;
    half_entry_load<G>(a.T, dead ? 0 : (int64_t)sl, l, gb, ntb, &h0, &h1);
    uint32_t row[UNR];
    float x[UNR];
#pragma unroll
    for (int t = 0; t < UNR; ++t) {
      const uint32_t i = s0 + ((uint32_t)t < len ? (uint32_t)t : 0u);
      row[t] = occ_get(a, i, valued, nto, &x[t]);
    }
    // ---- the key check: Get's find-or-insert (model_[key]) for a key away from home
    if (a.insert_keys) {
      const uint64_t ek =
          ((uint64_t)__float_as_uint(h1.w) << 32) | (uint64_t)__float_as_uint(h1.z);
      if (ek != key) {  // group-uniform
        int sf = 0;
        if (l == 0) {
          bool inserted;
          const int64_t r = tbl_insert(a.T, key, &inserted);
          if (r < 0) atomicOr(&a.dsw->err, insert_error(r));
          sf = r < 0 ? (int)kNoSlot : (int)r;
          nins = inserted ? 1 : 0;
        }
        sl = (uint32_t)__shfl(sf, gb, kWave);
        dead = sl == kNoSlot;
        if (!dead) half_entry_load<G>(a.T, (int64_t)sl, l, gb, ntb, &h0, &h1);
      }
    }
    if (dead) {  // not in the table (the error word says why): read as absent, no update
      h0 = make_float4(0.f, __int_as_float(-1), 0.f, 0.f);
      h1.x = 0.f;
    }
    float4 e = make_float4(h0.x, h0.z, h0.w, h1.x);  // {w, sqrt_g, z, fea_cnt}
    const int vrow = __float_as_int(h0.y);
    // V was pulled iff present and not (l1_shrk && w == 0) (SGDUpdater::Get, :40-43)
    const int vq = (vrow >= 0 && !(a.Pm.l1_shrk && e.x == 0.f)) ? vrow : -1;
    // ---- trip 2: the lane's pieces of V and Vaux, p and XV*p of the first occurrences' rows (a
    // key whose V takes no part reads the zero pad: 16-byte pieces at 16 l and 16 (G + l) bytes)
    const float* zp = a.zpad + ((cidx & 255u) << 4);
    uint16_t* hr = vq >= 0 ? half_row(a.T, vq) : nullptr;
    const uint16_t* rd = vq >= 0 ? hr : reinterpret_cast<const uint16_t*>(zp);
    const dfx_u4v pv = ldh(rd + 8 * l, ntb), pc = ldh(rd + d + 8 * l, ntb);
    float g0[CPL], pr[UNR], xr[UNR][CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) g0[k] = 0.f;
#pragma unroll
    for (int t = 0; t < UNR; ++t) {
      pr[t] = xs > d ? a.XVp[(int64_t)row[t] * xs + d] : a.p[row[t]];
      load_coords<CPL, true>(vq >= 0 ? a.XVp + (int64_t)row[t] * xs : zp, l, d, xr[t]);
    }
    float vcur[CPL], ccur[CPL];
    half8_widen(pv, vcur);
    half8_widen(pc, ccur);
    float gw = 0.f, acc[CPL];
    bwd_key_sums<G, CPL, true, UNR>(a, l, u, s0, s1, valued, d, xs, vq, row, x, pr, xr, vcur, g0, gw,
                                    acc);
    // Update(kGradient): UpdateW (FTRL), then UpdateV (AdaGrad) if V was pulled; the new V and the
    // new accumulator narrow to fp16 for the stores only (eta and V have used them unrounded)
    bool tr;
    const int dw = ftrl_update(a.Pm, gw, &e, &tr);
    if (!dead && l == 0) st4(reinterpret_cast<float*>(ent_at(a.T, (int64_t)sl)),
                             make_float4(e.x, __int_as_float(vrow), e.y, e.z), ntb);
    if (vq >= 0) {
      uint32_t hv[CPL], hc[CPL];
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const float gk = acc[k] + a.Pm.V_l2 * vcur[k];  // adagrad_update's g
        adagrad_update(a.Pm, acc[k], &vcur[k], &ccur[k]);
        hv[k] = vhalf_round(vcur[k], gk, e.y, CPL * l + k);
        hc[k] = vaux16_round(ccur[k], gk, e.y, CPL * l + k);
      }
      sth(hr + 8 * l, half8_pack(hv), ntb);
      sth(hr + d + 8 * l, half8_pack(hc), ntb);
    }
    if (l == 0) {
      dnew = dead ? 0 : dw;
      // InitV on a 0 -> nonzero transition (sgd_updater.cc:118-121); e.w is fea_cnt
      const bool need = !dead && tr && vrow < 0 && e.w > (float)a.Pm.V_threshold;
      a.flags[u] = need ? 1u : 0u;
      // InitV's slot: it reads the slots of flagged keys only (in the steady state none)
      if (need && a.insert_keys) a.slot[cidx] = sl;
      ninit = need ? 1 : 0;
      nlive = vq >= 0 ? 1u : 0u;
      nlocc = vq >= 0 ? len : 0u;
    }
  }
  bwd_block_stats(a, dnew, ninit, nins, nlive, nlocc);
}

static bool half_table_ok(const Table& T, int d) {
  return T.half && !T.es && !T.line && T.d == d && (d == 32 || d == 64 || d == 128);
}

// V_dim 128 (vrows=f16wide, below)
template <bool VALUED>
static int launch_fwd_half_wide(const FwdArgs& a, hipStream_t st, int* nblk);
// pass V's grid: about one listed key per group (fm.hip kBwdPassVBlocks, for the same reason)
constexpr int64_t kBwdHalfVBlocks = 32768;

int64_t bwd_half_blocks(int d, int64_t nseg_bound) {
  const int64_t spb = kFmNT / (d / 8);
  return (nseg_bound + spb - 1) / spb;
}

int launch_bwd_half(const BwdArgs& a, int64_t nseg_bound, hipStream_t st, long lds,
                    size_t lds_default) {
  const size_t lds_bytes = lds >= 0 ? (size_t)lds : lds_default;
  if (nseg_bound <= 0) return DFX_OK;
  if (!half_table_ok(a.T, a.d) || a.d == 128 || a.vlist) {
    set_error("vrows=f16: the one-pass fused backward needs V_dim 32 or 64 in the split layout "
              "(V_dim 128, vrows=f16wide, runs in two passes: bwd_two_pass=1)");
    return DFX_ERR_ARG;
  }
  const dim3 grid((unsigned)bwd_half_blocks(a.d, nseg_bound));
  if (a.d == 32) hipLaunchKernelGGL(k_fm_bwd_h<4>, grid, dim3(kFmNT), lds_bytes, st, a);
  else hipLaunchKernelGGL(k_fm_bwd_h<8>, grid, dim3(kFmNT), lds_bytes, st, a);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

// ---- the fused forward --------------------------------------------------------------------------
// k_fm_fwd_walk's structure over the split layout: one group of G = d / 8 lanes per row, the
// groups looping over rows on a resident grid; a row's ids staged in LDS kHfIds at a time (one
// coalesced trip); each trip of kHfNB nnz then issues its home-entry reads at once — even lanes
// {w, vrow}, odd lanes the key, 8 bytes each — checks the keys (a key away from home walks its
// probe chain), issues the visible keys' V pieces at once — 16 bytes, eight halves, per lane: 64
// bytes of one line per nnz at d = 32, one whole line at d = 64, where fp32 rows are one and two
// lines — and adds the trip in nnz order.  A coordinate's sums are one lane's, in nnz order, from
// the widened values, and the row ends in fwd_row_out (s over l = 0..d-1 in order): on a table
// whose V is all fp16-representable, pred, p and XV*p are k_fm_fwd_probe's over the same values
// in a vrows=f32 table, bit for bit.
constexpr int kHfNB = 8;
constexpr int kHfIds = (40 / kHfNB) * kHfNB;

template <int G, bool VALUED>
__global__ __launch_bounds__(kFmNT, 2) void k_fm_fwd_h(FwdArgs a) {
  constexpr int RPB = kFmNT / G, CPL = 8, d = 8 * G;
  __shared__ uint64_t s_id[RPB][kHfIds];
  __shared__ float s_x[VALUED ? RPB : 1][VALUED ? kHfIds : 1];
  __shared__ double red[kFmNT / kWave];
  const int g = threadIdx.x / G;
  const int l = threadIdx.x % G;
  const int gbase = (threadIdx.x % kWave) - l;
  const bool ntf = (a.nt & kNtFwdTable) != 0;
  double loss = 0;
  const int64_t rstride = (int64_t)gridDim.x * RPB;
  for (int64_t ri = (int64_t)blockIdx.x * RPB + g; ri < a.B; ri += rstride) {
    const int64_t r = fwd_row(a, ri);
    const uint64_t o0 = a.offs[r], o1 = a.offs[r + 1];
    float acc = 0.f;
    float xv[CPL], xxvv[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) { xv[k] = 0.f; xxvv[k] = 0.f; }
    uint64_t c_end = o0;  // the staged ids end here
    for (uint64_t j0 = o0; j0 < o1; j0 += kHfNB) {
      if (j0 >= c_end) {  // the row's next kHfIds ids, one trip (group-uniform)
        __builtin_amdgcn_wave_barrier();  // the last chunk's reads are done
#pragma unroll
        for (int m = 0; m < (kHfIds + G - 1) / G; ++m) {
          const uint64_t j = j0 + l + (uint64_t)G * m;
          if (j < o1 && l + G * m < kHfIds) {
            s_id[g][l + G * m] = a.index[j];
            if (VALUED) s_x[g][l + G * m] = a.val[j];
          }
        }
        __builtin_amdgcn_wave_barrier();
        c_end = j0 + kHfIds;
      }
      const int cb = (int)(j0 - (c_end - kHfIds));  // this trip's first id in the chunk
      const int nin = (int)((o1 - j0) < (uint64_t)kHfNB ? (o1 - j0) : (uint64_t)kHfNB);
      auto key_of = [&](int i) {
        const uint64_t id = s_id[g][i];
        const uint64_t mm = a.max_index == ~0ull ? (id == ~0ull ? 0ull : id) : id % a.max_index;
        return a.keys_ready ? id : reverse_bytes(mm);
      };
      // ---- the trip's home entries, all in flight
      float2 eh[kHfNB];  // even lanes {w, vrow}, odd lanes the key
#pragma unroll
      for (int t = 0; t < kHfNB; ++t) {
        const uint64_t key = key_of(cb + (t < nin ? t : nin - 1));
        const float* sl = reinterpret_cast<const float*>(ent_at(a.T, tbl_hash(key, a.T)));
        eh[t] = ld2(sl + ((l & 1) ? 6 : 0), ntf);
      }
      // ---- the key checks, then the visible keys' V pieces, all in flight
      float w[kHfNB];
      int vr[kHfNB];
      dfx_u4v pv[kHfNB];
#pragma unroll
      for (int t = 0; t < kHfNB; ++t) {
        w[t] = 0.f;
        vr[t] = -1;
        if (t < nin) {  // group-uniform
          const uint64_t key = key_of(cb + t);
          const float k0 = __shfl(eh[t].x, gbase + 1, kWave), k1 = __shfl(eh[t].y, gbase + 1, kWave);
          uint64_t ek = ((uint64_t)__float_as_uint(k1) << 32) | (uint64_t)__float_as_uint(k0);
          w[t] = __shfl(eh[t].x, gbase, kWave);
          vr[t] = __float_as_int(__shfl(eh[t].y, gbase, kWave));
          if (ek != key && ek != kEmptyKey) {  // a longer probe chain (group-uniform)
            uint64_t h = tbl_hash(key, a.T);
            for (uint64_t probe = 0; ek != key && ek != kEmptyKey && probe < a.T.mask; ++probe) {
              h = (h + 1) & a.T.mask;
              ek = ent_at(a.T, h)->key;
            }
            if (ek == key) {
              const Entry* e = ent_at(a.T, h);
              w[t] = e->w;
              vr[t] = e->vrow;
            }
          }
          // absent (inserted by this training step's backward): w = 0, no V
          if (ek != key) { w[t] = 0.f; vr[t] = -1; }
          // V is visible only if present and not (l1_shrk && w == 0) (sgd_updater.cc:40-43)
          if (a.l1_shrk && w[t] == 0.f) vr[t] = -1;
        }
        const uint16_t* rd = vr[t] >= 0 ? half_row(a.T, vr[t])
                                        : reinterpret_cast<const uint16_t*>(a.zpad + (t << 4));
        pv[t] = ldh(rd + 8 * l, ntf);
      }
      // ---- the trip's sums, in nnz order
#pragma unroll
      for (int t = 0; t < kHfNB; ++t) {
        if (t >= nin) break;  // group-uniform
        const float x = VALUED ? s_x[g][cb + t] : 1.f;
        // SpMV::Times skips w == 0 (spmv.h:124-125)
        if (w[t] != 0.f) acc = VALUED ? acc + w[t] * x : acc + w[t];
        if (vr[t] >= 0) {
          float vk[CPL];
          half8_widen(pv[t], vk);
          const float xx = x * x;  // XX_ (fm_loss.h:86-92)
#pragma unroll
          for (int k = 0; k < CPL; ++k) {
            xv[k] = VALUED ? xv[k] + vk[k] * x : xv[k] + vk[k];
            const float q = vk[k] * vk[k];  // VV (fm_loss.h:95-101)
            xxvv[k] = VALUED ? xxvv[k] + q * xx : xxvv[k] + q;
          }
        }
      }
    }
    fwd_row_out<G, CPL, d>(a, r, l, gbase, acc, xv, xxvv, &loss);
  }
  if (a.part) return;  // block-uniform: no loss partial in split mode
  for (int off = 32; off > 0; off >>= 1) loss += __shfl_xor(loss, off, kWave);
  if (lane_id() == 0) red[threadIdx.x / kWave] = loss;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int i = 0; i < kFmNT / kWave; ++i) s += red[i];
    a.loss_part[blockIdx.x] = s;
  }
}

template <int G, bool VALUED>
static int launch_fwd_half_g(const FwdArgs& a, hipStream_t st, int* nblk) {
  static int64_t resident = 0;  // per kernel
  const int64_t rpb = kFmNT / G, want = (a.B + rpb - 1) / rpb;
  if (resident <= 0) resident = resident_grid_for(k_fm_fwd_h<G, VALUED>, INT32_MAX);
  *nblk = (int)std::min<int64_t>(want, resident);
  hipLaunchKernelGGL((k_fm_fwd_h<G, VALUED>), dim3((unsigned)*nblk), dim3(kFmNT), 0, st, a);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

int launch_fwd_half(const FwdArgs& a, hipStream_t st, int* nblk) {
  *nblk = 0;
  if (!half_table_ok(a.T, a.d) || !a.index || a.part) {
    set_error("vrows=f16 / f16wide: the fused forward needs V_dim 32, 64 or 128 in the split layout "
              "and the batch's feature ids (the single context's fused step)");
    return DFX_ERR_ARG;
  }
  if (a.B <= 0) return DFX_OK;
  if (a.d == 128)
    return a.val ? launch_fwd_half_wide<true>(a, st, nblk) : launch_fwd_half_wide<false>(a, st, nblk);
  if (a.d == 32)
    return a.val ? launch_fwd_half_g<4, true>(a, st, nblk) : launch_fwd_half_g<4, false>(a, st, nblk);
  return a.val ? launch_fwd_half_g<8, true>(a, st, nblk) : launch_fwd_half_g<8, false>(a, st, nblk);
}

// ================================================================================================
// V_dim 128 (kwarg vrows=f16wide): the pool row is [V: 128 fp16 | Vaux: 128 fp16], 512 bytes, four
// adjacent lines where fp32 rows take eight.  A key is on 16 lanes, lane l the coordinates
// 8l..8l+7 — one 16-byte piece of V and one of Vaux, as above — but the step around the rows is the
// wide fp32 step's (fm.hip), not the one above: the backward runs in two passes, pass W
// (k_fm_bwd_w, which reads entries only and so serves this table as it is) and the pass V below over
// the keys pass W listed, and the chunk kernels (XV*p rows and p only) are the fp32 step's.
constexpr int kHwG = 16;  // lanes per row (forward) and per listed key (pass V)
// V pieces in flight per lane and trip of the forward: 8 x 16 bytes are 32 VGPRs beside the row's
// 16 sums, and the kernel compiles to ~110, four waves a SIMD; a whole lookup trip of 16 in flight
// is 32 more, three waves (by the register count; not measured)
constexpr int kHwNB = 8;

// ---- the forward --------------------------------------------------------------------------------
// With 16 lanes a row the lookups are spread over them (k_fm_fwd_probe's way) where k_fm_fwd_h has
// every lane of the group request every entry: a trip takes 16 nnz, lane l reads nnz l's id and
// value (one coalesced read each: no staging in LDS, the lanes' registers are the stage), forms the
// key, reads the home entry's {w, vrow} and key — the 16 home-entry reads of a trip are one issue
// — and walks the probe chain of a key away from home on its own.  Then kHwNB nnz at a time:
// their vrow comes from the lane that found it, every lane requests its piece of each visible
// key's V (one nnz: 16 lanes x 16 bytes, the V half of the row, two lines), all in flight, and
// the sums follow in nnz order from the widened values.  The row ends in fwd_row_out<16, 8, 128>:
// on a table whose V is all fp16-representable pred, p and XV*p are k_fm_fwd_probe's over the
// same values in a vrows=f32 table, bit for bit.
template <bool VALUED>
__global__ __launch_bounds__(kFmNT, 2) void k_fm_fwd_hw(FwdArgs a) {
  constexpr int G = kHwG, RPB = kFmNT / G, CPL = 8, d = 128;
  __shared__ double red[kFmNT / kWave];
  const int g = threadIdx.x / G;
  const int l = threadIdx.x % G;
  const int gbase = (threadIdx.x % kWave) - l;
  const bool ntf = (a.nt & kNtFwdTable) != 0;
  double loss = 0;
  const int64_t rstride = (int64_t)gridDim.x * RPB;
  for (int64_t ri = (int64_t)blockIdx.x * RPB + g; ri < a.B; ri += rstride) {
    const int64_t r = fwd_row(a, ri);
    const uint64_t o0 = a.offs[r], o1 = a.offs[r + 1];
    float acc = 0.f;
    float xv[CPL], xxvv[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) { xv[k] = 0.f; xxvv[k] = 0.f; }
    for (uint64_t j0 = o0; j0 < o1; j0 += G) {
      // ---- the lookup trip: this lane's nnz (a lane past the row's end holds w = 0, no V)
      float w = 0.f, x = 1.f;
      int vr = -1;
      if (j0 + l < o1) {
        const uint64_t id = a.index[j0 + l];
        if (VALUED) x = a.val[j0 + l];
        const uint64_t mm = a.max_index == ~0ull ? (id == ~0ull ? 0ull : id) : id % a.max_index;
        const uint64_t key = a.keys_ready ? id : reverse_bytes(mm);
        uint64_t h = tbl_hash(key, a.T);
        const float* sl = reinterpret_cast<const float*>(ent_at(a.T, h));
        const float2 e0 = ld2(sl, ntf), e1 = ld2(sl + 6, ntf);  // {w, vrow}, the key
        uint64_t ek = ((uint64_t)__float_as_uint(e1.y) << 32) | (uint64_t)__float_as_uint(e1.x);
        w = e0.x;
        vr = __float_as_int(e0.y);
        if (ek != key && ek != kEmptyKey) {  // a longer probe chain
          for (uint64_t probe = 0; ek != key && ek != kEmptyKey && probe < a.T.mask; ++probe) {
            h = (h + 1) & a.T.mask;
            ek = ent_at(a.T, h)->key;
          }
          if (ek == key) {
            const Entry* e = ent_at(a.T, h);
            w = e->w;
            vr = e->vrow;
          }
        }
        // absent (inserted by this training step's backward): w = 0, no V
        if (ek != key) { w = 0.f; vr = -1; }
        // V is visible only if present and not (l1_shrk && w == 0) (sgd_updater.cc:40-43)
        if (a.l1_shrk && w == 0.f) vr = -1;
      }
      const int nin = (int)((o1 - j0) < (uint64_t)G ? (o1 - j0) : (uint64_t)G);
#pragma unroll
      for (int t0 = 0; t0 < G; t0 += kHwNB) {
        if (t0 >= nin) break;  // group-uniform
        // ---- the visible keys' V pieces, all in flight (the others read the zero pad)
        int vt[kHwNB];
        dfx_u4v pv[kHwNB];
#pragma unroll
        for (int t = 0; t < kHwNB; ++t) {
          vt[t] = __shfl(vr, gbase + t0 + t, kWave);
          const uint16_t* rd = vt[t] >= 0 ? half_row(a.T, vt[t])
                                          : reinterpret_cast<const uint16_t*>(a.zpad + (t << 4));
          pv[t] = ldh(rd + 8 * l, ntf);
        }
        // ---- the sums, in nnz order
#pragma unroll
        for (int t = 0; t < kHwNB; ++t) {
          const float wt = __shfl(w, gbase + t0 + t, kWave);
          const float xt = VALUED ? __shfl(x, gbase + t0 + t, kWave) : 1.f;
          // SpMV::Times skips w == 0 (spmv.h:124-125)
          if (wt != 0.f) acc = VALUED ? acc + wt * xt : acc + wt;
          if (vt[t] >= 0) {
            float vk[CPL];
            half8_widen(pv[t], vk);
            const float xx = xt * xt;  // XX_ (fm_loss.h:86-92)
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
              xv[k] = VALUED ? xv[k] + vk[k] * xt : xv[k] + vk[k];
              const float q = vk[k] * vk[k];  // VV (fm_loss.h:95-101)
              xxvv[k] = VALUED ? xxvv[k] + q * xx : xxvv[k] + q;
            }
          }
        }
      }
    }
    fwd_row_out<G, CPL, d>(a, r, l, gbase, acc, xv, xxvv, &loss);
  }
  if (a.part) return;  // block-uniform: no loss partial in split mode
  for (int off = 32; off > 0; off >>= 1) loss += __shfl_xor(loss, off, kWave);
  if (lane_id() == 0) red[threadIdx.x / kWave] = loss;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0;
    for (int i = 0; i < kFmNT / kWave; ++i) s += red[i];
    a.loss_part[blockIdx.x] = s;
  }
}

template <bool VALUED>
static int launch_fwd_half_wide(const FwdArgs& a, hipStream_t st, int* nblk) {
  static int64_t resident = 0;  // per kernel
  const int64_t rpb = kFmNT / kHwG, want = (a.B + rpb - 1) / rpb;
  if (resident <= 0) resident = resident_grid_for(k_fm_fwd_hw<VALUED>, INT32_MAX);
  *nblk = (int)std::min<int64_t>(want, resident);
  hipLaunchKernelGGL((k_fm_fwd_hw<VALUED>), dim3((unsigned)*nblk), dim3(kFmNT), 0, st, a);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

// ---- the backward's pass V ------------------------------------------------------------------------
// Pass W (fm.hip k_fm_bwd_w<true>) has updated every key's entry and listed the keys whose V was
// pulled as {first occurrence or first chunk partial, V row, XXp, length}, and beside the list
// the entry's new sqrt_g per listed key (bwd_list_sg: the roundings hash it).  Here a listed key
// takes 16 lanes: lane l loads its V piece and its Vaux piece — 32 pieces, the row's four lines,
// each byte requested once — beside the first trip's occurrences.  The sums are k_fm_bwd_v's at 8
// coordinates per lane: grad_u = (0 - V XXp) + sum (XV*p) x in occurrence order, 16 occurrences
// per trip (lane l reads occurrence l's row and value, the terms shuffled from the lanes in
// order) with UNR rows of XV*p in flight; a chunked key reads its partials in double, exactly as
// the fp32 pass does.  Every coordinate's terms and order are one lane's own: the sums are those
// of a vrows=f32 table that holds the same values.  Then adagrad_update from the widened old
// values, the two stochastic rounds (vhalf.h, j the coordinate's index in the row), and one
// 16-byte store of V and one of Vaux per lane.

// pass W's per-block counts into the step's counters, by pass V's first block (fm.hip
// bwd_fold_wstat's sums)
__device__ __forceinline__ void half_fold_wstat(const BwdArgs& a) {
  __shared__ long long rs[kFmNT / kWave];
  __shared__ unsigned rq[kFmNT / kWave];
  __shared__ unsigned long long ri[kFmNT / kWave];
  long long s = 0;
  unsigned q = 0;
  unsigned long long i2 = 0;
  for (int i = threadIdx.x; i < a.nwstat; i += kFmNT) {
    const int4 w = a.wstat[i];
    s += w.x;
    q += (unsigned)w.y;
    i2 += (unsigned long long)w.z;
  }
  for (int off = 32; off > 0; off >>= 1) {
    s += __shfl_xor(s, off, kWave);
    q += __shfl_xor(q, off, kWave);
    i2 += __shfl_xor(i2, off, kWave);
  }
  if (lane_id() == 0) {
    rs[threadIdx.x / kWave] = s;
    rq[threadIdx.x / kWave] = q;
    ri[threadIdx.x / kWave] = i2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < kFmNT / kWave; ++i) {
      s += rs[i];
      q += rq[i];
      i2 += ri[i];
    }
    if (s) atomicAdd((unsigned long long*)&a.dsw->new_w, (unsigned long long)s);
    if (q) atomicAdd(&a.dsw->n_init, q);
    if (i2) atomicAdd(&a.dsw->n_keys, i2);
  }
}

__global__ __launch_bounds__(kFmNT) void k_fm_bwd_hv(BwdArgs a) {
  constexpr int G = kHwG, CPL = 8, EPB = kFmNT / G, UNR = 4, d = 128;
  const int g = threadIdx.x / G;
  const int l = threadIdx.x % G;
  const int gb = (int)(threadIdx.x % kWave) - l;
  if (blockIdx.x == 0) half_fold_wstat(a);
  const int64_t n = (int64_t)*a.vcount;
  const int64_t xs = a.xs > d ? a.xs : d;
  const bool valued = a.occ_x != nullptr;
  const bool ntb = (a.nt & kNtBwdTable) != 0;
  const float* lsg = bwd_list_sg(a);
  for (int64_t j = (int64_t)blockIdx.x * EPB + g; j < n; j += (int64_t)gridDim.x * EPB) {
    const uint4 it = a.vlist[j];
    const float sg = lsg[j];
    const int vq = (int)it.y;
    const float xxp = __uint_as_float(it.z);
    const uint32_t len = it.w;
    const uint32_t s0 = it.x, s1 = s0 + len;  // (it.x is the first chunk of a chunked key)
    const bool chunked = a.choff && len > (uint32_t)kChunkOcc;
    // ---- one trip: the lane's pieces of V and Vaux, and the first occurrences' rows and values
    uint16_t* hr = half_row(a.T, vq);
    const dfx_u4v pv = ldh(hr + 8 * l, ntb), pc = ldh(hr + d + 8 * l, ntb);
    float xl = 1.f;
    uint32_t rl = 0u;
    if (!chunked) rl = occ_get(a, s0 + (uint32_t)l < s1 ? s0 + (uint32_t)l : s1 - 1, valued, false, &xl);
    float vcur[CPL], ccur[CPL], acc[CPL];
    half8_widen(pv, vcur);
    half8_widen(pc, ccur);
    // grad_u = (g0 - V*XXp) + sum (XV_ p) x, g0 = 0 (fm_loss.h:185-202, spmm.h:127-159)
    if (chunked) {
      const uint32_t nc = hot_chunks_read((len + kChunkOcc - 1) / kChunkOcc);
      double accp[CPL];
#pragma unroll
      for (int k = 0; k < CPL; ++k) accp[k] = 0;
      for (uint32_t c = 0; c < nc; ++c) {
        const double* pp = a.part + (int64_t)(s0 + c) * (d + 2) + 2 + CPL * l;
#pragma unroll
        for (int k = 0; k < CPL; ++k) accp[k] += pp[k];
      }
#pragma unroll
      for (int k = 0; k < CPL; ++k) acc[k] = (float)((double)(0.f - vcur[k] * xxp) + accp[k]);
    } else {
#pragma unroll
      for (int k = 0; k < CPL; ++k) acc[k] = 0.f - vcur[k] * xxp;
      for (uint32_t i0 = s0; i0 < s1; i0 += G) {
        if (i0 != s0) {
          const uint32_t i = i0 + (uint32_t)l < s1 ? i0 + (uint32_t)l : s1 - 1;
          rl = occ_get(a, i, valued, false, &xl);
        }
        const uint32_t nt = s1 - i0 < (uint32_t)G ? s1 - i0 : (uint32_t)G;
#pragma unroll
        for (int t0 = 0; t0 < G; t0 += UNR) {
          if ((uint32_t)t0 >= nt) break;  // group-uniform
          float xw[UNR], xrw[UNR][CPL];
#pragma unroll
          for (int t = 0; t < UNR; ++t) {
            // (lanes past the segment hold its last occurrence: a row that exists, unused)
            const uint32_t r = (uint32_t)__shfl((int)rl, gb + t0 + t, kWave);
            xw[t] = __shfl(xl, gb + t0 + t, kWave);
            load_coords<CPL, true>(a.XVp + (int64_t)r * xs, l, d, xrw[t]);
          }
#pragma unroll
          for (int t = 0; t < UNR; ++t) {
            if ((uint32_t)(t0 + t) < nt) {
#pragma unroll
              for (int k = 0; k < CPL; ++k)
                acc[k] = valued ? acc[k] + xrw[t][k] * xw[t] : acc[k] + xrw[t][k];
            }
          }
        }
      }
    }
    // UpdateV (AdaGrad) per coordinate; the new V and the new accumulator narrow to fp16 for the
    // stores only (eta and V have used them unrounded)
    uint32_t hv[CPL], hc[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
      const float gk = acc[k] + a.Pm.V_l2 * vcur[k];  // adagrad_update's g
      adagrad_update(a.Pm, acc[k], &vcur[k], &ccur[k]);
      hv[k] = vhalf_round(vcur[k], gk, sg, CPL * l + k);
      hc[k] = vaux16_round(ccur[k], gk, sg, CPL * l + k);
    }
    sth(hr + 8 * l, half8_pack(hv), ntb);
    sth(hr + d + 8 * l, half8_pack(hc), ntb);
  }
}

int launch_bwd_half_v(const BwdArgs& a, int64_t nseg_bound, hipStream_t st, size_t lds_bytes) {
  if (!half_table_ok(a.T, a.d) || a.d != 128 || !a.vlist || !a.vcount || !a.wstat) {
    set_error("vrows=f16wide: pass V needs V_dim 128 in the split layout and pass W's list");
    return DFX_ERR_ARG;
  }
  if (nseg_bound <= 0) return DFX_OK;
  const int64_t epb = kFmNT / kHwG;
  const int64_t gv = std::min<int64_t>((nseg_bound + epb - 1) / epb, kBwdHalfVBlocks);
  hipLaunchKernelGGL(k_fm_bwd_hv, dim3((unsigned)gv), dim3(kFmNT), lds_bytes, st, a);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

// ---- f16_widen on the device, all 65536 bit patterns (dfx_half_widen_table) -------------------
__global__ void k_half_widen_table(uint32_t* out) {
  const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
  float f[8];
  dfx_u4v p = {h, h, h, h};
  half8_widen(p, f);  // (the kernels' own path: f[0] is the low half widened)
  out[h] = f32_bits(f[0]);
}

// ---- the narrowing functions on the device (dfx_half_round_table) ------------------------------
// in: n tuples {bits of nv, bits of g, bits of sg, j}; out: n triples {vhalf_round(nv, g, sg, j),
// vaux16_round(|nv|, g, sg, j), f16_nearest(nv)} — the step kernels' own inline functions
__global__ void k_half_round_table(const uint32_t* in, uint32_t* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float nv = bits_f32(in[4 * i]), g = bits_f32(in[4 * i + 1]), sg = bits_f32(in[4 * i + 2]);
  const int j = (int)in[4 * i + 3];
  out[3 * i] = vhalf_round(nv, g, sg, j);
  out[3 * i + 1] = vaux16_round(bits_f32(in[4 * i] & 0x7FFFFFFFu), g, sg, j);
  out[3 * i + 2] = f16_nearest(nv);
}

}  // namespace dfx

using namespace dfx;

extern "C" int dfx_half_widen_table(dfx_ctx* ctx, uint32_t* out_host) {
  DFX_CHECK_ARG(ctx && out_host, "null argument");
  Context* c = &ctx->c;
  DFX_TRY(c->ws.rowtmp.ensure(65536 * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_half_widen_table, dim3(256), dim3(256), 0, c->stream,
                     c->ws.rowtmp.as<uint32_t>());
  DFX_HIP(hipGetLastError());
  DFX_HIP(hipMemcpyAsync(out_host, c->ws.rowtmp.p, 65536 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                         c->stream));
  DFX_HIP(hipStreamSynchronize(c->stream));
  return DFX_OK;
}

extern "C" int dfx_half_round_table(dfx_ctx* ctx, int64_t n, const uint32_t* in_host,
                                    uint32_t* out_host) {
  DFX_CHECK_ARG(ctx && in_host && out_host && n > 0 && n <= (1 << 24), "bad argument");
  Context* c = &ctx->c;
  const size_t in_bytes = (size_t)n * 16, out_bytes = (size_t)n * 12;
  DFX_TRY(c->ws.rowtmp.ensure(in_bytes + out_bytes));
  uint32_t* in = c->ws.rowtmp.as<uint32_t>();
  uint32_t* out = in + 4 * n;
  DFX_HIP(hipMemcpyAsync(in, in_host, in_bytes, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_half_round_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                     in, out, n);
  DFX_HIP(hipGetLastError());
  DFX_HIP(hipMemcpyAsync(out_host, out, out_bytes, hipMemcpyDeviceToHost, c->stream));
  DFX_HIP(hipStreamSynchronize(c->stream));
  return DFX_OK;
}
