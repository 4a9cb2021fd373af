// The fused backward over line slots (kwarg slot_layout=line): k_fm_bwd_line and its launcher;
// and the V_dim 24 line slot with fp16 V and Vaux, whose forward lives here too.
// A translation unit of its own, built without packed fp32 arithmetic (Makefile).
#include "fm_bwd_sums.h"
#include "fm_fwd_out.h"

namespace dfx {

// ---- the fused backward over line slots (kwarg slot_layout=line, V_dim 4 / 8 / 12) ----------
// A line slot [Entry 32 B | V | Vaux | pad] holds a key's whole state in one 128-byte line, as
// 4 + d / 2 pieces of 16 bytes (common.h Table::line).  k_fm_bwd's lanes each load both entry
// halves, V and Vaux — four loads per lane, and Vaux from a second random line in the pool.
// Here the group's G = d / 4 (rounded up to a power of two) lanes request every piece once, in
// one issue to that one line, and the entry's halves reach the other lanes by shuffles:
//   d = 4   G = 1   the lane: both halves, V, Vaux (no shuffle; one line instead of two)
//   d = 8   G = 2   lane l: entry half l, V piece l, Vaux piece l
//   d = 12  G = 4   lanes 0..2: V piece l, Vaux piece l; lane 3 (no coordinates): both halves —
//                   two loads per lane, the eight pieces of the line
// So V and Vaux arrive in the lane that owns their coordinates, the lane layout is k_fm_bwd's
// (lane l: coordinates 4l..4l+3) and the sums are bwd_key_sums': same terms, same order.  The
// key is checked after the trip: away from home (or absent) lane 0 walks the chain / inserts
// (tbl_insert) and the group loads the found slot's line the same way.  The write-back is one
// issue to the line again — the hot entry half from the lane that loaded it (every lane holds
// the same FTRL state), V from its lanes — and Vaux behind it.
template <int G>
__device__ __forceinline__ float4 line_bcast(float4 v, int src) {
  if constexpr (G == 1) return v;
  return make_float4(__shfl(v.x, src, kWave), __shfl(v.y, src, kWave), __shfl(v.z, src, kWave),
                     __shfl(v.w, src, kWave));
}

// the group's trip to slot s: h0 = {w, vrow, sqrt_g, z} and h1 = {fea_cnt, pad, key} in every
// lane, v / c = the lane's V / Vaux coordinates (junk in d = 12's lane 3, which owns none)
template <int G>
__device__ __forceinline__ void line_load(const Table& T, int64_t s, int l, int gb, bool nt,
                                          float4* h0, float4* h1, float (&v)[4], float (&c)[4]) {
  const float* sp = reinterpret_cast<const float*>(ent_at(T, s));
  const int d = T.d;
  float4 fv, fc;
  if constexpr (G == 1) {
    *h0 = ld4(sp, nt);
    *h1 = ld4(sp + 4, nt);
    fv = ld4(sp + 8, nt);
    fc = ld4(sp + 8 + d, nt);
  } else if constexpr (G == 2) {
    const float4 eh = ld4(sp + 4 * l, nt);
    fv = ld4(sp + 8 + 4 * l, nt);
    fc = ld4(sp + 8 + d + 4 * l, nt);
    *h0 = line_bcast<G>(eh, gb);
    *h1 = line_bcast<G>(eh, gb + 1);
  } else {
    static_assert(G == 4, "line slots: 1, 2 or 4 lanes per key");
    const bool el = l == G - 1;  // the entry's lane
    fv = ld4(sp + (el ? 0 : 8 + 4 * l), nt);
    fc = ld4(sp + (el ? 4 : 8 + d + 4 * l), nt);
    *h0 = line_bcast<G>(fv, gb + G - 1);
    *h1 = line_bcast<G>(fc, gb + G - 1);
  }
  v[0] = fv.x; v[1] = fv.y; v[2] = fv.z; v[3] = fv.w;
  c[0] = fc.x; c[1] = fc.y; c[2] = fc.z; c[3] = fc.w;
}

// the write-back to slot s: the hot entry half (unless the key is dead), and V and Vaux when the
// key's V was updated (live)
template <int G>
__device__ __forceinline__ void line_store(const Table& T, int64_t s, int l, bool nt, bool dead,
                                           bool live, float4 e, int vrow, const float (&v)[4],
                                           const float (&c)[4]) {
  float* sp = reinterpret_cast<float*>(ent_at(T, s));
  const int d = T.d;
  const float4 hot = make_float4(e.x, __int_as_float(vrow), e.y, e.z);
  const float4 fv = make_float4(v[0], v[1], v[2], v[3]), fc = make_float4(c[0], c[1], c[2], c[3]);
  if constexpr (G == 4) {
    const bool el = l == G - 1;
    if (el ? !dead : live) st4(el ? sp : sp + 8 + 4 * l, el ? hot : fv, nt);
    if (!el && live) st4(sp + 8 + d + 4 * l, fc, nt);
  } else {
    if (l == 0 && !dead) st4(sp, hot, nt);
    if (live) {
      st4(sp + 8 + 4 * l, fv, nt);
      st4(sp + 8 + d + 4 * l, fc, nt);
    }
  }
}

template <int G>
__global__ __launch_bounds__(kFmNT) void k_fm_bwd_line(BwdArgs a) {
  constexpr int CPL = 4, UNR = 4, SPB = kFmNT / G;
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
    const int d = a.d;
    const int64_t xs = a.xs > d ? a.xs : d;
    const uint32_t len = s1 - s0;
    // ---- the key's line (its home slot, or the slot the Get pass found) and the first UNR
    // occurrences of its segment, mutually independent
    uint64_t key = 0;
    uint32_t sl = a.insert_keys ? 0u : a.slot[cidx];
    bool dead = !a.insert_keys && sl == kNoSlot;
    if (a.insert_keys) {
      key = ldnt(a.uniq + cidx, nto);
      sl = (uint32_t)tbl_hash(key, a.T);
    }
    float4 h0, h1;
    float vcur[CPL], ccur[CPL];
    line_load<G>(a.T, dead ? 0 : (int64_t)sl, l, gb, ntb, &h0, &h1, vcur, ccur);
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
        if (!dead) line_load<G>(a.T, (int64_t)sl, l, gb, ntb, &h0, &h1, vcur, ccur);
      }
    }
    if (dead) {  // not in the table (the error word says why): read as absent, no update
      h0 = make_float4(0.f, __int_as_float(-1), 0.f, 0.f);
      h1.x = 0.f;
    }
    float4 e = make_float4(h0.x, h0.z, h0.w, h1.x);  // {w, sqrt_g, z, fea_cnt}
    const int vrow = __float_as_int(h0.y);           // (the key's own slot, or -1)
    // V was pulled iff present and not (l1_shrk && w == 0) (SGDUpdater::Get, :40-43)
    const int vq = (vrow >= 0 && !(a.Pm.l1_shrk && e.x == 0.f)) ? vrow : -1;
    // ---- p and XV*p of the first occurrences' rows (XV*p only for a key whose V takes part)
    const float* zp = a.zpad + ((cidx & 255u) << 4);
    float g0[CPL], pr[UNR], xr[UNR][CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) g0[k] = 0.f;
#pragma unroll
    for (int t = 0; t < UNR; ++t) {
      pr[t] = xs > d ? a.XVp[(int64_t)row[t] * xs + d] : a.p[row[t]];
      load_coords<CPL, true>(vq >= 0 ? a.XVp + (int64_t)row[t] * xs : zp, l, d, xr[t]);
    }
    float gw = 0.f, acc[CPL];
    bwd_key_sums<G, CPL, true, UNR>(a, l, u, s0, s1, valued, d, xs, vq, row, x, pr, xr, vcur, g0, gw,
                                    acc);
    // Update(kGradient): UpdateW (FTRL), then UpdateV (AdaGrad) if V was pulled
    bool tr;
    const int dw = ftrl_update(a.Pm, gw, &e, &tr);
    if (vq >= 0) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) adagrad_update(a.Pm, acc[k], &vcur[k], &ccur[k]);
    }
    line_store<G>(a.T, dead ? 0 : (int64_t)sl, l, ntb, dead, vq >= 0 && 4 * l < d, e, vrow, vcur,
                  ccur);
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

// ---- ... with fp16 Vaux (slot_layout=line vaux=f16, V_dim 16) ---------------------------------
// [Entry 32 B | V 64 B | Vaux 16 x fp16] is the line's eight pieces again, and a key's four lanes
// (lane l: coordinates 4l..4l+3, k_fm_bwd's d = 16 layout) request them once, two loads each:
//   lane l: V piece l;  lanes 0, 1: the entry halves;  lanes 2, 3: the two Vaux pieces (eight
//   halves each: the coordinates of lanes 0, 1 and of lanes 2, 3)
// G = 4 makes the group a DPP quad, so the pieces travel by quad_perm moves in the VALU, not
// through the LDS crossbar as line_bcast's shuffles do: the entry halves are lanes 0 and 1 of
// the quad broadcast, and a lane's four halves are dword pair l % 2 of lane 2 + l / 2's piece —
// quad_perm [2, 2, 3, 3] of its four dwords and a select, widened in registers (f16_widen).
// After the update every lane narrows its own four accumulators (vaux16_round) and the line is
// written in one issue as it was read: the hot entry half from lane 0, a V piece and the lane's
// own 8 bytes of Vaux from every lane — no trip back to lanes 2 and 3.
template <int CTRL>
__device__ __forceinline__ float4 quad_perm(float4 v) {
  auto mv = [](float x) {
    const int i = __float_as_int(x);
    return __int_as_float(__builtin_amdgcn_update_dpp(i, i, CTRL, 0xF, 0xF, false));
  };
  return make_float4(mv(v.x), mv(v.y), mv(v.z), mv(v.w));
}

__device__ __forceinline__ void line16_load(const Table& T, int64_t s, int l, bool nt, float4* h0,
                                            float4* h1, float (&v)[4], float (&c)[4]) {
  const float* sp = reinterpret_cast<const float*>(ent_at(T, s));
  const float4 fv = ld4(sp + 8 + 4 * l, nt);
  const float4 fx = ld4(sp + (l < 2 ? 4 * l : 16 + 4 * l), nt);  // (Vaux: floats 24..31)
  *h0 = quad_perm<0x00>(fx);                                    // quad_perm:[0,0,0,0]
  *h1 = quad_perm<0x55>(fx);                                    // quad_perm:[1,1,1,1]
  const float4 cx = quad_perm<0xFA>(fx);                        // quad_perm:[2,2,3,3]
  const uint32_t c01 = __float_as_uint((l & 1) ? cx.z : cx.x);
  const uint32_t c23 = __float_as_uint((l & 1) ? cx.w : cx.y);
  v[0] = fv.x; v[1] = fv.y; v[2] = fv.z; v[3] = fv.w;
  c[0] = f16_widen(c01 & 0xFFFFu); c[1] = f16_widen(c01 >> 16);
  c[2] = f16_widen(c23 & 0xFFFFu); c[3] = f16_widen(c23 >> 16);
}

__global__ __launch_bounds__(kFmNT) void k_fm_bwd_line16(BwdArgs a) {
  constexpr int G = 4, CPL = 4, UNR = 4, SPB = kFmNT / G;
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
    constexpr int d = 16;
    const int64_t xs = a.xs > d ? a.xs : d;
    const uint32_t len = s1 - s0;
    // ---- the key's line and the first UNR occurrences of its segment, as in k_fm_bwd_line
    uint64_t key = 0;
    uint32_t sl = a.insert_keys ? 0u : a.slot[cidx];
    bool dead = !a.insert_keys && sl == kNoSlot;
    if (a.insert_keys) {
      key = ldnt(a.uniq + cidx, nto);
      sl = (uint32_t)tbl_hash(key, a.T);
    }
    float4 h0, h1;
    float vcur[CPL], ccur[CPL];
    line16_load(a.T, dead ? 0 : (int64_t)sl, l, ntb, &h0, &h1, vcur, ccur);
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
        if (!dead) line16_load(a.T, (int64_t)sl, l, ntb, &h0, &h1, vcur, ccur);
      }
    }
    if (dead) {  // not in the table (the error word says why): read as absent, no update
      h0 = make_float4(0.f, __int_as_float(-1), 0.f, 0.f);
      h1.x = 0.f;
    }
    float4 e = make_float4(h0.x, h0.z, h0.w, h1.x);  // {w, sqrt_g, z, fea_cnt}
    const int vrow = __float_as_int(h0.y);           // (the key's own slot, or -1)
    // V was pulled iff present and not (l1_shrk && w == 0) (SGDUpdater::Get, :40-43)
    const int vq = (vrow >= 0 && !(a.Pm.l1_shrk && e.x == 0.f)) ? vrow : -1;
    // ---- p and XV*p of the first occurrences' rows (XV*p only for a key whose V takes part)
    const float* zp = a.zpad + ((cidx & 255u) << 4);
    float g0[CPL], pr[UNR], xr[UNR][CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) g0[k] = 0.f;
#pragma unroll
    for (int t = 0; t < UNR; ++t) {
      pr[t] = xs > d ? a.XVp[(int64_t)row[t] * xs + d] : a.p[row[t]];
      load_coords<CPL, true>(vq >= 0 ? a.XVp + (int64_t)row[t] * xs : zp, l, d, xr[t]);
    }
    float gw = 0.f, acc[CPL];
    bwd_key_sums<G, CPL, true, UNR>(a, l, u, s0, s1, valued, d, xs, vq, row, x, pr, xr, vcur, g0, gw,
                                    acc);
    // Update(kGradient): UpdateW (FTRL), then UpdateV (AdaGrad) if V was pulled; the new
    // accumulators narrow to fp16 for the store only (eta and V have used them unrounded)
    bool tr;
    const int dw = ftrl_update(a.Pm, gw, &e, &tr);
    uint32_t ch[CPL] = {0u, 0u, 0u, 0u};
    if (vq >= 0) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const float gk = acc[k] + a.Pm.V_l2 * vcur[k];  // adagrad_update's g
        adagrad_update(a.Pm, acc[k], &vcur[k], &ccur[k]);
        ch[k] = vaux16_round(ccur[k], gk, e.y, 4 * l + k);
      }
    }
    // ---- the write-back: one issue to the line
    if (!dead) {
      float* sp = reinterpret_cast<float*>(ent_at(a.T, (int64_t)sl));
      if (l == 0) st4(sp, make_float4(e.x, __int_as_float(vrow), e.y, e.z), ntb);
      if (vq >= 0) {
        st4(sp + 8 + 4 * l, make_float4(vcur[0], vcur[1], vcur[2], vcur[3]), ntb);
        st2(sp + 24 + 2 * l, make_float2(__uint_as_float(ch[0] | (ch[1] << 16)),
                                         __uint_as_float(ch[2] | (ch[3] << 16))), ntb);
      }
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

// ---- ... with fp16 V and Vaux (slot_layout=line vrows=f16, V_dim 24) ---------------------------
// [Entry 32 B | V 24 x fp16 | Vaux 24 x fp16] is the line's eight pieces with no pad: 0-1 the
// entry, 2-4 V, 5-7 Vaux.  A key's four lanes are a DPP quad; lanes 0..2 own the coordinates
// 8l..8l+7 (k_fm_bwd's bwd_cpl = 8 layout: a coordinate's terms and their order are one lane's
// own) and lane 3 owns none, as at d = 12.  The quad requests the eight pieces once, two loads a
// lane in one issue: lane l < 3 V piece 2 + l and Vaux piece 5 + l, lane 3 the entry's halves,
// which reach lanes 0..2 by quad_perm [3,3,3,3] moves in the VALU.  V and Vaux widen in registers
// by the integer path (half8_widen), the arithmetic is fp32 on the widened old values, and the
// two results narrow per coordinate (vhalf_round / vaux16_round, j the coordinate).  The
// write-back is one issue again: the hot entry half from lane 3 (every lane holds the same FTRL
// state), one V piece and one Vaux piece from each of lanes 0..2.
__device__ __forceinline__ dfx_u4v f4_bits(float4 v) {
  dfx_u4v p = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z),
               __float_as_uint(v.w)};
  return p;
}
__device__ __forceinline__ float4 bits_f4(dfx_u4v p) {
  return make_float4(__uint_as_float(p[0]), __uint_as_float(p[1]), __uint_as_float(p[2]),
                     __uint_as_float(p[3]));
}

// the quad's trip to slot s: h0 / h1 the entry's halves in every lane, v / c the lane's eight V /
// Vaux coordinates widened (junk in lane 3, which owns none)
__device__ __forceinline__ void line24_load(const Table& T, int64_t s, int l, bool nt, float4* h0,
                                            float4* h1, float (&v)[8], float (&c)[8]) {
  const float* sp = reinterpret_cast<const float*>(ent_at(T, s));
  const bool el = l == 3;  // the entry's lane
  const float4 fa = ld4(sp + (el ? 0 : 8 + 4 * l), nt);   // piece 2 + l, or entry half 0
  const float4 fb = ld4(sp + (el ? 4 : 20 + 4 * l), nt);  // piece 5 + l, or entry half 1
  *h0 = quad_perm<0xFF>(fa);                              // quad_perm:[3,3,3,3]
  *h1 = quad_perm<0xFF>(fb);
  half8_widen(f4_bits(fa), v);
  half8_widen(f4_bits(fb), c);
}

__global__ __launch_bounds__(kFmNT) void k_fm_bwd_line24(BwdArgs a) {
  constexpr int G = 4, CPL = 8, UNR = 2, SPB = kFmNT / G, d = 24;
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
    // ---- the key's line and the first UNR occurrences of its segment, as in k_fm_bwd_line
    uint64_t key = 0;
    uint32_t sl = a.insert_keys ? 0u : a.slot[cidx];
    bool dead = !a.insert_keys && sl == kNoSlot;
    if (a.insert_keys) {
      key = ldnt(a.uniq + cidx, nto);
      sl = (uint32_t)tbl_hash(key, a.T);
    }
    float4 h0, h1;
    float vcur[CPL], ccur[CPL];
    line24_load(a.T, dead ? 0 : (int64_t)sl, l, ntb, &h0, &h1, vcur, ccur);
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
        if (!dead) line24_load(a.T, (int64_t)sl, l, ntb, &h0, &h1, vcur, ccur);
      }
    }
    if (dead) {  // not in the table (the error word says why): read as absent, no update
      h0 = make_float4(0.f, __int_as_float(-1), 0.f, 0.f);
      h1.x = 0.f;
    }
    float4 e = make_float4(h0.x, h0.z, h0.w, h1.x);  // {w, sqrt_g, z, fea_cnt}
    const int vrow = __float_as_int(h0.y);           // (the key's own slot, or -1)
    // V was pulled iff present and not (l1_shrk && w == 0) (SGDUpdater::Get, :40-43)
    const int vq = (vrow >= 0 && !(a.Pm.l1_shrk && e.x == 0.f)) ? vrow : -1;
    // ---- p and XV*p of the first occurrences' rows (XV*p only for a key whose V takes part;
    // lane 3's chunk is outside the row: it reads chunk 0 and is ignored, load_coords)
    const float* zp = a.zpad + ((cidx & 255u) << 4);
    float g0[CPL], pr[UNR], xr[UNR][CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) g0[k] = 0.f;
#pragma unroll
    for (int t = 0; t < UNR; ++t) {
      pr[t] = xs > d ? a.XVp[(int64_t)row[t] * xs + d] : a.p[row[t]];
      load_coords<CPL, true>(vq >= 0 ? a.XVp + (int64_t)row[t] * xs : zp, l, d, xr[t]);
    }
    float gw = 0.f, acc[CPL];
    bwd_key_sums<G, CPL, true, UNR>(a, l, u, s0, s1, valued, d, xs, vq, row, x, pr, xr, vcur, g0, gw,
                                    acc);
    // Update(kGradient): UpdateW (FTRL), then UpdateV (AdaGrad) if V was pulled; the new V and the
    // new accumulator narrow to fp16 for the stores only (eta and V have used them unrounded)
    bool tr;
    const int dw = ftrl_update(a.Pm, gw, &e, &tr);
    // ---- the write-back: one issue to the line
    float* sp = reinterpret_cast<float*>(ent_at(a.T, dead ? 0 : (int64_t)sl));
    if (l == G - 1) {
      if (!dead) st4(sp, make_float4(e.x, __int_as_float(vrow), e.y, e.z), ntb);
    } else if (vq >= 0) {
      uint32_t hv[CPL], hc[CPL];
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const float gk = acc[k] + a.Pm.V_l2 * vcur[k];  // adagrad_update's g
        adagrad_update(a.Pm, acc[k], &vcur[k], &ccur[k]);
        hv[k] = vhalf_round(vcur[k], gk, e.y, CPL * l + k);
        hc[k] = vaux16_round(ccur[k], gk, e.y, CPL * l + k);
      }
      st4(sp + 8 + 4 * l, bits_f4(half8_pack(hv)), ntb);
      st4(sp + 20 + 4 * l, bits_f4(half8_pack(hc)), ntb);
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

// blocks of k_fm_bwd_line24 over nseg_bound keys (BwdArgs::live_part): four lanes a key, where
// bwd_lanes' float4 layout of d = 24 would take eight
int64_t bwd_line24_blocks(int64_t nseg_bound) {
  const int64_t spb = kFmNT / 4;
  return (nseg_bound + spb - 1) / spb;
}

// ---- the fused forward over such a table ---------------------------------------------------------
// k_fm_fwd_walk's structure: a quad per row, the groups looping over rows on a resident grid, a
// row's ids staged in LDS kL24Ids at a time, kL24NB nnz a trip.  For each nnz of the trip every
// lane sends one kind of request to the home slot, all in flight: lanes 0..2 V piece 2 + l (16
// bytes, eight halves), lane 3 the entry as two 8-byte loads — {w, vrow} and the key — into the
// four registers the other lanes fill with V (both 16-byte halves would hold eight per nnz, 64
// in flight where this holds 32; the line is fetched whole either way).  The entry's words reach
// the quad by quad_perm [3,3,3,3]; the key check follows the trip (a key away from home walks its
// chain and its V piece is reloaded from the found slot), and the sums run in nnz order from the
// widened values.  Lane 3 owns no coordinates: what it sums is dropped by fwd_row_out's
// q * CPL + k < d guards.  On a table whose V is all fp16 values pred, p and XV*p are those of an
// fp32 table holding the same values, bit for bit.
constexpr int kL24NB = 8;
constexpr int kL24Ids = (40 / kL24NB) * kL24NB;

template <bool VALUED>
__global__ __launch_bounds__(kFmNT, 2) void k_fm_fwd_line24(FwdArgs a) {
  constexpr int G = 4, RPB = kFmNT / G, CPL = 8, d = 24;
  __shared__ uint64_t s_id[RPB][kL24Ids];
  __shared__ float s_x[VALUED ? RPB : 1][VALUED ? kL24Ids : 1];
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
    for (uint64_t j0 = o0; j0 < o1; j0 += kL24NB) {
      if (j0 >= c_end) {  // the row's next kL24Ids ids, one trip (group-uniform)
        __builtin_amdgcn_wave_barrier();  // the last chunk's reads are done
#pragma unroll
        for (int m = 0; m < (kL24Ids + G - 1) / G; ++m) {
          const uint64_t j = j0 + l + (uint64_t)G * m;
          if (j < o1 && l + G * m < kL24Ids) {
            s_id[g][l + G * m] = a.index[j];
            if (VALUED) s_x[g][l + G * m] = a.val[j];
          }
        }
        __builtin_amdgcn_wave_barrier();
        c_end = j0 + kL24Ids;
      }
      const int cb = (int)(j0 - (c_end - kL24Ids));  // this trip's first id in the chunk
      const int nin = (int)((o1 - j0) < (uint64_t)kL24NB ? (o1 - j0) : (uint64_t)kL24NB);
      auto key_of = [&](int i) {
        const uint64_t id = s_id[g][i];
        const uint64_t mm = a.max_index == ~0ull ? (id == ~0ull ? 0ull : id) : id % a.max_index;
        return a.keys_ready ? id : reverse_bytes(mm);
      };
      // ---- the trip's home slots, all in flight: lanes 0..2 a V piece, lane 3 {w, vrow, key}
      float4 q[kL24NB];
#pragma unroll
      for (int t = 0; t < kL24NB; ++t) {
        const uint64_t key = key_of(cb + (t < nin ? t : nin - 1));
        const float* sl = reinterpret_cast<const float*>(ent_at(a.T, tbl_hash(key, a.T)));
        if (l < 3) {
          q[t] = ld4(sl + 8 + 4 * l, ntf);
        } else {
          const float2 e0 = ld2(sl, ntf), e1 = ld2(sl + 6, ntf);
          q[t] = make_float4(e0.x, e0.y, e1.x, e1.y);
        }
      }
      // ---- the key checks and the sums, in nnz order
#pragma unroll
      for (int t = 0; t < kL24NB; ++t) {
        if (t >= nin) break;  // group-uniform
        const uint64_t key = key_of(cb + t);
        const float4 en = quad_perm<0xFF>(q[t]);  // quad_perm:[3,3,3,3]: {w, vrow, key}
        uint64_t ek = ((uint64_t)__float_as_uint(en.w) << 32) | (uint64_t)__float_as_uint(en.z);
        float w = en.x;
        int vr = __float_as_int(en.y);
        float4 vv = q[t];
        if (ek != key && ek != kEmptyKey) {  // a longer probe chain (group-uniform)
          uint64_t h = tbl_hash(key, a.T);
          for (uint64_t probe = 0; ek != key && ek != kEmptyKey && probe < a.T.mask; ++probe) {
            h = (h + 1) & a.T.mask;
            ek = ent_at(a.T, h)->key;
          }
          if (ek == key) {
            const Entry* e = ent_at(a.T, h);
            w = e->w;
            vr = e->vrow;
            // (lane 3 reads Vaux piece 0 of the same slot: in bounds, unused)
            vv = ld4(reinterpret_cast<const float*>(e) + 8 + 4 * l, ntf);
          }
        }
        // absent (inserted by this training step's backward): w = 0, no V
        if (ek != key) { w = 0.f; vr = -1; }
        const float x = VALUED ? s_x[g][cb + t] : 1.f;
        // SpMV::Times skips w == 0 (spmv.h:124-125)
        if (w != 0.f) acc = VALUED ? acc + w * x : acc + w;
        // V is visible only if present and not (l1_shrk && w == 0) (sgd_updater.cc:40-43)
        if (vr >= 0 && !(a.l1_shrk && w == 0.f)) {
          float vk[CPL];
          half8_widen(f4_bits(vv), vk);
          const float xx = x * x;  // XX_ (fm_loss.h:86-92)
#pragma unroll
          for (int k = 0; k < CPL; ++k) {
            xv[k] = VALUED ? xv[k] + vk[k] * x : xv[k] + vk[k];
            const float qq = vk[k] * vk[k];  // VV (fm_loss.h:95-101)
            xxvv[k] = VALUED ? xxvv[k] + qq * xx : xxvv[k] + qq;
          }
        }
      }
    }
    fwd_row_out<G, CPL, d>(a, r, l, gbase, acc, xv, xxvv, &loss);
  }
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
static int launch_fwd_line24_v(const FwdArgs& a, hipStream_t st, int* nblk) {
  static int64_t resident = 0;  // per kernel
  const int64_t rpb = kFmNT / 4, want = (a.B + rpb - 1) / rpb;
  if (resident <= 0) resident = resident_grid_for(k_fm_fwd_line24<VALUED>, INT32_MAX);
  *nblk = (int)std::min<int64_t>(want, resident);
  hipLaunchKernelGGL((k_fm_fwd_line24<VALUED>), dim3((unsigned)*nblk), dim3(kFmNT), 0, st, a);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

int launch_fwd_line24(const FwdArgs& a, hipStream_t st, int* nblk) {
  *nblk = 0;
  if (a.T.line != 3 || a.T.d != 24 || a.d != 24 || !a.index || a.part) {
    set_error("slot_layout=line vrows=f16: the fused forward needs V_dim 24 and the batch's "
              "feature ids (the single context's fused step)");
    return DFX_ERR_ARG;
  }
  if (a.B <= 0) return DFX_OK;
  return a.val ? launch_fwd_line24_v<true>(a, st, nblk) : launch_fwd_line24_v<false>(a, st, nblk);
}

// the fused backward of a line table: G = the lanes of d / 4 float4 (bwd_lanes' layout, so
// bwd_fused_blocks counts its blocks too; d = 24: four lanes, bwd_line24_blocks)
int launch_bwd_line(const BwdArgs& a, int64_t nseg_bound, hipStream_t st, long lds,
                    size_t lds_default) {
  const size_t lds_bytes = lds >= 0 ? (size_t)lds : lds_default;
  if (nseg_bound <= 0) return DFX_OK;
  if (line_es(a.d, a.T.line == 2, a.T.line == 3) == 0 || a.T.d != a.d || a.vlist) {
    set_error("line slots: the fused backward needs V_dim 4, 8 or 12, or 16 with vaux=f16, or 24 "
              "with vrows=f16");
    return DFX_ERR_ARG;
  }
  const int G = a.d == 4 ? 1 : a.d == 8 ? 2 : 4;
  const int64_t spb = kFmNT / G;
  const dim3 grid((unsigned)((nseg_bound + spb - 1) / spb));
  if (a.T.line == 3) hipLaunchKernelGGL(k_fm_bwd_line24, grid, dim3(kFmNT), lds_bytes, st, a);
  else if (a.T.line == 2) hipLaunchKernelGGL(k_fm_bwd_line16, grid, dim3(kFmNT), lds_bytes, st, a);
  else if (G == 1) hipLaunchKernelGGL(k_fm_bwd_line<1>, grid, dim3(kFmNT), lds_bytes, st, a);
  else if (G == 2) hipLaunchKernelGGL(k_fm_bwd_line<2>, grid, dim3(kFmNT), lds_bytes, st, a);
  else hipLaunchKernelGGL(k_fm_bwd_line<4>, grid, dim3(kFmNT), lds_bytes, st, a);
  DFX_HIP(hipGetLastError());
  return DFX_OK;
}

}  // namespace dfx
