// The per-key sums and the block epilogue of the fused backwards that give a key a few lanes and
// its state one trip: the line backward (fm_line.hip) and the half-row backward (fm_half.hip).
#pragma once
#include "fm_lanes.h"

namespace dfx {

// One key's sums over its occurrences [s0, s1) for the line backward (k_fm_bwd_line): g_w into
// gw and, when the key's V takes part (vq >= 0), grad_u of lane l's CPL coordinates into acc.
// row / x / pr / xr: the first UNR occurrences' rows, values, p and XV*p, loaded by the caller
// beside the key's state; u: the key's segment (its chunks' partials); vcur, g0: V and the
// gradient so far.  The terms, their order and the three forms (a short segment from registers,
// a chunked one from its partials, the walk) are k_fm_bwd's for groups under 8 lanes, restated
// here, not called from there: k_fm_bwd inlines its own text, so that what it compiles to for
// the split and fat layouts stays what it was (taking these sums through this function changed
// its register allocation).  A change to either text belongs in both; tests/
// test_gpu_line_slots.py holds the two to the same bits.
template <int G, int CPL, bool VEC, int UNR>
__device__ __forceinline__ void bwd_key_sums(const BwdArgs& a, int l, int64_t u, uint32_t s0,
                                             uint32_t s1, bool valued, int d, int64_t xs, int vq,
                                             const uint32_t (&row)[UNR], const float (&x)[UNR],
                                             const float (&pr)[UNR], const float (&xr)[UNR][CPL],
                                             const float (&vcur)[CPL], const float (&g0)[CPL],
                                             float& gw, float (&acc)[CPL]) {
  // (k_fm_bwd's groups of 8 lanes and more walk G occurrences per trip, the terms shuffled from
  // the lanes in occurrence order: the same terms in the same order as the per-lane walk here,
  // which the half-row backward's G = 8 takes)
  static_assert(G <= 8, "a few lanes per key");
  const uint32_t len = s1 - s0;
  float xxp = 0.f;
  // ---- pass 1: g_w and XXp (SpMV::TransTimes, spmv.h:139-171: skip p == 0)
  // ---- pass 2: grad_u = (g0 - V*XXp) + sum (XV_ p) x (fm_loss.h:185-202, spmm.h:127-159)
  // Both sums run in occurrence order; a segment of <= UNR occurrences (the common case)
  // is computed from the registers loaded above.
  if (len <= (uint32_t)UNR) {
#pragma unroll
    for (int t = 0; t < UNR; ++t) {
      if ((uint32_t)t < len && pr[t] != 0.f) {
        if (valued) {
          gw += pr[t] * x[t];
          xxp += pr[t] * (x[t] * x[t]);
        } else {
          gw += pr[t];
          xxp += pr[t];
        }
      }
    }
    if (vq >= 0) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) acc[k] = g0[k] - vcur[k] * xxp;
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
        if ((uint32_t)t < len) {
#pragma unroll
          for (int k = 0; k < CPL; ++k)
            acc[k] = valued ? acc[k] + xr[t][k] * x[t] : acc[k] + xr[t][k];
        }
      }
    }
  } else if (a.choff && len > (uint32_t)kChunkOcc) {
    // a long segment (a skewed key): its chunks' partial sums (k_fm_bwd_chunks), combined in
    // chunk order, all in double and rounded once — the sums differ from the reference's
    // sequential float sums only by that float rounding (reordering error)
    const uint32_t c0 = a.choff[u];
    const uint32_t nc = hot_chunks_read((len + kChunkOcc - 1) / kChunkOcc);
    const int P = d + 2;
    double gwd = 0, xxpd = 0, accp[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) accp[k] = 0;
    for (uint32_t c = 0; c < nc; ++c) {
      const double* pc = a.part + (int64_t)(c0 + c) * P;
      gwd += pc[0];
      xxpd += pc[1];
      if (vq >= 0) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const int cd = l * CPL + k;
          accp[k] += cd < d ? pc[2 + cd] : 0.0;
        }
      }
    }
    gw = (float)gwd;
    xxp = (float)xxpd;
    if (vq >= 0) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) acc[k] = (float)((double)(g0[k] - vcur[k] * xxp) + accp[k]);
    }
  } else {
    // Both walks keep the next trip's rows in flight beside this trip's row reads (the
    // segment's occ_row / occ_x are contiguous; the p / XV*p reads are the random ones), so a
    // trip costs one memory round trip instead of two.  Same terms, same order.
    uint32_t rw[UNR];
    float xw[UNR];
#pragma unroll
    for (int t = 0; t < UNR; ++t) {  // the first trip's rows: already loaded (level 2)
      rw[t] = row[t];
      xw[t] = x[t];
    }
    for (uint32_t i0 = s0; i0 < s1; i0 += UNR) {
      float pw[UNR];
#pragma unroll
      for (int t = 0; t < UNR; ++t)
        pw[t] = row_p(a, rw[t], d, xs);
      const uint32_t in = i0 + UNR;
      uint32_t rn[UNR];
      float xn[UNR];
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
        const uint32_t i = in + t < s1 ? in + t : s1 - 1;
        xn[t] = 1.f;
        rn[t] = in < s1 ? occ_get(a, i, valued, false, &xn[t]) : 0u;
      }
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
        if (i0 + t < s1 && pw[t] != 0.f) {
          if (valued) {
            gw += pw[t] * xw[t];
            xxp += pw[t] * (xw[t] * xw[t]);
          } else {
            gw += pw[t];
            xxp += pw[t];
          }
        }
      }
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
        rw[t] = rn[t];
        xw[t] = xn[t];
      }
    }
    if (vq >= 0) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) acc[k] = g0[k] - vcur[k] * xxp;
#pragma unroll
      for (int t = 0; t < UNR; ++t) {
        rw[t] = row[t];
        xw[t] = x[t];
      }
      for (uint32_t i0 = s0; i0 < s1; i0 += UNR) {
        float xrw[UNR][CPL];
#pragma unroll
        for (int t = 0; t < UNR; ++t)
          load_coords<CPL, VEC>(a.XVp + (int64_t)rw[t] * xs, l, d, xrw[t]);
        // the next trip's rows, in flight beside this trip's XV*p rows
        const uint32_t in = i0 + UNR;
        uint32_t rn[UNR];
        float xn[UNR];
#pragma unroll
        for (int t = 0; t < UNR; ++t) {
          const uint32_t i = in + t < s1 ? in + t : s1 - 1;
          xn[t] = 1.f;
          rn[t] = in < s1 ? occ_get(a, i, valued, false, &xn[t]) : 0u;
        }
#pragma unroll
        for (int t = 0; t < UNR; ++t) {
          if (i0 + t < s1) {
#pragma unroll
            for (int k = 0; k < CPL; ++k)
              acc[k] = valued ? acc[k] + xrw[t][k] * xw[t] : acc[k] + xrw[t][k];
          }
        }
#pragma unroll
        for (int t = 0; t < UNR; ++t) {
          rw[t] = rn[t];
          xw[t] = xn[t];
        }
      }
    }
  }
}

// The line backward's block epilogue, k_fm_bwd's restated (see bwd_key_sums): the lanes' new_w,
// InitV-request, insert and live-V counts summed over the block and added to the step's counters
// (every thread of the block calls it)
__device__ __forceinline__ void bwd_block_stats(const BwdArgs& a, int dnew, int ninit, int nins,
                                                unsigned nlive, unsigned nlocc) {
  __shared__ int red[kFmNT / kWave];
  __shared__ int redn[kFmNT / kWave];
  __shared__ int redi[kFmNT / kWave];
  __shared__ unsigned redl[kFmNT / kWave], redo[kFmNT / kWave];
  // new_w, and the InitV requests (dsw->n_init gates the InitV pass on the device)
  for (int off = 32; off > 0; off >>= 1) {
    dnew += __shfl_xor(dnew, off, kWave);
    ninit += __shfl_xor(ninit, off, kWave);
    nins += __shfl_xor(nins, off, kWave);
    nlive += __shfl_xor(nlive, off, kWave);
    nlocc += __shfl_xor(nlocc, off, kWave);
  }
  if (lane_id() == 0) {
    red[threadIdx.x / kWave] = dnew;
    redn[threadIdx.x / kWave] = ninit;
    redi[threadIdx.x / kWave] = nins;
    redl[threadIdx.x / kWave] = nlive;
    redo[threadIdx.x / kWave] = nlocc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0, q = 0, i2 = 0;
    unsigned long long lv = 0, lo = 0;
    for (int i = 0; i < kFmNT / kWave; ++i) {
      s += red[i];
      q += redn[i];
      i2 += redi[i];
      lv += redl[i];
      lo += redo[i];
    }
    // one-word atomics serialise (~88 per us) and a cold model has a new w in
    // nearly every block: the counts go to a stripe of their own line; n_init is a gate only
    unsigned long long* nw = (unsigned long long*)&a.dsw->new_w;
    unsigned long long* nk = &a.dsw->n_keys;
    if (a.stripes) {
      nw = a.stripes + (blockIdx.x % kBwStripes) * 16;
      nk = nw + 1;
    }
    if (s) atomicAdd(nw, (unsigned long long)(long long)s);
    if (q && __hip_atomic_load(&a.dsw->n_init, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
      atomicOr(&a.dsw->n_init, 1u);
    if (i2) atomicAdd(nk, (unsigned long long)i2);
    if (a.live_part) a.live_part[blockIdx.x] = make_uint2((unsigned)lv, (unsigned)lo);
  }
}

}  // namespace dfx
