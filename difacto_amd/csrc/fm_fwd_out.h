// One forward row's finish, shared by the fused forwards of fm.hip and fm_half.hip.
#pragma once
#include "fm_lanes.h"

namespace dfx {

// One row's outputs once its sums are complete (G lanes, CPL coordinates per lane): the split's
// partial, or FMLoss::Predict's finish — s = sum_l (XV_l^2 - XXVV_l) serially over l, the
// clip — then CalcGrad's p, XV_ * p, Evaluate's logloss and the AUC lane's snapshot.
// Loss::Evaluate's term of one row (loss.h:57-66), in double.  Not inlined: a caller that loops
// over rows would otherwise hold exp's and log's double constants in VGPRs across its loop.
__device__ __noinline__ double row_logloss(float label, float pr) {
  const double yy = label > 0 ? 1.0 : -1.0;
  return log(1.0 + exp(-yy * (double)pr));
}

template <int G, int CPL, int DK = 0>
__device__ __forceinline__ void fwd_row_out(const FwdArgs& a, int64_t r, int l, int gbase,
                                            float acc, const float (&xv)[CPL],
                                            const float (&xxvv)[CPL], double* loss) {
  const int d = DK > 0 ? DK : a.d;  // DK: V_dim known to the caller
  if (a.part) {
    // owner-computes split: this owner's share of the row (split.hip k_split_combine)
    float* pr_row = a.part + r * split_part_floats(d, a.part_n);
    if (a.part_n > 1) {  // [XV | sum w x | sum_l XXVV_l (serial over l) | 0 0]
      float sx = 0.f;
      for (int q = 0; q < G; ++q) {
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
          const float tk = __shfl(xxvv[k], gbase + q, kWave);
          if (q * CPL + k < d) sx += tk;
        }
      }
#pragma unroll
      for (int m = 0; m < CPL / 4; ++m)
        if (l * CPL + 4 * m < d)
          *reinterpret_cast<float4*>(pr_row + l * CPL + 4 * m) =
              make_float4(xv[4 * m], xv[4 * m + 1], xv[4 * m + 2], xv[4 * m + 3]);
      if (l == 0) {
        pr_row[d] = acc;
        pr_row[d + 1] = sx;
        pr_row[d + 2] = pr_row[d + 3] = 0.f;
      }
    } else {
#pragma unroll
      for (int m = 0; m < CPL / 4; ++m) {
        if (l * CPL + 4 * m < d) {
          *reinterpret_cast<float4*>(pr_row + l * CPL + 4 * m) =
              make_float4(xv[4 * m], xv[4 * m + 1], xv[4 * m + 2], xv[4 * m + 3]);
          *reinterpret_cast<float4*>(pr_row + d + l * CPL + 4 * m) =
              make_float4(xxvv[4 * m], xxvv[4 * m + 1], xxvv[4 * m + 2], xxvv[4 * m + 3]);
        }
      }
      if (l == 0) {
        pr_row[2 * d] = acc;
        pr_row[2 * d + 1] = pr_row[2 * d + 2] = pr_row[2 * d + 3] = 0.f;
      }
    }
  }
  float pr = acc;
  if (d > 0 && !a.part) {
    // s = sum_l (XV_l^2 - XXVV_l), serially over l = 0..d-1 (fm_loss.h:110-113)
    float t4[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) t4[k] = xv[k] * xv[k] - xxvv[k];
    float s = 0.f;
    for (int q = 0; q < G; ++q) {
#pragma unroll
      for (int k = 0; k < CPL; ++k) {
        const float tk = __shfl(t4[k], gbase + q, kWave);
        if (q * CPL + k < d) s += tk;
      }
    }
    double y = (double)acc + .5 * (double)s;  // float += double (fm_loss.h:114)
    pr = (float)y;
    pr = pr > 20.f ? 20.f : (pr < -20.f ? -20.f : pr);  // clip (fm_loss.h:118)
  }
  const float p = a.part ? 0.f : logit_p(a.label[r], pr, a.rw, r);
  const int64_t xs = a.xs > d ? a.xs : d;
  if (a.part) {
    // the partial is all this kernel writes
  } else if (l == 0) {
    a.p_out[r] = p;
    if (xs > d) a.XVp[r * xs + d] = p;
    a.pred[r] = pr;
    *loss += row_logloss(a.label[r], pr);  // Loss::Evaluate (loss.h:57-66)
    if (a.auc_key) {  // the AUC lane's snapshot: orderable key of pred, label > 0
      uint32_t u = __float_as_uint(pr + 0.0f);  // -0 == +0, as operator< sees them
      a.auc_key[r] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
      a.auc_lab[r] = a.label[r] > 0 ? 1u : 0u;
    }
  }
#pragma unroll
  for (int m = 0; m < CPL / 4; ++m)  // XV_ *= p (fm_loss.h:196-199)
    if (d > 0 && l * CPL + 4 * m < d && !a.part)
      *reinterpret_cast<float4*>(a.XVp + r * xs + l * CPL + 4 * m) =
          make_float4(xv[4 * m] * p, xv[4 * m + 1] * p, xv[4 * m + 2] * p, xv[4 * m + 3] * p);
}

}  // namespace dfx
