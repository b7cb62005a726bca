// Keras-form Adam (nrms.py:69-80) on ONE element: the update every optimizer kernel of the library applies -- the stand-alone passes
// (adam_keras_kernel, adam_keras_scalar_kernel, adam_keras_fixed_kernel) and the kernels that apply the optimizer where a gradient element
// is produced (ebn_dvn_finale_f32, ebn_grad_finish_adam_f32) instead of in a pass of their own.
#pragma once
#include "ebn_common.h"

// The ONE copy of the update.  Its rounding is fixed in the source, so that every kernel that inlines it gives the same bits for the same
// inputs: the fused multiply-adds are explicit, and contraction is off for the rest -- under HIP's default -ffp-contract=fast-honor-pragmas
// the backend may otherwise fuse a multiply of this function with an add of it (or of the caller around it), and did so differently at
// different call sites: the stand-alone passes formed m as fma(g' - m, 1 - b1, m), the fused launches as m + (1 - b1) (g' - m).  The
// rounding kept is the fused launches' one -- what a default one-rank NRMS / NRMSDocVec step has always computed.  Division and square
// root are the correctly rounded ones (no -ffast-math).
//   g' = g gscale;  m += (g' - m) (1 - b1);  v += (g'^2 - v) (1 - b2);  theta -= alpha m / (sqrt(v) + eps)
static __device__ __forceinline__ void ebn_adam_element(float& theta, float g, float& m, float& v, float alpha, float omb1, float omb2,
                                                        float eps, float gscale) {
#pragma clang fp contract(off)
  const float gg = g * gscale;
  m = m + __builtin_fmaf(g, gscale, -m) * omb1;  // g' - m in one rounding, then the product and the sum rounded each
  v = __builtin_fmaf(__builtin_fmaf(gg, gg, -v), omb2, v);
  theta = theta - (alpha * m) / (sqrtf(v) + eps);
}

// Adam on the flat parameter buffers: an element is addressed by the ADDRESS of its gradient (grad + offset).
struct EbnAdamFlat {
  const float* grad;  // base of the flat gradient buffer
  float* theta;
  float* m;
  float* v;
  const ebn_step_state* st;
  float omb1, omb2, eps, gscale;
};

static __device__ __forceinline__ void ebn_adam_flat_apply(const EbnAdamFlat& ad, float alpha, int64_t off, float g) {
  float t = ad.theta[off], mm = ad.m[off], vv = ad.v[off];
  ebn_adam_element(t, g, mm, vv, alpha, ad.omb1, ad.omb2, ad.eps, ad.gscale);
  ad.theta[off] = t;
  ad.m[off] = mm;
  ad.v[off] = vv;
}
