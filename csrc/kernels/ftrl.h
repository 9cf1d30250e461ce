// FTRL-Proximal on one element: TensorFlow's ApplyFtrl / SparseApplyFtrl with the
// V2 shrinkage term.  Shared by the row-sparse rule (sparse_optim.hip kind 6),
// the dense multi-tensor rule (ops.hip kind 6) and the one-GPU sparse-LR step
// (sparse_lr.hip).
//
//   g_s     = g + 2 l2_shrinkage var          (== g when shrinkage is 0)
//   acc_new = acc + g g                       (the unshrunk g)
//   sigma   = (acc_new^p - acc^p) / lr        (p = -learning_rate_power >= 0)
//   linear += g_s - sigma var
//   quad    = acc_new^p / lr + 2 l2
//   var     = |linear| > l1 ? (sign(linear) l1 - linear) / quad : 0
#pragma once
#include <hip/hip_runtime.h>

namespace dtfk {

// acc^p: p == 0.5 (the default) is a square root, p == 0 is exactly 1 (sigma == 0)
__device__ __forceinline__ float ftrl_pow(float a, float p) {
  return p == 0.5f ? sqrtf(a) : (p == 0.f ? 1.f : powf(a, p));
}

// g: the duplicate-summed, unshrunk gradient.  The zero branch is a select on
// |linear| > l1: the untaken division (0 / 0 at acc == 0, g == 0, l2 == 0)
// never reaches var.
__device__ __forceinline__ void ftrl_update(float& var, float& acc, float& lin, float g, float lr, float p, float l1,
                                            float l2, float shrink) {
  const float gs = shrink != 0.f ? g + 2.f * shrink * var : g;
  const float an = acc + g * g;
  const float pn = ftrl_pow(an, p);
  const float sigma = p == 0.f ? 0.f : (pn - ftrl_pow(acc, p)) / lr;
  const float l = lin + gs - sigma * var;
  const float quad = pn / lr + 2.f * l2;
  var = fabsf(l) > l1 ? (copysignf(l1, l) - l) / quad : 0.f;
  acc = an;
  lin = l;
}

}  // namespace dtfk
