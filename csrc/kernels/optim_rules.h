// The optimizer rules, once: kind numbers, hyper-parameters, which slots a kind
// has, and the update of ONE element with its gradient already scaled.  Used by
// the dense multi-tensor kernel (ops.hip: multi_tensor_apply), the row-sparse
// kernel (sparse_optim.hip: rows_apply) and, for FTRL, the one-GPU sparse-LR
// step (sparse_lr.hip).  The Python owner of the same facts is optim/rules.py.
//
// Slot a / slot b per kind (TF's slot names):
//   momentum  a = Momentum              adagrad  a = Adagrad (accumulator)
//   adam(w)   a = Adam (m), b = Adam_1 (v)
//   rmsprop   a = RMSProp (mean square), b = Momentum
//   ftrl      a = Ftrl (accum), b = Ftrl_1 (linear)
//
// FAST_RSQRT is the one difference between the two kernels: x / sqrtf(a) in the
// dense kernel (false), x * rsqrtf(a) in the row kernel (true).  Each kernel
// keeps the form it had before the rules were shared, so that both stay bit
// compatible with their earlier results; the two forms differ in the last bit.
#pragma once
#include <hip/hip_runtime.h>

namespace dtfk {

enum OptimKind : int {   // = optim/rules.py RULES[...].kind
  OPT_SGD = 0, OPT_MOMENTUM = 1, OPT_ADAM = 2, OPT_ADAMW = 3, OPT_ADAGRAD = 4, OPT_RMSPROP = 5, OPT_FTRL = 6
};

// The row kernel's fields come first and in one run: its kernel arguments then
// load as they did before the struct was shared.
struct OptimHyper {
  float lr;
  float momentum;
  float decay;          // RMSProp's rho
  float eps;
  int nesterov;
  float p, l1, l2, shrink;   // FTRL: p = -learning_rate_power >= 0, l1, l2, l2_shrinkage
  float beta1, beta2;   // Adam / AdamW
  float weight_decay;   // dense kernel only: L2 on the gradient (sgd, momentum, adam), decoupled for adamw
};

constexpr __host__ __device__ bool uses_slot_a(int kind) { return kind != OPT_SGD; }
constexpr __host__ __device__ bool uses_slot_b(int kind) {
  return kind == OPT_ADAM || kind == OPT_ADAMW || kind == OPT_RMSPROP || kind == OPT_FTRL;
}

// tf.train.FtrlOptimizer's range checks, for the launchers
inline bool ftrl_hyper_ok(const OptimHyper& h) { return h.p >= 0.f && h.l1 >= 0.f && h.l2 >= 0.f && h.shrink >= 0.f; }

#ifdef __HIPCC__
// GradientDescent: var -= lr g
__device__ __forceinline__ void rule_sgd(float& var, float g, float lr) { var -= lr * g; }

// Momentum: acc = mu acc + g; var -= lr acc   (Nesterov: lr (g + mu acc))
__device__ __forceinline__ void rule_momentum(float& var, float& acc, float g, float lr, const OptimHyper& h) {
  const float a = h.momentum * acc + g;
  acc = a;
  var -= lr * (h.nesterov ? g + h.momentum * a : a);
}

// TF ApplyAdagrad: acc += g^2; var -= lr g / sqrt(acc)
template <bool FAST_RSQRT>
__device__ __forceinline__ void rule_adagrad(float& var, float& acc, float g, float lr) {
  const float a = acc + g * g;
  acc = a;
  var -= FAST_RSQRT ? lr * g * rsqrtf(a) : lr * g / sqrtf(a);
}

// TF ApplyRMSProp: ms = rho ms + (1 - rho) g^2; mom = mu mom + lr g / sqrt(ms + eps); var -= mom
template <bool FAST_RSQRT>
__device__ __forceinline__ void rule_rmsprop(float& var, float& ms, float& mom, float g, float lr,
                                             const OptimHyper& h) {
  const float s = h.decay * ms + (1.f - h.decay) * g * g;
  const float mo = h.momentum * mom + (FAST_RSQRT ? lr * g * rsqrtf(s + h.eps) : lr * g / sqrtf(s + h.eps));
  ms = s;
  mom = mo;
  var -= mo;
}

// TF AdamOptimizer; lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), eps outside the sqrt
__device__ __forceinline__ void rule_adam(float& var, float& m, float& v, float g, float lr_t, const OptimHyper& h) {
  const float mv = h.beta1 * m + (1.f - h.beta1) * g;
  const float vv = h.beta2 * v + (1.f - h.beta2) * g * g;
  m = mv;
  v = vv;
  var -= lr_t * mv / (sqrtf(vv) + h.eps);
}

// FTRL-Proximal: TensorFlow's ApplyFtrl / SparseApplyFtrl with the V2 shrinkage term.
//
//   g_s     = g + 2 l2_shrinkage var          (== g when shrinkage is 0)
//   acc_new = acc + g g                       (the unshrunk g)
//   sigma   = (acc_new^p - acc^p) / lr        (p = -learning_rate_power >= 0)
//   linear += g_s - sigma var
//   quad    = acc_new^p / lr + 2 l2
//   var     = |linear| > l1 ? (sign(linear) l1 - linear) / quad : 0
//
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
#endif  // __HIPCC__

}  // namespace dtfk
