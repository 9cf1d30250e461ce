// Device helpers the MLP kernel files share (graph_mlp.hip, mlp_eval.hip): the pixel
// conversion and the hidden activation, defined once so that the training step and the
// evaluation cannot drift apart.  Device code: mlp_api.h is also included by host-compiled
// files and cannot hold these.
#pragma once
#include "common.h"

namespace dtfk {

__device__ __forceinline__ float act_fwd(float z, int act) {
  return act == 0 ? 1.f / (1.f + expf(-z)) : fmaxf(z, 0.f);
}
// derivative from the activation's output (sigmoid: a(1-a); relu: a > 0)
__device__ __forceinline__ float act_bwd(float a, int act) {
  return act == 0 ? a * (1.f - a) : (a > 0.f ? 1.f : 0.f);
}

// A uint8 pixel as the float32 the MNIST loader feeds: k / 255 correctly rounded
// (numpy's float32 division; data/mnist.py), so a uint8 feed -- training or
// evaluation -- is bit-identical to the float one.
__device__ __forceinline__ float px255(uint32_t k) { return __fdiv_rn((float)k, 255.f); }

}  // namespace dtfk
