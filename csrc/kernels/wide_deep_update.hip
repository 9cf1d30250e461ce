// Reached by: WideDeepTrainPlan.update (csrc/bind_wide_deep.cpp), WideDeep(fused_step="combined"), FFMPlan.update (csrc/bind_ffm.cpp: B P bags of width P K); tests/test_wide_deep_update_gpu.py
// The table update of the one-GPU Wide&Deep training step: table_update.h's
// one-writer scheme (described there) on the wide table [V, 1] and the embedding
// table [V, D], an occurrence weighted by its value and the combiner's scale of
// its bag, which wd_update_scale computes here.
#include "common.h"
#include "wide_deep_update.h"

namespace dtfk {
namespace wdu {

using tu::WAVES;

// scale[b] of a bag: embedding_bag_bwd's formula and wave_sum order
__global__ __launch_bounds__(256) void wd_update_scale(const long long* __restrict__ offsets,
                                                       const float* __restrict__ vals, int B, int mode,
                                                       float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  const long long s = offsets[b], e = offsets[b + 1];
  float ws = 0.f;
  for (long long j = s + lane; j < e; j += 64) {
    const float w = vals ? vals[j] : 1.f;
    ws += mode == 2 ? w * w : w;
  }
  ws = wave_sum(ws);
  float sc = 1.f;
  if (mode == 1 && e > s) sc = 1.f / fmaxf(ws, 1e-30f);
  if (mode == 2 && e > s) sc = rsqrtf(fmaxf(ws, 1e-30f));
  if (lane == 0) scale[b] = sc;
}

__global__ __launch_bounds__(256) void wd_update_runs(const tu::Args a) { tu::update_runs<false>(a); }
__global__ __launch_bounds__(256) void wd_update_carry(const tu::Args a) { tu::update_carry<false>(a); }

}  // namespace wdu
}  // namespace dtfk

extern "C" hipError_t dtfk_wd_update_scale(const long long* offsets, const float* vals, int B, int mode, float* scale,
                                           hipStream_t stream) {
  using namespace dtfk::wdu;
  if (B <= 0) return hipSuccess;
  if (mode != 1 && mode != 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wd_update_scale, dim3((unsigned)((B + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, stream, offsets,
                     vals, B, mode, scale);
  return hipGetLastError();
}

extern "C" hipError_t dtfk_wd_update(const dtfk::tu::Args* a, hipStream_t stream) {
  return dtfk::tu::launch(a, stream, dtfk::wdu::wd_update_runs, dtfk::wdu::wd_update_carry);
}
