// Reached by: sharded-table sparse optimizers (Wide&Deep sparse_opt=adagrad/rmsprop/momentum/ftrl); tests/test_sparse_optim_gpu.py, test_ftrl_gpu.py, test_optim_rules_gpu.py
// Row-sparse optimizer updates of a sharded embedding table, on its owner
// (parallel/sharded_embedding.py: ShardedEmbedding.set_optimizer).
//
// TensorFlow applies an IndexedSlices gradient with its SparseApply* ops:
// duplicate indices are summed first (Optimizer._apply_sparse_duplicate_indices),
// then every touched row is updated on its own -- rows the batch did not touch
// keep their value AND their slots.  The owner has already summed the
// duplicates of a step (every rank that looked a row up sends its gradient);
// this kernel is the per-row update, by the rules of optim_rules.h (slot_a,
// slot_b as named there): kinds sgd, momentum, adagrad, rmsprop and ftrl.  Adam
// is not row-local (m / v decay on every row): a sharded table runs the fused
// multi-tensor Adam over its shard instead.
//
// rows[i] < 0 marks an entry with no update
// (exchange padding, the non-first copies of a duplicated row).  Rows with
// rows[i] >= 0 are distinct, so every element has exactly one writer: plain
// loads and stores, no atomics.  One thread per (entry, column), 4 columns
// per thread when D % 4 == 0.  `skip` (device int32, may be null): a voided
// step (sharded-exchange overflow) changes nothing.
#include "common.h"
#include "ops_api.h"
#include "optim_rules.h"

namespace dtfk {
namespace sparse_optim {

constexpr bool row_local(int kind) {
  return kind == OPT_SGD || kind == OPT_MOMENTUM || kind == OPT_ADAGRAD || kind == OPT_RMSPROP || kind == OPT_FTRL;
}

// `kind` is a run-time, wave-uniform branch
__device__ __forceinline__ void update1(float& var, float& a, float& b, float g, int kind, const OptimHyper& h) {
  switch (kind) {
    case OPT_SGD: rule_sgd(var, g, h.lr); break;
    case OPT_MOMENTUM: rule_momentum(var, a, g, h.lr, h); break;
    case OPT_ADAGRAD: rule_adagrad<true>(var, a, g, h.lr); break;
    case OPT_RMSPROP: rule_rmsprop<true>(var, a, b, g, h.lr, h); break;
    default: ftrl_update(var, a, b, g, h.lr, h.p, h.l1, h.l2, h.shrink); break;   // OPT_FTRL
  }
}

template <int V>
__global__ __launch_bounds__(256) void rows_apply(float* __restrict__ table, float* __restrict__ slot_a,
                                                  float* __restrict__ slot_b, const long long* __restrict__ rows,
                                                  const float* __restrict__ g, long long n, int D, int kind,
                                                  OptimHyper h, const int* __restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;
  const int dv = D / V;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * dv) return;
  const long long i = e / dv;
  const int c = (int)(e - i * dv) * V;
  const long long r = rows[i];
  if (r < 0) return;
  const size_t o = (size_t)r * D + c;
  const size_t go = (size_t)i * D + c;
  float var[V], a[V], b[V], gg[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    var[k] = table[o + k];
    a[k] = slot_a != nullptr ? slot_a[o + k] : 0.f;
    b[k] = slot_b != nullptr ? slot_b[o + k] : 0.f;
    gg[k] = g[go + k];
  }
#pragma unroll
  for (int k = 0; k < V; ++k) update1(var[k], a[k], b[k], gg[k], kind, h);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    table[o + k] = var[k];
    if (slot_a != nullptr) slot_a[o + k] = a[k];
    if (slot_b != nullptr) slot_b[o + k] = b[k];
  }
}

}  // namespace sparse_optim
}  // namespace dtfk

extern "C" hipError_t dtfk_sparse_rows_apply(float* table, float* slot_a, float* slot_b, const long long* rows,
                                             const float* g, long long n, int D, int kind,
                                             const dtfk::OptimHyper& h, const int* skip, hipStream_t s) {
  using namespace dtfk;
  using namespace dtfk::sparse_optim;
  if (n <= 0 || D <= 0) return hipSuccess;
  if (!row_local(kind)) return hipErrorInvalidValue;
  if (uses_slot_a(kind) && slot_a == nullptr) return hipErrorInvalidValue;
  if (uses_slot_b(kind) && slot_b == nullptr) return hipErrorInvalidValue;
  if (kind == OPT_FTRL && !ftrl_hyper_ok(h)) return hipErrorInvalidValue;
  const bool v4 = D % 4 == 0;
  const long long work = n * (v4 ? D / 4 : D);
  const unsigned grid = (unsigned)((work + 255) / 256);
  const auto kernel = v4 ? rows_apply<4> : rows_apply<1>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, table, slot_a, slot_b, rows, g, n, D, kind, h, skip);
  return hipGetLastError();
}
