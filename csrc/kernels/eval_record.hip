// Reached by: the reduce step of every forward-only evaluation (dtfk_slr_eval in sparse_lr.hip; csrc/bind_wide_deep.cpp WideDeepEvalPlan.evaluate after wd_eval_rows) and csrc/bind_eval_record.cpp eval_record_reduce; tests/test_eval_record_gpu.py, test_sparse_lr_eval_gpu.py, test_wide_deep_eval_gpu.py
// The evaluation record's one writer (layout: eval_record.h).  A model's rows
// kernel leaves per-row loss, p = sigmoid(z) and out-of-range id count in
// scratch; eval_record_reduce, one workgroup, sums the row losses in a fixed
// order in fp64, bins every p over streaming_auc's thresholds (auc_bin.h, the
// function ops.hip auc_hist compiles) in an LDS histogram, and adds both to the
// record with plain loads and stores.  The record accumulates across calls;
// `reset` (a kernel argument, not a memset node) starts it over.  No float
// atomics: two runs give the same bits.
#include "auc_bin.h"
#include "common.h"
#include "eval_record.h"

namespace dtfk {
namespace evrec {

constexpr int THREADS = 256;

// Every thread passes every barrier (no early return).  The histogram is built
// EBINS bins at a time (one pass for T < EBINS).
constexpr int EBINS = 4096;   // 2 x 16 KB of LDS

__global__ __launch_bounds__(THREADS) void eval_record_reduce(const float* __restrict__ lrow,
                                                              const float* __restrict__ prow,
                                                              const int* __restrict__ brow,
                                                              const float* __restrict__ labels, int B, int T, int reset,
                                                              long long* __restrict__ rec) {
  __shared__ unsigned int h[2][EBINS];
  __shared__ double redl[THREADS / 64];
  __shared__ long long redb[THREADS / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double sl = 0.0;
  long long sb = 0;
  for (int i = threadIdx.x; i < B; i += THREADS) {   // fixed order: thread, then lanes, then waves
    sl += (double)lrow[i];
    sb += brow[i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sl += __shfl_xor(sl, off, 64);
    sb += __shfl_xor(sb, off, 64);
  }
  if (lane == 0) {
    redl[wv] = sl;
    redb[wv] = sb;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tl = 0.0;
    long long tb = 0;
    for (int k = 0; k < THREADS / 64; ++k) {
      tl += redl[k];
      tb += redb[k];
    }
    const double l0 = reset ? 0.0 : __longlong_as_double(rec[0]);
    rec[0] = __double_as_longlong(l0 + tl);
    rec[1] = (reset ? 0 : rec[1]) + B;
    rec[2] = (reset ? 0 : rec[2]) + tb;
  }
  const int nb = T + 1;
  long long* pos = rec + 3;
  long long* neg = rec + 3 + nb;
  for (int c0 = 0; c0 < nb; c0 += EBINS) {
    const int cn = min(EBINS, nb - c0);
    for (int i = threadIdx.x; i < cn; i += THREADS) {
      h[0][i] = 0;
      h[1][i] = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < B; i += THREADS) {
      const int k = tf_threshold_bin(prow[i], T) - c0;   // labels: nonzero = positive (TF casts to bool)
      if (k >= 0 && k < cn) atomicAdd(&h[labels[i] != 0.f ? 0 : 1][k], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cn; i += THREADS) {
      pos[c0 + i] = (reset ? 0 : pos[c0 + i]) + (long long)h[0][i];
      neg[c0 + i] = (reset ? 0 : neg[c0 + i]) + (long long)h[1][i];
    }
    __syncthreads();
  }
}

static_assert(LOSS == 0 && ROWS == 1 && BAD == 2 && HEAD == 3,
              "eval_record_reduce writes rec[0 .. 2] and the histograms from rec + 3");

}  // namespace evrec
}  // namespace dtfk

extern "C" hipError_t dtfk_eval_reduce(const float* lrow, const float* prow, const int* brow, const float* labels,
                                       int B, int T, int reset, long long* rec, hipStream_t stream) {
  using namespace dtfk::evrec;
  if (!reduce_args_ok(lrow, prow, brow, labels, B, T, rec)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(eval_record_reduce, dim3(1), dim3(THREADS), 0, stream, lrow, prow, brow, labels, B, T, reset, rec);
  return hipGetLastError();
}
