// The evaluation record every forward-only evaluation adds its batches to, and
// the host interface of its reduce kernel (csrc/kernels/eval_record.hip).  As
// int64 on the device:
//
//   {loss sum (fp64 bits), rows, bad ids, pos[T + 1], neg[T + 1]}
//
// pos / neg: streaming_auc's histograms over T thresholds (auc_bin.h).  The
// layout is written down here and in models/eval_record.py, nowhere else.
// Includable from host .cpp files.
#pragma once
#include <hip/hip_runtime_api.h>

namespace dtfk {
namespace evrec {

constexpr int LOSS = 0;   // the sum of the row losses, the bits of a double
constexpr int ROWS = 1;
constexpr int BAD = 2;    // ids outside [0, F)
constexpr int HEAD = 3;   // pos starts here, neg at HEAD + T + 1

inline long long length(int T) { return HEAD + 2 * ((long long)T + 1); }
// T of a record of n entries; -1: no record has that length (T >= 2)
inline int thresholds_of(long long n) {
  return (n >= length(2) && n <= length((1 << 30) - 1) && (n - HEAD) % 2 == 0) ? (int)((n - HEAD) / 2 - 1) : -1;
}

// whether dtfk_eval_reduce takes these arguments
inline bool reduce_args_ok(const float* lrow, const float* prow, const int* brow, const float* labels, int B, int T,
                           const long long* rec) {
  return B >= 1 && T >= 2 && rec != nullptr && lrow != nullptr && prow != nullptr && brow != nullptr &&
         labels != nullptr;
}

}  // namespace evrec
}  // namespace dtfk

extern "C" {
// The per-row loss / sigmoid(z) / bad-id count of B rows and their labels (all
// device memory) into the record `rec` of T thresholds, on `stream`: one
// workgroup, plain loads and stores.  reset != 0 starts the record over, else
// the batch is added.  hipErrorInvalidValue, before any launch, for arguments
// reduce_args_ok refuses.
hipError_t dtfk_eval_reduce(const float* lrow, const float* prow, const int* brow, const float* labels, int B, int T,
                            int reset, long long* rec, hipStream_t stream);
}
