// streaming_auc's threshold binning, shared by every kernel that fills the
// positive / negative histograms (ops.hip auc_hist, eval_record.hip
// eval_record_reduce): both compile this one function, so a prediction lands in
// the same bin whichever kernel scored it.
#pragma once
#include <hip/hip_runtime.h>

namespace dtfk {

// streaming_auc's thresholds (TF contrib.metrics): t_0 = -1e-7, t_j = j/(T-1) for
// 0 < j < T-1 (a Python double rounded to fp32), t_{T-1} = 1 + 1e-7.  Bin k of a
// prediction p = #{i : t_i < p} in [0, T]; the confusion counts at threshold i
// (predicted positive <=> p > t_i) are then suffix sums over bins > i.
__device__ __forceinline__ int tf_threshold_bin(float p, int T) {
  if (!(p > -1e-7f)) return 0;          // (also NaN)
  if (p > 1.f + 1e-7f) return T;
  int lo = 1, hi = T - 1;               // first interior j with t_j >= p
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const float t = (float)((double)mid / (double)(T - 1));
    if (t < p) lo = mid + 1; else hi = mid;
  }
  return lo;                            // 1 (t_0) + (lo - 1) interior thresholds below p
}

}  // namespace dtfk
