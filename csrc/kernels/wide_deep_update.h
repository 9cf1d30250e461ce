// Host interface of csrc/kernels/wide_deep_update.hip: the one-writer update of
// the Wide&Deep tables (wide [V, 1]: Args::lin, embedding [V, D]: Args::row) from
// one sorted pass over a batch's ids, for every row-local rule of optim_rules.h.
// The args and the scheme: table_update.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include "table_update.h"

extern "C" {
// scale[b] of the mean (mode 1) / sqrtn (mode 2) combiner for every bag, as embedding_bag_bwd computes it.
hipError_t dtfk_wd_update_scale(const long long* offsets, const float* vals, int B, int mode, float* scale,
                                hipStream_t stream);
// wd_update_runs, then wd_update_carry, on `stream`.  hipErrorInvalidValue before any launch: what
// table_update.h's check refuses.
hipError_t dtfk_wd_update(const dtfk::tu::Args* a, hipStream_t stream);
}
