// Host interface of csrc/kernels/wide_deep_update.hip: the one-writer update of
// the Wide&Deep tables (wide [V, 1] and embedding [V, D]) from one sorted pass
// over a batch's ids, for every row-local rule of optim_rules.h.
#pragma once
#include <hip/hip_runtime_api.h>

#include "optim_rules.h"

namespace dtfk {
namespace wdu {

constexpr int CHUNK = 64;     // sorted positions per wave
constexpr int MAXD = 128;

struct Args {
  const int* sids;            // [N] the ids in ascending order (stable sort); outside [0, V): no part in anything
  const long long* perm;      // [N] the CSR position of each sorted position
  const int* bag_of;          // [N] the bag of each CSR position
  const float* vals;          // [N] by CSR position, or null: every value is 1
  const float* scale;         // [B] the combiner's scale per bag, or null (sum)
  const float* dz;            // [B] the wide table's bag gradient
  const float* demb;          // [B, D] the embedding table's bag gradient
  float *wide, *wide_a, *wide_b;   // [V] table and its slots (null where the kind has none)
  float *emb, *emb_a, *emb_b;      // [V, D], 16-byte aligned
  float* part;                // [chunks, 2, D + 4]: a chunk's leading / trailing partial sums (columns, then wide)
  long long N, V;
  int D, kind;
  OptimHyper h;
  const int* skip;            // device word, may be null: nonzero changes nothing
};

}  // namespace wdu
}  // namespace dtfk

extern "C" {
// Floats of Args::part for N ids.
long long dtfk_wd_update_part_floats(long long N, int D);
// scale[b] of the mean (mode 1) / sqrtn (mode 2) combiner for every bag, as embedding_bag_bwd computes it.
hipError_t dtfk_wd_update_scale(const long long* offsets, const float* vals, int B, int mode, float* scale,
                                hipStream_t stream);
// wd_update_runs, then wd_update_carry, on `stream`.  hipErrorInvalidValue before any launch: a kind that is
// not row-local, a missing slot, FTRL hyper-parameters out of range, D not a multiple of 4 in 4 .. 128,
// V >= 2^31 or N >= 2^31.
hipError_t dtfk_wd_update(const dtfk::wdu::Args* a, hipStream_t stream);
}
