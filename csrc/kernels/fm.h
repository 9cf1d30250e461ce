// Host interface of csrc/kernels/fm.hip: the second-order factorization machine
// (Rendle 2010) on one GPU.  fm_rows scores a CSR batch (and, training, leaves the
// bag gradients); fm_update_runs + fm_update_carry write every touched row of the
// linear table w [F] and the factor table V [F, K] once, by a row-local rule of
// optim_rules.h (the args and the scheme: table_update.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include "table_update.h"

namespace dtfk {
namespace fm {

constexpr int MAXK = 128;
constexpr int MAXRPW = 64;    // rows per wave of fm_rows: one lane holds each row's offsets

struct RowArgs {
  const float* w;             // [F]
  const float* V;             // [F, K], 16-byte aligned
  const float* bias;          // [1]
  long long F;
  int K, B;
  const long long* ids;       // [nnz]; outside [0, F): skipped and counted in brow
  const long long* offsets;   // [B + 1]
  const float* vals;          // [nnz], or null: every value is 1
  const float* labels;        // [B]
  float* lrow;                // [B] sigmoid cross-entropy of the row
  float* prow;                // [B] sigmoid(z); may be null when training
  int* brow;                  // [B] ids outside the table
  float* z_out;               // [B] or null
  float* p_out;               // [B] or null: a second copy of prow
  // training only
  float* dz;                  // [B] (sigmoid(z) - y) gscale
  float* demb;                // [B, K] dz S, 16-byte aligned
  float gscale;
};

}  // namespace fm
}  // namespace dtfk

extern "C" {
// 1 if the kernels take K factors: a multiple of 4 in 4 .. 128.
int dtfk_fm_supported(int K);
// The rows per wave the automatic rule picks for a batch of B rows.
int dtfk_fm_rpw(int B);
// fm_rows on `stream`; train != 0 also writes dz and demb.  rpw: rows per wave, 1 .. 64, or 0 (automatic).
// hipErrorInvalidValue before any launch: an unsupported K, a missing or misaligned pointer, B < 1, F < 1.
hipError_t dtfk_fm_rows(const dtfk::fm::RowArgs* a, int train, int rpw, hipStream_t stream);
// fm_update_runs, then fm_update_carry, on `stream`: table_update.h's FM form, Args::lin = w, Args::row = V.
// hipErrorInvalidValue before any launch: what table_update.h's check refuses.
hipError_t dtfk_fm_update(const dtfk::tu::Args* a, hipStream_t stream);
}
