// Host interface of csrc/kernels/ffm.hip: the field-aware factorization machine
// (Juan et al. 2016) on one GPU.  ffm_rows scores a batch given as a CSR over
// (row, field) bags and, training, leaves the bag gradients in the form
// table_update.h's one-writer update takes (wide_deep_update.h dtfk_wd_update with
// B * P bags of width P * K): this file has no update kernels of its own.
#pragma once
#include <hip/hip_runtime_api.h>

namespace dtfk {
namespace ffm {

constexpr int MAXP = 32;      // fields: a lane holds each bag offset of a row, a half wave one tile row's 16-byte blocks
constexpr int MAXW = 128;     // P * K: the update's width limit

struct RowArgs {
  const float* w;             // [F]
  const float* V;             // [F, P * K], 16-byte aligned; columns q K .. (q + 1) K: the vector aimed at field q
  const float* bias;          // [1]
  long long F;
  int P, K, B;
  const long long* ids;       // [nnz]; outside [0, F): skipped and counted in brow
  const long long* offsets;   // [B * P + 1]: bag r P + p holds row r's entries of field p
  const float* vals;          // [nnz], or null: every value is 1
  const float* labels;        // [B]
  float* lrow;                // [B] sigmoid cross-entropy of the row
  float* prow;                // [B] sigmoid(z); may be null when training
  int* brow;                  // [B] ids outside the table
  float* z_out;               // [B] or null
  float* p_out;               // [B] or null: a second copy of prow
  // training only
  float* dz;                  // [B] (sigmoid(z) - y) gscale
  float* dzbag;               // [B * P] the row's dz, once per bag
  float* G;                   // [B * P, P * K] bag gradients: block q of bag (r, p) is dz_r A_r[q][p, :], 0 for q == p; 16-byte aligned
  float gscale;
};

}  // namespace ffm
}  // namespace dtfk

extern "C" {
// 1 if the kernel takes P fields of K factors: K a multiple of 4, 2 <= P <= 32, P * K <= 128.
int dtfk_ffm_supported(int P, int K);
// The LDS bytes of one row's tile (P rows of the padded stride); *waves (may be null): the waves per workgroup.
int dtfk_ffm_tile_bytes(int P, int K, int* waves);
// ffm_rows on `stream`; train != 0 also writes dz, dzbag and G.
// hipErrorInvalidValue before any launch: an unsupported shape, a missing or misaligned pointer, B < 1, F < 1,
// B * P >= 2^31.
hipError_t dtfk_ffm_rows(const dtfk::ffm::RowArgs* a, int train, hipStream_t stream);
}
