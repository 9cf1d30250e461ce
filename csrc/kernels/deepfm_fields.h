// Host interface of csrc/kernels/deepfm_fields.hip: DeepFM (Guo et al. 2017) with
// fields on one GPU.  The batch is the (row, field) bag form of ffm.h, the tower's
// input the concatenation of the P per-field sums A_r[p] (K wide each), the FM term
// the one of deepfm.h over all of the row's entries.  dfmf_rows scores a bag batch
// and, training, leaves the tower's activations and gradients, the row's pooled
// factors S, dz once per bag and the bag gradient
//   demb[r P + p, :] = dz_r S_r + da_0,r[p K : (p + 1) K];
// the table update is fm.h's (dtfk_fm_update over the B P bags, with dzbag and demb
// viewed as [B P, K]), the sums wide_deep_train.h's, the evaluation's reduce
// eval_record.h's.
#pragma once
#include <hip/hip_runtime_api.h>

#include "wide_deep_train.h"

namespace dtfk {
namespace dfmf {

constexpr int MAXP = 64;       // fields: one lane holds the start of each bag of a row

struct Args {
  // wdt::Args as deepfm.h uses it, with  f.D = K (the table's width),  f.dims[0] = P K,
  // f.offsets [B P + 1],  act[0] [B, P K] the concatenation,  demb [B, P K] = [B P, K]
  wdt::Args t;
  int P;                       // fields
  float* S;                    // [B, K] the row's pooled factors (training only)
  float* dzbag;                // [B P] dz_r once per bag (training only)
};

}  // namespace dfmf
}  // namespace dtfk

extern "C" {
// 1 if dfmf_rows takes P fields of K factors and this tower: K a multiple of 4 in 4 .. 128, 1 <= P <= 64,
// P K <= 512, dims[0] == P K, nl in 2 .. 4, hidden widths multiples of 16 up to 512, dims[nl] == 1.
int dtfk_dfmf_supported(int P, int K, int nl, const int* dims);
// Dynamic + static LDS bytes of one workgroup: the two activation buffers of wde::strides(P K, ..), the
// S area (4 K per tile row) and 12 bytes per tile row (FM score, bad ids, dz).
long long dtfk_dfmf_lds_bytes(int P, int K, int nl, const int* dims, int tile);
// dfmf_rows on `stream`; train == 0: lrow, prow, brow and, where given, z_out / p_out, nothing else;
// train != 0: lrow, brow, z_out, dz, dzbag, S, act, dzl, demb.  tile: 16, 32 or 0 (deepfm.h's rule).
// hipErrorInvalidValue before any launch: an unsupported shape, mode != 0, a missing or misaligned
// pointer, B < 1, B P >= 2^31, F < 1, another tile, or more LDS than 160 KiB.
hipError_t dtfk_dfmf_rows(const dtfk::dfmf::Args* a, int train, int tile, hipStream_t stream);
}
