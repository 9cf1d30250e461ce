// Host interface of csrc/kernels/deepfm.hip: DeepFM (Guo et al. 2017) on one GPU,
// a factorization machine and an MLP tower that read the same factor table.
// dfm_rows scores a CSR batch and, training, leaves the tower's activations and
// gradients and the bag gradient demb = dz S + da_0; the table update is fm.h's
// (dtfk_fm_update, with this kernel's dz and demb), the sums wide_deep_train.h's
// and the evaluation's reduce eval_record.h's.  This is the form without fields (the
// tower reads the pooled S); the form whose tower reads the concatenated per-field
// embeddings is deepfm_fields.h.
//
// The argument struct is wide_deep_train.h's wdt::Args:  f.Wt = w [F], f.E = V [F, K],
// f.D = K, f.mode = 0 (sum: there is no combiner scale), the tower in f.W / f.b /
// f.dims / f.nl, act[0] = S [B, K], act[l], dzl[l], demb [B, K], dz [B], gscale.
#pragma once
#include <hip/hip_runtime_api.h>

#include "wide_deep_train.h"

extern "C" {
// 1 if dfm_rows takes K factors and this tower: dtfk_wd_eval_supported's answer with D = K.
int dtfk_dfm_supported(int K, int nl, const int* dims);
// The row tile (16 or 32) the automatic rule picks for B rows of this tower: the
// Wide&Deep evaluation's rule as it stands, not measured for this kernel.
int dtfk_dfm_tile(int B, int nl, const int* dims);
// Dynamic + static LDS bytes of one workgroup for this shape and tile: wd_train_rows's plus 4 tile (dz per row).
long long dtfk_dfm_lds_bytes(int K, int nl, const int* dims, int tile);
// dfm_rows on `stream`; train == 0: lrow, prow, brow and, where given, z_out / p_out, nothing else;
// train != 0: lrow, brow, z_out, dz, act, dzl, demb.  tile: 16, 32 or 0 (automatic).
// hipErrorInvalidValue before any launch: an unsupported shape, mode != 0, a missing or misaligned
// pointer, B < 1, F < 1, another tile, or more LDS than 160 KiB.
hipError_t dtfk_dfm_rows(const dtfk::wdt::Args* a, int train, int tile, hipStream_t stream);
}
