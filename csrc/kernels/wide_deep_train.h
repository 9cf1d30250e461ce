// Host interface of csrc/kernels/wide_deep_train.hip (the one-GPU Wide&Deep
// training step's rows kernel: bags, tower forward, head and the backward
// through the tower in one launch; and the small fixed-order reduce after it).
#pragma once
#include <hip/hip_runtime_api.h>

#include "wide_deep_eval.h"

namespace dtfk {
namespace wdt {

struct Args {
  // tables, batch, tower, bias, B, lrow [B], brow [B], z_out [B] (all three
  // required here); prow and p_out are not used
  wde::Args f;
  float* act[wde::MAXL];       // act[0] [B, D]: the scaled bag output; act[l] [B, dims[l]]: hidden layer l after ReLU
  float* dzl[wde::MAXL];       // dzl[l] [B, dims[l]], l = 1 .. nl - 1: the gradient at hidden layer l's pre-activation
  float* demb;                 // [B, D]: the gradient at the scaled bag output
  float* dz;                   // [B]: (sigmoid(z) - y) gscale, also the wide table's bag gradient
  float gscale;                // the loss's scale per row (a mean over the batch: 1 / B)
};

}  // namespace wdt
}  // namespace dtfk

extern "C" {
// 1 if wd_train_rows takes this tower: the towers of dtfk_wd_eval_supported.
int dtfk_wd_train_supported(int D, int nl, const int* dims);
// The row tile (16 or 32) the automatic rule picks for B rows of this tower.
int dtfk_wd_train_tile(int B, int nl, const int* dims);
// Dynamic + static LDS bytes of one workgroup for this shape and tile.
long long dtfk_wd_train_lds_bytes(int D, int nl, const int* dims, int tile);
// The rows kernel on `stream`; tile: 16, 32 or 0 (automatic).
hipError_t dtfk_wd_train_rows(const dtfk::wdt::Args* a, int tile, hipStream_t stream);
// loss[0] = sum(lrow) / B and dsum[0] = dsum2[0] = sum(dz), each summed in
// float64 in one fixed order by one workgroup (dsum2 may be null).
hipError_t dtfk_wd_train_sums(const float* lrow, const float* dz, int B, float* loss, float* dsum, float* dsum2,
                              hipStream_t stream);
}
