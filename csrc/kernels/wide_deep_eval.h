// Host interface of csrc/kernels/wide_deep_eval.hip (the rows kernel of the
// forward-only Wide&Deep evaluation; the reduce that follows it: eval_record.h).
#pragma once
#include <hip/hip_runtime_api.h>

namespace dtfk {
namespace wde {

constexpr int MAXL = 4;        // tower layers: 1 to 3 hidden + the width-1 last one
constexpr int MAXD = 128;      // embedding columns (a multiple of 4)
constexpr int MAXW = 512;      // hidden width (a multiple of 16)

struct Args {
  const float* Wt;             // wide table [F] (= [F, 1])
  const float* E;              // embedding table [F, D]
  long long F;
  int D, mode;                 // mode: 0 sum, 1 mean, 2 sqrtn (ops.hip embedding_bag_fwd's)
  const long long* ids;        // [nnz]
  const long long* offsets;    // [B + 1]
  const float* vals;           // [nnz] or null (all 1)
  const float* labels;         // [B]
  const float* W[MAXL];        // layer l: [dims[l], dims[l + 1]] row-major
  const float* b[MAXL];        // [dims[l + 1]]
  int dims[MAXL + 1];          // dims[0] = D, dims[nl] = 1
  int nl;                      // layers, the last one included (2 .. MAXL)
  const float* bias;           // the shared bias, one value
  int B;
  float* lrow;                 // [B] per-row loss
  float* prow;                 // [B] per-row sigmoid(z)
  int* brow;                   // [B] per-row out-of-range ids
  float* z_out;                // [B] or null
  float* p_out;                // [B] or null
  int ld0, ld1;                // row strides (floats) of the two LDS activation buffers: filled by the host entry
  int lsh;                     // log2 of the lanes that read one table row (16 bytes each): filled by the host entry
};

}  // namespace wde
}  // namespace dtfk

extern "C" {
// 1 if wd_eval_rows takes this tower: D % 4 == 0, 4 <= D <= 128, nl in 2 .. 4,
// every hidden width a multiple of 16 up to 512, dims[nl] == 1.
int dtfk_wd_eval_supported(int D, int nl, const int* dims);
// The row tile (16 or 32) the automatic rule picks for B rows of this tower.
int dtfk_wd_eval_tile(int B, int nl, const int* dims);
// Dynamic + static LDS bytes of one workgroup for this shape and tile.
long long dtfk_wd_eval_lds_bytes(int D, int nl, const int* dims, int tile);
// The rows kernel on `stream`; tile: 16, 32 or 0 (automatic).
hipError_t dtfk_wd_eval_rows(const dtfk::wde::Args* a, int tile, hipStream_t stream);
}
