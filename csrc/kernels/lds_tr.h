// The M/N-contiguous LDS operand image and its transposed fragment read, shared by the
// large-tile GEMM (gemm_big.hip) and the convolution's weight gradient (conv_igemm.hip): the
// staging side and the reading side must agree on the swizzle, so both take it from here.
#pragma once
#include "common.h"

namespace dtfk {

// M/N-contiguous [BK][R] bf16: byte offset of (k, 16-byte chunk ch = mn/8).
// A transposed fragment read (frag_tr, ds_read_b64_tr_b16) takes a 32-byte
// segment from each of 16 k-rows (k = 32 s + {0..3, 8..11, 16..19, 24..27});
// the chunk XOR spreads them over the bank row.  R >= 128 (rows >= 256 B):
// k bits 0, 1, 3 pick one of 8 segments.  R = 64 (128-byte rows, two per
// 256-byte bank row): k bit 0 already picks the half, so the XOR takes bits 1
// and 3 -- the masked R >= 128 XOR there (2 (k & 3)) collided with bit 0 and
// left half the banks unused: 2x the LDS cycles of every B read of a 192-wide
// tile's second quadrant column (SQ_LDS_BANK_CONFLICT 5x, profiles/gemm_layout_ab_r6.txt).
__device__ __forceinline__ int mn_swz(int k) { return (k & 3) | (((k >> 3) & 1) << 2); }
template <int R>
__device__ __forceinline__ int mn_sw(int k) {
  if constexpr (R == 64) return (((k >> 1) & 1) | (((k >> 3) & 1) << 1)) << 1;
  else return (mn_swz(k) << 1) & (R / 8 - 1);
}
template <int R>
__device__ __forceinline__ int mn_off(int k, int ch) {
  return k * (2 * R) + ((ch ^ mn_sw<R>(k)) << 4);
}

// MFMA 16x16x32 operand fragment of rows [rb, rb+16), k-sub s (k = 32 s ...) of an
// M/N-contiguous image: lane l gets (row rb + (l&15), k = 32 s + 8 (l>>4) + j), j = 0..7.
template <int R>
__device__ __forceinline__ bf16x8 frag_tr(const uint8_t* img, int rb, int s, int lane) {
  // ds_read_b64_tr_b16: lane 4q+p of a 16-lane group addresses row k0+q,
  // columns 4p..4p+3 of the 4x16 block; lane i receives column i, row q in q
  const int k = s * 32 + 8 * (lane >> 4) + ((lane & 15) >> 2);
  const int mn = rb + 4 * (lane & 3);
  const int off = mn_off<R>(k, mn >> 3) + ((mn & 7) << 1);
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(img + off));
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(img + off + 4 * 2 * R));
  typedef __attribute__((ext_vector_type(8))) short v8s;
  const v8s v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

}  // namespace dtfk
