// What the fused attention kernels share: attention.hip (whole-S LDS images, S <= 256)
// and attention_long.hip (streamed key / query blocks, S >= 384) include this header; the
// operand fragments, the transposed LDS read, the dropout rule and
// the host helpers of the launchers are written once.  Included by .hip files only.
#pragma once
#include "common.h"

namespace dtfk {
namespace attn {

constexpr int D = 64;
constexpr int KP = 72;     // padded row of a [S][64] LDS image (144 B: rows spread over banks)

__device__ __forceinline__ uint4 add_bias8(uint4 u, const float* __restrict__ bias) {
  if (!bias) return u;
  const float4 b0 = *reinterpret_cast<const float4*>(bias);
  const float4 b1 = *reinterpret_cast<const float4*>(bias + 4);
  const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
  uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int j = 0; j < 4; ++j)
    w[j] = pack2bf(bf2f(w[j] & 0xffff) + bb[2 * j], bf2f(w[j] >> 16) + bb[2 * j + 1]);
  return uint4{w[0], w[1], w[2], w[3]};
}

__device__ __forceinline__ uint4 ld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }

__device__ __forceinline__ bf16x8 as_frag(uint4 u) { return __builtin_bit_cast(bf16x8, u); }

// The permuted 32-key fragment of a TRANSPOSED operand straight from a
// row-major [S][KP] image with the gfx950 transposed LDS read
// (ds_read_b64_tr_b16: per 16-lane group, lane 4q+p addresses row q, columns
// 4p..4p+3 of a 4 x 16 block; lane i receives column i): lane (g, c) gets
// column col0 + c of rows row0 + 4g + 0..3 (elements 0..3) and row0 + 16 + 4g +
// 0..3 (elements 4..7) -- the k-slot order of the score accumulators.  Replaces
// a second, transposed LDS image written with 2-byte scatter stores.  EXEC must
// be full (wave-uniform control flow only).
typedef __attribute__((ext_vector_type(4))) short v4s_t;
typedef __attribute__((address_space(3))) v4s_t lds_v4s_t;
__device__ __forceinline__ bf16x8 ld_tr_pair(const uint16_t* img, int row0, int col0, int l) {
  const int g = l >> 4, q = (l >> 2) & 3, p = l & 3;
  const uint16_t* a = img + (row0 + 4 * g + q) * KP + col0 + 4 * p;
  const v4s_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)(a));
  const v4s_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)(a + 16 * KP));
  typedef __attribute__((ext_vector_type(8))) short v8s_t;
  const v8s_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}

__device__ __forceinline__ bf16x8 pack8(const float* f) {
  return as_frag(uint4{pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7])});
}

__device__ __forceinline__ float keepf(uint64_t seed, uint64_t i, uint32_t thresh, float inv_keep) {
  return (thresh == 0u) ? 1.f : (hash32(seed, i) >= thresh ? inv_keep : 0.f);
}

}  // namespace attn
}  // namespace dtfk

// dropout threshold of the launchers: keep(i) = hash32(seed, i) >= p * 2^32
static inline uint32_t attn_thresh(float p) {
  if (p <= 0.f) return 0u;
  double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
}
