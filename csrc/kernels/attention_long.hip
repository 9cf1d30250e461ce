// Reached by: attention.hip (dtfk_attn_fwd / dtfk_attn_bwd pass S > 256 on); models/bert.py at max_position 384 / 512; tests/test_attention_long_gpu.py
// Fused multi-head self-attention for long sequences (head dim 64, S = 384 ...
// 2048, S % 128 == 0): the kernels of attention.hip with the whole-S LDS images
// replaced by 64-row blocks streamed through two LDS buffers, and the score row
// replaced by a running softmax.  Contracts, MFMA orientation (S^T = K Q^T, P^T
// from registers, transposed operands through ld_tr_pair) and the dropout rule
// are attention.hip's; see its header.
//
//   attn_long_fwd      a wave owns 16 queries (fragments in registers) and walks
//                      the key blocks: z = scale s + mask, running max m,
//                      alpha = exp(m_old - m), e = exp(z - m),
//                      l = alpha l + sum(e)  (the UNDROPPED e),
//                      acc = alpha acc + bf16(e keep) V;  O = acc / l,
//                      lse = m + log(l).  The rescale is applied in every block
//                      (alpha is exactly 1 where the max did not rise).
//   attn_long_bwd_dq   attn_bwd_dq's loop over streamed K / V blocks: D, P~ from
//                      lse, dS, dQ^T in registers.
//   attn_long_bwd_dkv  a workgroup owns 128 keys (a wave 16, dK / dV in
//                      accumulators) and walks the query blocks: Q / dO images,
//                      lse and D of the block's 128 queries.
//
// Staging is split around the MFMAs: block j+1's global loads are issued before
// block j's products and stored to the other LDS buffer after them; one barrier
// per block (the buffer written in step j was last read in step j-1, which every
// wave left through that step's barrier).  All waves are active (S % 128 == 0),
// so control flow around ld_tr_pair is uniform.  No atomics and no sums across
// workgroups: results are bit-identical from run to run.
#include "common.h"
#include "attention_device.h"
#include "transformer_api.h"

namespace dtfk {
namespace attn {

constexpr int KB = 64;           // rows of one streamed block (keys, or queries in attn_long_bwd_dkv)
constexpr int IMG = KB * KP;     // one row image, in bf16 elements

static_assert(KB * 8 == 512, "a block image is one 16-byte chunk per thread");

// One block image [KB][64] is 512 16-byte chunks, one per thread: row tid >> 3, columns
// 8 (tid & 7) ... + 7.  src is the block's first row (uniform), so a thread's address is a
// 32-bit offset from a scalar base, and the bias is added at the store (add_bias8's
// arithmetic, as stage_store's) from wherever bias64 points: global memory before the loop,
// an LDS copy inside it, where 8 values riding in registers across the block's products
// would cost 8 VGPRs a stage -- the kernels sit at the 128 that two workgroups per CU allow.
__device__ __forceinline__ uint4 blk_load(const uint16_t* __restrict__ src, int row_stride) {
  return ld16(src + (uint32_t)((threadIdx.x >> 3) * row_stride + (threadIdx.x & 7) * 8));
}
__device__ __forceinline__ void blk_store(uint4 v, const float* bias64, uint16_t* rows) {
  const int part = threadIdx.x & 7;
  v = add_bias8(v, bias64 ? bias64 + part * 8 : nullptr);
  *reinterpret_cast<uint4*>(rows + (threadIdx.x >> 3) * KP + part * 8) = v;
}

__global__ __launch_bounds__(512, 4) void attn_long_fwd(const uint16_t* __restrict__ qkv, const float* __restrict__ bias,
                                                     const float* __restrict__ mask, uint16_t* __restrict__ ctx,
                                                     float* __restrict__ lse, int S, int NH, float scale,
                                                     uint32_t thresh, float inv_keep, uint64_t seed) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  uint16_t* Ks = lds;                                        // [2][KB][KP]
  uint16_t* Vs = lds + 2 * IMG;                              // [2][KB][KP] (read transposed: ld_tr_pair)
  float* Ms = reinterpret_cast<float*>(lds + 4 * IMG);       // [2][KB] the block's mask values
  float* Bl = Ms + 2 * KB;                                   // [2][64] this head's k and v bias
  const int b = blockIdx.z, h = blockIdx.y;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  const long long RS = 3LL * NH * D;
  const uint16_t* base = qkv + (long long)b * S * RS + h * D;
  const float* bq = bias ? bias + h * D : nullptr;
  const float* bk = bias ? bias + (NH + h) * D : nullptr;
  const float* bv = bias ? bias + (2 * NH + h) * D : nullptr;
  const float* mrow = mask ? mask + (long long)b * S : nullptr;
  const int nb = S / KB;
  const int rs = 3 * NH * D;   // a block's rows span 64 * rs elements: 32-bit offsets
  uint4 rk = blk_load(base + NH * D, rs), rv = blk_load(base + 2 * NH * D, rs);
  float mreg = 0.f;
  if (mrow && threadIdx.x < KB) mreg = mrow[threadIdx.x];
  const int q = blockIdx.x * 128 + w * 16 + c;
  uint4 qraw[2];   // this wave's query fragments, in flight with the first stage
#pragma unroll
  for (int s = 0; s < 2; ++s) qraw[s] = ld16(base + (long long)q * RS + 32 * s + 8 * g);
  blk_store(rk, bk, Ks);
  blk_store(rv, bv, Vs);
  if (threadIdx.x < KB) Ms[threadIdx.x] = mreg;
  if (bias && threadIdx.x < 2 * D) Bl[threadIdx.x] = bk[(threadIdx.x >> 6) * NH * D + (threadIdx.x & 63)];
  __syncthreads();

  bf16x8 bqf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) bqf[s] = as_frag(add_bias8(qraw[s], bq ? bq + 32 * s + 8 * g : nullptr));
  const long long row = ((long long)b * NH + h) * S + q;
  const uint64_t ebase = (uint64_t)row * S;
  float mx = -3.0e38f;   // finite: exp(m_old - m) of the first block is 0, not exp(-inf + inf)
  float lsum = 0.f;      // this lane's share of l (its keys 4g+i of every tile); the four groups meet at the end
  f32x4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int j = 0; j < nb; ++j) {
    const int cur = j & 1;
    const bool more = j + 1 < nb;   // uniform
    if (more) {
      const uint16_t* nx = base + (long long)(j + 1) * KB * RS;
      rk = blk_load(nx + NH * D, rs);
      rv = blk_load(nx + 2 * NH * D, rs);
      if (mrow && threadIdx.x < KB) mreg = mrow[(j + 1) * KB + threadIdx.x];
    }
    const uint16_t* Kc = Ks + cur * IMG;
    const uint16_t* Vc = Vs + cur * IMG;
    const float* Mc = Ms + cur * KB;
    f32x4 sc[KB / 16];
#pragma unroll
    for (int t = 0; t < KB / 16; ++t) {
      sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 2; ++s) sc[t] = mfma16x16x32(ld_bf16x8(Kc + (16 * t + c) * KP + 32 * s + 8 * g), bqf[s], sc[t]);
    }
    float bm = -3.0e38f;
#pragma unroll
    for (int t = 0; t < KB / 16; ++t) {
      const float4 mk = *reinterpret_cast<const float4*>(Mc + 16 * t + 4 * g);
      const float m4[4] = {mk.x, mk.y, mk.z, mk.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sc[t][i] = sc[t][i] * scale + m4[i];
        bm = fmaxf(bm, sc[t][i]);
      }
    }
    bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
    bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
    const float mn = fmaxf(mx, bm);
    const float alpha = __expf(mx - mn);
    mx = mn;
    float bs = 0.f;
#pragma unroll
    for (int t = 0; t < KB / 16; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sc[t][i] = __expf(sc[t][i] - mx);
        bs += sc[t][i];
      }
    lsum = alpha * lsum + bs;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[u][i] *= alpha;
    const uint64_t eb = ebase + (uint64_t)j * KB;
#pragma unroll
    for (int kb = 0; kb < KB / 32; ++kb) {
      float f[8];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k0 = 32 * kb + 4 * g + i;
        f[i] = sc[2 * kb][i] * keepf(seed, eb + k0, thresh, inv_keep);
        f[4 + i] = sc[2 * kb + 1][i] * keepf(seed, eb + k0 + 16, thresh, inv_keep);
      }
      const bf16x8 pb = pack8(f);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = mfma16x16x32(ld_tr_pair(Vc, 32 * kb, 16 * u, l), pb, acc[u]);
    }
    if (more) {
      blk_store(rk, bias ? Bl : nullptr, Ks + (cur ^ 1) * IMG);
      blk_store(rv, bias ? Bl + D : nullptr, Vs + (cur ^ 1) * IMG);
      if (threadIdx.x < KB) Ms[(cur ^ 1) * KB + threadIdx.x] = mreg;
    }
    __syncthreads();
  }
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  const float inv = 1.f / lsum;
  if (g == 0) lse[row] = mx + __logf(lsum);
  uint16_t* out = ctx + ((long long)b * S + q) * NH * D + h * D;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    *reinterpret_cast<uint2*>(out + 16 * u + 4 * g) =
        uint2{pack2bf(acc[u][0] * inv, acc[u][1] * inv), pack2bf(acc[u][2] * inv, acc[u][3] * inv)};
}

__global__ __launch_bounds__(512, 4) void attn_long_bwd_dq(const uint16_t* __restrict__ qkv, const float* __restrict__ bias,
                                                        const float* __restrict__ mask, const uint16_t* __restrict__ ctx,
                                                        const uint16_t* __restrict__ dctx, const float* __restrict__ lse,
                                                        float* __restrict__ Dbuf, uint16_t* __restrict__ dqkv, int S,
                                                        int NH, float scale, uint32_t thresh, float inv_keep,
                                                        uint64_t seed, float* __restrict__ bpart) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  uint16_t* Ks = lds;                                        // [2][KB][KP] (also read transposed: ld_tr_pair)
  uint16_t* Vs = lds + 2 * IMG;                              // [2][KB][KP]
  float* Ms = reinterpret_cast<float*>(lds + 4 * IMG);       // [2][KB]
  float* Bl = Ms + 2 * KB;                                   // [2][64] this head's k and v bias
  const int b = blockIdx.z, h = blockIdx.y;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  const long long RS = 3LL * NH * D, HS = (long long)NH * D;
  const uint16_t* base = qkv + (long long)b * S * RS + h * D;
  const float* bq = bias ? bias + h * D : nullptr;
  const float* bk = bias ? bias + (NH + h) * D : nullptr;
  const float* bv = bias ? bias + (2 * NH + h) * D : nullptr;
  const float* mrow = mask ? mask + (long long)b * S : nullptr;
  const int nb = S / KB;
  const int rs = 3 * NH * D;   // a block's rows span 64 * rs elements: 32-bit offsets
  uint4 rk = blk_load(base + NH * D, rs), rv = blk_load(base + 2 * NH * D, rs);
  float mreg = 0.f;
  if (mrow && threadIdx.x < KB) mreg = mrow[threadIdx.x];
  const int q = blockIdx.x * 128 + w * 16 + c;
  const uint16_t* dor = dctx + ((long long)b * S + q) * HS + h * D;
  uint4 qraw[2], doraw[2];   // this wave's fragments, in flight with the first stage
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    qraw[s] = ld16(base + (long long)q * RS + 32 * s + 8 * g);
    doraw[s] = ld16(dor + 32 * s + 8 * g);
  }
  blk_store(rk, bk, Ks);
  blk_store(rv, bv, Vs);
  if (threadIdx.x < KB) Ms[threadIdx.x] = mreg;
  if (bias && threadIdx.x < 2 * D) Bl[threadIdx.x] = bk[(threadIdx.x >> 6) * NH * D + (threadIdx.x & 63)];
  __syncthreads();

  bf16x8 bqf[2], bdo[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bqf[s] = as_frag(add_bias8(qraw[s], bq ? bq + 32 * s + 8 * g : nullptr));
    bdo[s] = as_frag(doraw[s]);
  }
  // D = rowsum(dO * O): lane group g covers d = 16g .. 16g+15
  const uint16_t* orow = ctx + ((long long)b * S + q) * HS + h * D + 16 * g;
  float dsum = 0.f;
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    const uint4 ov = ld16(orow + 8 * half), dv = ld16(dor + 16 * g + 8 * half);
    const uint32_t a[4] = {ov.x, ov.y, ov.z, ov.w}, d4[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      dsum += bf2f(a[i] & 0xffff) * bf2f(d4[i] & 0xffff) + bf2f(a[i] >> 16) * bf2f(d4[i] >> 16);
  }
  dsum += __shfl_xor(dsum, 16, 64);
  dsum += __shfl_xor(dsum, 32, 64);
  const long long row = ((long long)b * NH + h) * S + q;
  if (g == 0) Dbuf[row] = dsum;
  const float L = lse[row];
  const uint64_t ebase = (uint64_t)row * S;
  f32x4 acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int j = 0; j < nb; ++j) {
    const int cur = j & 1;
    const bool more = j + 1 < nb;   // uniform
    if (more) {
      const uint16_t* nx = base + (long long)(j + 1) * KB * RS;
      rk = blk_load(nx + NH * D, rs);
      rv = blk_load(nx + 2 * NH * D, rs);
      if (mrow && threadIdx.x < KB) mreg = mrow[(j + 1) * KB + threadIdx.x];
    }
    const uint16_t* Kc = Ks + cur * IMG;
    const uint16_t* Vc = Vs + cur * IMG;
    const float* Mc = Ms + cur * KB;
    const uint64_t eb = ebase + (uint64_t)j * KB;
#pragma unroll 2
    for (int kb = 0; kb < KB / 32; ++kb) {
      float f[8];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * kb + tt;
        f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          sv = mfma16x16x32(ld_bf16x8(Kc + (16 * t + c) * KP + 32 * s + 8 * g), bqf[s], sv);
          dp = mfma16x16x32(ld_bf16x8(Vc + (16 * t + c) * KP + 32 * s + 8 * g), bdo[s], dp);
        }
        const float4 mk = *reinterpret_cast<const float4*>(Mc + 16 * t + 4 * g);
        const float m4[4] = {mk.x, mk.y, mk.z, mk.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = 16 * t + 4 * g + i;
          const float P = __expf(sv[i] * scale + m4[i] - L);
          const float dpd = dp[i] * keepf(seed, eb + key, thresh, inv_keep);
          f[4 * tt + i] = P * (dpd - dsum);
        }
      }
      const bf16x8 dsb = pack8(f);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = mfma16x16x32(ld_tr_pair(Kc, 32 * kb, 16 * u, l), dsb, acc[u]);
    }
    if (more) {
      blk_store(rk, bias ? Bl : nullptr, Ks + (cur ^ 1) * IMG);
      blk_store(rv, bias ? Bl + D : nullptr, Vs + (cur ^ 1) * IMG);
      if (threadIdx.x < KB) Ms[(cur ^ 1) * KB + threadIdx.x] = mreg;
    }
    __syncthreads();
  }
  uint16_t* dq = dqkv + ((long long)b * S + q) * RS + h * D;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    *reinterpret_cast<uint2*>(dq + 16 * u + 4 * g) =
        uint2{pack2bf(acc[u][0] * scale, acc[u][1] * scale), pack2bf(acc[u][2] * scale, acc[u][3] * scale)};
  if (bpart != nullptr) {
    // q-bias gradient partials: this wave's 16 queries summed per dimension
    // (lanes c = 0..15 of a group hold the 16 queries) -> bpart[b * S/16 + wave row][h * 64 + d]
    float cs[16];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = acc[u][i] * scale;
        v += __shfl_xor(v, 1, 64);
        v += __shfl_xor(v, 2, 64);
        v += __shfl_xor(v, 4, 64);
        v += __shfl_xor(v, 8, 64);
        cs[4 * u + i] = v;
      }
    if (c == 0) {
      float* pr = bpart + ((long long)b * (S / 16) + blockIdx.x * 8 + w) * RS + h * D;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        *reinterpret_cast<float4*>(pr + 16 * u + 4 * g) = float4{cs[4 * u], cs[4 * u + 1], cs[4 * u + 2], cs[4 * u + 3]};
    }
  }
}

__global__ __launch_bounds__(512, 4) void attn_long_bwd_dkv(const uint16_t* __restrict__ qkv, const float* __restrict__ bias,
                                                         const float* __restrict__ mask, const uint16_t* __restrict__ dctx,
                                                         const float* __restrict__ lse, const float* __restrict__ Dbuf,
                                                         uint16_t* __restrict__ dqkv, int S, int NH, float scale,
                                                         uint32_t thresh, float inv_keep, uint64_t seed,
                                                         float* __restrict__ bpart) {
  extern __shared__ __attribute__((aligned(16))) uint16_t lds[];
  uint16_t* Qs = lds;                                        // [2][KB][KP] (also read transposed: ld_tr_pair)
  uint16_t* dOs = lds + 2 * IMG;                             // [2][KB][KP] (likewise)
  float* Ls = reinterpret_cast<float*>(lds + 4 * IMG);       // [2][KB] lse of the block's query rows
  float* Dl = Ls + 2 * KB;                                   // [2][KB] rowsum(dO * O)
  float* Bl = Dl + 2 * KB;                                   // [64] this head's q bias
  const int b = blockIdx.z, h = blockIdx.y;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, c = l & 15;
  const long long RS = 3LL * NH * D, HS = (long long)NH * D;
  const uint16_t* base = qkv + (long long)b * S * RS + h * D;
  const uint16_t* dbase = dctx + (long long)b * S * HS + h * D;
  const float* bqp = bias ? bias + h * D : nullptr;
  const long long rbase = ((long long)b * NH + h) * S;
  const int nb = S / KB;
  const int rs = 3 * NH * D, hs = NH * D;   // a block's rows span 64 * rs elements: 32-bit offsets
  uint4 rq = blk_load(base, rs), rd = blk_load(dbase, hs);
  const int k0 = blockIdx.x * 128 + w * 16;
  const int key = k0 + c;
  uint4 kraw[2], vraw[2];   // this wave's key / value fragments, in flight with the first stage
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    kraw[s] = ld16(base + (long long)key * RS + NH * D + 32 * s + 8 * g);
    vraw[s] = ld16(base + (long long)key * RS + 2 * NH * D + 32 * s + 8 * g);
  }
  float lsv = 0.f, dlv = 0.f;
  if (threadIdx.x < KB) {
    lsv = lse[rbase + threadIdx.x];
    dlv = Dbuf[rbase + threadIdx.x];
  }
  blk_store(rq, bqp, Qs);
  blk_store(rd, nullptr, dOs);
  if (threadIdx.x < KB) {
    Ls[threadIdx.x] = lsv;
    Dl[threadIdx.x] = dlv;
  }
  if (bias && threadIdx.x < D) Bl[threadIdx.x] = bqp[threadIdx.x];
  __syncthreads();

  const float* bk = bias ? bias + (NH + h) * D : nullptr;
  const float* bv = bias ? bias + (2 * NH + h) * D : nullptr;
  bf16x8 kf[2], vf[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    kf[s] = as_frag(add_bias8(kraw[s], bk ? bk + 32 * s + 8 * g : nullptr));
    vf[s] = as_frag(add_bias8(vraw[s], bv ? bv + 32 * s + 8 * g : nullptr));
  }
  const float mk = mask ? mask[(long long)b * S + key] : 0.f;
  f32x4 dv[4], dk[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    dv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    dk[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  for (int j = 0; j < nb; ++j) {
    const int cur = j & 1;
    const bool more = j + 1 < nb;   // uniform
    if (more) {
      rq = blk_load(base + (long long)(j + 1) * KB * RS, rs);
      rd = blk_load(dbase + (long long)(j + 1) * KB * HS, hs);
      if (threadIdx.x < KB) {
        lsv = lse[rbase + (j + 1) * KB + threadIdx.x];
        dlv = Dbuf[rbase + (j + 1) * KB + threadIdx.x];
      }
    }
    const uint16_t* Qc = Qs + cur * IMG;
    const uint16_t* dOc = dOs + cur * IMG;
    const float* Lc = Ls + cur * KB;
    const float* Dc = Dl + cur * KB;
    for (int qb = 0; qb < KB / 32; ++qb) {
      float pd[8], ds[8];
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int t = 2 * qb + tt;
        f32x4 sv = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          sv = mfma16x16x32(ld_bf16x8(Qc + (16 * t + c) * KP + 32 * s + 8 * g), kf[s], sv);
          dp = mfma16x16x32(ld_bf16x8(dOc + (16 * t + c) * KP + 32 * s + 8 * g), vf[s], dp);
        }
        const float4 L4 = *reinterpret_cast<const float4*>(Lc + 16 * t + 4 * g);
        const float4 D4 = *reinterpret_cast<const float4*>(Dc + 16 * t + 4 * g);
        const float Lq[4] = {L4.x, L4.y, L4.z, L4.w}, Ds[4] = {D4.x, D4.y, D4.z, D4.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int q = j * KB + 16 * t + 4 * g + i;
          const float P = __expf(sv[i] * scale + mk - Lq[i]);
          const float kp = keepf(seed, (uint64_t)(rbase + q) * S + key, thresh, inv_keep);
          pd[4 * tt + i] = P * kp;
          ds[4 * tt + i] = P * (dp[i] * kp - Ds[i]);
        }
      }
      const bf16x8 ap = pack8(pd), as = pack8(ds);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        dv[u] = mfma16x16x32(ap, ld_tr_pair(dOc, 32 * qb, 16 * u, l), dv[u]);
        dk[u] = mfma16x16x32(as, ld_tr_pair(Qc, 32 * qb, 16 * u, l), dk[u]);
      }
    }
    if (more) {
      blk_store(rq, bias ? Bl : nullptr, Qs + (cur ^ 1) * IMG);
      blk_store(rd, nullptr, dOs + (cur ^ 1) * IMG);
      if (threadIdx.x < KB) {
        Ls[(cur ^ 1) * KB + threadIdx.x] = lsv;
        Dl[(cur ^ 1) * KB + threadIdx.x] = dlv;
      }
    }
    __syncthreads();
  }
  // lane holds dV/dK[key k0 + 4g + i][d 16u + c]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint16_t* rowp = dqkv + ((long long)b * S + k0 + 4 * g + i) * RS + h * D + c;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      rowp[NH * D + 16 * u] = f2bf(dk[u][i] * scale);
      rowp[2 * NH * D + 16 * u] = f2bf(dv[u][i]);
    }
  }
  if (bpart != nullptr) {
    // k / v-bias gradient partials: this wave's 16 keys (4 per lane x the 4 lane
    // groups g) summed per dimension d = 16u + c
    float* pr = bpart + ((long long)b * (S / 16) + k0 / 16) * RS + h * D + c;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float sk = (dk[u][0] + dk[u][1]) + (dk[u][2] + dk[u][3]);
      float sv = (dv[u][0] + dv[u][1]) + (dv[u][2] + dv[u][3]);
      sk += __shfl_xor(sk, 16, 64);
      sk += __shfl_xor(sk, 32, 64);
      sv += __shfl_xor(sv, 16, 64);
      sv += __shfl_xor(sv, 32, 64);
      if (g == 0) {
        pr[NH * D + 16 * u] = sk * scale;
        pr[2 * NH * D + 16 * u] = sv;
      }
    }
  }
}

}  // namespace attn
}  // namespace dtfk

using namespace dtfk::attn;

static bool attn_long_shape(int B, int S, int NH) {
  return B > 0 && NH > 0 && S % KB == 0 && S >= 384 && S <= 2048 && B <= 65535 && NH <= 65535;
}

extern "C" {

hipError_t dtfk_attn_long_fwd(const void* qkv, const float* bias, const float* mask, void* ctx, float* lse, int B,
                              int S, int NH, float scale, float p, unsigned long long seed, hipStream_t st) {
  if (!attn_long_shape(B, S, NH)) return hipErrorInvalidValue;
  const dim3 grid(S / 128, NH, B);
  const float ik = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const size_t lds = (size_t)(4 * IMG) * 2 + (2 * KB + 2 * D) * sizeof(float);   // 37.9 KB: below the 64 KB opt-in
  hipLaunchKernelGGL(attn_long_fwd, grid, dim3(512), lds, st, (const uint16_t*)qkv, bias, mask, (uint16_t*)ctx, lse, S,
                     NH, scale, attn_thresh(p), ik, (uint64_t)seed);
  return hipGetLastError();
}

// dqkv [B, S, 3, NH, 64] is fully written; Dbuf [B, NH, S] fp32 is written by attn_long_bwd_dq and
// read by attn_long_bwd_dkv; bpart (optional): [B * S / 16, 3 * NH * 64] fp32, as dtfk_attn_bwd's
hipError_t dtfk_attn_long_bwd(const void* qkv, const float* bias, const float* mask, const void* ctx,
                              const void* dctx, const float* lse, float* Dbuf, void* dqkv, int B, int S, int NH,
                              float scale, float p, unsigned long long seed, float* bpart, hipStream_t st) {
  if (!attn_long_shape(B, S, NH)) return hipErrorInvalidValue;
  const dim3 grid(S / 128, NH, B);
  const float ik = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const uint32_t th = attn_thresh(p);
  const size_t lds_q = (size_t)(4 * IMG) * 2 + (2 * KB + 2 * D) * sizeof(float);
  const size_t lds_kv = (size_t)(4 * IMG) * 2 + (4 * KB + D) * sizeof(float);
  hipLaunchKernelGGL(attn_long_bwd_dq, grid, dim3(512), lds_q, st, (const uint16_t*)qkv, bias, mask,
                     (const uint16_t*)ctx, (const uint16_t*)dctx, lse, Dbuf, (uint16_t*)dqkv, S, NH, scale, th, ik,
                     (uint64_t)seed, bpart);
  hipLaunchKernelGGL(attn_long_bwd_dkv, grid, dim3(512), lds_kv, st, (const uint16_t*)qkv, bias, mask,
                     (const uint16_t*)dctx, lse, Dbuf, (uint16_t*)dqkv, S, NH, scale, th, ik, (uint64_t)seed, bpart);
  return hipGetLastError();
}

}  // extern "C"
