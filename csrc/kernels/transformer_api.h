// The host entry points of the fused transformer kernels (transformer.hip, attention.hip),
// declared once: csrc/bind_transformer.cpp and csrc/bind_ops.cpp call through these
// declarations and both defining files include them, so a definition that disagrees with its
// declaration does not compile.  Host-only: no device code here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

// ---- transformer.hip
// y = LN(dropout(x + bias) + res)
hipError_t dtfk_bdrln_fwd(const void* x, const float* bias, const void* res, const float* gamma, const float* beta,
                          void* y, void* s_out, float* mean, float* rstd, int N, int H, float eps, float p,
                          unsigned long long seed, hipStream_t st);
// y = dropout(LN(word[ids] + typ[tt] + pos[t % S])), s = bf16 of the sum
hipError_t dtfk_emb_ln_fwd(const float* word, const int64_t* ids, const float* typ, const int64_t* tt,
                           const float* pos, int S, const float* gamma, const float* beta, void* y, void* s_out,
                           float* mean, float* rstd, int N, int H, float eps, float p, unsigned long long seed,
                           hipStream_t st);
hipError_t dtfk_emb_bwd_aux(const void* ds, const int64_t* tt, int B, int S, int H, float* pos_grad, float* part,
                            int accumulate, hipStream_t st);
hipError_t dtfk_ln_fwd_f32in(const float* x, const float* gamma, const float* beta, void* y, void* s_out,
                             float* mean, float* rstd, int N, int H, float eps, float p, unsigned long long seed,
                             hipStream_t st);
hipError_t dtfk_ln_bwd(const void* dy, const void* s, const float* mean, const float* rstd, const float* gamma,
                       void* ds, void* dxb, float* part_g, float* part_b, float* part_bias, int grid, int N, int H,
                       float p, unsigned long long seed, hipStream_t st);
hipError_t dtfk_colsum_partials(const float* part, float* out, int P, int H, hipStream_t st);
// outs[i] (+)= column sums of parts[i] ([P, H] each), up to nbuf buffers in one launch
hipError_t dtfk_colsum_partials_multi(const float* const* parts, float* const* outs, int nbuf, int P, int H,
                                      int accumulate, hipStream_t st);
// out (+)= column sums of a bf16 [N, H] matrix (part: P * H floats)
hipError_t dtfk_colsum_bf16(const void* x, float* part, float* out, int N, int H, int P, int accumulate,
                            hipStream_t st);
// out (+)= sum over the leading dim of slabs [S, n]
hipError_t dtfk_slab_sum(const float* slabs, float* out, int S, long long n, int accumulate, hipStream_t st);
hipError_t dtfk_bias_gelu_fwd(const void* x, const float* bias, void* y, long long n, int H, hipStream_t st);
hipError_t dtfk_bias_gelu_bwd(const void* dy, const void* x, const float* bias, void* dx, float* part, int N, int H,
                              int row_slices, hipStream_t st);
hipError_t dtfk_softmax_fwd(const void* S, const float* mask, void* P, void* Pd, int rows, int Sk, int rows_per_batch,
                            float scale, float p, unsigned long long seed, hipStream_t st);
hipError_t dtfk_softmax_bwd(const void* dPd, const void* P, void* dS, int rows, int Sk, float scale, float p,
                            unsigned long long seed, hipStream_t st);
hipError_t dtfk_dropout_bf16(const void* x, void* y, long long n, float p, unsigned long long seed, hipStream_t st);

// ---- attention.hip
int dtfk_attn_supported(int S, int d);
hipError_t dtfk_attn_fwd(const void* qkv, const float* bias, const float* mask, void* ctx, float* lse, int B, int S,
                         int NH, float scale, float p, unsigned long long seed, hipStream_t st);
hipError_t dtfk_attn_bwd(const void* qkv, const float* bias, const float* mask, const void* ctx, const void* dctx,
                         const float* lse, float* Dbuf, void* dqkv, int B, int S, int NH, float scale, float p,
                         unsigned long long seed, float* bpart, hipStream_t st);

// ---- attention_long.hip: S = 384 ... 2048, S % 128 == 0, same arguments; reached through the two above
hipError_t dtfk_attn_long_fwd(const void* qkv, const float* bias, const float* mask, void* ctx, float* lse, int B,
                              int S, int NH, float scale, float p, unsigned long long seed, hipStream_t st);
hipError_t dtfk_attn_long_bwd(const void* qkv, const float* bias, const float* mask, const void* ctx,
                              const void* dctx, const float* lse, float* Dbuf, void* dqkv, int B, int S, int NH,
                              float scale, float p, unsigned long long seed, float* bpart, hipStream_t st);

}  // extern "C"
