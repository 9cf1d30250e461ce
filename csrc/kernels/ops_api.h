// The host entry points of the generic op / optimizer kernel files (ops.hip, random.hip,
// sparse_optim.hip, sparse_route.hip, hogwild.hip), declared once: csrc/bind_ops.cpp calls
// through these declarations and every defining file includes them, so a definition that
// disagrees with its declaration does not compile.  Host-only: no device code here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "optim_rules.h"

extern "C" {

// ---- ops.hip
hipError_t dtfk_bucket_pack(const float* g, uint16_t* c, int64_t n, float scale, int fp16, hipStream_t s);
hipError_t dtfk_bucket_unpack(const uint16_t* c, float* g, int64_t n, float scale, int fp16, hipStream_t s);
hipError_t dtfk_act_backward(const float* dy, const float* y, const float* z, float* dz, int64_t n, int act,
                             hipStream_t s);
hipError_t dtfk_col_sum(const float* X, float* out, int M, int N, int accum, hipStream_t s);
hipError_t dtfk_logit3_xent(const float* a, const float* b, const float* bias, const float* t, float* loss,
                            float* dz, int n, hipStream_t s);
hipError_t dtfk_logit3_xent_bwd(const float* dz, const float* g, float* d, float* gbias, int accum, int n,
                                hipStream_t s);
hipError_t dtfk_multi_copy(const void* const* src, void* const* dst, const long long* bytes, int n, hipStream_t s);
hipError_t dtfk_bag_index(const int64_t* offsets, int B, int* bag_of, int64_t N, hipStream_t s);
hipError_t dtfk_softmax_xent(const float* logits, const int64_t* labels, const float* ydense, float* loss_rows,
                             float* grad, int64_t* correct, int B, int C, float grad_scale, int naive,
                             hipStream_t s);
hipError_t dtfk_sigmoid_xent(const float* x, const float* t, float* loss, float* grad, int64_t n,
                             float grad_scale, hipStream_t s);
hipError_t dtfk_xent_fwd_bf16(const void* logits, const float* bias, const int64_t* labels, float* lse_rows,
                              float* loss_rows, int B, int C, hipStream_t s);
hipError_t dtfk_xent_bwd_bf16(const void* logits, const float* bias, const int64_t* labels, const float* lse_rows,
                              const float* dloss, void* grad, int B, int C, float scale, hipStream_t s);
hipError_t dtfk_embedding_bag_fwd(const float* W, int64_t V, int D, const int64_t* ids, const int64_t* offsets,
                                  const float* psw, int B, int mode, float* out, int64_t* bad, const int64_t* remap,
                                  hipStream_t s);
hipError_t dtfk_embedding_bag_bwd(float* target, int64_t V, int D, const int64_t* ids, const int64_t* offsets,
                                  const float* psw, const float* dout, int B, int mode, float lr,
                                  hipStream_t s);
hipError_t dtfk_embedding_bag_bwd_sorted(float* target, int64_t V, int D, const int* rows, const int64_t* occ,
                                         const int* bag_of, const float* psw, const float* dout, int64_t N,
                                         hipStream_t s);
hipError_t dtfk_argmax_correct(const float* x, const int64_t* labels, int B, int C, int64_t* count,
                               hipStream_t s);
hipError_t dtfk_auc_hist(const float* pred, const float* label, int64_t n, int nbins, unsigned long long* pos,
                         unsigned long long* neg, hipStream_t s);
hipError_t dtfk_multi_tensor_apply(const void* tab, const void* chunks, int nchunks, int kind, int gbf,
                                   const float* lr_ptr, float gscale, const dtfk::OptimHyper& h,
                                   const long long* step, const int* skip, hipStream_t s);
hipError_t dtfk_multi_tensor_sumsq(const void* tab, const void* chunks, int nchunks, int gbf, float* out,
                                   hipStream_t s);
int dtfk_mt_chunk();
int dtfk_tensor_rec_bytes();

// ---- random.hip
hipError_t dtfk_philox_normal(float* out, long long rows, int dim, long long row_mul, long long row_add,
                              unsigned long long seed, float mean, float stddev, hipStream_t stream);

// ---- sparse_optim.hip
hipError_t dtfk_sparse_rows_apply(float* table, float* slot_a, float* slot_b, const long long* rows, const float* g,
                                  long long n, int D, int kind, const dtfk::OptimHyper& h, const int* skip,
                                  hipStream_t s);

// ---- sparse_route.hip
int dtfk_route_max_world();
hipError_t dtfk_route_flags(const void* sids, int ids32, int N, int W, int* flag, int* onehot, hipStream_t stream);
hipError_t dtfk_route_scatter(const void* sids, int ids32, const int64_t* perm, const int* incl, const int* owncum,
                              int N, int W, int cap, int* inv_sorted, int64_t* inverse, int64_t* uniq, int* dest,
                              int64_t* send, int* count, hipStream_t stream);

// ---- hogwild.hip
hipError_t dtfk_hogwild_pull(const float* shared, float* local, long long n, hipStream_t s);
hipError_t dtfk_hogwild_sgd(float* shared, const float* g, float* local, float lr, long long n, int locking,
                            unsigned long long* counter, long long* gstep_out, hipStream_t s);
hipError_t dtfk_hogwild_counter(unsigned long long* counter, long long* out, long long set, int do_set, hipStream_t s);
hipError_t dtfk_hogwild_gather_rows(const long long* ids, int n, int D, const float* const* shards, int W, float* out,
                                    hipStream_t s);
hipError_t dtfk_hogwild_scatter_sgd(const long long* ids, const float* g, int n, int D, float* const* shards, int W,
                                    float lr, int locking, hipStream_t s);

}  // extern "C"
