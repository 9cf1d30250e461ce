// The host entry points of the sparse logistic-regression kernels (sparse_lr.hip), declared
// once: csrc/bind_sparse.cpp calls through these declarations and sparse_lr.hip includes them,
// so a definition that disagrees with its declaration does not compile.  Host-only: no device
// code here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

hipError_t dtfk_slr_step(float* W, long long F, const void* ids, int ids32, const long long* offsets,
                         const float* vals, const float* labels, float* bias, int B, const float* lr_ptr, float lr_val,
                         float* dz, float* lrow, float* loss_out, int* bad, void* gvar, int gkind, hipStream_t stream);
hipError_t dtfk_slr_stage(const void* src, void* dst, long long bytes, hipStream_t stream);
void dtfk_slr_set_rows_per_wg(int rpw);
hipError_t dtfk_slr_step_direct(float* W, long long F, const void* hids, int ids32, const long long* hoffsets,
                                const float* hvals, const float* hlabels, void* ids_d, long long* off_d, float* vals_d,
                                float* bias, int B, float lr_val, float* dz, float* lrow, float* loss_out, int* bad,
                                void* gvar, int gkind, hipStream_t stream);
hipError_t dtfk_slr_ftrl_step(float* W, long long F, const void* ids, int ids32, const long long* offsets,
                              const float* vals, const float* labels, float* bias, int B, const float* lr_ptr,
                              float lr_val, float* dz, float* lrow, float* loss_out, int* bad, void* gvar, int gkind,
                              float* acc, float* lin, float* gsum, float* bslots, float lr_power, float l1, float l2,
                              float shrink, hipStream_t stream);
hipError_t dtfk_slr_ftrl_step_direct(float* W, long long F, const void* hids, int ids32, const long long* hoffsets,
                                     const float* hvals, const float* hlabels, void* ids_d, long long* off_d,
                                     float* vals_d, float* bias, int B, float lr_val, float* dz, float* lrow,
                                     float* loss_out, int* bad, void* gvar, int gkind, float* acc, float* lin,
                                     float* gsum, float* bslots, float lr_power, float l1, float l2, float shrink,
                                     hipStream_t stream);
hipError_t dtfk_slr_eval(const float* W, long long F, const void* ids, int ids32, const long long* offsets,
                         const float* vals, const float* labels, float* labels_d, int direct, const float* bias, int B,
                         float* lrow, float* prow, int* brow, int* bad, float* z_out, float* p_out, int T, int reset,
                         long long* rec, hipStream_t stream);

}  // extern "C"
