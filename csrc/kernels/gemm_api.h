// The host entry points of the GEMM kernel files (gemm.hip, gemm_big.hip), declared once:
// csrc/bind_ops.cpp calls through these declarations and both defining files include them, so
// a definition that disagrees with its declaration does not compile.  Host-only: no device
// code here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

// ---- gemm.hip
// C = act(alpha * op(A) op(B) + bias) (+ beta * C), fp32 / bf16 operands; Z: the pre-activation
hipError_t dtfk_gemm(const void* A, int a_bf16, int lda, int transA, const void* B, int b_bf16, int ldb,
                     int transB, void* C, int c_bf16, int ldc, float* Z, const float* bias, int M, int N,
                     int K, float alpha, float beta, int act, hipStream_t stream);

// ---- gemm_big.hip
hipError_t dtfk_gemm_big(const void* A, int lda, int transA, const void* B, int ldb, int transB, void* C,
                         int c_bf16, int ldc, const float* bias, int M, int N, int K, float alpha, float beta,
                         int act, int split_k, int variant, void* ws, hipStream_t stream);
long long dtfk_gemm_big_workspace(int M, int N, int K, int c_bf16, float beta, int act, int split_k, int variant);
int dtfk_gemm_big_supported(const void* A, int lda, int transA, const void* B, int ldb, int transB, int c_bf16, int M,
                            int N, int K, float beta, int act, int split_k);
hipError_t dtfk_gemm_bn_stats(const void* A, int lda, int transA, const void* B, int ldb, int transB, void* C, int ldc,
                              float* colpart, int M, int N, int K, hipStream_t stream);
int dtfk_gemm_bn_stat_rows(int M);
hipError_t dtfk_gemm_dgelu(const void* A, int lda, int transA, const void* B, int ldb, int transB, void* C, int ldc,
                           const void* aux, const float* bias, float* colpart, int M, int N, int K, hipStream_t stream);
hipError_t dtfk_gemm_gelu_aux(const void* A, int lda, int transA, const void* B, int ldb, int transB, void* C,
                              int ldc, void* aux, const float* bias, int M, int N, int K, hipStream_t stream);
hipError_t dtfk_gemm_big_cfg(int cfg, const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N,
                             int K, hipStream_t stream);

}  // extern "C"
