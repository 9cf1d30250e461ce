// The host entry points of the fused NHWC BatchNorm kernels (bn.hip), declared once:
// csrc/bind_bn.cpp calls through these declarations and bn.hip includes them, so a definition
// that disagrees with its declaration does not compile.  Host-only: no device code here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

int dtfk_bn_partial_rows(int M, int C);
hipError_t dtfk_bn_fwd(const void* x, const void* res, const float* gamma, const float* beta, void* y, float* part,
                       float* mean, float* invstd, float* scale, float* shift, float* run_mean, float* run_var,
                       int M, int C, float momentum, float eps, int relu, hipStream_t st);
// bn_fwd with the statistics partials [2, P, C] supplied by the producer of x
hipError_t dtfk_bn_fwd_parts(const void* x, const void* res, const float* gamma, const float* beta, void* y,
                             const float* part, int P, float* mean, float* invstd, float* scale, float* shift,
                             float* run_mean, float* run_var, int M, int C, float momentum, float eps, int relu,
                             hipStream_t st);
hipError_t dtfk_bn_apply(const void* x, const void* res, const float* scale, const float* shift, void* y, int M, int C,
                         int relu, hipStream_t st);
hipError_t dtfk_bn_bwd(const void* dy, const void* x, const void* res, const float* gamma, const float* mean,
                       const float* invstd, const float* scale, const float* shift, float* part, float* coef,
                       void* dx, void* dres, float* dgamma, float* dbeta, int M, int C, int relu, int accum,
                       int write_g, hipStream_t st);
// the backward from an already ReLU-masked g and its [2, P, C] partials: finalize + apply only
hipError_t dtfk_bn_bwd_parts(const void* g, const void* x, const float* gamma, const float* mean, const float* invstd,
                             const float* part, int P, float* coef, void* dx, float* dgamma, float* dbeta, int M, int C,
                             int accum, hipStream_t st);
// the statistics partials of x alone ([2, P, C], P = dtfk_bn_partial_rows(M, C))
hipError_t dtfk_bn_stat_partials(const void* x, float* part, int M, int C, hipStream_t st);

}  // extern "C"
