// The host entry points of the NHWC bf16 pooling kernels (pool.hip), declared once:
// csrc/bind_bn.cpp calls through these declarations and pool.hip includes them, so a definition
// that disagrees with its declaration does not compile.  Host-only: no device code here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

// idx: uint8 window position of each output's max
hipError_t dtfk_maxpool_fwd(const void* x, void* y, void* idx, int N, int H, int W, int C, int Ho, int Wo, int k,
                            int s, int p, hipStream_t st);
hipError_t dtfk_maxpool_bwd(const void* dy, const void* idx, void* dx, int N, int H, int W, int C, int Ho, int Wo,
                            int k, int s, int p, hipStream_t st);
// full[:, :, s*i, s*j] += comp
hipError_t dtfk_strided_add(void* full, const void* comp, int N, int H, int W, int C, int Ho, int Wo, int s,
                            hipStream_t st);

}  // extern "C"
