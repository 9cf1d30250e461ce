// The host entry points of the implicit-GEMM convolution kernels (conv_igemm.hip), declared
// once: csrc/bind_bn.cpp calls through these declarations and conv_igemm.hip includes them, so
// a definition that disagrees with its declaration does not compile.  Host-only: no device
// code here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

extern "C" {

// ---- 3x3 (pad 1) or 1x1 (pad 0) filters, ks = 3 or 1
int dtfk_conv_supported(int N, int H, int W, int C, int K, int stride, int ks);
long long dtfk_conv_tiles(int N, int H, int W, int stride, int ks);
hipError_t dtfk_conv_fwd(const void* x, const void* w, void* y, float* part, int N, int H, int W, int C, int K,
                         int stride, int bn, int ks, int accum, const void* bnx, const float* bnst,
                         const void* bnres, hipStream_t stream);
hipError_t dtfk_conv_wflip(const void* w, void* wt, int K, int C, int ks, hipStream_t stream);
// several filters flipped in one launch: tab [n, 5] rows {w, wt, K, C, ks}, tiles [m, 4]
hipError_t dtfk_conv_wflip_multi(const long long* tab, const int* tiles, int ntiles, hipStream_t stream);
long long dtfk_conv_wgrad_plan(int N, int H, int W, int C, int K, int stride, int ks, int* splits_out, int* sps_out);
// the launch plan dtfk_conv_wgrad uses: out = {splits, steps per split, bm, bnw, xcd, G}; returns the workspace floats
long long dtfk_conv_wgrad_launch_plan(int N, int H, int W, int C, int K, int stride, int ks, int out[6]);
hipError_t dtfk_conv_wgrad(const void* dy, const void* x, float* dw, float* ws, int N, int H, int W, int C, int K,
                           int stride, int ks, int kcrs, hipStream_t stream);

// ---- the 3x3 forms of the same
int dtfk_conv3x3_supported(int N, int H, int W, int C, int K, int stride);
long long dtfk_conv3x3_tiles(int N, int H, int W, int stride);
hipError_t dtfk_conv3x3_fwd(const void* x, const void* w, void* y, float* part, int N, int H, int W, int C, int K,
                            int stride, int bn, hipStream_t stream);
hipError_t dtfk_conv3x3_wflip(const void* w, void* wt, int K, int C, hipStream_t stream);
long long dtfk_conv3x3_wgrad_plan(int N, int H, int W, int C, int K, int stride, int* splits_out, int* sps_out);
hipError_t dtfk_conv3x3_wgrad(const void* dy, const void* x, float* dw, float* ws, int N, int H, int W, int C, int K,
                              int stride, int kcrs, hipStream_t stream);

// ---- input gradient of the stride-2 3x3 convolution
long long dtfk_conv3x3_dx2_tiles(int N, int H, int W);
int dtfk_conv3x3_dx2_supported(int N, int H, int W, int C, int K);
hipError_t dtfk_conv3x3_dx2(const void* dy, const void* wt, void* dx, float* part, int N, int H, int W, int C, int K,
                            int bn, int accum, const void* bnx, const float* bnst, hipStream_t stream);

}  // extern "C"
