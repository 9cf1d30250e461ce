// Reached by: the one-GPU fused Wide&Deep training step (csrc/bind_wide_deep.cpp WideDeepTrainPlan: models/wide_deep.py WideDeep(fused_step=True) _train_step_fused); tests/test_wide_deep_train_gpu.py, scripts/bench_models.py --model wide_deep --fused-step
// The per-row half of a models/wide_deep.py training step on one GPU, where
// every table row is local: ids in, gradients with respect to the bag outputs
// out, in one launch.  No dedup, no routing, no remap, no autograd graph, no
// launch per layer.  What stays outside: the weight gradients (act^T dzl, one
// gemm per layer), the two scatter-SGD table updates and the dense optimizer.
//
//   forward   wd_eval_rows's (wide_deep_eval.hip): bags, hidden layers, head --
//             the same code (wide_deep_bags.h, wide_deep_rows.h), plus
//               act[0] = the scaled bag output, act[l] = relu(act[l-1] W_{l-1} + b_{l-1})
//             stored to global [B, dims[l]] for the weight gradients.
//   head      t = h w_last + b_last;  z = (wide + t) + bias;  lrow = xent(z, y);
//             dz = (sigmoid(z) - y) gscale        (also the wide table's bag gradient)
//   backward  da_nh = dz w_last^T;  for l = nh .. 1 (nh hidden layers):
//               dzl[l] = da_l * (act[l] > 0)      act_backward's ReLU rule
//               da_{l-1} = dzl[l] W_{l-1}^T;      demb = da_0
//
//   wd_train_rows  one workgroup (4 waves) per tile of TM = 16 or 32 batch rows.
//     All arithmetic is fp32: exact products on v_mfma_f32_16x16x4_f32, fp32
//     accumulation, as ops.linear_act on fp32 operands.
//     backward layer  out[TM][K] = G[TM][N] W^T with W [K][N] as it lies in
//       memory: the product's reduction dimension n is W's contiguous one.  A
//       work item is (16-row tile, 64 output columns k); the waves take items in
//       turn.  A = the gradient tile in LDS, read like the forward's (one 16-byte
//       read per 16-deep block: lane group g holds n = 16 nb + 4 g .. + 3).  B:
//       lane (r, g) loads 16 bytes along row c0 + 4 r + j of W at n = 16 nb +
//       4 g, j = 0 .. 3: the same four n as its A read, so MFMA step s multiplies
//       A's and B's component s.  Sixteen lanes read 64 contiguous bytes of each
//       of 16 weight rows per load.  No transposed copy of W exists.  Four
//       blocks of operands are in flight per wave, as in the forward: the
//       weights come from L2 here too.  N is a hidden width (a multiple of 16):
//       no ragged reduction block; the ragged last column chunk (K % 64 != 0, and
//       K = D a multiple of 4 in the first layer) reads clamped weight rows and
//       is not stored.  The C layout is the forward's, so the epilogue reads the
//       mask and writes dzl[l] in place, a lane touching only its own elements.
//     gradient tiles reuse the two activation buffers: dzl[nh] overwrites
//       act[nh] in its buffer, and every backward layer writes into the buffer
//       it does not read, which is the one that held act[l].
//     ReLU masks  are read from LDS, from the very words dzl[l] then overwrites,
//       wherever act[l] is still there: always for l = nh and l = nh - 1.  With
//       three hidden layers act[1]'s buffer was reused for act[3], and layer 1's
//       mask is read from the tile's own act[1] rows in global memory (written
//       by this workgroup before a workgroup barrier; rows >= B read row B - 1's).
//   wd_train_sums  one workgroup: mean(lrow) and sum(dz) in float64, in one
//     fixed order -> the returned loss and the gradients of b_last and the
//     shared bias.
//
// Ragged edges as in wd_eval_rows: rows >= B are empty bags with dz = 0, and
// nothing of them is stored; nothing is read or written past the last row, id
// or column.  No inter-workgroup waits, no float atomics: two runs give the
// same bits.
//
// LDS budget: wd_eval_rows's, byte for byte (the backward adds no buffer):
//     bytes = 4 TM ((K0 + 4) + (K1 + 4)) + 8 TM,
//     K0 = max(ceil16(D), hidden[1]),  K1 = max(hidden[0], hidden[2])
//   D <= 128, hidden 512-512-512:  66,176 B at TM = 16 (2 workgroups per CU), 132,352 B at TM = 32 (1);
//   D = 64, hidden 512-256:  49,792 B at TM = 16 (3 workgroups per CU), 99,584 B at TM = 32 (1);
//   D = 16, hidden 32-16:  3,712 B at TM = 16.
// Tile rule (dtfk_wd_train_tile): the evaluation's rule as it stands.  It is not
// yet measured for training, where a tile does about three times the work.
#include "common.h"
#include "wide_deep_train.h"
#include "wide_deep_rows.h"

namespace dtfk {
namespace wdt {

using namespace wde;

// TM: rows per workgroup.
template <int TM>
__global__ __launch_bounds__(THREADS) void wd_train_rows(Args ta) {
  extern __shared__ float4 wdt_smem[];
  __shared__ float wide_s[TM];
  __shared__ int bad_s[TM];
  const wde::Args& a = ta.f;
  float* buf0 = reinterpret_cast<float*>(wdt_smem);
  float* buf1 = buf0 + TM * a.ld0;
  const int lane = threadIdx.x & 63, w = uni((int)(threadIdx.x >> 6));
  const long long row0 = (long long)blockIdx.x * TM;

  // ---- bags: the scaled embedding tile in buf0, wide sums and bad counts per row
#include "wide_deep_bags.h"
  __syncthreads();
  const int rows = (int)min((long long)TM, B - row0);                  // the tile's rows inside the batch (>= 1)

  // act[0]: the tile's bag outputs, 16 bytes per thread
  {
    const int q4 = D >> 2;
    float* g0 = ta.act[0] + (size_t)row0 * D;
    for (int i = threadIdx.x; i < rows * q4; i += THREADS) {
      const int rr = i / q4, c = 4 * (i - rr * q4);
      *reinterpret_cast<float4*>(g0 + (size_t)rr * D + c) = *reinterpret_cast<const float4*>(buf0 + rr * a.ld0 + c);
    }
  }

  // ---- tower forward: hidden layers, ping-pong between the two buffers, act[l + 1] stored
  const int nh = a.nl - 1;
  float* in = buf0;
  float* out = buf1;
  int ldi = a.ld0, ldo = a.ld1;
#pragma unroll
  for (int l = 0; l < MAXL - 1; ++l) {
    if (l < nh) {                                                      // (workgroup-uniform)
      const int K = a.dims[l], N = a.dims[l + 1];
      float* gl = ta.act[l + 1] + (size_t)row0 * N;
      if (K & 15) layer<TM, true, true>(in, ldi, out, ldo, a.W[l], a.b[l], K, N, w, lane, gl, rows);
      else layer<TM, false, true>(in, ldi, out, ldo, a.W[l], a.b[l], K, N, w, lane, gl, rows);
      __syncthreads();
      float* tp = in; in = out; out = tp;
      const int tl = ldi; ldi = ldo; ldo = tl;
    }
  }

  // ---- the width-1 last layer, the head and dzl[nh] = dz w_last * (act[nh] > 0), in place: a wave per row
  const int KL = a.dims[nh];
  const float* wl = a.W[nh];
  const float bl = a.b[nh][0], bias = a.bias[0];
  float* gl = ta.dzl[nh] + (size_t)row0 * KL;
  for (int rr = w; rr < TM; rr += NW) {
    float acc = 0.f;
    for (int k = lane; k < KL; k += 64) acc = fmaf(in[rr * ldi + k], wl[k], acc);
    acc = wave_sum(acc);
    const long long row = row0 + rr;
    float dz = 0.f;                                                    // rows >= B: no gradient
    if (rr < rows) {                                                   // (wave-uniform)
      const float t = acc + bl;
      const float z = (wide_s[rr] + t) + bias;
      const float y = a.labels[row];
      const float p = 1.f / (1.f + __expf(-z));
      dz = (p - y) * ta.gscale;
      if (lane == 0) {
        a.lrow[row] = xent(z, y);
        a.brow[row] = bad_s[rr];
        a.z_out[row] = z;
        ta.dz[row] = dz;
      }
    }
    for (int k = lane; k < KL; k += 64) {
      const float h = in[rr * ldi + k];
      const float gk = h > 0.f ? dz * wl[k] : 0.f;
      in[rr * ldi + k] = gk;
      if (rr < rows) gl[(size_t)rr * KL + k] = gk;
    }
  }
  __syncthreads();

  // ---- backward through the hidden layers: da_l = dzl[l + 1] W_l^T, into the buffer that held act[l]
#pragma unroll
  for (int l = MAXL - 2; l >= 0; --l) {
    if (l < nh) {                                                      // (workgroup-uniform)
      const int K = a.dims[l], N = a.dims[l + 1];
      if (l == 0) {
        layer_bwd<TM, true, false>(in, ldi, out, ldo, a.W[0], K, N, w, lane, nullptr, ta.demb + (size_t)row0 * K, rows);
      } else {
        float* gd = ta.dzl[l] + (size_t)row0 * K;
        // act[l] is still in `out` unless act[l + 2] was written over it
        if (l + 2 <= nh)
          layer_bwd<TM, false, true>(in, ldi, out, ldo, a.W[l], K, N, w, lane, ta.act[l] + (size_t)row0 * K, gd, rows);
        else
          layer_bwd<TM, false, false>(in, ldi, out, ldo, a.W[l], K, N, w, lane, nullptr, gd, rows);
        __syncthreads();
        float* tp = in; in = out; out = tp;
        const int tl = ldi; ldi = ldo; ldo = tl;
      }
    }
  }
}

// loss[0] = sum(lrow) / B, dsum[0] (and dsum2[0]) = sum(dz): thread t adds rows
// t, t + 256, ... in float64, then a fixed tree over the 256 partial sums.
__global__ __launch_bounds__(THREADS) void wd_train_sums(const float* __restrict__ lrow, const float* __restrict__ dz, int B,
                                                         float* __restrict__ loss, float* __restrict__ dsum,
                                                         float* __restrict__ dsum2) {
  __shared__ double sl[THREADS], sd[THREADS];
  double l = 0.0, d = 0.0;
  for (int i = threadIdx.x; i < B; i += THREADS) {
    l += (double)lrow[i];
    d += (double)dz[i];
  }
  sl[threadIdx.x] = l;
  sd[threadIdx.x] = d;
  __syncthreads();
  for (int h = THREADS / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      sl[threadIdx.x] += sl[threadIdx.x + h];
      sd[threadIdx.x] += sd[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    loss[0] = (float)(sl[0] / (double)B);
    dsum[0] = (float)sd[0];
    if (dsum2 != nullptr) dsum2[0] = (float)sd[0];
  }
}

template <int TM>
static hipError_t launch(const Args& a, size_t lds, hipStream_t stream) {
  static bool raised = false;   // dynamic LDS beyond 64 KiB needs the attribute (once per kernel)
  if (!raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&wd_train_rows<TM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 8 * TM);
    if (e != hipSuccess) return e;
    raised = true;
  }
  const unsigned grid = (unsigned)(((long long)a.f.B + TM - 1) / TM);
  hipLaunchKernelGGL((wd_train_rows<TM>), dim3(grid), dim3(THREADS), lds, stream, a);
  return hipGetLastError();
}

}  // namespace wdt
}  // namespace dtfk

extern "C" {

int dtfk_wd_train_supported(int D, int nl, const int* dims) { return dtfk_wd_eval_supported(D, nl, dims); }

int dtfk_wd_train_tile(int B, int nl, const int* dims) { return dtfk_wd_eval_tile(B, nl, dims); }

long long dtfk_wd_train_lds_bytes(int D, int nl, const int* dims, int tile) {
  int ld0, ld1;
  dtfk::wde::strides(D, nl, dims, ld0, ld1);
  return 4LL * tile * (ld0 + ld1) + 8LL * tile;
}

hipError_t dtfk_wd_train_rows(const dtfk::wdt::Args* p, int tile, hipStream_t stream) {
  if (p == nullptr) return hipErrorInvalidValue;
  const dtfk::wde::Args& f = p->f;
  if (f.B < 1 || !dtfk_wd_train_supported(f.D, f.nl, f.dims) || f.mode < 0 || f.mode > 2 || f.F < 1)
    return hipErrorInvalidValue;
  // (ids may be null: a batch of empty rows has no entries, and none is read)
  if (f.Wt == nullptr || f.E == nullptr || f.offsets == nullptr || f.labels == nullptr || f.bias == nullptr ||
      f.lrow == nullptr || f.brow == nullptr || f.z_out == nullptr || p->dz == nullptr || p->demb == nullptr)
    return hipErrorInvalidValue;
  // table rows, the hidden layers' weights and biases, and the [B, width] outputs move 16 bytes at a time
  uintptr_t al = reinterpret_cast<uintptr_t>(f.E) | reinterpret_cast<uintptr_t>(p->demb) |
                 reinterpret_cast<uintptr_t>(p->act[0]);
  for (int l = 0; l < f.nl; ++l) {
    if (f.W[l] == nullptr || f.b[l] == nullptr || p->act[l] == nullptr) return hipErrorInvalidValue;
    if (l >= 1 && p->dzl[l] == nullptr) return hipErrorInvalidValue;
    if (l < f.nl - 1) al |= reinterpret_cast<uintptr_t>(f.W[l]) | reinterpret_cast<uintptr_t>(f.b[l]);
    al |= reinterpret_cast<uintptr_t>(p->act[l]);
    if (l >= 1) al |= reinterpret_cast<uintptr_t>(p->dzl[l]);
  }
  if (al & 15) return hipErrorInvalidValue;
  if (tile == 0) tile = dtfk_wd_train_tile(f.B, f.nl, f.dims);
  if (tile != 16 && tile != 32) return hipErrorInvalidValue;
  dtfk::wdt::Args a = *p;
  dtfk::wde::strides(f.D, f.nl, f.dims, a.f.ld0, a.f.ld1);
  const size_t lds = 4 * (size_t)tile * (size_t)(a.f.ld0 + a.f.ld1);
  if (lds + 8 * (size_t)tile > 160 * 1024) return hipErrorInvalidValue;
  a.f.lsh = 0;
  while ((4 << a.f.lsh) < f.D) ++a.f.lsh;   // LPR = 2^lsh lanes of 16 bytes cover a table row
  return tile == 16 ? dtfk::wdt::launch<16>(a, lds, stream) : dtfk::wdt::launch<32>(a, lds, stream);
}

hipError_t dtfk_wd_train_sums(const float* lrow, const float* dz, int B, float* loss, float* dsum, float* dsum2,
                              hipStream_t stream) {
  if (lrow == nullptr || dz == nullptr || B < 1 || loss == nullptr || dsum == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dtfk::wdt::wd_train_sums, dim3(1), dim3(dtfk::wde::THREADS), 0, stream, lrow, dz, B, loss, dsum,
                     dsum2);
  return hipGetLastError();
}

}  // extern "C"
