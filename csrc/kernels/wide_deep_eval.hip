// Reached by: one-GPU Wide&Deep forward-only evaluation (csrc/bind_wide_deep.cpp WideDeepEvalPlan: models/wide_deep.py evaluate / auc_update / evaluate_stream); tests/test_wide_deep_eval_gpu.py, scripts/bench_wide_deep_eval.py
// Forward-only evaluation of models/wide_deep.py on one GPU, where every table
// row is local: no dedup, no routing, no remap, no [B, D] / [B, H] round trips.
//
//   wide_r = sum_j Wt[id_j] v_j
//   emb_r  = combine_j E[id_j, :] v_j      sum | mean | sqrtn (ops.hip embedding_bag_fwd's scale, 1e-30 floor)
//   h      = relu(h W_l + b_l) over the hidden layers;  t_r = h w_last + b_last
//   z_r    = (wide_r + t_r) + bias;  loss_r = sigmoid_xent(z_r, y_r);  p_r = sigmoid(z_r)
//
//   wd_eval_rows  one workgroup (4 waves) per tile of TM = 16 or 32 batch rows.
//     bags    a wave per row, lanes across the D columns, 16 bytes (4 columns)
//             per lane: a table row is one coalesced read by LPR = 2^k >= D / 4
//             adjacent lanes, and one load instruction fetches the rows of
//             64 / LPR entries (4 at D = 64).  The row's ids and values are read
//             64 at a time, one per lane, in place -- the next row's before this
//             row's table rows are requested -- and the wide weight is read by
//             the lane that holds the id.  Ids reach the loading lanes by lane
//             shuffles, 16 load instructions in flight per lane; the 64 / LPR
//             partial rows are summed by a butterfly.  An id outside [0, F) is
//             skipped for both tables and counted once.  The scaled embedding
//             tile goes to LDS (columns D .. 16-multiple: 0).
//     tower   every hidden layer on v_mfma_f32_16x16x4_f32 (exact fp32 products,
//             fp32 accumulate: a fused multiply-add chain over k, no bf16
//             anywhere).  A work item is (16-row tile, 64 output columns); the
//             waves take items in turn.  A comes from LDS (one 16-byte read per
//             16-deep K block: lane group g holds k = 16 kb + 4 g .. + 3), the
//             weights stream from L2 (lane r holds columns c0 + 4 r .. + 3 of a
//             weight row: 16-byte loads, four K blocks of operands in flight
//             per wave), bias + ReLU in the epilogue, activations ping-pong
//             between two LDS buffers.
//     head    the width-1 last layer and the logit are per-row wave reductions;
//             per-row loss, p and bad count go to scratch, z and p to the
//             caller's [B] tensors if given.
//   reduce  eval_record_reduce (eval_record.hip, host entry dtfk_eval_reduce): every
//           model's reduce sums the scratch into the evaluation record.
//
// Ragged edges are branch-free: rows >= B are empty bags whose results are not
// stored; the ragged last K block of the first layer (D % 16 != 0) reads clamped
// weight rows and masks them (the LDS pad columns are 0); the ragged last column
// chunk (N % 64 != 0) reads clamped columns and is not stored.  Nothing is read
// past the last row, id or column.  No inter-workgroup waits, no float atomics:
// two runs give the same bits.
//
// LDS budget (MI355X: 160 KiB = 163,840 B per CU, a single workgroup may take
// all of it; workgroups per CU <= floor(160 KiB / LDS per workgroup)).  The two
// activation buffers hold the inputs of the even / odd layers, row stride = the
// widest of them + 4 floats (16-byte aligned rows):
//     bytes = 4 TM ((K0 + 4) + (K1 + 4)) + 8 TM,
//     K0 = max(ceil16(D), hidden[1]),  K1 = max(hidden[0], hidden[2])
//   worst supported shape (D <= 128, hidden 512-512-512): 4 TM 1032 + 8 TM
//     = 66,176 B at TM = 16 (2 workgroups per CU), 132,352 B at TM = 32 (1);
//   D = 64, hidden 512-256:  4 TM (260 + 516) + 8 TM = 49,792 B at TM = 16 (3
//     workgroups per CU), 99,584 B at TM = 32 (1);
//   D = 16, hidden 32-16:  4 TM (20 + 36) + 8 TM = 3,712 B at TM = 16.
// Tile rule (dtfk_wd_eval_tile), from profiles/wide_deep_eval_ab.json: 16 rows,
// except 32 rows where every hidden width is at most 64 (one column chunk per
// layer: a 16-row tile leaves three of the four waves without a work item) and
// there are at least 16384 rows (1024 16-row tiles, four per CU).  Measured at
// D = 64: 512-256 is 1.3-1.7x slower on 32-row tiles at every batch size (a wave
// then runs its two row tiles' items one after the other); towers of 16 or 64 are
// 4 % faster on them from 16384 rows and 1.3-1.6x slower at 500 and 4096, where
// 32-row tiles leave CUs idle.
#include "common.h"
#include "wide_deep_eval.h"
#include "wide_deep_rows.h"

namespace dtfk {
namespace wde {

// TM: rows per workgroup.
template <int TM>
__global__ __launch_bounds__(THREADS) void wd_eval_rows(Args a) {
  extern __shared__ float4 wde_smem[];
  __shared__ float wide_s[TM];
  __shared__ int bad_s[TM];
  float* buf0 = reinterpret_cast<float*>(wde_smem);
  float* buf1 = buf0 + TM * a.ld0;
  const int lane = threadIdx.x & 63, w = uni((int)(threadIdx.x >> 6));
  const long long row0 = (long long)blockIdx.x * TM;

  // ---- bags: the scaled embedding tile in buf0, wide sums and bad counts per row
#include "wide_deep_bags.h"
  __syncthreads();

  // ---- tower: hidden layers, ping-pong between the two buffers
  float* in = buf0;
  float* out = buf1;
  int ldi = a.ld0, ldo = a.ld1;
#pragma unroll
  for (int l = 0; l < MAXL - 1; ++l) {
    if (l < a.nl - 1) {                                                // (workgroup-uniform)
      const int K = a.dims[l], N = a.dims[l + 1];
      if (K & 15) layer<TM, true>(in, ldi, out, ldo, a.W[l], a.b[l], K, N, w, lane);
      else layer<TM, false>(in, ldi, out, ldo, a.W[l], a.b[l], K, N, w, lane);
      __syncthreads();
      float* tp = in; in = out; out = tp;
      const int tl = ldi; ldi = ldo; ldo = tl;
    }
  }

  // ---- the width-1 last layer and the head: a wave per row
  const int KL = a.dims[a.nl - 1];
  const float* wl = a.W[a.nl - 1];
  const float bl = a.b[a.nl - 1][0], bias = a.bias[0];
  for (int rr = w; rr < TM; rr += NW) {
    float acc = 0.f;
    for (int k = lane; k < KL; k += 64) acc = fmaf(in[rr * ldi + k], wl[k], acc);
    acc = wave_sum(acc);
    const long long row = row0 + rr;
    if (lane == 0 && row < B) {
      const float t = acc + bl;
      const float z = (wide_s[rr] + t) + bias;
      const float p = 1.f / (1.f + __expf(-z));
      a.lrow[row] = xent(z, a.labels[row]);
      a.prow[row] = p;
      a.brow[row] = bad_s[rr];
      if (a.z_out != nullptr) a.z_out[row] = z;
      if (a.p_out != nullptr) a.p_out[row] = p;
    }
  }
}

template <int TM>
static hipError_t launch(const Args& a, size_t lds, hipStream_t stream) {
  static bool raised = false;   // dynamic LDS beyond 64 KiB needs the attribute (once per kernel)
  if (!raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&wd_eval_rows<TM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 8 * TM);
    if (e != hipSuccess) return e;
    raised = true;
  }
  const unsigned grid = (unsigned)(((long long)a.B + TM - 1) / TM);
  hipLaunchKernelGGL((wd_eval_rows<TM>), dim3(grid), dim3(THREADS), lds, stream, a);
  return hipGetLastError();
}

}  // namespace wde
}  // namespace dtfk

extern "C" {

int dtfk_wd_eval_supported(int D, int nl, const int* dims) {
  using namespace dtfk::wde;
  if (D < 4 || D > MAXD || (D & 3) || nl < 2 || nl > MAXL || dims == nullptr || dims[0] != D || dims[nl] != 1) return 0;
  for (int l = 1; l < nl; ++l)
    if (dims[l] < 16 || dims[l] > MAXW || (dims[l] & 15)) return 0;
  return 1;
}

int dtfk_wd_eval_tile(int B, int nl, const int* dims) {
  if (B < 16384) return 16;
  for (int l = 1; l < nl; ++l)
    if (dims[l] > 64) return 16;
  return 32;
}

long long dtfk_wd_eval_lds_bytes(int D, int nl, const int* dims, int tile) {
  int ld0, ld1;
  dtfk::wde::strides(D, nl, dims, ld0, ld1);
  return 4LL * tile * (ld0 + ld1) + 8LL * tile;
}

hipError_t dtfk_wd_eval_rows(const dtfk::wde::Args* p, int tile, hipStream_t stream) {
  using namespace dtfk::wde;
  if (p == nullptr || p->B < 1 || !dtfk_wd_eval_supported(p->D, p->nl, p->dims) || p->mode < 0 || p->mode > 2 ||
      p->F < 1)
    return hipErrorInvalidValue;
  // (ids may be null: a batch of empty rows has no entries, and none is read)
  if (p->Wt == nullptr || p->E == nullptr || p->offsets == nullptr || p->labels == nullptr ||
      p->bias == nullptr || p->lrow == nullptr || p->prow == nullptr || p->brow == nullptr)
    return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(p->E) & 15) return hipErrorInvalidValue;   // table rows are read 16 bytes at a time
  for (int l = 0; l < p->nl; ++l) {
    if (p->W[l] == nullptr || p->b[l] == nullptr) return hipErrorInvalidValue;
    // the hidden layers' weights and biases are read 16 bytes at a time
    if (l < p->nl - 1 && ((reinterpret_cast<uintptr_t>(p->W[l]) | reinterpret_cast<uintptr_t>(p->b[l])) & 15))
      return hipErrorInvalidValue;
  }
  if (tile == 0) tile = dtfk_wd_eval_tile(p->B, p->nl, p->dims);
  if (tile != 16 && tile != 32) return hipErrorInvalidValue;
  Args a = *p;
  strides(a.D, a.nl, a.dims, a.ld0, a.ld1);
  const size_t lds = 4 * (size_t)tile * (size_t)(a.ld0 + a.ld1);
  if (lds + 8 * (size_t)tile > 160 * 1024) return hipErrorInvalidValue;
  a.lsh = 0;
  while ((4 << a.lsh) < a.D) ++a.lsh;   // LPR = 2^lsh lanes of 16 bytes cover a table row
  return tile == 16 ? launch<16>(a, lds, stream) : launch<32>(a, lds, stream);
}

}  // extern "C"
