// Reached by: models/mlp.py evaluate() (FusedMLPTrainer.evaluate, GemmMLPTrainer.evaluate, examples/mnist_example.py's test accuracy) and the compat Session's lowered loss / accuracy fetch (compat/lowering.py MLPStepPlan.run_eval); tests/test_mlp_eval_gpu.py, scripts/bench_eval.py
// Forward-only evaluation of the reference model over N rows (example.py:187,
// "Test-Accuracy"):
//   a2 = act(x W1 + b1); z3 = a2 W2 + b2
//   loss_i = -sum(y_ log softmax(z3))   (naive)  |  logsumexp(z3) - sum(y_ z3)   (stable)
//   pred_i = argmax(z3), first maximum on ties (TF / NumPy)
// accumulated into a device record {loss_sum (fp64), correct, rows}, so a large
// set is evaluated chunk by chunk on one stream and read back once.  Every
// product is exact fp32 on the matrix cores (v_mfma_f32_16x16x4_f32, fp32
// accumulate) as in graph_mlp.hip: the numbers are the fp32 graph's up to
// summation order.  (No bf16 split here: a float feed's k / 255 is not exact in
// bf16, and the pass streams x once.)
//
//   mlp_eval_tiles   one workgroup per 32 rows (two 16-row MFMA tiles) covers
//                    ALL hidden columns, so x is read once; its 4 waves take
//                    interleaved 16-deep K blocks (lane group g holds
//                    k = 16j + 4g .. +3 as one float4 / 4 pixels of x: no
//                    shuffles), W1 comes from L2, and the next K block's loads
//                    are issued before the current block's MFMAs.  A lane's
//                    hidden columns are CONTIGUOUS in W1 (hidden_col: MFMA tile
//                    j, lane r -> 4 r + j, ...), so a W1 row reaches the lane's
//                    7 / 8 tiles as 16- / 8- / 4-byte loads instead of one
//                    4-byte gather per tile (H % 4 == 0 and a 16-byte aligned
//                    W1; 4-byte loads otherwise).  The waves'
//                    partial tiles are summed through LDS in a fixed tree;
//                    waves 0 / 1 then finish one row tile each: a2 into LDS,
//                    z3 (MFMA), softmax with 16-lane reductions, loss, argmax,
//                    optional pred / logits, and the tile's {loss, correct}.
//   mlp_eval_reduce  ONE workgroup sums the tile partials in a fixed order (fp64
//                    loss, integer count) into the record: no float atomics,
//                    two runs give the same bits.  `reset` starts the record
//                    over (no memset node: small memset nodes are not re-applied
//                    on graph replay on this stack, common.h).
// Ragged edges are branch-free (clamped addresses, masked values, as l1_tile in
// graph_mlp.hip): nothing is read past row N - 1 or column K - 1.
// Shapes: any N >= 1, K >= 1, H <= 128, C <= 16.
// Measured (profiles/mlp_eval_ab.json, 10,000 x 784): 46 us on uint8 rows, 58 us
// on float32; the matrix cores are busy 20 % of the SIMD cycles (floor 11 us)
// and the waves wait at s_waitcnt 53 % of theirs -- at 2 waves per SIMD the
// one-block-ahead prefetch does not cover the operand latency.  Next: a deeper
// operand pipeline, 16-row workgroups for more waves per SIMD.
#include "common.h"
#include "mlp_api.h"
#include "mlp_device.h"

namespace dtfk {
namespace mlpe {

constexpr int MAXH = 128;
constexpr int CP = 16;                  // classes padded to one MFMA tile
constexpr int RT = 2;                   // 16-row MFMA tiles per workgroup
constexpr int ROWS = 16 * RT;
constexpr int NW = 4;                   // waves: interleaved 16-deep K blocks
constexpr int LDA = MAXH + 4;           // a2 row stride in LDS (floats)
constexpr int RED = 256;                // threads of mlp_eval_reduce

enum { X_F32 = 0, X_F32V = 1, X_U8 = 2 };   // x as floats | float4s (K % 4 == 0, 16-byte aligned) | 4 pixels per load

struct Args {
  const float* x;
  const uint8_t* xu;
  const void* labels;
  const float* W1;
  const float* b1;
  const float* W2;
  const float* b2;
  float* part_loss;     // [tiles]
  int* part_correct;    // [tiles]
  int* pred;            // [N] or null
  float* logits;        // [N][C] or null
  int N, K, H, C, act, naive, label_kind;
};

// The hidden column that lane r of MFMA column tile j computes.  Any bijection
// serves (b1 and the a2 store use the same one); this one makes a lane's columns
// contiguous in a W1 row: tiles 0-3 are columns 4 r .. 4 r + 3 (0 .. 63); with 8
// tiles, tiles 4-7 are 64 + 4 r .. + 3; with 7, tiles 4-5 are 64 + 2 r .. + 1
// (64 .. 95) and tile 6 is 96 + r (96 .. 111).
template <int HT>
__device__ __forceinline__ int hidden_col(int j, int r) {
  static_assert(HT == 7 || HT == 8, "7 or 8 hidden tiles");
  if (j < 4) return 4 * r + j;
  if (HT == 8) return 64 + 4 * r + (j - 4);
  return j < 6 ? 64 + 2 * r + (j - 4) : 96 + r;
}

// One 16-deep K block of a wave's operands: x for both row tiles, W1 for every
// hidden tile.  Lane (r, g): x[row r][k + s], W1[k + s][hidden_col(j, r)], k = 16 kb + 4 g.
template <int HT>
struct KBlock {
  float xa[RT][4];
  float wb[HT][4];
};

// Addresses are always clamped into the arrays.  MASK (the ragged last block of
// K only): values at k >= K are zeroed.  The full blocks of the main loop carry
// no selects -- a load whose only use is one arm of a select is sunk into a
// branch around that use and waited for there, which would put the prefetch
// behind the MFMAs again.  Columns >= H hold some valid column's values here
// and are zeroed where a2 is written.  WV: H % 4 == 0 and W1 16-byte aligned.
template <int XK, int HT, bool WV, bool MASK>
__device__ __forceinline__ void load_block(KBlock<HT>& b, const float* const (&xr)[RT],
                                           const uint8_t* const (&xur)[RT], const float* __restrict__ W1, int kb,
                                           int g, int r, int K, int H) {
  const int k = kb * 16 + 4 * g;
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    if constexpr (XK == X_U8) {
      const uint32_t v = *reinterpret_cast<const uint32_t*>(xur[t] + min(k, K - 4));
      const bool ok = !MASK || k < K;              // K % 4 == 0: the 4 pixels are all in or all out
#pragma unroll
      for (int s = 0; s < 4; ++s) b.xa[t][s] = ok ? px255((v >> (8 * s)) & 255u) : 0.f;
    } else if constexpr (XK == X_F32V) {
      const float4 v = *reinterpret_cast<const float4*>(xr[t] + min(k, K - 4));
      const bool ok = !MASK || k < K;
      b.xa[t][0] = ok ? v.x : 0.f; b.xa[t][1] = ok ? v.y : 0.f; b.xa[t][2] = ok ? v.z : 0.f; b.xa[t][3] = ok ? v.w : 0.f;
    } else {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float v = xr[t][min(k + s, K - 1)];
        b.xa[t][s] = (!MASK || k + s < K) ? v : 0.f;
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float* wr = W1 + (size_t)min(k + s, K - 1) * H;
    const bool kok = !MASK || k + s < K;
    float v[8];
    if constexpr (WV) {
      const float4 lo = *reinterpret_cast<const float4*>(wr + min(4 * r, H - 4));
      v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w;
      if constexpr (HT == 8) {
        const float4 hi = *reinterpret_cast<const float4*>(wr + min(64 + 4 * r, H - 4));
        v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
      } else {
        const float2 mid = *reinterpret_cast<const float2*>(wr + min(64 + 2 * r, H - 2));
        v[4] = mid.x, v[5] = mid.y;
        v[6] = wr[min(96 + r, H - 1)];
      }
    } else {
#pragma unroll
      for (int j = 0; j < HT; ++j) v[j] = wr[min(hidden_col<HT>(j, r), H - 1)];
    }
#pragma unroll
    for (int j = 0; j < HT; ++j) b.wb[j][s] = kok ? v[j] : 0.f;
  }
}

template <int HT>
__device__ __forceinline__ void mma_block(f32x4 (&acc)[RT][HT], const KBlock<HT>& b) {
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int j = 0; j < HT; ++j) acc[t][j] = mfma4(b.xa[t][s], b.wb[j][s], acc[t][j]);
}

template <int XK, int HT, bool WV>
__global__ __launch_bounds__(NW * 64) void mlp_eval_tiles(Args a) {
  __shared__ f32x4 red[2][RT * HT][64];   // the waves' partial tiles (fixed tree: (w0 + w2) + (w1 + w3))
  __shared__ float a2s[ROWS * LDA];       // a2 rows of both tiles, columns >= H are 0
  __shared__ float w2s[HT * 16 * CP];     // W2 [16 HT][CP], zero padded
  __shared__ float b1s[HT * 16];          // b1 (columns >= H: b1[H - 1], unused)
  __shared__ float b2s[CP];
  __shared__ float labs[ROWS * CP];       // the tile's labels as one-hot rows, classes >= C are 0
  __shared__ float lsum[RT];
  __shared__ int csum[RT];
  const int N = a.N, K = a.K, H = a.H, C = a.C;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const long long row0 = (long long)blockIdx.x * ROWS;
  const float* xr[RT];
  const uint8_t* xur[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const size_t row = (size_t)min(row0 + 16 * t + r, (long long)N - 1);   // rows >= N: row N - 1 again, masked below
    xr[t] = a.x + row * K;
    xur[t] = a.xu + row * K;
  }
  // The small operands (W2, b1, b2, this tile's labels as one-hot rows): every
  // global load first, the LDS stores behind the first K block's loads -- a
  // load -> store loop waits one memory round trip per iteration, and loading
  // them where the head uses them put ~10 us of round trips behind the K loop.
  // First read behind the barriers of the tile sum.
  constexpr int W2N = HT * 16 * CP / (NW * 64);   // 7 or 8 values per thread
  constexpr int LBN = ROWS * CP / (NW * 64);      // 2
  float w2v[W2N];
  int labraw[LBN];                                // float bits (one-hot rows) or the row's class id
#pragma unroll
  for (int q = 0; q < W2N; ++q) {
    const int i = tid + q * NW * 64, h = i / CP, c = i % CP;
    w2v[q] = a.W2[min(h, H - 1) * C + min(c, C - 1)];
  }
  const float bsv = *(tid < HT * 16 ? a.b1 + min(tid, H - 1) : a.b2 + min(tid - HT * 16, C - 1));
  size_t lrow[LBN];
#pragma unroll
  for (int q = 0; q < LBN; ++q) lrow[q] = (size_t)min(row0 + (tid + q * NW * 64) / CP, (long long)N - 1);
  if (a.label_kind == 2) {                        // (wave-uniform; only loads inside the branches)
#pragma unroll
    for (int q = 0; q < LBN; ++q)
      labraw[q] = __float_as_int(reinterpret_cast<const float*>(a.labels)[lrow[q] * C + min((tid + q * NW * 64) % CP, C - 1)]);
  } else if (a.label_kind == 0) {
#pragma unroll
    for (int q = 0; q < LBN; ++q) labraw[q] = reinterpret_cast<const uint8_t*>(a.labels)[lrow[q]];
  } else {
#pragma unroll
    for (int q = 0; q < LBN; ++q) labraw[q] = reinterpret_cast<const int*>(a.labels)[lrow[q]];
  }
  f32x4 acc[RT][HT];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int j = 0; j < HT; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nfull = K / 16;               // whole K blocks: wave w takes w, w + NW, ...
  // two operand sets, ping-pong: the next block's loads go out before this
  // block's MFMAs (past the last whole block: clamped addresses, the values
  // are never used)
  KBlock<HT> cur, nxt;
  load_block<XK, HT, WV, false>(cur, xr, xur, a.W1, w, g, r, K, H);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < W2N; ++q) {
    const int i = tid + q * NW * 64, h = i / CP, c = i % CP;
    w2s[i] = (h < H && c < C) ? w2v[q] : 0.f;
  }
  if (tid < HT * 16) b1s[tid] = bsv;
  else if (tid < HT * 16 + CP) b2s[tid - HT * 16] = bsv;
#pragma unroll
  for (int q = 0; q < LBN; ++q) {
    const int i = tid + q * NW * 64, c = i % CP;
    const float lv = a.label_kind == 2 ? __int_as_float(labraw[q]) : (labraw[q] == c ? 1.f : 0.f);
    labs[i] = c < C ? lv : 0.f;
  }
  for (int kb = w; kb < nfull; kb += 2 * NW) {
    load_block<XK, HT, WV, false>(nxt, xr, xur, a.W1, kb + NW, g, r, K, H);
    __builtin_amdgcn_sched_barrier(0);      // keep the loads above the MFMAs they run under
    mma_block<HT>(acc, cur);
    __builtin_amdgcn_sched_barrier(0);
    load_block<XK, HT, WV, false>(cur, xr, xur, a.W1, kb + 2 * NW, g, r, K, H);
    __builtin_amdgcn_sched_barrier(0);
    if (kb + NW < nfull) mma_block<HT>(acc, nxt);
  }
  if ((K & 15) != 0 && (nfull % NW) == w) {   // the ragged last block, by the wave whose turn it is
    load_block<XK, HT, WV, true>(cur, xr, xur, a.W1, nfull, g, r, K, H);
    mma_block<HT>(acc, cur);
  }
  // tile sums in a fixed order: waves 2, 3 -> waves 0, 1; then wave 0 keeps row
  // tile 0 and wave 1 row tile 1, each adding the other's half
  if (w >= 2) {
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int j = 0; j < HT; ++j) red[w - 2][t * HT + j][lane] = acc[t][j];
  }
  __syncthreads();
  if (w < 2) {
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
      for (int j = 0; j < HT; ++j) acc[t][j] += red[w][t * HT + j][lane];
  }
  __syncthreads();
  f32x4 mine[HT];
  if (w < 2) {
#pragma unroll
    for (int j = 0; j < HT; ++j) {
      red[w][j][lane] = w == 0 ? acc[1][j] : acc[0][j];   // the other wave's row tile (no dynamic index)
      mine[j] = w == 0 ? acc[0][j] : acc[1][j];
    }
  }
  __syncthreads();
  if (w < 2) {
    // a2 = act(z2 + b1) of row tile w: C layout, lane holds rows 4g + i, column hidden_col(j, r)
#pragma unroll
    for (int j = 0; j < HT; ++j) {
      const f32x4 t4 = mine[j] + red[1 - w][j][lane];
      const int col = hidden_col<HT>(j, r);
      const float bv = b1s[col];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        a2s[(16 * w + 4 * g + i) * LDA + col] = col < H ? act_fwd(t4[i] + bv, a.act) : 0.f;
    }
  }
  __syncthreads();
  float loss_part = 0.f;
  int corr_part = 0;
  if (w < 2) {
    // z3 = a2 W2 (two accumulators: the dependent-accumulator latency of one chain)
    f32x4 z0 = {0.f, 0.f, 0.f, 0.f}, z1 = {0.f, 0.f, 0.f, 0.f};
    const float* ar = a2s + (16 * w + r) * LDA;
#pragma unroll 4
    for (int k = 0; k < HT * 16; k += 8) {
      z0 = mfma4(ar[k + g], w2s[(k + g) * CP + r], z0);
      z1 = mfma4(ar[k + 4 + g], w2s[(k + 4 + g) * CP + r], z1);
    }
    const f32x4 z4 = z0 + z1;
    const bool cl = r < C;
    const float b2v = b2s[r];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long m = row0 + 16 * w + 4 * g + i;    // row; column r = class
      const bool valid = m < N;
      const float lab = labs[(16 * w + 4 * g + i) * CP + r];
      const float z = cl ? z4[i] + b2v : -INFINITY;
      const float mx = row16_max(z);
      const float e = cl ? expf(z - mx) : 0.f;
      const float s = row16_sum(e);
      // loss term: naive -y_ log(softmax) exactly as the graph computes it
      // (0 * log(0) = NaN like TF); stable -y_ (z - max - log sum exp)
      const float lt = cl ? -lab * (a.naive ? logf(e / s) : (z - mx - logf(s))) : 0.f;
      const float lrow = row16_sum(lt);
      // first-maximum argmax of z3 and of y_
      const float pi = row16_min(cl && z == mx ? (float)r : 1e9f);
      const float lm = row16_max(cl ? lab : -INFINITY);
      const float li = row16_min(cl && lab == lm ? (float)r : 1e9f);
      if (valid) {
        if (a.logits != nullptr && cl) a.logits[(size_t)m * C + r] = z;
        if (r == 0) {
          if (a.pred != nullptr) a.pred[m] = (int)pi;
          loss_part += lrow;
          corr_part += pi == li ? 1 : 0;
        }
      }
    }
    // (lanes with r == 0 hold the sums of their 4 rows)
    loss_part += __shfl_xor(loss_part, 16, 64);
    loss_part += __shfl_xor(loss_part, 32, 64);
    corr_part += __shfl_xor(corr_part, 16, 64);
    corr_part += __shfl_xor(corr_part, 32, 64);
    if (lane == 0) {
      lsum[w] = loss_part;
      csum[w] = corr_part;
    }
  }
  __syncthreads();
  if (tid == 0) {
    a.part_loss[blockIdx.x] = lsum[0] + lsum[1];
    a.part_correct[blockIdx.x] = csum[0] + csum[1];
  }
}

// The tile partials into the record, in a fixed order: thread t sums tiles
// t, t + RED, ... (fp64), then a fixed tree over the threads.
__global__ __launch_bounds__(RED) void mlp_eval_reduce(const float* __restrict__ part_loss,
                                                       const int* __restrict__ part_correct, int tiles, long long rows,
                                                       int reset, Record* rec) {
  __shared__ double ls[RED];
  __shared__ long long cs[RED];
  const int tid = threadIdx.x;
  double l = 0.0;
  long long c = 0;
  for (int t = tid; t < tiles; t += RED) {
    l += (double)part_loss[t];
    c += part_correct[t];
  }
  ls[tid] = l;
  cs[tid] = c;
  __syncthreads();
  for (int s = RED / 2; s > 0; s >>= 1) {
    if (tid < s) {
      ls[tid] += ls[tid + s];
      cs[tid] += cs[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    Record v = reset ? Record{0.0, 0, 0} : *rec;
    v.loss_sum += ls[0];
    v.correct += cs[0];
    v.rows += rows;
    *rec = v;
  }
}

template <int HT, bool WV>
static void launch_tiles(int xk, const Args& a, int tiles, hipStream_t stream) {
  const dim3 grid(tiles), block(NW * 64);
  if (xk == X_U8) hipLaunchKernelGGL((mlp_eval_tiles<X_U8, HT, WV>), grid, block, 0, stream, a);
  else if (xk == X_F32V) hipLaunchKernelGGL((mlp_eval_tiles<X_F32V, HT, WV>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((mlp_eval_tiles<X_F32, HT, WV>), grid, block, 0, stream, a);
}

}  // namespace mlpe
}  // namespace dtfk

// Scratch (4-byte words) of one evaluation of N rows: the per-tile {loss, correct}.
extern "C" long long dtfk_mlp_eval_part_words(long long N) {
  return 2 * ((N + dtfk::mlpe::ROWS - 1) / dtfk::mlpe::ROWS);
}

extern "C" hipError_t dtfk_mlp_eval(const dtfk::mlpe::Eval* p, hipStream_t stream) {
  using namespace dtfk::mlpe;
  const int N = p->N, K = p->K, H = p->H, C = p->C;
  if (N < 1 || K < 1 || H < 1 || H > MAXH || C < 1 || C > CP) return hipErrorInvalidValue;
  if ((p->x == nullptr) == (p->xu == nullptr) || p->labels == nullptr || p->part == nullptr || p->rec == nullptr ||
      p->W1 == nullptr || p->b1 == nullptr || p->W2 == nullptr || p->b2 == nullptr)
    return hipErrorInvalidValue;
  if (p->label_kind < 0 || p->label_kind > 2 || p->act < 0 || p->act > 1) return hipErrorInvalidValue;
  if (p->xu != nullptr && ((K & 3) || (reinterpret_cast<uintptr_t>(p->xu) & 3))) return hipErrorInvalidValue;
  const int xk = p->xu != nullptr ? X_U8
                                  : (((K & 3) == 0 && (reinterpret_cast<uintptr_t>(p->x) & 15) == 0) ? X_F32V : X_F32);
  const int tiles = (int)(((long long)N + ROWS - 1) / ROWS);
  Args a{p->x, p->xu, p->labels, p->W1, p->b1, p->W2, p->b2, p->part, reinterpret_cast<int*>(p->part + tiles),
         p->pred, p->logits, N, K, H, C, p->act, p->naive, p->label_kind};
  const bool wv = (H & 3) == 0 && (reinterpret_cast<uintptr_t>(p->W1) & 15) == 0;
  if (H <= 112) {                                        // the reference's 100 hidden units: 7 tiles, not 8
    if (wv) launch_tiles<7, true>(xk, a, tiles, stream);
    else launch_tiles<7, false>(xk, a, tiles, stream);
  } else {
    if (wv) launch_tiles<8, true>(xk, a, tiles, stream);
    else launch_tiles<8, false>(xk, a, tiles, stream);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(mlp_eval_reduce, dim3(1), dim3(RED), 0, stream, p->part, a.part_correct, tiles, (long long)N,
                     p->reset, p->rec);
  return hipGetLastError();
}
