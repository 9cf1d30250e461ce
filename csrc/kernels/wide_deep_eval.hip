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

namespace dtfk {
namespace wde {

constexpr int THREADS = 256;
constexpr int NW = THREADS / 64;

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long uni(long long v) {
  const unsigned lo = (unsigned)uni((int)(unsigned)v), hi = (unsigned)uni((int)(v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// One 16-deep K block of weights for 64 output columns: lane (r, g) gets
// W[16 kb + 4 g + s][col .. col + 3], s = 0 .. 3.  Rows are clamped into the
// matrix; MASK (K % 16 != 0): rows >= K are zeroed.
template <bool MASK>
__device__ __forceinline__ void load_w(float4 (&b)[4], const float* __restrict__ wc, int kb, int g, int K, int N) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int k = 16 * kb + 4 * g + s;
    const float4 v = *reinterpret_cast<const float4*>(wc + (size_t)min(k, K - 1) * N);
    const bool ok = !MASK || k < K;
    b[s] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

constexpr int PF = 4;   // K blocks of operands in flight per wave

// acc[j] += A block (lane: row r, k = 4 g + s) x W block (lane: k = 4 g + s, columns col + j)
__device__ __forceinline__ void mma_block(f32x4 (&acc)[4], const float4 av, const float4 (&b)[4]) {
  const float as[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    acc[0] = mfma4(as[s], b[s].x, acc[0]);
    acc[1] = mfma4(as[s], b[s].y, acc[1]);
    acc[2] = mfma4(as[s], b[s].z, acc[2]);
    acc[3] = mfma4(as[s], b[s].w, acc[3]);
  }
}

// out[TM][N] = relu(in[TM][K] W + bv): in / out are LDS tiles of row strides
// ldi / ldo; in's columns K .. ceil16(K) are 0.
template <int TM, bool MASK>
__device__ __forceinline__ void layer(const float* __restrict__ in, int ldi, float* __restrict__ out, int ldo,
                                      const float* __restrict__ W, const float* __restrict__ bv, int K, int N, int w,
                                      int lane) {
  const int r = lane & 15, g = lane >> 4;
  const int nkb = (K + 15) >> 4, nch = (N + 63) >> 6, items = (TM / 16) * nch;
  for (int it = w; it < items; it += NW) {
    const int t = it / nch, c0 = (it - t * nch) * 64;
    const int col = min(c0 + 4 * r, N - 4);                  // N % 16 == 0: a clamped lane repeats the last 4 columns
    const float* ar = in + (16 * t + r) * ldi + 4 * g;
    const float* wc = W + col;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // PF K blocks of operands in flight (a ring of register sets, statically
    // indexed): one block ahead left the loop waiting ~1300 cycles per block on
    // the weights' L2 latency against 512 cycles of MFMA issue.
    int kb = 0;
    if (nkb >= PF) {
      float4 b[PF][4], av[PF];
#pragma unroll
      for (int p = 0; p < PF; ++p) {
        load_w<MASK>(b[p], wc, p, g, K, N);
        av[p] = *reinterpret_cast<const float4*>(ar + 16 * p);
      }
      for (; kb + PF <= nkb; kb += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
          mma_block(acc, av[p], b[p]);
          const int nx = min(kb + p + PF, nkb - 1);            // (past the last block: it again, unused)
          load_w<MASK>(b[p], wc, nx, g, K, N);
          av[p] = *reinterpret_cast<const float4*>(ar + 16 * nx);
        }
      }
    }
    for (; kb < nkb; ++kb) {                                   // the last nkb % PF blocks (all of a short K)
      float4 b[4];
      load_w<MASK>(b, wc, kb, g, K, N);
      mma_block(acc, *reinterpret_cast<const float4*>(ar + 16 * kb), b);
    }
    // C layout: lane holds rows 4 g + i of the tile, column col + j in acc[j][i]
    const float4 b4 = *reinterpret_cast<const float4*>(bv + col);
    if (c0 + 4 * r < N) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float4 v;
        v.x = fmaxf(acc[0][i] + b4.x, 0.f);
        v.y = fmaxf(acc[1][i] + b4.y, 0.f);
        v.z = fmaxf(acc[2][i] + b4.z, 0.f);
        v.w = fmaxf(acc[3][i] + b4.w, 0.f);
        *reinterpret_cast<float4*>(out + (16 * t + 4 * g + i) * ldo + col) = v;
      }
    }
  }
}

// The first chunk (up to 64 entries, one per lane) of a wave's row: the raw id
// and value of entry `lane`, read in place.  Nothing is read for an empty row
// or past the row's last entry (the lanes past it repeat the last one).
struct Chunk {
  long long raw;
  float v;
};
__device__ __forceinline__ Chunk load_chunk(const Args& a, long long c, int cnt, int lane) {
  Chunk ch{-1, 0.f};
  if (cnt > 0) {                                                      // (wave-uniform)
    const long long j = c + min(lane, cnt - 1);
    ch.raw = a.ids[j];
    ch.v = a.vals != nullptr ? a.vals[j] : 1.f;
  }
  return ch;
}

// TM: rows per workgroup.
template <int TM>
__global__ __launch_bounds__(THREADS) void wd_eval_rows(Args a) {
  extern __shared__ float4 wde_smem[];
  __shared__ float wide_s[TM];
  __shared__ int bad_s[TM];
  constexpr int RPW = TM / NW;                                         // rows per wave
  constexpr int GS = 16;                                               // table-row loads in flight per lane
  float* buf0 = reinterpret_cast<float*>(wde_smem);
  float* buf1 = buf0 + TM * a.ld0;
  const int lane = threadIdx.x & 63, w = uni((int)(threadIdx.x >> 6));
  const long long row0 = (long long)blockIdx.x * TM;
  const int D = a.D, D16 = (D + 15) & ~15, B = a.B;
  const long long F = a.F;

  // ---- bags: wave w takes rows w, w + NW, ... of the tile.  A table row is read
  // by LPR = 2^lsh >= D / 4 adjacent lanes, 16 bytes each, so one load
  // instruction fetches the rows of EP = 64 / LPR entries.
  const int lsh = a.lsh, LPR = 1 << lsh, EP = 64 >> lsh;
  const int sub = lane & (LPR - 1), q = lane >> lsh;
  const int colc = min(4 * sub, D - 4);
  // the wave's row offsets: lane i holds row w + NW i's (rows >= B: an empty bag)
  long long so = 0, eo = 0;
  if (lane < RPW) {
    const long long row = row0 + w + NW * lane, rowc = min(row, (long long)B - 1);
    so = a.offsets[rowc];
    eo = row < B ? a.offsets[rowc + 1] : so;
  }
  const int solo = (int)(unsigned)so, sohi = (int)(so >> 32), eolo = (int)(unsigned)eo, eohi = (int)(eo >> 32);
  auto row_range = [&](int i, long long& s, long long& e) {
    s = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(sohi, i) << 32) |
                    (unsigned)__builtin_amdgcn_readlane(solo, i));
    e = (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(eohi, i) << 32) |
                    (unsigned)__builtin_amdgcn_readlane(eolo, i));
  };
  long long s, e;
  row_range(0, s, e);
  Chunk cur = load_chunk(a, s, (int)min(64LL, e - s), lane);
  for (int i = 0; i < RPW; ++i) {
    const int rr = w + NW * i;
    // the next row's first chunk is requested before this row's table rows
    long long sn = 0, en = 0;
    if (i + 1 < RPW) row_range(i + 1, sn, en);
    const Chunk nxt = load_chunk(a, sn, (int)min(64LL, en - sn), lane);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float wacc = 0.f, ws = 0.f;
    int nbad = 0;
    for (long long c = s; c < e; c += 64) {
      const int cnt = (int)min(64LL, e - c);
      const Chunk ch = c == s ? cur : load_chunk(a, c, cnt, lane);
      const bool in = lane < cnt;
      const bool ok = in && ch.raw >= 0 && ch.raw < F;                 // out of range: skipped for both tables
      const long long id = ok ? ch.raw : -1;
      const float v = ok ? ch.v : 0.f;
      nbad += (in && !ok) ? 1 : 0;
      const float wt = a.Wt[ok ? ch.raw : 0];
      const int idlo = (int)(unsigned)id, idhi = (int)(id >> 32), vbits = __float_as_int(v);
      const int nsteps = (cnt + EP - 1) >> (6 - lsh);
      for (int t0 = 0; t0 < nsteps; t0 += GS) {
        float4 x[GS];
        float vv[GS];
        bool on[GS];
#pragma unroll
        for (int u = 0; u < GS; ++u) {                                 // step t: entry t EP + q, for every q
          const int src = min(min(t0 + u, nsteps - 1) * EP + q, 63);  // (a lane >= cnt holds id = -1)
          const int lo = __shfl(idlo, src, 64), hi = __shfl(idhi, src, 64);
          vv[u] = __int_as_float(__shfl(vbits, src, 64));
          on[u] = hi >= 0 && t0 + u < nsteps;                          // skipped entries and steps past the chunk: row 0, unused
          const unsigned long long rid = hi >= 0 ? (((unsigned long long)(unsigned)hi << 32) | (unsigned)lo) : 0ull;
          x[u] = *reinterpret_cast<const float4*>(a.E + (size_t)rid * D + colc);
        }
#pragma unroll
        for (int u = 0; u < GS; ++u) {
          acc.x = on[u] ? fmaf(vv[u], x[u].x, acc.x) : acc.x;
          acc.y = on[u] ? fmaf(vv[u], x[u].y, acc.y) : acc.y;
          acc.z = on[u] ? fmaf(vv[u], x[u].z, acc.z) : acc.z;
          acc.w = on[u] ? fmaf(vv[u], x[u].w, acc.w) : acc.w;
        }
      }
      wacc = ok ? fmaf(wt, v, wacc) : wacc;
      ws += a.mode == 2 ? v * v : v;                                   // (v = 0 where skipped)
    }
    for (int off = LPR; off < 64; off <<= 1) {                         // the EP partial rows of a column block
      acc.x += __shfl_xor(acc.x, off, 64);
      acc.y += __shfl_xor(acc.y, off, 64);
      acc.z += __shfl_xor(acc.z, off, 64);
      acc.w += __shfl_xor(acc.w, off, 64);
    }
    wacc = wave_sum(wacc);
    ws = wave_sum(ws);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nbad += __shfl_xor(nbad, off, 64);
    float scale = 1.f;                                                 // embedding_bag_fwd's rule
    if (a.mode == 1 && e > s) scale = 1.f / fmaxf(ws, 1e-30f);
    if (a.mode == 2 && e > s) scale = rsqrtf(fmaxf(ws, 1e-30f));
    // every lane now holds the sums of column block `sub`; lane l < D16 / 4 writes block l (l >= LPR: padding)
    if (4 * lane < D16) {
      const bool cok = 4 * lane < D;
      *reinterpret_cast<float4*>(buf0 + rr * a.ld0 + 4 * lane) =
          cok ? make_float4(acc.x * scale, acc.y * scale, acc.z * scale, acc.w * scale) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (lane == 0) {
      wide_s[rr] = wacc;
      bad_s[rr] = nbad;
    }
    cur = nxt;
    s = sn;
    e = en;
  }
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

static inline int ceil16(int v) { return (v + 15) & ~15; }

// widths of the even / odd layers' inputs -> the two buffers' row strides
static void strides(int D, int nl, const int* dims, int& ld0, int& ld1) {
  int k0 = ceil16(D), k1 = 16;
  for (int l = 1; l < nl; ++l) {
    if (l & 1) k1 = dims[l] > k1 ? dims[l] : k1;
    else k0 = dims[l] > k0 ? dims[l] : k0;
  }
  ld0 = k0 + 4;
  ld1 = k1 + 4;
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
