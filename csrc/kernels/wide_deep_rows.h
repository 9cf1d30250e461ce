// Device code that the tower row kernels share (wide_deep_eval.hip wd_eval_rows,
// wide_deep_train.hip wd_train_rows, deepfm.hip dfm_rows, deepfm_fields.hip
// dfmf_rows): the exact-fp32 MFMA
// hidden layer with its four-deep operand ring, its backward (layer_bwd: described
// in wide_deep_train.hip's header) and the bag reader's helpers (the Wide&Deep
// reader itself: wide_deep_bags.h).  Included by those four .hip files only, after
// common.h and wide_deep_eval.h; the designs are described in wide_deep_eval.hip's
// and wide_deep_train.hip's headers.
#pragma once

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
// ldi / ldo; in's columns K .. ceil16(K) are 0.  STORE: the tile's rows below
// `rows` also go to the global gout[rows][N] (the training step's act[l]).
template <int TM, bool MASK, bool STORE = false>
__device__ __forceinline__ void layer(const float* __restrict__ in, int ldi, float* __restrict__ out, int ldo,
                                      const float* __restrict__ W, const float* __restrict__ bv, int K, int N, int w,
                                      int lane, float* __restrict__ gout = nullptr, int rows = 0) {
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
        if constexpr (STORE) {
          const int row = 16 * t + 4 * g + i;
          if (row < rows) *reinterpret_cast<float4*>(gout + (size_t)row * N + col) = v;
        }
      }
    }
  }
}

// One 16-deep block of W^T for 64 output columns: lane (r, g) gets
// W[col + j][16 nb + 4 g .. + 3], j = 0 .. 3 (col + 3 < K: rows inside the matrix).
__device__ __forceinline__ void load_wt(float4 (&b)[4], const float* __restrict__ wr, int nb, int N) {
#pragma unroll
  for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const float4*>(wr + (size_t)j * N + 16 * nb);
}

// acc[j] += A block (lane: row r, n = 4 g + s) x W^T block (lane: n = 4 g + s in b[j]'s component s, column col + j)
__device__ __forceinline__ void mma_block_t(f32x4 (&acc)[4], const float4 av, const float4 (&b)[4]) {
  acc[0] = mfma4(av.x, b[0].x, acc[0]);
  acc[1] = mfma4(av.x, b[1].x, acc[1]);
  acc[2] = mfma4(av.x, b[2].x, acc[2]);
  acc[3] = mfma4(av.x, b[3].x, acc[3]);
  acc[0] = mfma4(av.y, b[0].y, acc[0]);
  acc[1] = mfma4(av.y, b[1].y, acc[1]);
  acc[2] = mfma4(av.y, b[2].y, acc[2]);
  acc[3] = mfma4(av.y, b[3].y, acc[3]);
  acc[0] = mfma4(av.z, b[0].z, acc[0]);
  acc[1] = mfma4(av.z, b[1].z, acc[1]);
  acc[2] = mfma4(av.z, b[2].z, acc[2]);
  acc[3] = mfma4(av.z, b[3].z, acc[3]);
  acc[0] = mfma4(av.w, b[0].w, acc[0]);
  acc[1] = mfma4(av.w, b[1].w, acc[1]);
  acc[2] = mfma4(av.w, b[2].w, acc[2]);
  acc[3] = mfma4(av.w, b[3].w, acc[3]);
}

// da[TM][K] = G[TM][N] W^T, W [K][N] row-major; G is an LDS tile of row stride ldg.
//   FIRST (the tower's first layer): da is demb; the tile's rows below `rows` go
//     to gout[rows][K], nothing to LDS.
//   else: dzl = da * (act > 0) goes to the LDS tile `out` (row stride ldo) and,
//     for rows below `rows`, to gout[rows][K]; act is read from `out` itself, or
//     (GMASK) from the tile's global rows gact[rows][K].
//   FMS (deepfm.hip, with FIRST): the table is shared with a factorization machine,
//     demb = da + dz_s[row] gact[row][:], where gact is the tile's act[0] = S rows in
//     global memory and dz_s the tile's dz in LDS (rows >= `rows`: row rows - 1's, not stored).
//   FIELDS (deepfm_fields.hip, with FMS): da is P blocks of fk columns, one per field, and every
//     block takes the same dz S: gact is the tile's S [TM][fk] in LDS, read at column col mod fk
//     (fk % 4 == 0: a 16-byte column group lies inside one field).
template <int TM, bool FIRST, bool GMASK, bool FMS = false, bool FIELDS = false>
__device__ __forceinline__ void layer_bwd(const float* __restrict__ G, int ldg, float* out, int ldo,
                                          const float* __restrict__ W, int K, int N, int w, int lane,
                                          const float* gact, float* __restrict__ gout, int rows,
                                          const float* dz_s = nullptr, int fk = 0) {
  const int r = lane & 15, g = lane >> 4;
  const int nnb = N >> 4, nch = (K + 63) >> 6, items = (TM / 16) * nch;
  for (int it = w; it < items; it += NW) {
    const int t = it / nch, c0 = (it - t * nch) * 64;
    const int col = min(c0 + 4 * r, K - 4);                   // K % 4 == 0: a clamped lane repeats the last 4 columns
    const float* ar = G + (16 * t + r) * ldg + 4 * g;
    const float* wr = W + (size_t)col * N + 4 * g;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    int nb = 0;
    if (nnb >= PF) {                                           // the forward's ring of PF operand sets
      float4 b[PF][4], av[PF];
#pragma unroll
      for (int p = 0; p < PF; ++p) {
        load_wt(b[p], wr, p, N);
        av[p] = *reinterpret_cast<const float4*>(ar + 16 * p);
      }
      for (; nb + PF <= nnb; nb += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
          mma_block_t(acc, av[p], b[p]);
          const int nx = min(nb + p + PF, nnb - 1);            // (past the last block: it again, unused)
          load_wt(b[p], wr, nx, N);
          av[p] = *reinterpret_cast<const float4*>(ar + 16 * nx);
        }
      }
    }
    for (; nb < nnb; ++nb) {                                   // the last nnb % PF blocks (all of a short N)
      float4 b[4];
      load_wt(b, wr, nb, N);
      mma_block_t(acc, *reinterpret_cast<const float4*>(ar + 16 * nb), b);
    }
    // C layout: lane holds rows 4 g + i of the tile, column col + j in acc[j][i]
    if (c0 + 4 * r < K) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = 16 * t + 4 * g + i;
        float4 v = make_float4(acc[0][i], acc[1][i], acc[2][i], acc[3][i]);
        if constexpr (!FIRST) {
          float* op = out + row * ldo + col;
          const float4 h = GMASK ? *reinterpret_cast<const float4*>(gact + (size_t)min(row, rows - 1) * K + col)
                                 : *reinterpret_cast<const float4*>(op);
          v.x = h.x > 0.f ? v.x : 0.f;
          v.y = h.y > 0.f ? v.y : 0.f;
          v.z = h.z > 0.f ? v.z : 0.f;
          v.w = h.w > 0.f ? v.w : 0.f;
          *reinterpret_cast<float4*>(op) = v;
        }
        if constexpr (FMS) {
          float4 sv;
          if constexpr (FIELDS) sv = *reinterpret_cast<const float4*>(gact + row * fk + col % fk);
          else sv = *reinterpret_cast<const float4*>(gact + (size_t)min(row, rows - 1) * K + col);
          const float d = dz_s[row];
          v.x += d * sv.x;
          v.y += d * sv.y;
          v.z += d * sv.z;
          v.w += d * sv.w;
        }
        if (row < rows) *reinterpret_cast<float4*>(gout + (size_t)row * K + col) = v;
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

// widths of the even / odd layers' inputs -> the two LDS buffers' row strides
static inline void strides(int D, int nl, const int* dims, int& ld0, int& ld1) {
  int k0 = (D + 15) & ~15, k1 = 16;
  for (int l = 1; l < nl; ++l) {
    if (l & 1) k1 = dims[l] > k1 ? dims[l] : k1;
    else k0 = dims[l] > k0 ? dims[l] : k0;
  }
  ld0 = k0 + 4;
  ld1 = k1 + 4;
}

}  // namespace wde
}  // namespace dtfk
