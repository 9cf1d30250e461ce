// Reached by: DeepFMPlan (csrc/bind_deepfm.cpp), models/deepfm.py DeepFMTrainer; tests/test_deepfm_gpu.py, scripts/bench_fm.py --hidden
// DeepFM (Guo et al. 2017) on one GPU: a factorization machine and an MLP tower
// that read the same factor table.  This file is the form without fields: the
// batches are CSR rows and the tower reads the pooled factors S_r (as wide_deep's
// tower reads its sum-combined bag).  The form with fields, whose tower reads the
// concatenation of the per-field embeddings as the paper's does, is
// deepfm_fields.hip (dfmf_rows, over the (row, field) bag form).
//
//   S_r[f] = sum_i x_i V[id_i, f]        Q_r[f] = sum_i x_i^2 V[id_i, f]^2
//   fm_r   = sum_i x_i w[id_i] + 0.5 sum_f (S_r[f]^2 - Q_r[f])
//   a_0    = S_r;   a_l = relu(a_{l-1} W_{l-1} + b_{l-1}), l = 1 .. nh;   t_r = a_nh . w_last + b_last
//   z_r    = (fm_r + t_r) + b           loss_r = sigmoid_xent(z_r, y_r)
//   dz_r   = (sigmoid(z_r) - y_r) gscale
//   da_nh  = dz w_last^T;   dzl[l] = da_l * (a_l > 0);   da_{l-1} = dzl[l] W_{l-1}^T
//   demb_r = dz_r S_r + da_0,r
//
// demb is all the table update needs: dL/dV[j, f] = sum_occ x demb_r[f] - V[j, f] q_j
// is fm.hip's formula, so fm_update_runs / fm_update_carry run unchanged after this.
//
//   dfm_rows<TM, TRAIN>  one workgroup (4 waves) per tile of TM = 16 or 32 batch rows.
//     bags    wave w takes rows w, w + 4, ... of the tile.  A factor row is read by
//             LPR = 2^lsh >= K / 4 adjacent lanes, 16 bytes each: one load
//             instruction fetches the rows of EP = 64 / LPR entries, GS = 16 loads
//             in flight per lane.  A lane keeps two float4 sums per entry stream,
//             x v and (x v)^2, so S and Q come from the one pass (fm_rows's
//             arithmetic).  Entries arrive 64 at a time, one id / value / w[id] per
//             lane; the next chunk -- of this row, or the first of the wave's next
//             row -- is requested before the current chunk's table rows.  After
//             the __shfl_xor fold over offsets >= LPR, S goes to the first LDS
//             activation buffer (row stride ld0, columns K .. ceil16(K) zeroed);
//             the pairwise term is summed over the column blocks < K / 4 only
//             (K = 20: LPR = 8, blocks 5 .. 7 re-read block 4 and take no part),
//             and the FM score and the bad-id count go to one LDS word per row.
//     tower   wide_deep_rows.h's layer<TM, MASK, STORE> as it stands; TRAIN stores
//             act[0] = S and every act[l] to global memory.
//     head    a wave per row; TRAIN also leaves dz in an LDS word per row (rows >= B: 0)
//             and dzl[nh] in place.  TRAIN = false stops here: lrow, prow, brow, z_out,
//             p_out and nothing else.
//     backward  wide_deep_rows.h's layer_bwd; the first layer's epilogue adds
//             dz_s[row] S[row][col .. col + 3], S read back from the tile's own act[0]
//             rows in global memory (written by this workgroup before a workgroup
//             barrier, as layer 1's mask with three hidden layers).  S is still in LDS
//             only with one hidden layer, so the global read is the one code path.
//
// Ragged edges: rows >= B are empty bags with dz = 0, and nothing of them is
// stored; clamped lanes re-read the last valid 16 bytes and do not store; nothing is
// read or written past the last row, id or column.  No inter-workgroup waits, no
// float atomics: two runs give the same bits.
//
// LDS: wd_train_rows's budget plus dz's word per row,
//     bytes = 4 TM ((K0 + 4) + (K1 + 4)) + 12 TM,
//     K0 = max(ceil16(K), hidden[1]),  K1 = max(hidden[0], hidden[2])
//   K = 64, hidden 512-256: 49,856 B at TM = 16;  K = 4, hidden 16: 2,752 B at TM = 16.
// Tile rule (dtfk_dfm_tile): the Wide&Deep evaluation's as it stands, not measured here.
#include "common.h"
#include "deepfm.h"
#include "wide_deep_rows.h"

namespace dtfk {
namespace dfm {

using namespace wde;

constexpr int GS = 16;                          // table-row loads in flight per lane

template <int TM, bool TRAIN>
__global__ __launch_bounds__(THREADS) void dfm_rows(const wdt::Args ta) {
  extern __shared__ float4 dfm_smem[];
  __shared__ float fm_s[TM];
  __shared__ int bad_s[TM];
  __shared__ float dz_s[TM];
  const wde::Args& a = ta.f;
  float* buf0 = reinterpret_cast<float*>(dfm_smem);
  float* buf1 = buf0 + TM * a.ld0;
  const int lane = threadIdx.x & 63, w = uni((int)(threadIdx.x >> 6));
  const long long row0 = (long long)blockIdx.x * TM;
  const int K0 = a.D, K16 = (K0 + 15) & ~15, B = a.B;
  const long long F = a.F;

  // ---- bags: S in buf0, the FM score and the bad-id count per row
  {
    constexpr int RPW = TM / NW;                                       // rows per wave
    const int lsh = a.lsh, LPR = 1 << lsh, EP = 64 >> lsh;
    const int sub = lane & (LPR - 1), q = lane >> lsh;
    const int colc = min(4 * sub, K0 - 4);
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
#pragma unroll 1
    for (int i = 0; i < RPW; ++i) {
      const int rr = w + NW * i;
      long long sn = 0, en = 0;
      if (i + 1 < RPW) row_range(i + 1, sn, en);
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), sq = make_float4(0.f, 0.f, 0.f, 0.f);
      float wacc = 0.f;
      int nbad = 0;
      long long c = s;
      do {
        const int cnt = (int)max(0LL, min(64LL, e - c));               // 0: an empty row
        // the next chunk, of this row or the first of the next one, before this chunk's table rows
        const long long nc = c + 64;
        const bool more = nc < e;
        const long long ns = more ? nc : sn, ne = more ? e : en;
        const Chunk nxt = load_chunk(a, ns, (int)max(0LL, min(64LL, ne - ns)), lane);
        const bool in = lane < cnt;
        const bool ok = in && cur.raw >= 0 && cur.raw < F;             // out of range: skipped for both parts
        const long long id = ok ? cur.raw : -1;
        const float v = ok ? cur.v : 0.f;
        nbad += (in && !ok) ? 1 : 0;
        const float wt = a.Wt[ok ? cur.raw : 0];
        const int idlo = (int)(unsigned)id, idhi = (int)(id >> 32), vbits = __float_as_int(v);
        const int nsteps = (cnt + EP - 1) >> (6 - lsh);
        for (int t0 = 0; t0 < nsteps; t0 += GS) {
          float4 x[GS];
          float vv[GS];
          bool on[GS];
#pragma unroll
          for (int u = 0; u < GS; ++u) {                               // step t: entry t EP + q, for every q
            const int src = min(min(t0 + u, nsteps - 1) * EP + q, 63); // (a lane >= cnt holds id = -1)
            const int lo = __shfl(idlo, src, 64), hi = __shfl(idhi, src, 64);
            vv[u] = __int_as_float(__shfl(vbits, src, 64));
            on[u] = hi >= 0 && t0 + u < nsteps;                        // skipped entries and steps past the chunk: row 0, unused
            const unsigned long long rid = hi >= 0 ? (((unsigned long long)(unsigned)hi << 32) | (unsigned)lo) : 0ull;
            x[u] = *reinterpret_cast<const float4*>(a.E + (size_t)rid * K0 + colc);
          }
#pragma unroll
          for (int u = 0; u < GS; ++u) {
            const float tx = on[u] ? vv[u] * x[u].x : 0.f, ty = on[u] ? vv[u] * x[u].y : 0.f;
            const float tz = on[u] ? vv[u] * x[u].z : 0.f, tw = on[u] ? vv[u] * x[u].w : 0.f;
            acc.x += tx; acc.y += ty; acc.z += tz; acc.w += tw;
            sq.x = fmaf(tx, tx, sq.x); sq.y = fmaf(ty, ty, sq.y); sq.z = fmaf(tz, tz, sq.z); sq.w = fmaf(tw, tw, sq.w);
          }
        }
        wacc = ok ? fmaf(wt, v, wacc) : wacc;
        cur = nxt;
        c = nc;
      } while (c < e);
      for (int off = LPR; off < 64; off <<= 1) {                       // the EP partial rows of a column block
        acc.x += __shfl_xor(acc.x, off, 64); acc.y += __shfl_xor(acc.y, off, 64);
        acc.z += __shfl_xor(acc.z, off, 64); acc.w += __shfl_xor(acc.w, off, 64);
        sq.x += __shfl_xor(sq.x, off, 64); sq.y += __shfl_xor(sq.y, off, 64);
        sq.z += __shfl_xor(sq.z, off, 64); sq.w += __shfl_xor(sq.w, off, 64);
      }
      // every lane now holds S and Q of column block `sub`; lane l < K / 4 speaks for block l,
      // lanes K / 4 .. K16 / 4 write the padding
      const bool colown = 4 * lane < K0;
      if (4 * lane < K16)
        *reinterpret_cast<float4*>(buf0 + rr * a.ld0 + 4 * lane) = colown ? acc : make_float4(0.f, 0.f, 0.f, 0.f);
      float pair = 0.f;
      if (colown)
        pair = 0.5f * (((acc.x * acc.x - sq.x) + (acc.y * acc.y - sq.y)) + ((acc.z * acc.z - sq.z) + (acc.w * acc.w - sq.w)));
      pair = wave_sum(pair);
      wacc = wave_sum(wacc);
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) nbad += __shfl_xor(nbad, off, 64);
      if (lane == 0) {
        fm_s[rr] = wacc + pair;
        bad_s[rr] = nbad;
      }
      s = sn;
      e = en;
    }
  }
  __syncthreads();
  const int rows = (int)min((long long)TM, B - row0);                  // the tile's rows inside the batch (>= 1)

  // act[0] = S: the tile's rows, 16 bytes per thread
  if constexpr (TRAIN) {
    const int q4 = K0 >> 2;
    float* g0 = ta.act[0] + (size_t)row0 * K0;
    for (int i = threadIdx.x; i < rows * q4; i += THREADS) {
      const int rr = i / q4, c = 4 * (i - rr * q4);
      *reinterpret_cast<float4*>(g0 + (size_t)rr * K0 + c) = *reinterpret_cast<const float4*>(buf0 + rr * a.ld0 + c);
    }
  }

  // ---- tower forward: hidden layers, ping-pong between the two buffers; TRAIN: act[l + 1] stored
  const int nh = a.nl - 1;
  float* in = buf0;
  float* out = buf1;
  int ldi = a.ld0, ldo = a.ld1;
#pragma unroll
  for (int l = 0; l < MAXL - 1; ++l) {
    if (l < nh) {                                                      // (workgroup-uniform)
      const int K = a.dims[l], N = a.dims[l + 1];
      float* gl = nullptr;
      if constexpr (TRAIN) gl = ta.act[l + 1] + (size_t)row0 * N;
      if (K & 15) layer<TM, true, TRAIN>(in, ldi, out, ldo, a.W[l], a.b[l], K, N, w, lane, gl, rows);
      else layer<TM, false, TRAIN>(in, ldi, out, ldo, a.W[l], a.b[l], K, N, w, lane, gl, rows);
      __syncthreads();
      float* tp = in; in = out; out = tp;
      const int tl = ldi; ldi = ldo; ldo = tl;
    }
  }

  // ---- the width-1 last layer and the head: a wave per row; TRAIN: dz and dzl[nh] = dz w_last * (act[nh] > 0) in place
  const int KL = a.dims[nh];
  const float* wl = a.W[nh];
  const float bl = a.b[nh][0], bias = a.bias[0];
  for (int rr = w; rr < TM; rr += NW) {
    float acc = 0.f;
    for (int k = lane; k < KL; k += 64) acc = fmaf(in[rr * ldi + k], wl[k], acc);
    acc = wave_sum(acc);
    const long long row = row0 + rr;
    float dz = 0.f;                                                    // rows >= B: no gradient
    if (rr < rows) {                                                   // (wave-uniform)
      const float t = acc + bl;
      const float z = (fm_s[rr] + t) + bias;
      const float y = a.labels[row];
      const float p = 1.f / (1.f + __expf(-z));
      dz = (p - y) * ta.gscale;
      if (lane == 0) {
        a.lrow[row] = xent(z, y);
        a.brow[row] = bad_s[rr];
        if (a.z_out != nullptr) a.z_out[row] = z;
        if constexpr (TRAIN) {
          ta.dz[row] = dz;
        } else {
          a.prow[row] = p;
          if (a.p_out != nullptr) a.p_out[row] = p;
        }
      }
    }
    if constexpr (TRAIN) {
      if (lane == 0) dz_s[rr] = dz;
      float* gl = ta.dzl[nh] + (size_t)row0 * KL;
      for (int k = lane; k < KL; k += 64) {
        const float h = in[rr * ldi + k];
        const float gk = h > 0.f ? dz * wl[k] : 0.f;
        in[rr * ldi + k] = gk;
        if (rr < rows) gl[(size_t)rr * KL + k] = gk;
      }
    }
  }
  if constexpr (TRAIN) {
    __syncthreads();

    // ---- backward through the hidden layers: da_l = dzl[l + 1] W_l^T, into the buffer that held act[l]
#pragma unroll
    for (int l = MAXL - 2; l >= 0; --l) {
      if (l < nh) {                                                      // (workgroup-uniform)
        const int K = a.dims[l], N = a.dims[l + 1];
        if (l == 0) {
          // demb = da_0 + dz S, S from the tile's own act[0] rows
          layer_bwd<TM, true, false, true>(in, ldi, out, ldo, a.W[0], K, N, w, lane, ta.act[0] + (size_t)row0 * K,
                                           ta.demb + (size_t)row0 * K, rows, dz_s);
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
}

constexpr size_t STATIC_LDS = 12;               // bytes per tile row: fm_s, bad_s, dz_s

template <int TM, bool TRAIN>
static hipError_t launch(const wdt::Args& a, size_t lds, hipStream_t stream) {
  static bool raised = false;   // dynamic LDS beyond 64 KiB needs the attribute (once per kernel)
  if (!raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&dfm_rows<TM, TRAIN>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (int)STATIC_LDS * TM);
    if (e != hipSuccess) return e;
    raised = true;
  }
  const unsigned grid = (unsigned)(((long long)a.f.B + TM - 1) / TM);
  hipLaunchKernelGGL((dfm_rows<TM, TRAIN>), dim3(grid), dim3(THREADS), lds, stream, a);
  return hipGetLastError();
}

}  // namespace dfm
}  // namespace dtfk

extern "C" {

int dtfk_dfm_supported(int K, int nl, const int* dims) { return dtfk_wd_eval_supported(K, nl, dims); }

int dtfk_dfm_tile(int B, int nl, const int* dims) { return dtfk_wd_eval_tile(B, nl, dims); }

long long dtfk_dfm_lds_bytes(int K, int nl, const int* dims, int tile) {
  int ld0, ld1;
  dtfk::wde::strides(K, nl, dims, ld0, ld1);
  return 4LL * tile * (ld0 + ld1) + (long long)dtfk::dfm::STATIC_LDS * tile;
}

hipError_t dtfk_dfm_rows(const dtfk::wdt::Args* p, int train, int tile, hipStream_t stream) {
  using namespace dtfk;
  if (p == nullptr) return hipErrorInvalidValue;
  const wde::Args& f = p->f;
  if (f.B < 1 || f.F < 1 || f.mode != 0 || !dtfk_dfm_supported(f.D, f.nl, f.dims)) return hipErrorInvalidValue;
  // (ids may be null: a batch of empty rows has no entries, and none is read)
  if (f.Wt == nullptr || f.E == nullptr || f.offsets == nullptr || f.labels == nullptr || f.bias == nullptr ||
      f.lrow == nullptr || f.brow == nullptr)
    return hipErrorInvalidValue;
  if (train ? (f.z_out == nullptr || p->dz == nullptr || p->demb == nullptr) : f.prow == nullptr)
    return hipErrorInvalidValue;
  // table rows, the hidden layers' weights and biases, and the [B, width] outputs move 16 bytes at a time
  uintptr_t al = reinterpret_cast<uintptr_t>(f.E);
  if (train) al |= reinterpret_cast<uintptr_t>(p->demb);
  for (int l = 0; l < f.nl; ++l) {
    if (f.W[l] == nullptr || f.b[l] == nullptr) return hipErrorInvalidValue;
    if (l < f.nl - 1) al |= reinterpret_cast<uintptr_t>(f.W[l]) | reinterpret_cast<uintptr_t>(f.b[l]);
    if (!train) continue;
    if (p->act[l] == nullptr || (l >= 1 && p->dzl[l] == nullptr)) return hipErrorInvalidValue;
    al |= reinterpret_cast<uintptr_t>(p->act[l]);
    if (l >= 1) al |= reinterpret_cast<uintptr_t>(p->dzl[l]);
  }
  if (al & 15) return hipErrorInvalidValue;
  if (tile == 0) tile = dtfk_dfm_tile(f.B, f.nl, f.dims);
  if (tile != 16 && tile != 32) return hipErrorInvalidValue;
  wdt::Args a = *p;
  wde::strides(f.D, f.nl, f.dims, a.f.ld0, a.f.ld1);
  const size_t lds = 4 * (size_t)tile * (size_t)(a.f.ld0 + a.f.ld1);
  if (lds + dfm::STATIC_LDS * (size_t)tile > 160 * 1024) return hipErrorInvalidValue;
  a.f.lsh = 0;
  while ((4 << a.f.lsh) < f.D) ++a.f.lsh;   // LPR = 2^lsh lanes of 16 bytes cover a table row
  if (train) return tile == 16 ? dfm::launch<16, true>(a, lds, stream) : dfm::launch<32, true>(a, lds, stream);
  return tile == 16 ? dfm::launch<16, false>(a, lds, stream) : dfm::launch<32, false>(a, lds, stream);
}

}  // extern "C"
