// Reached by: DeepFMPlan(num_fields = P) (csrc/bind_deepfm.cpp), models/deepfm.py DeepFMTrainer(num_fields = P);
// tests/test_deepfm_fields_gpu.py, scripts/bench_fm.py --tower-fields
// DeepFM (Guo et al. 2017) with fields on one GPU: the tower reads the concatenation of
// the per-field embeddings, the FM term all of the row's entries.  A batch is the
// (row, field) bag form of ffm.hip: bag r P + p holds row r's entries of field p.
//
//   A_r[p]  = sum_{i in bag (r, p)} x_i V[id_i, :]                     (K wide; 0 for an empty bag)
//   S_r     = sum_p A_r[p]        Q_r[f] = sum_i x_i^2 V[id_i, f]^2    (over all of the row's entries)
//   fm_r    = sum_i x_i w[id_i] + 0.5 sum_f (S_r[f]^2 - Q_r[f])
//   a_0     = [A_r[0] | ... | A_r[P - 1]]  (P K wide);  a_l, t_r, z_r, loss_r, dz_r, dzl[l], da_l: deepfm.hip's
//   demb[r P + p, :] = dz_r S_r + da_0,r[p K : (p + 1) K]
//
// demb laid out [B, P K] is the [B P, K] bag gradient of fm.hip's one-writer update, byte for
// byte, and dzbag [B P] (dz_r once per bag) its linear gradient and the source of q_j.
//
//   dfmf_rows<TM, TRAIN>  one workgroup (4 waves) per tile of TM = 16 or 32 batch rows.
//     bags    wave w takes rows w, w + 4, ... of the tile and streams a row's entries through
//             all P bags in CSR order (they are contiguous, offsets[r P] .. offsets[(r + 1) P]).
//             Lane q < P holds the row's bag offset q (the row's end is a scalar of its own, so
//             P = 64 fits a wave); the next row's offsets are loaded while
//             this row's entries stream.  Entries arrive 64 at a time, one id / value / w[id]
//             per lane, and the next chunk -- of this row, or the first of the wave's next row --
//             is requested before the current chunk's table rows.  A lane finds its entry's
//             field by counting the bag offsets at or below its position.  A table row of K
//             floats is read by LPR = 2^lsh >= K / 4 adjacent lanes, 16 bytes each: one load
//             instruction (a step) fetches the rows of EP = 64 / LPR consecutive entries,
//             GS = 16 steps are issued back to back whatever bags the entries lie in.
//             x v of a step goes two ways.  (1) Every lane adds it, and its square, to two
//             float4 register sums kept over the whole row: S and Q after one __shfl_xor fold
//             (dfm_rows's arithmetic).  (2) The entries of a step that share a bag are
//             consecutive slots and are combined by a segmented Hillis-Steele scan over the
//             slots (skipped, wave-uniformly, for a chunk with one entry per bag); the last
//             slot of each run adds the run's sum to the bag's K columns of the row's LDS tile
//             row (read, add, write).  One step has one writer per bag and the steps follow
//             each other in program order: no atomics, and the order depends only on the
//             batch's layout, so two runs give the same bits.  The tile row, padding columns
//             P K .. ceil16(P K) included, is zeroed by its wave first.
//             S goes to a [TM, K] LDS area after the tower's two buffers, the FM score and the
//             bad-id count to one LDS word per row.
//     tower, head   dfm_rows's, with dims[0] = P K; TRAIN stores act[0] (the concatenation),
//             S [B, K] and dzbag besides dz.
//     backward      wide_deep_rows.h's layer_bwd; the first layer's epilogue (FIELDS) adds
//             dz_s[row] S[row][col mod K .. + 3] from the LDS S area to each of the P blocks.
//
// Ragged edges: rows >= B are rows of empty bags with dz = 0, and nothing of them is stored;
// clamped lanes re-read valid bytes and do not store; nothing is read or written past the
// last row, bag, id or column.  No inter-workgroup waits, no float atomics.
//
// LDS: bytes = 4 TM ((K0 + 4) + (K1 + 4)) + 4 TM K + 12 TM,
//     K0 = max(ceil16(P K), hidden[1]),  K1 = max(hidden[0], hidden[2])
//   P = 39, K = 8, hidden 512-256: 54,464 B at TM = 16;  P = 4, K = 128, hidden 64-32-16: 91,520 B at TM = 32.
// Tile rule: dtfk_dfm_tile's (the Wide&Deep evaluation's), not measured for this kernel.
#include "common.h"
#include "deepfm.h"
#include "deepfm_fields.h"
#include "wide_deep_rows.h"

namespace dtfk {
namespace dfmf {

using namespace wde;

constexpr int GS = 16;                          // steps (table-row loads) in flight per lane

// LDS accesses of the wave before this point are done before those after it, in every lane
__device__ __forceinline__ void lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// lane i's 64-bit value, as a wave-uniform one
__device__ __forceinline__ long long lane_ll(long long v, int i) {
  const int lo = (int)(unsigned)v, hi = (int)(v >> 32);
  return (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, i) << 32) |
                     (unsigned)__builtin_amdgcn_readlane(lo, i));
}

// what a lane knows of its entry, in one word for one shuffle
constexpr int PK_TAIL = 1 << 6, PK_OK = 1 << 7, PK_IN = 1 << 14;      // field: bits 0 .. 5, run start: bits 8 .. 13

template <int TM, bool TRAIN>
__global__ __launch_bounds__(THREADS) void dfmf_rows(const Args fa) {
  extern __shared__ float4 dfmf_smem[];
  __shared__ float fm_s[TM];
  __shared__ int bad_s[TM];
  __shared__ float dz_s[TM];
  const wdt::Args& ta = fa.t;
  const wde::Args& a = ta.f;
  float* buf0 = reinterpret_cast<float*>(dfmf_smem);
  float* buf1 = buf0 + TM * a.ld0;
  float* S_s = buf1 + TM * a.ld1;                                      // [TM][K]
  const int lane = threadIdx.x & 63, w = uni((int)(threadIdx.x >> 6));
  const long long row0 = (long long)blockIdx.x * TM;
  const int P = fa.P, K = a.D, W0 = a.dims[0], W16 = (W0 + 15) & ~15, B = a.B;
  const long long F = a.F;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // ---- bags: the P per-field sums in buf0, S in S_s, the FM score and the bad-id count per row
  {
    constexpr int RPW = TM / NW;                                       // rows per wave
    const int lsh = a.lsh, LPR = 1 << lsh, EP = 64 >> lsh;
    const int sub = lane & (LPR - 1), q = lane >> lsh;
    const bool colact = 4 * sub < K;                                   // the lanes past K / 4 re-read the last block
    const int col = min(4 * sub, K - 4);
    // row w + NW i's bag offsets 0 .. P - 1, one per lane (lanes >= P: the last of them again), and its end, offset
    // P, as a wave-uniform value of its own (P = 64 leaves no lane for it); rows >= B: empty bags
    auto bag_offsets = [&](int i) {
      const long long row = row0 + w + NW * i;
      return a.offsets[row < B ? row * P + min(lane, P - 1) : (long long)B * P];
    };
    auto row_end = [&](int i) {
      const long long row = row0 + w + NW * i;
      return uni(a.offsets[min(row + 1, (long long)B) * P]);
    };
    long long bo = bag_offsets(0);
    long long s = lane_ll(bo, 0), e = row_end(0);
    Chunk cur = load_chunk(a, s, (int)max(0LL, min(64LL, e - s)), lane);
#pragma unroll 1
    for (int i = 0; i < RPW; ++i) {
      const int rr = w + NW * i;
      long long bon = bo, sn = 0, en = 0;
      if (i + 1 < RPW) {
        bon = bag_offsets(i + 1);
        sn = lane_ll(bon, 0);
        en = row_end(i + 1);
      }
      float* __restrict__ A = buf0 + rr * a.ld0;
      for (int c4 = lane; 4 * c4 < W16; c4 += 64) *reinterpret_cast<f32x4*>(A + 4 * c4) = zero;
      lds_order();
      f32x4 acc = zero, sq = zero;
      float wacc = 0.f;
      int nbad = 0;
      long long c = s;
      do {
        const int cnt = (int)max(0LL, min(64LL, e - c));               // 0: a row without entries
        // the next chunk, of this row or the first of the next one, before this chunk's table rows
        const long long nc = c + 64;
        const bool more = nc < e;
        const long long ns = more ? nc : sn, ne = more ? e : en;
        const Chunk nxt = load_chunk(a, ns, (int)max(0LL, min(64LL, ne - ns)), lane);
        const bool in = lane < cnt;
        const bool ok = in && cur.raw >= 0 && cur.raw < F;             // out of range: skipped for every part
        const long long id = ok ? cur.raw : 0;
        const float v = ok ? cur.v : 0.f;
        nbad += (in && !ok) ? 1 : 0;
        const float wt = a.Wt[id];
        // the field of this lane's entry: the bag offsets 1 .. P - 1 at or below its position
        const int rel = (int)max(0LL, min(64LL, bo - c));
        int p = 0;
        for (int f = 1; f < P; ++f) p += lane >= __builtin_amdgcn_readlane(rel, f) ? 1 : 0;
        // runs of one bag inside the chunk
        const int pprev = __shfl_up(p, 1, 64), pnext = __shfl_down(p, 1, 64);
        const unsigned long long heads = __ballot(lane == 0 || pprev != p);
        const unsigned long long live = cnt == 64 ? ~0ull : (1ull << cnt) - 1;
        const bool multi = (heads & live) != live;                     // some bag holds two entries of the chunk
        const int rs = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));
        const bool tail = lane == cnt - 1 || pnext != p;
        const int pkall = in ? (p | (tail ? PK_TAIL : 0) | (ok ? PK_OK : 0) | (rs << 8) | PK_IN) : 0;
        const int idlo = (int)(unsigned)id, idhi = (int)(id >> 32), vbits = __float_as_int(v);
        const int nsteps = (cnt + EP - 1) >> (6 - lsh);
        for (int t0 = 0; t0 < nsteps; t0 += GS) {
          f32x4 x[GS];
          float vv[GS];
          int pk[GS];
#pragma unroll
          for (int u = 0; u < GS; ++u) {                               // step t: entry t EP + q, for every slot q
            const int src = min(min(t0 + u, nsteps - 1) * EP + q, 63);
            const int lo = __shfl(idlo, src, 64), hi = __shfl(idhi, src, 64);
            vv[u] = __int_as_float(__shfl(vbits, src, 64));
            pk[u] = __shfl(pkall, src, 64);                            // (skipped entries and lanes past the chunk: row 0, unused)
            const unsigned long long rid = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
            x[u] = *reinterpret_cast<const f32x4*>(a.E + (size_t)rid * K + col);
          }
#pragma unroll
          for (int u = 0; u < GS; ++u) {
            if (t0 + u >= nsteps) break;                               // (wave-uniform)
            const int src = (t0 + u) * EP + q;
            f32x4 t = (pk[u] & PK_OK) ? vv[u] * x[u] : zero;
            acc += t;                                                  // S and Q: the row's register sums
#pragma unroll
            for (int k = 0; k < 4; ++k) sq[k] = fmaf(t[k], t[k], sq[k]);
            if (multi) {
              const int st = (pk[u] >> 8) & 63;
              for (int off = 1; off < EP; off <<= 1) {                 // segmented scan over the step's slots
                f32x4 up;
#pragma unroll
                for (int k = 0; k < 4; ++k) up[k] = __shfl_up(t[k], off << lsh, 64);
                if (q >= off && st <= src - off) t += up;
              }
            }
            if ((pk[u] & PK_IN) && colact && ((pk[u] & PK_TAIL) || q == EP - 1)) {
              f32x4* ap = reinterpret_cast<f32x4*>(A + (pk[u] & 63) * K + 4 * sub);
              *ap = *ap + t;
            }
            lds_order();
          }
        }
        wacc = ok ? fmaf(wt, v, wacc) : wacc;
        cur = nxt;
        c = nc;
      } while (c < e);
      for (int off = LPR; off < 64; off <<= 1) {                       // the EP partial rows of a column block
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc[k] += __shfl_xor(acc[k], off, 64);
          sq[k] += __shfl_xor(sq[k], off, 64);
        }
      }
      // every lane now holds S and Q of column block `sub`; lane l < K / 4 speaks for block l
      const bool colown = 4 * lane < K;
      float pair = 0.f;
      if (colown) {
        *reinterpret_cast<f32x4*>(S_s + rr * K + 4 * lane) = acc;
        pair = 0.5f * (((acc[0] * acc[0] - sq[0]) + (acc[1] * acc[1] - sq[1])) +
                       ((acc[2] * acc[2] - sq[2]) + (acc[3] * acc[3] - sq[3])));
      }
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
      bo = bon;
    }
  }
  __syncthreads();
  const int rows = (int)min((long long)TM, B - row0);                  // the tile's rows inside the batch (>= 1)

  // act[0] = the concatenation and S: the tile's rows, 16 bytes per thread
  if constexpr (TRAIN) {
    const int q4 = W0 >> 2, k4 = K >> 2;
    float* g0 = ta.act[0] + (size_t)row0 * W0;
    for (int i = threadIdx.x; i < rows * q4; i += THREADS) {
      const int rr = i / q4, c = 4 * (i - rr * q4);
      *reinterpret_cast<float4*>(g0 + (size_t)rr * W0 + c) = *reinterpret_cast<const float4*>(buf0 + rr * a.ld0 + c);
    }
    float* gs = fa.S + (size_t)row0 * K;
    for (int i = threadIdx.x; i < rows * k4; i += THREADS)
      *reinterpret_cast<float4*>(gs + 4 * (size_t)i) = *reinterpret_cast<const float4*>(S_s + 4 * i);
  }

  // ---- tower forward: hidden layers, ping-pong between the two buffers; TRAIN: act[l + 1] stored
  const int nh = a.nl - 1;
  float* in = buf0;
  float* out = buf1;
  int ldi = a.ld0, ldo = a.ld1;
#pragma unroll
  for (int l = 0; l < MAXL - 1; ++l) {
    if (l < nh) {                                                      // (workgroup-uniform)
      const int Kl = a.dims[l], N = a.dims[l + 1];
      float* gl = nullptr;
      if constexpr (TRAIN) gl = ta.act[l + 1] + (size_t)row0 * N;
      if (Kl & 15) layer<TM, true, TRAIN>(in, ldi, out, ldo, a.W[l], a.b[l], Kl, N, w, lane, gl, rows);
      else layer<TM, false, TRAIN>(in, ldi, out, ldo, a.W[l], a.b[l], Kl, N, w, lane, gl, rows);
      __syncthreads();
      float* tp = in; in = out; out = tp;
      const int tl = ldi; ldi = ldo; ldo = tl;
    }
  }

  // ---- the width-1 last layer and the head: a wave per row; TRAIN: dz, dzbag and dzl[nh] = dz w_last * (act[nh] > 0) in place
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
      if constexpr (TRAIN) {
        if (lane < P) fa.dzbag[row * P + lane] = dz;
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
        const int Kl = a.dims[l], N = a.dims[l + 1];
        if (l == 0) {
          // demb = da_0 + dz S on each of the P blocks, S from the LDS area
          layer_bwd<TM, true, false, true, true>(in, ldi, out, ldo, a.W[0], Kl, N, w, lane, S_s,
                                                 ta.demb + (size_t)row0 * Kl, rows, dz_s, K);
        } else {
          float* gd = ta.dzl[l] + (size_t)row0 * Kl;
          // act[l] is still in `out` unless act[l + 2] was written over it
          if (l + 2 <= nh)
            layer_bwd<TM, false, true>(in, ldi, out, ldo, a.W[l], Kl, N, w, lane, ta.act[l] + (size_t)row0 * Kl, gd, rows);
          else
            layer_bwd<TM, false, false>(in, ldi, out, ldo, a.W[l], Kl, N, w, lane, nullptr, gd, rows);
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
static hipError_t launch(const Args& a, size_t lds, hipStream_t stream) {
  static bool raised = false;   // dynamic LDS beyond 64 KiB needs the attribute (once per kernel)
  if (!raised) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&dfmf_rows<TM, TRAIN>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (int)STATIC_LDS * TM);
    if (e != hipSuccess) return e;
    raised = true;
  }
  const unsigned grid = (unsigned)(((long long)a.t.f.B + TM - 1) / TM);
  hipLaunchKernelGGL((dfmf_rows<TM, TRAIN>), dim3(grid), dim3(THREADS), lds, stream, a);
  return hipGetLastError();
}

// dynamic LDS bytes: the two activation buffers and the S area
static size_t dynamic_lds(int P, int K, int nl, const int* dims, int tile, int& ld0, int& ld1) {
  strides(P * K, nl, dims, ld0, ld1);
  return 4 * (size_t)tile * (size_t)(ld0 + ld1 + K);
}

}  // namespace dfmf
}  // namespace dtfk

extern "C" {

int dtfk_dfmf_supported(int P, int K, int nl, const int* dims) {
  using namespace dtfk;
  if (K < 4 || K > wde::MAXD || (K & 3) || P < 1 || P > dfmf::MAXP || P * K > wde::MAXW) return 0;
  if (nl < 2 || nl > wde::MAXL || dims == nullptr || dims[0] != P * K || dims[nl] != 1) return 0;
  for (int l = 1; l < nl; ++l)
    if (dims[l] < 16 || dims[l] > wde::MAXW || (dims[l] & 15)) return 0;
  return 1;
}

long long dtfk_dfmf_lds_bytes(int P, int K, int nl, const int* dims, int tile) {
  int ld0, ld1;
  return (long long)dtfk::dfmf::dynamic_lds(P, K, nl, dims, tile, ld0, ld1) + (long long)dtfk::dfmf::STATIC_LDS * tile;
}

hipError_t dtfk_dfmf_rows(const dtfk::dfmf::Args* p, int train, int tile, hipStream_t stream) {
  using namespace dtfk;
  if (p == nullptr) return hipErrorInvalidValue;
  const wdt::Args& t = p->t;
  const wde::Args& f = t.f;
  if (f.B < 1 || f.F < 1 || f.mode != 0 || !dtfk_dfmf_supported(p->P, f.D, f.nl, f.dims) ||
      (long long)f.B * p->P >= (1ll << 31))
    return hipErrorInvalidValue;
  // (ids may be null: a batch of empty bags has no entries, and none is read)
  if (f.Wt == nullptr || f.E == nullptr || f.offsets == nullptr || f.labels == nullptr || f.bias == nullptr ||
      f.lrow == nullptr || f.brow == nullptr)
    return hipErrorInvalidValue;
  if (train ? (f.z_out == nullptr || t.dz == nullptr || t.demb == nullptr || p->S == nullptr || p->dzbag == nullptr)
            : f.prow == nullptr)
    return hipErrorInvalidValue;
  // table rows, the hidden layers' weights and biases, and the [B, width] outputs move 16 bytes at a time
  uintptr_t al = reinterpret_cast<uintptr_t>(f.E);
  if (train) al |= reinterpret_cast<uintptr_t>(t.demb) | reinterpret_cast<uintptr_t>(p->S);
  for (int l = 0; l < f.nl; ++l) {
    if (f.W[l] == nullptr || f.b[l] == nullptr) return hipErrorInvalidValue;
    if (l < f.nl - 1) al |= reinterpret_cast<uintptr_t>(f.W[l]) | reinterpret_cast<uintptr_t>(f.b[l]);
    if (!train) continue;
    if (t.act[l] == nullptr || (l >= 1 && t.dzl[l] == nullptr)) return hipErrorInvalidValue;
    al |= reinterpret_cast<uintptr_t>(t.act[l]);
    if (l >= 1) al |= reinterpret_cast<uintptr_t>(t.dzl[l]);
  }
  if (al & 15) return hipErrorInvalidValue;
  if (tile == 0) tile = dtfk_dfm_tile(f.B, f.nl, f.dims);
  if (tile != 16 && tile != 32) return hipErrorInvalidValue;
  dfmf::Args a = *p;
  const size_t lds = dfmf::dynamic_lds(p->P, f.D, f.nl, f.dims, tile, a.t.f.ld0, a.t.f.ld1);
  if (lds + dfmf::STATIC_LDS * (size_t)tile > 160 * 1024) return hipErrorInvalidValue;
  a.t.f.lsh = 0;
  while ((4 << a.t.f.lsh) < f.D) ++a.t.f.lsh;   // LPR = 2^lsh lanes of 16 bytes cover a table row
  if (train) return tile == 16 ? dfmf::launch<16, true>(a, lds, stream) : dfmf::launch<32, true>(a, lds, stream);
  return tile == 16 ? dfmf::launch<16, false>(a, lds, stream) : dfmf::launch<32, false>(a, lds, stream);
}

}  // extern "C"
