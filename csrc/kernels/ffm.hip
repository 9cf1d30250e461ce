// Reached by: FFMPlan (csrc/bind_ffm.cpp), models/ffm.py FFMTrainer; tests/test_ffm_gpu.py
// The field-aware factorization machine on one GPU (Juan et al. 2016), entries of one
// field sum-pooled.  A batch is a CSR over (row, field) bags: bag r P + p holds row r's
// entries of field p.  With V[j, q K : (q + 1) K] feature j's vector aimed at field q:
//
//   A_r[p][q, :] = sum_{i in bag (r, p)} x_i V[id_i, q K : (q + 1) K]
//   z_r          = b + sum_i x_i w[id_i] + sum_{p < q} < A_r[p][q, :], A_r[q][p, :] >
//
// ffm_rows<TRAIN>: one wave per batch row.  The wave's tile A[P][P K] lives in LDS, in
// rows of `stride` floats; 3 or 4 waves per workgroup, as many as fit in 64 KB
// (dtfk_ffm_tile_bytes), and no workgroup barrier: a wave only ever touches its own tile.
//   * Lane q <= P holds the row's bag offset q.  Entries arrive in chunks of 64, one id /
//     value / w[id] per lane; the next chunk is requested before the current chunk's
//     table rows.  A lane finds its entry's field by counting the bag offsets at or below
//     its position (P - 1 readlanes per chunk).
//   * A table row of P K floats is read by LPR = 2^lsh >= P K / 4 adjacent lanes, 16 bytes
//     each, so one load instruction fetches the rows of EP = 64 / LPR consecutive entries
//     (a step); GS = 16 steps are issued back to back before the first use, whatever bags
//     the entries lie in.
//   * x v goes to tile row p in a fixed order: the entries of one step that share a bag
//     are consecutive slots and are combined by a segmented Hillis-Steele scan over the
//     slots (skipped, wave-uniformly, for a chunk with one entry per bag); the last slot
//     of each run adds the run's sum to its tile row (LDS read, add, write).  One step has
//     one writer per tile row and the steps follow each other in program order, so there
//     are no atomics and the order depends only on the batch's layout: the same batch
//     gives the same bits on every run.
//   * The pair term: a half wave per tile row p (two rows per pass), lane c of it owns the
//     16-byte block c of the row, that is field q = 4 c / K and factors koff .. koff + 3;
//     for q > p it multiplies the block by the transposed one, A[q][p K + koff ..], four
//     fmaf per pass, then wave_sum.  The longest chain of rounded additions is therefore
//     4 ceil(P / 2) + 6.  The transposed reads of a half wave are `stride` floats apart
//     per field: stride = P K + K for an even P and P K for an odd one, so stride / K is
//     odd and the K-float blocks of consecutive fields fall on distinct banks (a stride of
//     P K = 128 floats would put all of them on the same ones).
//   * TRAIN: dz_r = (sigmoid(z_r) - y_r) gscale, once per row and once per bag, and the bag
//     gradients G[(r, p)][q K ..] = dz_r A_r[q][p K ..] (0 for q == p), read from the tile
//     by the same transposed blocks and stored as coalesced 16-byte rows.  They are what
//     table_update.h's update takes as demb over B P bags; same-field pairs do not
//     interact, so the gradient has no self term and needs none of the FM form's q_j.
// Ids outside [0, F) are skipped and counted per batch row.
// MFMA does not fit: every product pairs two blocks of one row's own tile, there is no
// operand shared across rows to put into a matrix instruction.
#include "common.h"
#include "ffm.h"

namespace dtfk {
namespace ffm {

constexpr int MAXWAVES = 4;
constexpr int GS = 16;                          // steps (table-row loads) in flight per lane

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// LDS accesses of the wave before this point are done before those after it, in every lane
__device__ __forceinline__ void lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Up to 64 entries, one per lane: the raw id and the value.  Nothing is read for
// cnt == 0; the lanes past the last entry repeat it.
struct Chunk {
  long long raw;
  float v;
};
__device__ __forceinline__ Chunk load_chunk(const RowArgs& a, long long c, int cnt, int lane) {
  Chunk ch{-1, 0.f};
  if (cnt > 0) {                                                       // (wave-uniform)
    const long long j = c + min(lane, cnt - 1);
    ch.raw = a.ids[j];
    ch.v = a.vals != nullptr ? a.vals[j] : 1.f;
  }
  return ch;
}

// what a lane knows of its entry, in one word for one shuffle
constexpr int PK_TAIL = 1 << 6, PK_OK = 1 << 7, PK_IN = 1 << 14;      // field: bits 0 .. 5, run start: bits 8 .. 13

template <bool TRAIN>
__global__ __launch_bounds__(64 * MAXWAVES) void ffm_rows(const RowArgs a, const int lsh, const int stride,
                                                          const int waves) {
  extern __shared__ f32x4 tiles[];
  const int lane = threadIdx.x & 63, wv = uni((int)(threadIdx.x >> 6));
  const long long row = (long long)blockIdx.x * waves + wv;
  if (row >= a.B) return;                                              // (wave-uniform)
  const int P = a.P, K = a.K, W = P * K;
  const long long F = a.F;
  float* __restrict__ A = reinterpret_cast<float*>(tiles) + (size_t)wv * P * stride;
  const int LPR = 1 << lsh, EP = 64 >> lsh;
  const int sub = lane & (LPR - 1), q = lane >> lsh;
  const bool colact = 4 * sub < W;                                     // the lanes past P K / 4 re-read the last block
  const int col = min(4 * sub, W - 4);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  for (int i = lane; i < (P * stride) >> 2; i += 64) reinterpret_cast<f32x4*>(A)[i] = zero;

  // the row's P + 1 bag offsets, one per lane
  long long bo = 0;
  if (lane <= P) bo = a.offsets[row * P + lane];
  const int bolo = (int)(unsigned)bo, bohi = (int)(bo >> 32);
  auto offset_of = [&](int i) {
    return (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(bohi, i) << 32) |
                       (unsigned)__builtin_amdgcn_readlane(bolo, i));
  };
  const long long s = offset_of(0), e = offset_of(P);
  lds_order();

  float wacc = 0.f;
  int nbad = 0;
  Chunk cur = load_chunk(a, s, (int)max(0LL, min(64LL, e - s)), lane);
  for (long long c = s; c < e; c += 64) {
    const int cnt = (int)min(64LL, e - c);
    const long long nc = c + 64;
    const Chunk nxt = load_chunk(a, nc, (int)max(0LL, min(64LL, e - nc)), lane);   // before this chunk's table rows
    const bool in = lane < cnt;
    const bool ok = in && cur.raw >= 0 && cur.raw < F;                 // out of range: skipped for both tables
    const long long id = ok ? cur.raw : 0;
    const float v = ok ? cur.v : 0.f;
    nbad += (in && !ok) ? 1 : 0;
    const float wt = a.w[id];
    // the field of this lane's entry: the bag offsets 1 .. P - 1 at or below its position
    const int rel = (int)max(0LL, min(64LL, bo - c));
    int p = 0;
    for (int f = 1; f < P; ++f) p += lane >= __builtin_amdgcn_readlane(rel, f) ? 1 : 0;
    // runs of one bag inside the chunk
    const int pprev = __shfl_up(p, 1, 64), pnext = __shfl_down(p, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || pprev != p);
    const unsigned long long live = cnt == 64 ? ~0ull : (1ull << cnt) - 1;
    const bool multi = (heads & live) != live;                         // some bag holds two entries of the chunk
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
      for (int u = 0; u < GS; ++u) {                                   // step t: entry t EP + q, for every slot q
        const int src = min(min(t0 + u, nsteps - 1) * EP + q, 63);
        const int lo = __shfl(idlo, src, 64), hi = __shfl(idhi, src, 64);
        vv[u] = __int_as_float(__shfl(vbits, src, 64));
        pk[u] = __shfl(pkall, src, 64);                                // (skipped entries and lanes past the chunk: row 0, unused)
        const unsigned long long rid = ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo;
        x[u] = *reinterpret_cast<const f32x4*>(a.V + (size_t)rid * W + col);
      }
#pragma unroll
      for (int u = 0; u < GS; ++u) {
        if (t0 + u >= nsteps) break;                                   // (wave-uniform)
        const int src = (t0 + u) * EP + q;
        f32x4 t = (pk[u] & PK_OK) ? vv[u] * x[u] : zero;
        if (multi) {
          const int st = (pk[u] >> 8) & 63;
          for (int off = 1; off < EP; off <<= 1) {                     // segmented scan over the step's slots
            f32x4 up;
#pragma unroll
            for (int k = 0; k < 4; ++k) up[k] = __shfl_up(t[k], off << lsh, 64);
            if (q >= off && st <= src - off) t += up;
          }
        }
        if ((pk[u] & PK_IN) && colact && ((pk[u] & PK_TAIL) || q == EP - 1)) {
          f32x4* ap = reinterpret_cast<f32x4*>(A + (pk[u] & 63) * stride + 4 * sub);
          *ap = *ap + t;
        }
        lds_order();
      }
    }
    wacc = ok ? fmaf(wt, v, wacc) : wacc;
    cur = nxt;
  }

  // the pair term: a half wave per tile row, lane c4 of it owns block c4 = (field qf, factors koff .. koff + 3)
  const int half = lane >> 5, c4 = lane & 31, K4 = K >> 2;
  const bool cact = 4 * c4 < W;
  const int qf = cact ? c4 / K4 : 0, koff = cact ? (c4 - qf * K4) * 4 : 0;
  float pair = 0.f;
  for (int p0 = 0; p0 < P; p0 += 2) {
    const int p = p0 + half;
    if (cact && p < P && qf > p) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(A + p * stride + 4 * c4);
      const f32x4 y = *reinterpret_cast<const f32x4*>(A + qf * stride + p * K + koff);
      pair = fmaf(x[0], y[0], pair); pair = fmaf(x[1], y[1], pair);
      pair = fmaf(x[2], y[2], pair); pair = fmaf(x[3], y[3], pair);
    }
  }
  pair = wave_sum(pair);
  wacc = wave_sum(wacc);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nbad += __shfl_xor(nbad, off, 64);
  const float z = (wacc + pair) + a.bias[0];
  const float y = a.labels[row];
  const float pr = 1.f / (1.f + __expf(-z));
  if (lane == 0) {
    a.lrow[row] = xent(z, y);
    a.brow[row] = nbad;
    if (a.prow != nullptr) a.prow[row] = pr;
    if (a.p_out != nullptr) a.p_out[row] = pr;
    if (a.z_out != nullptr) a.z_out[row] = z;
  }
  if constexpr (TRAIN) {
    const float dz = (pr - y) * a.gscale;
    if (lane == 0) a.dz[row] = dz;
    if (lane < P) a.dzbag[row * P + lane] = dz;
    for (int p0 = 0; p0 < P; p0 += 2) {                                // bag (row, p): block qf is dz A[qf][p K ..], transposed
      const int p = p0 + half;
      if (cact && p < P) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(A + qf * stride + p * K + koff);
        *reinterpret_cast<f32x4*>(a.G + (size_t)(row * P + p) * W + 4 * c4) = qf == p ? zero : dz * t;
      }
    }
  }
}

// floats between the tile's rows: stride / K odd (the header comment)
inline int tile_stride(int P, int K) { return P % 2 == 0 ? P * K + K : P * K; }

}  // namespace ffm
}  // namespace dtfk

extern "C" int dtfk_ffm_supported(int P, int K) {
  return K >= 4 && K % 4 == 0 && P >= 2 && P <= dtfk::ffm::MAXP && P * K <= dtfk::ffm::MAXW ? 1 : 0;
}

// As many waves as fit in 64 KB, four at the most: the largest tile, P = 32 and K = 4, is 32 x 132 floats = 16896
// bytes and gets three.  A wave shares nothing with its neighbours, so a larger workgroup would gain nothing, and
// at 160 KB per CU small ones pack better.
extern "C" int dtfk_ffm_tile_bytes(int P, int K, int* waves) {
  if (!dtfk_ffm_supported(P, K)) return 0;
  const int bytes = P * dtfk::ffm::tile_stride(P, K) * 4;
  if (waves != nullptr) *waves = 65536 / bytes < dtfk::ffm::MAXWAVES ? 65536 / bytes : dtfk::ffm::MAXWAVES;
  return bytes;
}

extern "C" hipError_t dtfk_ffm_rows(const dtfk::ffm::RowArgs* a, int train, hipStream_t stream) {
  using namespace dtfk::ffm;
  if (a == nullptr || !dtfk_ffm_supported(a->P, a->K) || a->B < 1 || a->F < 1 || (long long)a->B * a->P >= (1ll << 31))
    return hipErrorInvalidValue;
  // (ids may be null: a batch of empty bags has no entries, and none is read)
  if (a->w == nullptr || a->V == nullptr || a->bias == nullptr || a->offsets == nullptr || a->labels == nullptr ||
      a->lrow == nullptr || a->brow == nullptr)
    return hipErrorInvalidValue;
  if (train ? (a->dz == nullptr || a->dzbag == nullptr || a->G == nullptr) : a->prow == nullptr)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(a->V) | (train ? reinterpret_cast<uintptr_t>(a->G) : 0)) & 15)
    return hipErrorInvalidValue;
  int lsh = 0, waves = 0;
  while ((4 << lsh) < a->P * a->K) ++lsh;
  const int bytes = dtfk_ffm_tile_bytes(a->P, a->K, &waves);
  const dim3 grid((unsigned)(((long long)a->B + waves - 1) / waves)), block(64 * waves);
  const int stride = tile_stride(a->P, a->K);
  if (train) hipLaunchKernelGGL(ffm_rows<true>, grid, block, (size_t)waves * bytes, stream, *a, lsh, stride, waves);
  else hipLaunchKernelGGL(ffm_rows<false>, grid, block, (size_t)waves * bytes, stream, *a, lsh, stride, waves);
  return hipGetLastError();
}
