// Reached by: FMPlan (csrc/bind_fm.cpp), models/fm.py FMTrainer; tests/test_fm_gpu.py
// The second-order factorization machine on one GPU (Rendle 2010):
//
//   S_r[f] = sum_i x_i V[id_i, f]          Q_r[f] = sum_i x_i^2 V[id_i, f]^2
//   z_r    = b + sum_i x_i w[id_i] + 0.5 sum_f (S_r[f]^2 - Q_r[f])
//
// fm_rows<TRAIN>: one wave per batch row, rpw rows after each other per wave, four
// waves per workgroup; no LDS and no workgroup barrier.  A table row of K floats
// is read by LPR = 2^lsh >= K / 4 adjacent lanes, 16 bytes each, so one load
// instruction fetches the rows of EP = 64 / LPR entries; GS = 16 such loads are
// issued back to back before the first use.  A lane keeps two float4 sums per
// entry stream, x v and (x v)^2: S and Q come from the one pass over the table
// rows.  Entries arrive in chunks of 64 (one id / value load per lane, and one
// w[id] load: lanes own entries for the linear term); the next chunk -- of this
// row or of the wave's next row -- is requested before the current chunk's table
// rows.  The EP partial rows are combined by __shfl_xor over offsets >= LPR; the
// pairwise term is summed over the column blocks < K / 4 only (K = 20: LPR = 8,
// the lanes of blocks 5 .. 7 re-read block 4 and take no part in sum_f).
// Ids outside [0, F) are skipped and counted per row.
//   TRAIN = false: lrow, prow, brow (what eval_record.hip's reduce takes), z, p.
//   TRAIN = true:  also dz[r] = (sigmoid(z_r) - y_r) gscale and demb[r, :] = dz_r S_r.
//
// The gradient of a table row j needs nothing else from the forward pass:
//
//   dL/dw[j]    = sum_{occ of j} x dz_r
//   dL/dV[j, f] = sum_{occ of j} x demb[r, f]  -  V[j, f] q_j,     q_j = sum_{occ of j} x^2 dz_r
//
// fm_update_runs / fm_update_carry: the FM form of table_update.h's one-writer
// scheme (described there), w as the linear table and V as the row table.
#include "common.h"
#include "fm.h"

namespace dtfk {
namespace fm {

constexpr int WAVES = 4;
constexpr int GS = 16;                          // table-row loads in flight per lane (fm_rows)

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Up to 64 entries of a row, one per lane: the raw id and the value.  Nothing is
// read for cnt == 0; the lanes past the last entry repeat it.
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

template <bool TRAIN>
__global__ __launch_bounds__(64 * WAVES) void fm_rows(const RowArgs a, const int lsh, const int rpw) {
  const int lane = threadIdx.x & 63;
  const long long row0 = ((long long)blockIdx.x * WAVES + uni((int)(threadIdx.x >> 6))) * rpw;
  const int B = a.B, K = a.K;
  if (row0 >= B) return;                                               // (wave-uniform)
  const long long F = a.F;
  const int nrows = (int)min((long long)rpw, (long long)B - row0);
  const int LPR = 1 << lsh, EP = 64 >> lsh;
  const int sub = lane & (LPR - 1), q = lane >> lsh;
  const int colc = min(4 * sub, K - 4);
  const float bias = a.bias[0];

  // the wave's row offsets: lane i holds row row0 + i's
  long long so = 0, eo = 0;
  if (lane < nrows) {
    so = a.offsets[row0 + lane];
    eo = a.offsets[row0 + lane + 1];
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
  for (int i = 0; i < nrows; ++i) {
    long long sn = 0, en = 0;
    if (i + 1 < nrows) row_range(i + 1, sn, en);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), sq = make_float4(0.f, 0.f, 0.f, 0.f);
    float wacc = 0.f;
    int nbad = 0;
    long long c = s;
    do {
      const int cnt = (int)max(0LL, min(64LL, e - c));                 // 0: an empty row
      // the next chunk, of this row or the first of the next one, before this chunk's table rows
      const long long nc = c + 64;
      const bool more = nc < e;
      const long long ns = more ? nc : sn, ne = more ? e : en;
      const Chunk nxt = load_chunk(a, ns, (int)max(0LL, min(64LL, ne - ns)), lane);
      const bool in = lane < cnt;
      const bool ok = in && cur.raw >= 0 && cur.raw < F;               // out of range: skipped for both tables
      const long long id = ok ? cur.raw : -1;
      const float v = ok ? cur.v : 0.f;
      nbad += (in && !ok) ? 1 : 0;
      const float wt = a.w[ok ? cur.raw : 0];
      const int idlo = (int)(unsigned)id, idhi = (int)(id >> 32), vbits = __float_as_int(v);
      const int nsteps = (cnt + EP - 1) >> (6 - lsh);
      for (int t0 = 0; t0 < nsteps; t0 += GS) {
        float4 x[GS];
        float vv[GS];
        bool on[GS];
#pragma unroll
        for (int u = 0; u < GS; ++u) {                                 // step t: entry t EP + q, for every q
          const int src = min(min(t0 + u, nsteps - 1) * EP + q, 63);   // (a lane >= cnt holds id = -1)
          const int lo = __shfl(idlo, src, 64), hi = __shfl(idhi, src, 64);
          vv[u] = __int_as_float(__shfl(vbits, src, 64));
          on[u] = hi >= 0 && t0 + u < nsteps;                          // skipped entries and steps past the chunk: row 0, unused
          const unsigned long long rid = hi >= 0 ? (((unsigned long long)(unsigned)hi << 32) | (unsigned)lo) : 0ull;
          x[u] = *reinterpret_cast<const float4*>(a.V + (size_t)rid * K + colc);
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
    for (int off = LPR; off < 64; off <<= 1) {                         // the EP partial rows of a column block
      acc.x += __shfl_xor(acc.x, off, 64); acc.y += __shfl_xor(acc.y, off, 64);
      acc.z += __shfl_xor(acc.z, off, 64); acc.w += __shfl_xor(acc.w, off, 64);
      sq.x += __shfl_xor(sq.x, off, 64); sq.y += __shfl_xor(sq.y, off, 64);
      sq.z += __shfl_xor(sq.z, off, 64); sq.w += __shfl_xor(sq.w, off, 64);
    }
    // every lane now holds S and Q of column block `sub`; lane l < K / 4 speaks for block l
    const bool colown = 4 * lane < K;
    float pair = 0.f;
    if (colown)
      pair = 0.5f * (((acc.x * acc.x - sq.x) + (acc.y * acc.y - sq.y)) + ((acc.z * acc.z - sq.z) + (acc.w * acc.w - sq.w)));
    pair = wave_sum(pair);
    wacc = wave_sum(wacc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) nbad += __shfl_xor(nbad, off, 64);
    const long long row = row0 + i;
    const float z = (wacc + pair) + bias;
    const float y = a.labels[row];
    const float p = 1.f / (1.f + __expf(-z));
    if (lane == 0) {
      a.lrow[row] = xent(z, y);
      a.brow[row] = nbad;
      if (a.prow != nullptr) a.prow[row] = p;
      if (a.p_out != nullptr) a.p_out[row] = p;
      if (a.z_out != nullptr) a.z_out[row] = z;
    }
    if constexpr (TRAIN) {
      const float dz = (p - y) * a.gscale;
      if (lane == 0) a.dz[row] = dz;
      if (colown)
        *reinterpret_cast<float4*>(a.demb + (size_t)row * K + 4 * lane) =
            make_float4(dz * acc.x, dz * acc.y, dz * acc.z, dz * acc.w);
    }
    s = sn;
    e = en;
  }
}

// ---------------------------------------------------------------- the table update

__global__ __launch_bounds__(64 * WAVES) void fm_update_runs(const tu::Args a) { tu::update_runs<true>(a); }
__global__ __launch_bounds__(64 * WAVES) void fm_update_carry(const tu::Args a) { tu::update_carry<true>(a); }

}  // namespace fm
}  // namespace dtfk

extern "C" int dtfk_fm_supported(int K) { return K >= 4 && K <= dtfk::fm::MAXK && K % 4 == 0 ? 1 : 0; }

// Measured (profiles/fm_ab.json, evaluate at B = 500 and 4096, K = 64): one row per wave ties with two and beats
// four and eight, so one row per wave up to B = 4096; above that, not measured, the count doubles with B, and a
// wave requests a row's ids during the row before.
extern "C" int dtfk_fm_rpw(int B) {
  int rpw = 1;
  while (rpw < dtfk::fm::MAXRPW && (long long)B > 4096LL * rpw) rpw *= 2;
  return rpw;
}

extern "C" hipError_t dtfk_fm_rows(const dtfk::fm::RowArgs* a, int train, int rpw, hipStream_t stream) {
  using namespace dtfk::fm;
  if (a == nullptr || !dtfk_fm_supported(a->K) || a->B < 1 || a->F < 1) return hipErrorInvalidValue;
  // (ids may be null: a batch of empty rows has no entries, and none is read)
  if (a->w == nullptr || a->V == nullptr || a->bias == nullptr || a->offsets == nullptr || a->labels == nullptr ||
      a->lrow == nullptr || a->brow == nullptr)
    return hipErrorInvalidValue;
  if (train ? (a->dz == nullptr || a->demb == nullptr) : a->prow == nullptr) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(a->V) | (train ? reinterpret_cast<uintptr_t>(a->demb) : 0)) & 15)
    return hipErrorInvalidValue;
  if (rpw == 0) rpw = dtfk_fm_rpw(a->B);
  if (rpw < 1 || rpw > MAXRPW) return hipErrorInvalidValue;
  int lsh = 0;
  while ((4 << lsh) < a->K) ++lsh;
  const long long waves = ((long long)a->B + rpw - 1) / rpw;
  const dim3 grid((unsigned)((waves + WAVES - 1) / WAVES)), block(64 * WAVES);
  if (train) hipLaunchKernelGGL(fm_rows<true>, grid, block, 0, stream, *a, lsh, rpw);
  else hipLaunchKernelGGL(fm_rows<false>, grid, block, 0, stream, *a, lsh, rpw);
  return hipGetLastError();
}

extern "C" hipError_t dtfk_fm_update(const dtfk::tu::Args* a, hipStream_t stream) {
  return dtfk::tu::launch(a, stream, dtfk::fm::fm_update_runs, dtfk::fm::fm_update_carry);
}
