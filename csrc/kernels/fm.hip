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
// fm_update_runs / fm_update_carry: the one-writer scheme of wide_deep_update.hip
// (ids sorted once, a wave per 64 sorted positions, runs summed by a segmented
// scan in a fixed order, a run over a chunk edge folded by the carry kernel from
// per-chunk partials; no atomics, the same bits on every run).  Here a run also
// carries q (a partial is K + 2 floats in a stride of K + 4), and the writer
// forms  g[f] = sum[f] - V_old[j, f] q  from the row it has just loaded, before
// the rule of optim_rules.h.
#include "common.h"
#include "fm.h"

namespace dtfk {
namespace fm {

constexpr int WAVES = 4;
constexpr int GS = 16;                          // table-row loads in flight per lane (fm_rows)
constexpr int PASSES = 4;                       // gathered demb rows in flight per lane (fm_update_runs)

__host__ __device__ constexpr int part_stride(int K) { return K + 4; }   // columns, w's sum, q, padding to 16 bytes

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

// the head of the run that position q (0 .. 63) lies in
__device__ __forceinline__ int run_start(unsigned long long heads, int q) {
  return 63 - __clzll((long long)(heads & (~0ull >> (63 - q))));
}

// where the sum of the run [start, q] of a chunk goes: -1 = applied here, else the slot of `part`
__device__ __forceinline__ int run_slot(int start, int q, bool lead, bool trail) {
  if (start == 0 && (lead || (trail && q == 63))) return 0;
  return trail && q == 63 ? 1 : -1;
}

// four columns of a factor row: g = s - V_old qrun, then the rule
__device__ __forceinline__ void apply_factors(const UpdArgs& a, size_t o, f32x4 s, float qrun) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 var = *reinterpret_cast<const f32x4*>(a.V + o);
  f32x4 sa = a.V_a != nullptr ? *reinterpret_cast<const f32x4*>(a.V_a + o) : zero;
  f32x4 sb = a.V_b != nullptr ? *reinterpret_cast<const f32x4*>(a.V_b + o) : zero;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v1 = var[k], a1 = sa[k], b1 = sb[k];
    update1(v1, a1, b1, s[k] - v1 * qrun, a.kind, a.h);
    var[k] = v1; sa[k] = a1; sb[k] = b1;
  }
  *reinterpret_cast<f32x4*>(a.V + o) = var;
  if (a.V_a != nullptr) *reinterpret_cast<f32x4*>(a.V_a + o) = sa;
  if (a.V_b != nullptr) *reinterpret_cast<f32x4*>(a.V_b + o) = sb;
}

__device__ __forceinline__ void apply_linear(const UpdArgs& a, size_t o, float g) {
  float var = a.w[o], sa = a.w_a != nullptr ? a.w_a[o] : 0.f, sb = a.w_b != nullptr ? a.w_b[o] : 0.f;
  update1(var, sa, sb, g, a.kind, a.h);
  a.w[o] = var;
  if (a.w_a != nullptr) a.w_a[o] = sa;
  if (a.w_b != nullptr) a.w_b[o] = sb;
}

__global__ __launch_bounds__(64 * WAVES) void fm_update_runs(const UpdArgs a) {
  const int lane = threadIdx.x & 63;
  const long long c = (long long)blockIdx.x * WAVES + uni((int)(threadIdx.x >> 6));
  const long long p0 = c * CHUNK;
  if (p0 >= a.N) return;
  const int cnt = (int)(a.N - p0 < CHUNK ? a.N - p0 : CHUNK);
  const int K = a.K, PS = part_stride(K);

  // this lane's occurrence; row < 0: past the batch or an id outside the table
  int row = -1, b = 0;
  float x = 0.f;
  if (lane < cnt) {
    const int id = a.sids[p0 + lane];
    if (id >= 0 && id < a.F) {
      const long long j = a.perm[p0 + lane];
      row = id;
      b = a.bag_of[j];
      x = a.vals != nullptr ? a.vals[j] : 1.f;
    }
  }
  const int prev = __shfl_up(row, 1, 64);
  const unsigned long long heads = __ballot(lane == 0 || prev != row);
  const unsigned long long tails = (heads >> 1) | (1ull << 63);
  const int first = __shfl(row, 0, 64), last = __shfl(row, 63, 64);
  // the first run goes on from the previous chunk / the last one into the next
  const bool lead = first >= 0 && c > 0 && a.sids[p0 - 1] == first;
  const bool trail = last >= 0 && p0 + CHUNK < a.N && a.sids[p0 + CHUNK] == last;
  float* __restrict__ part = a.part + (size_t)c * 2 * PS;

  // ---- linear table and q: lanes own occurrences, one segmented scan for both sums
  float qs;
  {
    const float d = a.dz[b];
    float v = x * d;
    qs = (x * x) * d;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float vu = __shfl_up(v, off, 64), qu = __shfl_up(qs, off, 64);
      const int ru = __shfl_up(row, off, 64);
      if (lane >= off && ru == row) {
        v += vu;
        qs += qu;
      }
    }
    if (row >= 0 && ((tails >> lane) & 1)) {
      const int slot = run_slot(run_start(heads, lane), lane, lead, trail);
      if (slot >= 0) {
        part[slot * PS + K] = v;
        part[slot * PS + K + 1] = qs;
      } else {
        apply_linear(a, (size_t)row, v);
      }
    }
  }

  // ---- factor table: lanes across columns, R positions per pass
  const int G = K >> 2, R = 64 / G;
  const int g = lane / G, col = (lane - g * G) * 4;
  const bool live = g < R;
  const int carry_src = (R - 1) * G + (lane - g * G);
  f32x4 carry = {0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < cnt; q0 += PASSES * R) {
    f32x4 v[PASSES];
    int rq[PASSES];
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {                 // no branch: every lane shuffles and loads in every pass
      const int q = q0 + u * R + g, qc = q < 63 ? q : 63;
      const int bq = __shfl(b, qc, 64), rowq = __shfl(row, qc, 64);
      const float xq = __shfl(x, qc, 64);
      const bool on = live && q < 64;                  // else: a clamped address, times 0
      rq[u] = on ? rowq : -1;
      v[u] = (on ? xq : 0.f) * *reinterpret_cast<const f32x4*>(a.demb + (size_t)bq * K + col);
    }
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {
      const int base = q0 + u * R;
      if (base >= cnt) break;                          // wave-uniform
      const int q = base + g, qc = q < 63 ? q : 63;
      const int st = run_start(heads, qc);
      const float qrun = __shfl(qs, qc, 64);           // q of the run [st, q]
      f32x4 s = v[u];
      for (int off = 1; off < R; off <<= 1) {          // segmented scan over the pass's groups
        f32x4 up;
#pragma unroll
        for (int k = 0; k < 4; ++k) up[k] = __shfl_up(s[k], off * G, 64);
        if (g >= off && st <= q - off) s += up;
      }
      if (st < base) s += carry;                       // the run began in an earlier pass
#pragma unroll
      for (int k = 0; k < 4; ++k) carry[k] = __shfl(s[k], carry_src, 64);
      if (rq[u] >= 0 && ((tails >> qc) & 1)) {
        const int slot = run_slot(st, q, lead, trail);
        if (slot >= 0) *reinterpret_cast<f32x4*>(part + slot * PS + col) = s;
        else apply_factors(a, (size_t)rq[u] * K + col, s, qrun);
      }
    }
  }
}

__global__ __launch_bounds__(64 * WAVES) void fm_update_carry(const UpdArgs a) {
  const int lane = threadIdx.x & 63;
  const long long c = (long long)blockIdx.x * WAVES + uni((int)(threadIdx.x >> 6));
  const long long p0 = c * CHUNK;
  if (p0 + CHUNK >= a.N) return;                       // no next chunk: nothing goes on
  const int id = a.sids[p0 + CHUNK - 1];
  if (id < 0 || id >= a.F || a.sids[p0 + CHUNK] != id) return;
  if (c > 0 && a.sids[p0 - 1] == id) return;           // the run started in an earlier chunk: that wave folds it
  const int K = a.K, G = K >> 2, PS = part_stride(K);
  const long long nch = (a.N + CHUNK - 1) / CHUNK;
  // lanes < G: 4 columns each; lane G: w's sum and q
  const bool cols = lane < G, lin = lane == G;
  const float* __restrict__ part = a.part;
  const int slot = a.sids[p0] == id ? 0 : 1;           // a run that covers the whole chunk wrote the leading slot
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float accw = 0.f, accq = 0.f;
  {
    const float* p = part + (size_t)(c * 2 + slot) * PS;
    if (cols) acc = *reinterpret_cast<const f32x4*>(p + lane * 4);
    if (lin) accw = p[K], accq = p[K + 1];
  }
  for (long long k = c + 1; k < nch; k += 64) {
    // the next 64 chunk starts at once: the run goes on through the first n of them
    const long long kk = k + lane;
    const unsigned long long hit = __ballot(kk < nch && a.sids[kk * CHUNK] == id);
    const int n = ~hit == 0ull ? 64 : __ffsll((long long)~hit) - 1;
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
      const float* p = part + (size_t)(k + i) * 2 * PS;
      if (cols) acc += *reinterpret_cast<const f32x4*>(p + lane * 4);
      if (lin) accw += p[K], accq += p[K + 1];
    }
    if (n < 64) break;
  }
  const float qrun = __shfl(accq, G, 64);
  if (cols) apply_factors(a, (size_t)id * K + lane * 4, acc, qrun);
  if (lin) apply_linear(a, (size_t)id, accw);
}

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

extern "C" long long dtfk_fm_update_part_floats(long long N, int K) {
  return (N + dtfk::fm::CHUNK - 1) / dtfk::fm::CHUNK * 2 * dtfk::fm::part_stride(K);
}

extern "C" hipError_t dtfk_fm_update(const dtfk::fm::UpdArgs* a, hipStream_t stream) {
  using namespace dtfk;
  using namespace dtfk::fm;
  if (a == nullptr || !row_local(a->kind)) return hipErrorInvalidValue;
  if (uses_slot_a(a->kind) && (a->w_a == nullptr || a->V_a == nullptr)) return hipErrorInvalidValue;
  if (uses_slot_b(a->kind) && (a->w_b == nullptr || a->V_b == nullptr)) return hipErrorInvalidValue;
  if (a->kind == OPT_FTRL && !ftrl_hyper_ok(a->h)) return hipErrorInvalidValue;
  if (!dtfk_fm_supported(a->K)) return hipErrorInvalidValue;
  if (a->F < 1 || a->F >= (1ll << 31) || a->N < 0 || a->N >= (1ll << 31)) return hipErrorInvalidValue;
  if (a->N == 0) return hipSuccess;
  if (a->sids == nullptr || a->perm == nullptr || a->bag_of == nullptr || a->dz == nullptr || a->demb == nullptr ||
      a->w == nullptr || a->V == nullptr || a->part == nullptr)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(a->V) | reinterpret_cast<uintptr_t>(a->V_a) | reinterpret_cast<uintptr_t>(a->V_b) |
       reinterpret_cast<uintptr_t>(a->demb) | reinterpret_cast<uintptr_t>(a->part)) & 15)
    return hipErrorInvalidValue;
  const long long chunks = (a->N + CHUNK - 1) / CHUNK;
  const dim3 grid((unsigned)((chunks + WAVES - 1) / WAVES)), block(64 * WAVES);
  hipLaunchKernelGGL(fm_update_runs, grid, block, 0, stream, *a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || chunks == 1) return e;
  hipLaunchKernelGGL(fm_update_carry, grid, block, 0, stream, *a);
  return hipGetLastError();
}
