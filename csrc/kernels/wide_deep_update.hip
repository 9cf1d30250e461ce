// Reached by: WideDeepTrainPlan.update (csrc/bind_wide_deep.cpp), WideDeep(fused_step="combined"); tests/test_wide_deep_update_gpu.py
// The table update of the one-GPU Wide&Deep training step: a row's occurrences
// are summed first, then the row is written once.
//
// TensorFlow applies an IndexedSlices gradient by summing duplicate indices and
// updating every touched row once (optim_rules.h, sparse_optim.hip).  Here the
// gradient rows are never materialised: the batch's ids are sorted once (stable,
// so equal ids keep their CSR order), and occurrence p of the sorted order
// contributes  w_p demb[bag_p, :]  to the embedding row and  w_p dz[bag_p]  to
// the wide row of its id,  w_p = val_p scale[bag_p].  Both tables read the same
// ids: one pass updates both.
//
// wd_update_runs: a wave owns 64 consecutive sorted positions (a chunk), a
// workgroup 4 chunks.  Lane l holds position l's (row, bag, w); the chunk's run
// structure is two wave-uniform 64-bit masks (run heads, run tails).
//   * embedding table: lanes across columns, G = D / 4 lanes of one 16-byte load
//     per gathered demb row, R = 64 / G positions per pass, PASSES passes of
//     loads issued back to back with no branch between them (>= 8 rows in
//     flight; positions past the chunk and lanes past R G load a clamped address
//     and multiply by 0).  Inside a pass the R lane groups are combined by a
//     segmented Hillis-Steele scan over the run masks, a run that spans passes
//     is carried from the last group.
//   * wide table: lanes own occurrences, the same scan over equal rows.
// A run's sum is therefore taken in a fixed tree order, not one position after
// the other: the order depends only on the sorted positions, so the same batch
// gives the same bits on every run.
// A run that lies inside the chunk is applied there, by the group / lane that
// holds its sum: rule of `kind` on the row and its slots, plain loads and
// stores.  A run that continues from the previous chunk or into the next one is
// not: its partial sum goes to part[chunk][0] (leading; also a run that covers
// the whole chunk) or part[chunk][1] (trailing).
//
// wd_update_carry: one wave per chunk in which such a run starts.  It adds the
// run's partials in chunk order (the run ends where the id at a chunk start
// changes; at most the chunk count) and applies the rule once.  Every table
// element has exactly one writer, in one of the two kernels; no atomics, no
// waiting between workgroups: the stream orders the kernels.
#include "common.h"
#include "wide_deep_update.h"

namespace dtfk {
namespace wdu {

constexpr int PASSES = 4;                       // gathered rows in flight per lane
constexpr int WAVES = 4;

__host__ __device__ constexpr int part_stride(int D) { return D + 4; }   // columns, the wide sum, padding to 16 bytes

// the head of the run that position q (0 .. 63) lies in
__device__ __forceinline__ int run_start(unsigned long long heads, int q) {
  return 63 - __clzll((long long)(heads & (~0ull >> (63 - q))));
}

// where the sum of the run [start, q] of a chunk goes: -1 = applied here, else the slot of `part`
__device__ __forceinline__ int run_slot(int start, int q, bool lead, bool trail) {
  if (start == 0 && (lead || (trail && q == 63))) return 0;
  return trail && q == 63 ? 1 : -1;
}

__device__ __forceinline__ void apply_row4(float* __restrict__ t, float* __restrict__ sa, float* __restrict__ sb,
                                           size_t o, f32x4 g, int kind, const OptimHyper& h) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 var = *reinterpret_cast<const f32x4*>(t + o);
  f32x4 a = sa != nullptr ? *reinterpret_cast<const f32x4*>(sa + o) : zero;
  f32x4 b = sb != nullptr ? *reinterpret_cast<const f32x4*>(sb + o) : zero;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v1 = var[k], a1 = a[k], b1 = b[k];
    update1(v1, a1, b1, g[k], kind, h);
    var[k] = v1; a[k] = a1; b[k] = b1;
  }
  *reinterpret_cast<f32x4*>(t + o) = var;
  if (sa != nullptr) *reinterpret_cast<f32x4*>(sa + o) = a;
  if (sb != nullptr) *reinterpret_cast<f32x4*>(sb + o) = b;
}

__device__ __forceinline__ void apply_row1(float* __restrict__ t, float* __restrict__ sa, float* __restrict__ sb,
                                           size_t o, float g, int kind, const OptimHyper& h) {
  float var = t[o], a = sa != nullptr ? sa[o] : 0.f, b = sb != nullptr ? sb[o] : 0.f;
  update1(var, a, b, g, kind, h);
  t[o] = var;
  if (sa != nullptr) sa[o] = a;
  if (sb != nullptr) sb[o] = b;
}

// scale[b] of a bag: embedding_bag_bwd's formula and wave_sum order
__global__ __launch_bounds__(256) void wd_update_scale(const long long* __restrict__ offsets,
                                                       const float* __restrict__ vals, int B, int mode,
                                                       float* __restrict__ scale) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  const long long s = offsets[b], e = offsets[b + 1];
  float ws = 0.f;
  for (long long j = s + lane; j < e; j += 64) {
    const float w = vals ? vals[j] : 1.f;
    ws += mode == 2 ? w * w : w;
  }
  ws = wave_sum(ws);
  float sc = 1.f;
  if (mode == 1 && e > s) sc = 1.f / fmaxf(ws, 1e-30f);
  if (mode == 2 && e > s) sc = rsqrtf(fmaxf(ws, 1e-30f));
  if (lane == 0) scale[b] = sc;
}

__global__ __launch_bounds__(256) void wd_update_runs(const Args a) {
  if (a.skip != nullptr && *a.skip != 0) return;
  const int lane = threadIdx.x & 63;
  // the wave's number as a scalar: chunk, count and every pass bound below are wave-uniform to the compiler too
  const long long c = (long long)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long p0 = c * CHUNK;
  if (p0 >= a.N) return;
  const int cnt = (int)(a.N - p0 < CHUNK ? a.N - p0 : CHUNK);
  const int D = a.D;

  // this lane's occurrence; row < 0: past the batch or an id outside the table
  int row = -1, b = 0;
  float w = 0.f;
  if (lane < cnt) {
    const int id = a.sids[p0 + lane];
    if (id >= 0 && id < a.V) {
      const long long j = a.perm[p0 + lane];
      row = id;
      b = a.bag_of[j];
      w = (a.vals != nullptr ? a.vals[j] : 1.f) * (a.scale != nullptr ? a.scale[b] : 1.f);
    }
  }
  const int prev = __shfl_up(row, 1, 64);
  const unsigned long long heads = __ballot(lane == 0 || prev != row);
  const unsigned long long tails = (heads >> 1) | (1ull << 63);
  const int first = __shfl(row, 0, 64), last = __shfl(row, 63, 64);
  // the first run goes on from the previous chunk / the last one into the next
  const bool lead = first >= 0 && c > 0 && a.sids[p0 - 1] == first;
  const bool trail = last >= 0 && p0 + CHUNK < a.N && a.sids[p0 + CHUNK] == last;
  float* __restrict__ part = a.part + (size_t)c * 2 * part_stride(D);

  // ---- wide table: lanes own occurrences
  {
    float v = w * a.dz[b];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float vu = __shfl_up(v, off, 64);
      const int ru = __shfl_up(row, off, 64);
      if (lane >= off && ru == row) v += vu;
    }
    if (row >= 0 && ((tails >> lane) & 1)) {
      const int slot = run_slot(run_start(heads, lane), lane, lead, trail);
      if (slot >= 0) part[slot * part_stride(D) + D] = v;
      else apply_row1(a.wide, a.wide_a, a.wide_b, (size_t)row, v, a.kind, a.h);
    }
  }

  // ---- embedding table: lanes across columns, R positions per pass
  const int G = D >> 2, R = 64 / G;
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
      const float wq = __shfl(w, qc, 64);
      const bool on = live && q < 64;                  // else: a clamped address, times 0
      rq[u] = on ? rowq : -1;
      v[u] = (on ? wq : 0.f) * *reinterpret_cast<const f32x4*>(a.demb + (size_t)bq * D + col);
    }
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {
      const int base = q0 + u * R;
      if (base >= cnt) break;                          // wave-uniform
      const int q = base + g, qc = q < 63 ? q : 63;
      const int st = run_start(heads, qc);
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
        if (slot >= 0) *reinterpret_cast<f32x4*>(part + slot * part_stride(D) + col) = s;
        else apply_row4(a.emb, a.emb_a, a.emb_b, (size_t)rq[u] * D + col, s, a.kind, a.h);
      }
    }
  }
}

__global__ __launch_bounds__(256) void wd_update_carry(const Args a) {
  if (a.skip != nullptr && *a.skip != 0) return;
  const int lane = threadIdx.x & 63;
  const long long c = (long long)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long p0 = c * CHUNK;
  if (p0 + CHUNK >= a.N) return;                       // no next chunk: nothing goes on
  const int id = a.sids[p0 + CHUNK - 1];
  if (id < 0 || id >= a.V || a.sids[p0 + CHUNK] != id) return;
  if (c > 0 && a.sids[p0 - 1] == id) return;           // the run started in an earlier chunk: that wave folds it
  const int D = a.D, G = D >> 2, DS = part_stride(D);
  const long long nch = (a.N + CHUNK - 1) / CHUNK;
  // lanes < G: 4 columns each; lane G: the wide sum
  const bool cols = lane < G, wide = lane == G;
  const float* __restrict__ part = a.part;
  const int slot = a.sids[p0] == id ? 0 : 1;           // a run that covers the whole chunk wrote the leading slot
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float accw = 0.f;
  {
    const float* p = part + (size_t)(c * 2 + slot) * DS;
    if (cols) acc = *reinterpret_cast<const f32x4*>(p + lane * 4);
    if (wide) accw = p[D];
  }
  for (long long k = c + 1; k < nch; k += 64) {
    // the next 64 chunk starts at once: the run goes on through the first n of them
    const long long kk = k + lane;
    const unsigned long long hit = __ballot(kk < nch && a.sids[kk * CHUNK] == id);
    const int n = ~hit == 0ull ? 64 : __ffsll((long long)~hit) - 1;
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
      const float* p = part + (size_t)(k + i) * 2 * DS;
      if (cols) acc += *reinterpret_cast<const f32x4*>(p + lane * 4);
      if (wide) accw += p[D];
    }
    if (n < 64) break;
  }
  if (cols) apply_row4(a.emb, a.emb_a, a.emb_b, (size_t)id * D + lane * 4, acc, a.kind, a.h);
  if (wide) apply_row1(a.wide, a.wide_a, a.wide_b, (size_t)id, accw, a.kind, a.h);
}

}  // namespace wdu
}  // namespace dtfk

extern "C" long long dtfk_wd_update_part_floats(long long N, int D) {
  return (N + dtfk::wdu::CHUNK - 1) / dtfk::wdu::CHUNK * 2 * dtfk::wdu::part_stride(D);
}

extern "C" hipError_t dtfk_wd_update_scale(const long long* offsets, const float* vals, int B, int mode, float* scale,
                                           hipStream_t stream) {
  using namespace dtfk::wdu;
  if (B <= 0) return hipSuccess;
  if (mode != 1 && mode != 2) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wd_update_scale, dim3((unsigned)((B + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, stream, offsets,
                     vals, B, mode, scale);
  return hipGetLastError();
}

extern "C" hipError_t dtfk_wd_update(const dtfk::wdu::Args* a, hipStream_t stream) {
  using namespace dtfk;
  using namespace dtfk::wdu;
  if (!row_local(a->kind)) return hipErrorInvalidValue;
  if (uses_slot_a(a->kind) && (a->wide_a == nullptr || a->emb_a == nullptr)) return hipErrorInvalidValue;
  if (uses_slot_b(a->kind) && (a->wide_b == nullptr || a->emb_b == nullptr)) return hipErrorInvalidValue;
  if (a->kind == OPT_FTRL && !ftrl_hyper_ok(a->h)) return hipErrorInvalidValue;
  if (a->D < 4 || a->D > MAXD || a->D % 4 != 0) return hipErrorInvalidValue;
  if (a->V < 1 || a->V >= (1ll << 31) || a->N < 0 || a->N >= (1ll << 31)) return hipErrorInvalidValue;
  if (a->N == 0) return hipSuccess;
  const long long chunks = (a->N + CHUNK - 1) / CHUNK;
  const dim3 grid((unsigned)((chunks + WAVES - 1) / WAVES)), block(64 * WAVES);
  hipLaunchKernelGGL(wd_update_runs, grid, block, 0, stream, *a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || chunks == 1) return e;
  hipLaunchKernelGGL(wd_update_carry, grid, block, 0, stream, *a);
  return hipGetLastError();
}
