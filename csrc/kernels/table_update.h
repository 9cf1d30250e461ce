// The one-writer table update of the one-GPU sparse models: a row's occurrences
// are summed first, then the row is written once.  One body for its users:
// wide_deep_update.hip (wd_update_runs / wd_update_carry: the Wide&Deep tables)
// and fm.hip (fm_update_runs / fm_update_carry: FM and DeepFM, the FM form).
// Included by both hosts (the args, the sizes and the refusals) and, after
// common.h, by those two .hip files (the device bodies).
//
// TensorFlow applies an IndexedSlices gradient by summing duplicate indices and
// updating every touched row once (optim_rules.h, sparse_optim.hip).  Here the
// gradient rows are never materialised: the batch's ids are sorted once (stable,
// so equal ids keep their CSR order), and occurrence p of the sorted order
// contributes  w_p demb[bag_p, :]  to the row table's row and  w_p dz[bag_p]  to
// the linear table's row of its id,  w_p = val_p scale[bag_p].  Both tables read
// the same ids: one pass updates both.
//
// update_runs: a wave owns 64 consecutive sorted positions (a chunk), a
// workgroup 4 chunks.  Lane l holds position l's (row, bag, w); the chunk's run
// structure is two wave-uniform 64-bit masks (run heads, run tails).
//   * row table: lanes across columns, G = width / 4 lanes of one 16-byte load
//     per gathered demb row, R = 64 / G positions per pass, PASSES passes of
//     loads issued back to back with no branch between them (>= 8 rows in
//     flight; positions past the chunk and lanes past R G load a clamped address
//     and multiply by 0).  Inside a pass the R lane groups are combined by a
//     segmented Hillis-Steele scan over the run masks, a run that spans passes
//     is carried from the last group.
//   * linear table: lanes own occurrences, the same scan over equal rows.
// A run's sum is therefore taken in a fixed tree order, not one position after
// the other: the order depends only on the sorted positions, so the same batch
// gives the same bits on every run.
// A run that lies inside the chunk is applied there, by the group / lane that
// holds its sum: rule of `kind` on the row and its slots, plain loads and
// stores.  A run that continues from the previous chunk or into the next one is
// not: its partial sum goes to part[chunk][0] (leading; also a run that covers
// the whole chunk) or part[chunk][1] (trailing).
//
// update_carry: one wave per chunk in which such a run starts.  It adds the
// run's partials in chunk order (the run ends where the id at a chunk start
// changes; at most the chunk count) and applies the rule once.  Every table
// element has exactly one writer, in one of the two kernels; no atomics, no
// waiting between workgroups: the stream orders the kernels.
//
// The FM form (FM = true; no scale, no skip): the gradient of a factor row j is
//   sum_{occ of j} x demb[r, f]  -  V[j, f] q_j,     q_j = sum_{occ of j} x^2 dz_r.
// Here a run also carries q (a partial is width + 2 floats in a stride of
// width + 4), and the writer forms  g[f] = sum[f] - V_old[j, f] q  from the row
// it has just loaded, before the rule of optim_rules.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "optim_rules.h"

namespace dtfk {
namespace tu {

constexpr int CHUNK = 64;     // sorted positions per wave
constexpr int PASSES = 4;     // gathered demb rows in flight per lane
constexpr int WAVES = 4;
constexpr int MAXW = 128;

// a partial of `part`: the columns, the linear sum, q (FM form), padding to 16 bytes
constexpr __host__ __device__ int part_stride(int width) { return width + 4; }
// Floats of Args::part for N ids.
inline long long part_floats(long long N, int width) { return (N + CHUNK - 1) / CHUNK * 2 * part_stride(width); }

struct Args {
  const int* sids;            // [N] the ids in ascending order (stable sort); outside [0, rows): no part in anything
  const long long* perm;      // [N] the CSR position of each sorted position
  const int* bag_of;          // [N] the bag (batch row) of each CSR position
  const float* vals;          // [N] by CSR position, or null: every value is 1
  const float* scale;         // [B] the combiner's scale per bag, or null (sum); not read in the FM form
  const float* dz;            // [B] the linear table's bag gradient
  const float* demb;          // [B, width] the row table's bag gradient, 16-byte aligned
  float *lin, *lin_a, *lin_b;      // [rows] table and its slots (null where the kind has none)
  float *row, *row_a, *row_b;      // [rows, width], 16-byte aligned
  float* part;                // [chunks, 2, width + 4]: a chunk's leading / trailing partial sums, 16-byte aligned
  long long N, rows;
  int width, kind;
  OptimHyper h;
  const int* skip;            // device word, may be null: nonzero changes nothing; not read in the FM form
};

// What can be refused before the ids are sorted: a row-local kind with its slots, FTRL hyper-parameters in
// range, width a multiple of 4 in 4 .. 128, fewer than 2^31 table rows and ids.
inline bool values_ok(const Args& a) {
  if (!row_local(a.kind)) return false;
  if (uses_slot_a(a.kind) && (a.lin_a == nullptr || a.row_a == nullptr)) return false;
  if (uses_slot_b(a.kind) && (a.lin_b == nullptr || a.row_b == nullptr)) return false;
  if (a.kind == OPT_FTRL && !ftrl_hyper_ok(a.h)) return false;
  if (a.width < 4 || a.width > MAXW || a.width % 4 != 0) return false;
  return a.rows >= 1 && a.rows < (1ll << 31) && a.N >= 0 && a.N < (1ll << 31);
}

// The launchers' refusals: values_ok, and for a batch with ids every pointer a kernel reads without a test,
// the 16-byte ones aligned.
inline hipError_t check(const Args* a) {
  if (a == nullptr || !values_ok(*a)) return hipErrorInvalidValue;
  if (a->N == 0) return hipSuccess;
  if (a->sids == nullptr || a->perm == nullptr || a->bag_of == nullptr || a->dz == nullptr || a->demb == nullptr ||
      a->lin == nullptr || a->row == nullptr || a->part == nullptr)
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(a->row) | reinterpret_cast<uintptr_t>(a->row_a) |
       reinterpret_cast<uintptr_t>(a->row_b) | reinterpret_cast<uintptr_t>(a->demb) |
       reinterpret_cast<uintptr_t>(a->part)) & 15)
    return hipErrorInvalidValue;
  return hipSuccess;
}

#ifdef __HIPCC__
// check(), then `runs` and (more than one chunk) `carry` on `stream`: a file's two __global__ wrappers
inline hipError_t launch(const Args* a, hipStream_t stream, void (*runs)(const Args), void (*carry)(const Args)) {
  hipError_t e = check(a);
  if (e != hipSuccess || a->N == 0) return e;
  const long long chunks = (a->N + CHUNK - 1) / CHUNK;
  const dim3 grid((unsigned)((chunks + WAVES - 1) / WAVES)), block(64 * WAVES);
  hipLaunchKernelGGL(runs, grid, block, 0, stream, *a);
  e = hipGetLastError();
  if (e != hipSuccess || chunks == 1) return e;
  hipLaunchKernelGGL(carry, grid, block, 0, stream, *a);
  return hipGetLastError();
}

// the head of the run that position q (0 .. 63) lies in
__device__ __forceinline__ int run_start(unsigned long long heads, int q) {
  return 63 - __clzll((long long)(heads & (~0ull >> (63 - q))));
}

// where the sum of the run [start, q] of a chunk goes: -1 = applied here, else the slot of `part`
__device__ __forceinline__ int run_slot(int start, int q, bool lead, bool trail) {
  if (start == 0 && (lead || (trail && q == 63))) return 0;
  return trail && q == 63 ? 1 : -1;
}

// four columns of a row: the rule on g (FM: on g - V_old qrun)
template <bool FM>
__device__ __forceinline__ void apply_row4(float* t, float* sa, float* sb,
                                           size_t o, f32x4 g, float qrun, int kind, const OptimHyper& h) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 var = *reinterpret_cast<const f32x4*>(t + o);
  f32x4 a = sa != nullptr ? *reinterpret_cast<const f32x4*>(sa + o) : zero;
  f32x4 b = sb != nullptr ? *reinterpret_cast<const f32x4*>(sb + o) : zero;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v1 = var[k], a1 = a[k], b1 = b[k];
    update1(v1, a1, b1, FM ? g[k] - v1 * qrun : g[k], kind, h);
    var[k] = v1; a[k] = a1; b[k] = b1;
  }
  *reinterpret_cast<f32x4*>(t + o) = var;
  if (sa != nullptr) *reinterpret_cast<f32x4*>(sa + o) = a;
  if (sb != nullptr) *reinterpret_cast<f32x4*>(sb + o) = b;
}

__device__ __forceinline__ void apply_row1(float* t, float* sa, float* sb,
                                           size_t o, float g, int kind, const OptimHyper& h) {
  float var = t[o], a = sa != nullptr ? sa[o] : 0.f, b = sb != nullptr ? sb[o] : 0.f;
  update1(var, a, b, g, kind, h);
  t[o] = var;
  if (sa != nullptr) sa[o] = a;
  if (sb != nullptr) sb[o] = b;
}

template <bool FM>
__device__ __forceinline__ void update_runs(const Args& a) {
  if (!FM && a.skip != nullptr && *a.skip != 0) return;
  const int lane = threadIdx.x & 63;
  // the wave's number as a scalar: chunk, count and every pass bound below are wave-uniform to the compiler too
  const long long c = (long long)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long p0 = c * CHUNK;
  if (p0 >= a.N) return;
  const int cnt = (int)(a.N - p0 < CHUNK ? a.N - p0 : CHUNK);
  const int W = a.width;

  // this lane's occurrence; row < 0: past the batch or an id outside the table
  int row = -1, b = 0;
  float w = 0.f;
  if (lane < cnt) {
    const int id = a.sids[p0 + lane];
    if (id >= 0 && id < a.rows) {
      const long long j = a.perm[p0 + lane];
      row = id;
      b = a.bag_of[j];
      if constexpr (FM) w = a.vals != nullptr ? a.vals[j] : 1.f;
      else w = (a.vals != nullptr ? a.vals[j] : 1.f) * (a.scale != nullptr ? a.scale[b] : 1.f);
    }
  }
  const int prev = __shfl_up(row, 1, 64);
  const unsigned long long heads = __ballot(lane == 0 || prev != row);
  const unsigned long long tails = (heads >> 1) | (1ull << 63);
  const int first = __shfl(row, 0, 64), last = __shfl(row, 63, 64);
  // the first run goes on from the previous chunk / the last one into the next
  const bool lead = first >= 0 && c > 0 && a.sids[p0 - 1] == first;
  const bool trail = last >= 0 && p0 + CHUNK < a.N && a.sids[p0 + CHUNK] == last;
  float* __restrict__ part = a.part + (size_t)c * 2 * part_stride(W);

  // ---- linear table (FM: and q): lanes own occurrences, one segmented scan
  float qs = 0.f;
  {
    const float d = a.dz[b];
    float v = w * d;
    if (FM) qs = (w * w) * d;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float vu = __shfl_up(v, off, 64), qu = FM ? __shfl_up(qs, off, 64) : 0.f;
      const int ru = __shfl_up(row, off, 64);
      if (lane >= off && ru == row) {
        v += vu;
        if (FM) qs += qu;
      }
    }
    if (row >= 0 && ((tails >> lane) & 1)) {
      const int slot = run_slot(run_start(heads, lane), lane, lead, trail);
      if (slot >= 0) {
        part[slot * part_stride(W) + W] = v;
        if (FM) part[slot * part_stride(W) + W + 1] = qs;
      } else {
        apply_row1(a.lin, a.lin_a, a.lin_b, (size_t)row, v, a.kind, a.h);
      }
    }
  }

  // ---- row table: lanes across columns, R positions per pass
  const int G = W >> 2, R = 64 / G;
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
      v[u] = (on ? wq : 0.f) * *reinterpret_cast<const f32x4*>(a.demb + (size_t)bq * W + col);
    }
#pragma unroll
    for (int u = 0; u < PASSES; ++u) {
      const int base = q0 + u * R;
      if (base >= cnt) break;                          // wave-uniform
      const int q = base + g, qc = q < 63 ? q : 63;
      const int st = run_start(heads, qc);
      const float qrun = FM ? __shfl(qs, qc, 64) : 0.f;   // q of the run [st, q]
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
        if (slot >= 0) *reinterpret_cast<f32x4*>(part + slot * part_stride(W) + col) = s;
        else apply_row4<FM>(a.row, a.row_a, a.row_b, (size_t)rq[u] * W + col, s, qrun, a.kind, a.h);
      }
    }
  }
}

template <bool FM>
__device__ __forceinline__ void update_carry(const Args& a) {
  if (!FM && a.skip != nullptr && *a.skip != 0) return;
  const int lane = threadIdx.x & 63;
  const long long c = (long long)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long p0 = c * CHUNK;
  if (p0 + CHUNK >= a.N) return;                       // no next chunk: nothing goes on
  const int id = a.sids[p0 + CHUNK - 1];
  if (id < 0 || id >= a.rows || a.sids[p0 + CHUNK] != id) return;
  if (c > 0 && a.sids[p0 - 1] == id) return;           // the run started in an earlier chunk: that wave folds it
  const int W = a.width, G = W >> 2, PS = part_stride(W);
  const long long nch = (a.N + CHUNK - 1) / CHUNK;
  // lanes < G: 4 columns each; lane G: the linear sum (FM: and q)
  const bool cols = lane < G, lin = lane == G;
  const float* __restrict__ part = a.part;
  const int slot = a.sids[p0] == id ? 0 : 1;           // a run that covers the whole chunk wrote the leading slot
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float accw = 0.f, accq = 0.f;
  {
    const float* p = part + (size_t)(c * 2 + slot) * PS;
    if (cols) acc = *reinterpret_cast<const f32x4*>(p + lane * 4);
    if (lin) {
      accw = p[W];
      if (FM) accq = p[W + 1];
    }
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
      if (lin) {
        accw += p[W];
        if (FM) accq += p[W + 1];
      }
    }
    if (n < 64) break;
  }
  const float qrun = FM ? __shfl(accq, G, 64) : 0.f;
  if (cols) apply_row4<FM>(a.row, a.row_a, a.row_b, (size_t)id * W + lane * 4, acc, qrun, a.kind, a.h);
  if (lin) apply_row1(a.lin, a.lin_a, a.lin_b, (size_t)id, accw, a.kind, a.h);
}
#endif  // __HIPCC__

}  // namespace tu
}  // namespace dtfk
