// Reached by: csrc/bind_libsvm_gpu.cpp LibsvmGpuParser.parse and libsvm_gpu_parse_into (data/libsvm.py GpuLibsvmParser, DataProvider parser="gpu"); tests/test_libsvm_gpu_parse_gpu.py, scripts/bench_libsvm_parse.py
// libsvm text -> device CSR batches.  The bytes of a chunk are classified
// (whitespace, newline, token byte); three ranks -- pieces, valid lines (2 or
// more bytes), ':' bytes -- are counted per tile, scanned over the tiles by one
// workgroup and rebuilt per byte, so the lane that owns the first byte of a token
// knows its line and its entry number and parses it with libsvm_rule.h.  A token
// outside the rule raises the record's `irregular` word: the host then discards
// the result and parses the chunk with libc.  A second scan over the lines
// compacts the kept ones into labels / ids / vals and per-batch rebased offsets.
// Plain streaming kernels: no atomics, no inter-workgroup waits; every store is
// bounds-checked against the capacities dtfk_lsv_plan derives from n.
#include "libsvm_parse_api.h"
#include "libsvm_rule.h"

namespace dtfk {
namespace lsvk {

constexpr int THREADS = 256;
constexpr int BPT = 16;                      // text bytes per thread
constexpr int LSV_TILE = THREADS * BPT;      // text bytes per workgroup pass
constexpr int LPT = 4;                       // lines per thread
constexpr int LINE_TILE = THREADS * LPT;
constexpr int MAX_BLOCKS = 2048;             // memory-bound grid cap; the rest is strided

struct Ws {                                  // the workspace, carved by carve()
  int* t_nl;  int* t_vl;  int* t_col;        // per text tile: pieces ended, valid lines ended, ':' bytes
  int* l_keep;  int* l_nnz;                  // per line tile: kept lines, their entries
  float* label;  int* ord;  int* cstart;  int* cend;  int* kf;   // per valid line
  int* rowstart;  int* rowsrc;               // per kept row (+1)
  long long* raw_id;  float* raw_val;        // per ':' byte
  long long cap_lines, cap_entries, ntiles, nltiles;
};

static long long align16(long long b) { return (b + 15) & ~15ll; }

static long long carve(long long n, char* base, Ws* w) {
  w->cap_lines = n / 3 + 2;
  w->cap_entries = n / 4 + 2;
  w->ntiles = (n + 1 + LSV_TILE - 1) / LSV_TILE;
  w->nltiles = (w->cap_lines + LINE_TILE - 1) / LINE_TILE;
  long long off = 0;
  auto take = [&](long long bytes) { char* p = base + off; off += align16(bytes); return p; };
  w->raw_id = (long long*)take(8 * w->cap_entries);
  w->raw_val = (float*)take(4 * w->cap_entries);
  w->t_nl = (int*)take(4 * w->ntiles);
  w->t_vl = (int*)take(4 * w->ntiles);
  w->t_col = (int*)take(4 * w->ntiles);
  w->l_keep = (int*)take(4 * w->nltiles);
  w->l_nnz = (int*)take(4 * w->nltiles);
  w->label = (float*)take(4 * w->cap_lines);
  w->ord = (int*)take(4 * w->cap_lines);
  w->cstart = (int*)take(4 * w->cap_lines);
  w->cend = (int*)take(4 * w->cap_lines);
  w->kf = (int*)take(4 * w->cap_lines);
  w->rowstart = (int*)take(4 * (w->cap_lines + 1));
  w->rowsrc = (int*)take(4 * w->cap_lines);
  return off;
}

// ------------------------------------------------------------------ helpers
__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// exclusive prefix of v over the workgroup's threads, and the workgroup's total
__device__ __forceinline__ int block_excl_scan(int v, int* sm, int& total) {
  const int inc = wave_incl_scan(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();                         // the previous use of sm is over
  if (lane == 63) sm[wv] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < THREADS / 64; ++k) {
    const int s = sm[k];
    if (k < wv) base += s;
    total += s;
  }
  return base + inc - v;
}

// The chunk as the kernels see it: byte i < n is itself; position n is a newline
// when the text does not end in one (it closes the last line); anything else is
// whitespace.
struct Text {
  const unsigned char* t;
  long long n;
  bool virt;
  __device__ __forceinline__ unsigned char at(long long i) const {
    if (i < 0) return '\n';
    if (i < n) return t[i];
    return (i == n && virt) ? '\n' : ' ';
  }
};
__device__ __forceinline__ Text make_text(const unsigned char* t, long long n) {
  Text x;
  x.t = t;
  x.n = n;
  x.virt = n > 0 && t[n - 1] != '\n';
  return x;
}
__device__ __forceinline__ bool is_tok(unsigned char c) { return c != '\n' && !lsv::is_ws(c); }

// a thread's 16 positions from p0 (16-byte aligned): one vector load inside the text
__device__ __forceinline__ void load16(const Text& x, long long p0, unsigned char* b) {
  if (p0 + BPT <= x.n) {
    const uint4 v = *reinterpret_cast<const uint4*>(x.t + p0);
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < BPT; ++k) b[k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
  } else {
#pragma unroll
    for (int k = 0; k < BPT; ++k) b[k] = x.at(p0 + k);
  }
}

// ------------------------------------------------------------------ kernels
__global__ __launch_bounds__(THREADS) void lsv_init(int* __restrict__ ord, long long cap_lines,
                                                    long long* __restrict__ meta) {
  const long long stride = (long long)gridDim.x * THREADS;
  for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < cap_lines; i += stride) ord[i] = -1;
  if (blockIdx.x == 0 && threadIdx.x < LSV_META_HEAD) meta[threadIdx.x] = 0;
}

__global__ __launch_bounds__(THREADS) void lsv_count(const unsigned char* __restrict__ txt, long long n,
                                                     long long ntiles, int* __restrict__ t_nl,
                                                     int* __restrict__ t_vl, int* __restrict__ t_col) {
  __shared__ int sm[THREADS / 64];
  const Text x = make_text(txt, n);
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long p0 = tile * LSV_TILE + (long long)threadIdx.x * BPT;
    unsigned char b[BPT];
    load16(x, p0, b);
    bool nl1 = x.at(p0 - 1) == '\n', nl2 = x.at(p0 - 2) == '\n';
    int c_nl = 0, c_vl = 0, c_col = 0;
#pragma unroll
    for (int k = 0; k < BPT; ++k) {
      const bool nl = b[k] == '\n';
      c_nl += nl;
      c_vl += nl && !nl1 && !nl2;
      c_col += b[k] == ':';
      nl2 = nl1;
      nl1 = nl;
    }
    int tot_nl, tot_vl, tot_col;
    block_excl_scan(c_nl, sm, tot_nl);
    block_excl_scan(c_vl, sm, tot_vl);
    block_excl_scan(c_col, sm, tot_col);
    if (threadIdx.x == 0) {
      t_nl[tile] = tot_nl;
      t_vl[tile] = tot_vl;
      t_col[tile] = tot_col;
    }
  }
}

// a[0, n) -> its exclusive prefix sums, in place; returns the total (one workgroup)
__device__ int scan_in_place(int* a, long long n, int* sm) {
  int carry = 0;
  for (long long i0 = 0; i0 < n; i0 += THREADS) {
    const long long i = i0 + threadIdx.x;
    const int v = i < n ? a[i] : 0;
    int tot;
    const int ex = block_excl_scan(v, sm, tot);
    if (i < n) a[i] = carry + ex;
    carry += tot;
  }
  return carry;
}

__global__ __launch_bounds__(THREADS) void lsv_scan_text(int* t_nl, int* t_vl, int* t_col, long long ntiles,
                                                         long long cap_lines, long long cap_entries,
                                                         long long* __restrict__ meta) {
  __shared__ int sm[THREADS / 64];
  const int lines = scan_in_place(t_nl, ntiles, sm);
  const int vlines = scan_in_place(t_vl, ntiles, sm);
  const int colons = scan_in_place(t_col, ntiles, sm);
  if (threadIdx.x == 0) {
    meta[LSV_LINES] = lines;
    meta[LSV_VALID_LINES] = vlines;
    meta[LSV_COLONS] = colons;
    if (colons > cap_entries || vlines > cap_lines) meta[LSV_IRREGULAR] = 1;   // more ':' than entries fit
  }
}

__global__ __launch_bounds__(THREADS) void lsv_parse(const unsigned char* __restrict__ txt, long long n,
                                                     long long ntiles, const int* __restrict__ t_nl,
                                                     const int* __restrict__ t_vl, const int* __restrict__ t_col,
                                                     float* __restrict__ label, int* __restrict__ ord,
                                                     int* __restrict__ cstart, int* __restrict__ cend,
                                                     long long* __restrict__ raw_id, float* __restrict__ raw_val,
                                                     long long cap_lines, long long cap_entries,
                                                     long long* __restrict__ meta) {
  __shared__ int sm[THREADS / 64];
  const Text x = make_text(txt, n);
  auto at = [&](long long i) { return txt[i]; };
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long p0 = tile * LSV_TILE + (long long)threadIdx.x * BPT;
    unsigned char b[BPT];
    load16(x, p0, b);
    const unsigned char prev1 = x.at(p0 - 1);
    bool nl1 = prev1 == '\n', nl2 = x.at(p0 - 2) == '\n';
    {
      int c_nl = 0, c_vl = 0, c_col = 0;
      bool a1 = nl1, a2 = nl2;
#pragma unroll
      for (int k = 0; k < BPT; ++k) {
        const bool nl = b[k] == '\n';
        c_nl += nl;
        c_vl += nl && !a1 && !a2;
        c_col += b[k] == ':';
        a2 = a1;
        a1 = nl;
      }
      int tot;
      c_nl = block_excl_scan(c_nl, sm, tot) + t_nl[tile];
      c_vl = block_excl_scan(c_vl, sm, tot) + t_vl[tile];
      c_col = block_excl_scan(c_col, sm, tot) + t_col[tile];
      // the ranks in front of this thread's first byte
      int r_nl = c_nl, r_vl = c_vl, r_col = c_col;
      bool tok1 = is_tok(prev1);
      for (int k = 0; k < BPT; ++k) {
        const long long i = p0 + k;
        const unsigned char c = b[k];
        const bool nl = c == '\n';
        const bool tok = !nl && !lsv::is_ws(c);
        if (tok && !tok1) {                       // this lane owns the token that starts at i
          long long q = i + 1;
          while (q < n && is_tok(txt[q])) ++q;
          long long j = i - 1;
          while (j >= 0 && lsv::is_ws(txt[j])) --j;
          const bool first = j < 0 || txt[j] == '\n';
          const bool one_byte_piece = first && j == i - 1 && q == i + 1 && (q >= n || txt[q] == '\n');
          if (!one_byte_piece) {                  // (a piece shorter than 2 bytes is skipped silently)
            int kind = 0;
            long long idx = 0;
            float val = 0.f;
            const bool ok = lsv::parse_token(at, i, q, &kind, &idx, &val);
            if (!ok || (kind == 0) != first) {
              meta[LSV_IRREGULAR] = 1;
            } else if (kind == 0) {
              if (r_vl < cap_lines) {
                label[r_vl] = val;
                ord[r_vl] = r_nl;
                cstart[r_vl] = r_col;
              }
            } else if (r_col < cap_entries) {
              raw_id[r_col] = idx;
              raw_val[r_col] = val;
            }
          }
        }
        if (nl) {
          if (!nl1 && !nl2) {                     // the end of a piece of 2 or more bytes
            if (r_vl < cap_lines) cend[r_vl] = r_col;
            ++r_vl;
          }
          ++r_nl;
        }
        r_col += c == ':';
        nl2 = nl1;
        nl1 = nl;
        tok1 = tok;
      }
    }
  }
}

// per valid line: kf = its entry count when it is kept, -1 when it is not; per line tile the sums
__global__ __launch_bounds__(THREADS) void lsv_line_flags(const int* __restrict__ ord, const int* __restrict__ cstart,
                                                          const int* __restrict__ cend, int* __restrict__ kf,
                                                          int* __restrict__ l_keep, int* __restrict__ l_nnz,
                                                          long long cap_lines, long long cap_entries,
                                                          long long first_ordinal,
                                                          unsigned long long seed, double rate,
                                                          long long* __restrict__ meta) {
  __shared__ int sm[THREADS / 64];
  // No early return on the irregular word here: this kernel's own workgroups write it, so
  // the threads of one workgroup could read it differently in front of a barrier.
  long long V = meta[LSV_VALID_LINES];
  if (V > cap_lines) V = cap_lines;
  const long long nlt = (V + LINE_TILE - 1) / LINE_TILE;
  for (long long lt = blockIdx.x; lt < nlt; lt += gridDim.x) {
    int ck = 0, cn = 0;
    for (int k = 0; k < LPT; ++k) {
      const long long v = lt * LINE_TILE + (long long)threadIdx.x * LPT + k;
      if (v >= V) break;
      const int o = ord[v];
      int f = -1;
      if (o < 0) {
        meta[LSV_IRREGULAR] = 1;              // a line of 2 or more bytes without a label: whitespace only
      } else {
        const int nn = cend[v] - cstart[v];
        if (nn < 0 || cend[v] > cap_entries) meta[LSV_IRREGULAR] = 1;
        else if (lsv::keep(seed, (unsigned long long)(first_ordinal + o), rate)) f = nn;
      }
      kf[v] = f;
      ck += f >= 0;
      cn += f >= 0 ? f : 0;
    }
    int tk, tn;
    block_excl_scan(ck, sm, tk);
    block_excl_scan(cn, sm, tn);
    if (threadIdx.x == 0) {
      l_keep[lt] = tk;
      l_nnz[lt] = tn;
    }
  }
}

__global__ __launch_bounds__(THREADS) void lsv_scan_lines(int* l_keep, int* l_nnz, long long batch_size,
                                                          long long carry_rows, long long* __restrict__ meta) {
  __shared__ int sm[THREADS / 64];
  if (meta[LSV_IRREGULAR]) return;
  const long long V = meta[LSV_VALID_LINES];
  const long long nlt = (V + LINE_TILE - 1) / LINE_TILE;
  const int rows = scan_in_place(l_keep, nlt, sm);
  const int nnz = scan_in_place(l_nnz, nlt, sm);
  if (threadIdx.x == 0) {
    meta[LSV_ROWS] = rows;
    meta[LSV_NNZ] = nnz;
    meta[LSV_BATCHES] = rows > 0 ? (rows + carry_rows + batch_size - 1) / batch_size : 0;
  }
}

__global__ __launch_bounds__(THREADS) void lsv_place(const int* __restrict__ kf, const int* __restrict__ l_keep,
                                                     const int* __restrict__ l_nnz, const float* __restrict__ label,
                                                     const int* __restrict__ cstart, float* __restrict__ labels,
                                                     int* __restrict__ rowstart, int* __restrict__ rowsrc,
                                                     long long rows_cap, const long long* __restrict__ meta) {
  __shared__ int sm[THREADS / 64];
  if (meta[LSV_IRREGULAR]) return;
  const long long V = meta[LSV_VALID_LINES];
  const long long nlt = (V + LINE_TILE - 1) / LINE_TILE;
  for (long long lt = blockIdx.x; lt < nlt; lt += gridDim.x) {
    const long long v0 = lt * LINE_TILE + (long long)threadIdx.x * LPT;
    int f[LPT], ck = 0, cn = 0;
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
      f[k] = v0 + k < V ? kf[v0 + k] : -1;
      ck += f[k] >= 0;
      cn += f[k] >= 0 ? f[k] : 0;
    }
    int tot;
    int r = block_excl_scan(ck, sm, tot) + l_keep[lt];
    int s = block_excl_scan(cn, sm, tot) + l_nnz[lt];
#pragma unroll
    for (int k = 0; k < LPT; ++k) {
      if (f[k] < 0) continue;
      if (r < rows_cap) {
        labels[r] = label[v0 + k];
        rowstart[r] = s;
        rowsrc[r] = cstart[v0 + k];
      }
      ++r;
      s += f[k];
    }
  }
}

constexpr int GL = 8;   // lanes per row in the gather

__global__ __launch_bounds__(THREADS) void lsv_gather(const int* __restrict__ rowstart, const int* __restrict__ rowsrc,
                                                      const long long* __restrict__ raw_id,
                                                      const float* __restrict__ raw_val, long long* __restrict__ ids,
                                                      float* __restrict__ vals, long long nnz_cap,
                                                      long long cap_entries, const long long* __restrict__ meta) {
  if (meta[LSV_IRREGULAR]) return;
  const long long R = meta[LSV_ROWS], nnz = meta[LSV_NNZ];
  const int sub = threadIdx.x % GL;
  const long long stride = (long long)gridDim.x * (THREADS / GL);
  for (long long r = (long long)blockIdx.x * (THREADS / GL) + threadIdx.x / GL; r < R; r += stride) {
    const long long s = rowstart[r];
    const long long e = r + 1 < R ? rowstart[r + 1] : nnz;
    const long long src = rowsrc[r];
    for (long long k = sub; k < e - s; k += GL) {
      if (s + k < nnz_cap && src + k < cap_entries) {
        ids[s + k] = raw_id[src + k];
        vals[s + k] = raw_val[src + k];
      }
    }
  }
}

// offsets[b, j] of output row b * batch_size + j - carry_rows, rebased on the batch's first
// row (batch 0 starts at carry_nnz: it continues the carried rows); bases[b] into ids / vals
__global__ __launch_bounds__(THREADS) void lsv_offsets(const int* __restrict__ rowstart, long long batch_size,
                                                       long long carry_rows, long long carry_nnz,
                                                       long long* __restrict__ offsets, long long batch_cap,
                                                       long long* __restrict__ meta) {
  if (meta[LSV_IRREGULAR]) return;
  const long long R = meta[LSV_ROWS], nnz = meta[LSV_NNZ];
  long long nb = meta[LSV_BATCHES];
  if (nb > batch_cap) nb = batch_cap;
  long long* bases = meta + LSV_META_HEAD;
  const long long w = batch_size + 1, total = nb * w;
  const long long stride = (long long)gridDim.x * THREADS;
  for (long long e = (long long)blockIdx.x * THREADS + threadIdx.x; e < total; e += stride) {
    const long long b = e / w, j = e % w;
    const long long q = b * batch_size + j - carry_rows;
    long long br = b * batch_size - carry_rows;
    if (br < 0) br = 0;
    const long long base = br >= R ? nnz : rowstart[br];
    long long val = 0;
    if (q >= 0) val = (q >= R ? nnz : (long long)rowstart[q]) - base + (b == 0 ? carry_nnz : 0);
    offsets[e] = val;
    if (j == 0) bases[b] = base;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) bases[nb] = nnz;
}

static unsigned grid_for(long long work_items, long long per_block) {
  long long g = (work_items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (unsigned)(g < MAX_BLOCKS ? g : MAX_BLOCKS);
}

}  // namespace lsvk
}  // namespace dtfk

extern "C" int dtfk_lsv_tile_bytes(void) { return dtfk::lsvk::LSV_TILE; }

extern "C" int dtfk_lsv_plan(long long n, long long batch_size, long long carry_rows, LsvPlan* plan) {
  using namespace dtfk::lsvk;
  if (n < 0 || n >= (1ll << 31) || batch_size < 1 || carry_rows < 0 || carry_rows >= batch_size || !plan) return 0;
  Ws w;
  plan->ws_bytes = carve(n, nullptr, &w);
  plan->rows_cap = w.cap_lines;
  plan->nnz_cap = w.cap_entries;
  plan->batch_cap = (w.cap_lines + carry_rows) / batch_size + 1;
  plan->meta_len = LSV_META_HEAD + plan->batch_cap + 1;
  return 1;
}

extern "C" hipError_t dtfk_lsv_parse(const unsigned char* text, long long n, long long first_ordinal,
                                     unsigned long long seed, double rate, long long batch_size, long long carry_rows,
                                     long long carry_nnz, void* ws, long long ws_bytes, float* labels,
                                     long long rows_cap, long long* ids, float* vals, long long nnz_cap,
                                     long long* offsets, long long batch_cap, long long* meta, long long meta_len,
                                     hipStream_t stream) {
  using namespace dtfk::lsvk;
  LsvPlan p;
  if (!dtfk_lsv_plan(n, batch_size, carry_rows, &p)) return hipErrorInvalidValue;
  if (!(rate > 0.0 && rate <= 1.0) || carry_nnz < 0 || first_ordinal < 0) return hipErrorInvalidValue;
  if (!text || !ws || !labels || !ids || !vals || !offsets || !meta) return hipErrorInvalidValue;
  if (ws_bytes < p.ws_bytes || rows_cap < p.rows_cap || nnz_cap < p.nnz_cap || batch_cap < p.batch_cap ||
      meta_len < p.meta_len)
    return hipErrorInvalidValue;
  if (((uintptr_t)text & 15) || ((uintptr_t)ws & 15)) return hipErrorInvalidValue;
  Ws w;
  carve(n, (char*)ws, &w);
  const dim3 blk(THREADS);
  const unsigned g_text = grid_for(w.ntiles, 1), g_line = grid_for(w.cap_lines, LINE_TILE);
  hipLaunchKernelGGL(lsv_init, dim3(grid_for(w.cap_lines, THREADS)), blk, 0, stream, w.ord, w.cap_lines, meta);
  hipLaunchKernelGGL(lsv_count, dim3(g_text), blk, 0, stream, text, n, w.ntiles, w.t_nl, w.t_vl, w.t_col);
  hipLaunchKernelGGL(lsv_scan_text, dim3(1), blk, 0, stream, w.t_nl, w.t_vl, w.t_col, w.ntiles, w.cap_lines,
                     w.cap_entries, meta);
  hipLaunchKernelGGL(lsv_parse, dim3(g_text), blk, 0, stream, text, n, w.ntiles, w.t_nl, w.t_vl, w.t_col, w.label,
                     w.ord, w.cstart, w.cend, w.raw_id, w.raw_val, w.cap_lines, w.cap_entries, meta);
  hipLaunchKernelGGL(lsv_line_flags, dim3(g_line), blk, 0, stream, w.ord, w.cstart, w.cend, w.kf, w.l_keep, w.l_nnz,
                     w.cap_lines, w.cap_entries, first_ordinal, seed, rate, meta);
  hipLaunchKernelGGL(lsv_scan_lines, dim3(1), blk, 0, stream, w.l_keep, w.l_nnz, batch_size, carry_rows, meta);
  hipLaunchKernelGGL(lsv_place, dim3(g_line), blk, 0, stream, w.kf, w.l_keep, w.l_nnz, w.label, w.cstart, labels,
                     w.rowstart, w.rowsrc, rows_cap, meta);
  hipLaunchKernelGGL(lsv_gather, dim3(grid_for(w.cap_lines, THREADS / GL)), blk, 0, stream, w.rowstart, w.rowsrc,
                     w.raw_id, w.raw_val, ids, vals, nnz_cap, w.cap_entries, meta);
  hipLaunchKernelGGL(lsv_offsets, dim3(grid_for(p.batch_cap * (batch_size + 1), THREADS)), blk, 0, stream,
                     w.rowstart, batch_size, carry_rows, carry_nnz, offsets, batch_cap, meta);
  return hipGetLastError();
}
