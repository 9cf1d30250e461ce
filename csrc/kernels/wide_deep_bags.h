// The bag reader of one row tile, shared by the Wide&Deep row kernels as a
// fragment of the kernel's body: wide_deep_eval.hip wd_eval_rows and
// wide_deep_train.hip wd_train_rows include this file inside the kernel, where
// a function would go.  (An inlined function was tried first: the compiler
// optimizes its body once on its own, before inlining, and wd_eval_rows's
// registers and schedule then differ from the measured kernel's; as text in the
// kernel the evaluation's device code stays what it was.)
//
// In scope at the point of inclusion:
//   TM (rows per workgroup), NW, uni / Chunk / load_chunk (wide_deep_rows.h);
//   const wde::Args& a;  float* buf0 (the first LDS activation buffer, row stride a.ld0);
//   float wide_s[TM];  int bad_s[TM] (LDS);  int lane, w;  long long row0.
// Leaves: the scaled embedding tile in buf0 (columns D .. 16-multiple: 0), the wide
// sums in wide_s, the out-of-range id counts in bad_s, and the names D, D16, B, F.
// The including kernel synchronizes the workgroup afterwards.
  constexpr int RPW = TM / NW;                                         // rows per wave
  constexpr int GS = 16;                                               // table-row loads in flight per lane
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
