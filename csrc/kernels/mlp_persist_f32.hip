// Reached by: bench.py headline engine (PersistentMLPRunner), the resident Session engine (compat/resident.py), smoke(); tests/test_mlp_persist_gpu.py, test_resident_gpu.py
// Persistent, weight-stationary training kernel for the reference's 784-100-10
// MLP at the reference's precision: every product is an fp32 x fp32 MFMA
// (v_mfma_f32_16x16x4_f32, bitwise an fmaf chain), fp32 accumulate, fp32
// master weights held in VGPRs for the whole launch (example.py:77-118 is fp32
// end to end: x*W1+b1 -> sigmoid -> *W2+b2 -> softmax cross-entropy -> SGD).
//
// The f32-input MFMA runs at 1/16 of the f16 rate, so where the f16 engine
// (mlp_persist.hip) keeps a hidden block per CU, this one spreads each block's
// weights over 4 CUs:
//
//  * 28 compute workgroups (512 threads) c = (j, q): hidden block j (units
//    16j..16j+15, 7 blocks) x feature slice q (13, 12, 12, 12 tiles of 16
//    features; 49 tiles = 784 exactly).  Wave w owns local tiles w and w + 8 of
//    the slice: 4 fp32 VGPRs per lane and tile hold W1[16t+4g+e][16j+r]
//    (r = lane&15, g = lane>>4), which is at once its forward A operand
//    (k-step e) and the C layout of its weight gradient, so the SGD update is
//    in-register.
//  * per step:
//      P0  forward partial z^T[hidden][batch] of the wave's tiles for all 7
//          batch tiles (7 independent MFMA chains) -> LDS; wave w (batch tile
//          w) sums the 8 waves' partials in a fixed order.
//      E1  the slice partial of (j, batch tile w) goes to the 3 other slices of
//          block j as tagged 8-byte granules (the data is the flag); everyone
//          sums the 4 slices in slice order -> identical z in all 4.
//      P1  a2 = act(z/255 + b1), partial logits^T of block j (4 MFMAs; a2 is
//          the B operand straight from the accumulator layout).
//      E2  partial logits go to the workgroup of the same slice in every other
//          block; logits = b2 + sum_j (block order) -> identical in all 28.
//          The head's chain is only what dz2 needs: logits, m, ex, ssum, inv,
//          dz3, da2 = W2 dz3 (4 MFMAs), dz2 = da2 * act' -> LDS with the dz3 /
//          a2 rows, then the FIRST head flag.  Behind it: the row's loss / hit
//          (zy, argmax; the label's probability only for the naive loss) in
//          workgroup 0 alone -- nobody else reads them --, the tile's dW2 / db2
//          partial (8 MFMAs), then the SECOND head flag.
//      P2  dW1 tiles = x^T dz2 over the batch (28 MFMAs per tile, x^T bytes by
//          transposing LDS reads of the same row-major image the forward
//          reads: ds_read_b64_tr_b8), W1 -= lr/(255 B) dW1 in registers;
//          wave 7 also, once the seven second flags are up: the fold of the
//          tiles' dW2 / db2 partials, db1, metrics, update of the LDS
//          copies of W2[block j], b1[block j], b2 -- identical in every
//          workgroup that holds them (same inputs, same order).
//      P2 runs without a workgroup barrier: each 32-row batch chunk of the
//          weight gradient starts as soon as the heads of its batch tiles have
//          set their first LDS flags (the partial that only wave 7's fold consumes
//          is not in front of them); wave 7 signals the next step's stage with a
//          flag.  The head was the step's longest compute segment and two heads
//          serialise on a SIMD: 311 -> 192 instructions from the E2 gather to the
//          last head MFMA in 27 workgroups, 280 -> 164 to the last dz2 plane
//          store (profiles/mlp_persist_f32_head_ab.json).
//      Operand preparation (one-GPU split engine, PREP in compute()): the pixel
//          bytes become bf16 MFMA operands away from the MFMAs that use them --
//          the step's x^T operands of P2 in the E1 window (wave 7: behind its
//          stage DMA), the NEXT step's x operands of P0 where the staged step is
//          read (wave 7: behind its stage DMA; the head waves: after P2, once
//          wave 7's flag says the stage landed -- it lands inside their E2 gather
//          by now, but preparing between two polls there did not pay, see PREP
//          in compute(); the launch's first step in the prologue; a launch's
//          last step prepares nothing).  P0 is split8 + MFMAs, and only the dz2
//          piece reads sit between a head flag and a chunk's MFMAs.  Same
//          operands, same order: same bits.
//      Workgroup 0's metrics: its head waves write the per-row loss / hit behind
//          their first flag and in front of their second one, and its wave 7
//          reduces them in front of barrier A (MET_FAST in compute(), same
//          engine: the sums by VALU lane permutes, the ring slot by a 32-bit
//          modulo).  Workgroup 0's wave 7 still reaches barrier A after the
//          others'; handing the rows of tiles 4..6 to waves 0..2, and a flag of
//          their own for the rows behind the partial, were built bit-equal,
//          measured and taken out (figures: profiles/mlp_persist_f32_head_ab.json).
//    One LDS barrier and two inter-workgroup edges per step; the data of
//    every edge is double-buffered by step parity and tagged with the global
//    exchange sequence number, so buffers are never reset between launches.
//  * x enters the MFMAs as exact integers 0..255 (v_cvt_f32_ubyte); the 1/255
//    pixel scale and the 1/B loss mean are applied to the fp32 sums.
//  * 16 COPIER workgroups pull chunk c+1 from pinned host memory over PCIe into
//    the other device stage (a record per step: row-major x [112][784] u8, rows
//    >= B zero, then 128 label bytes; 87,936 B) while the compute workgroups run
//    chunk c.
//  * wave 7 stages ONE image per step (the slice's 112 rows x 208 B, + labels)
//    with LDS-DMA while the gathers poll: half the bytes of the row-major +
//    feature-major pair it replaced, 6.84 -> 6.64 us/step.  Dense (planar) granule
//    slots with padding lanes masked out of both edges measured 2 % SLOWER than
//    the interleaved slots below, alone and on top of this, and are not in
//    (profiles/mlp_persist_f32_handoff_bytes_ab.json).
//  * N GPUs (MULTI, NW = the peer-table width W is unrolled for: 2, 4, 8):
//    after P2 every compute workgroup exchanges its gradient (its dW1 tiles +
//    the block's small gradients) with the same workgroup on every peer through
//    IPC-mapped uncached buffers -- 28 CUs per GPU carry the peer traffic, every
//    peer read a 16-B system-scope buffer load, all NW in flight at once -- and
//    sums the ranks in rank order (bit-identical replicas).  Publication order:
//    the slot bytes go to uncached (MTYPE UC) memory with plain stores, every
//    storing wave waits for them (vmcnt(0)), then a workgroup barrier, then ONE
//    relaxed system-scope flag store; consumers poll the flag with system-scope
//    loads and read the bytes with system-scope (sc0 sc1) loads, never served
//    from a cache of the reading device.
//
// Placement: packed (default) runs workgroup c as blockIdx 8c, so under the
// observed round-robin dispatch all 28 share one XCD and both edges stay in one
// L2 (plain stores); spread (several ranks on one GPU: tests) runs them as
// blocks 0..27.  A per-launch census of HW_REG_XCC_ID picks each edge's store
// flavour (plain if L2-local, write-through otherwise): speed only, never
// correctness.  Measured on MI355X (profiles/mlp_persist_f32_phases_r3_prologue.json,
// BENCH_r04.json): ~8.1 us/step; the per-step critical path is the two hops
// (~1.3 and ~1.9 us after the last producer) plus producer skew, not the MFMA
// phases (~0.5 forward + ~1.1 weight gradient).
//
// RES (the resident Session engine, compat/resident.py): ONE launch serves
// Session.run calls -- per run the copiers wait on a pinned-host doorbell, stage
// the run's record, and the compute workgroups stage it at the top of the step
// (no in-step prefetch: the next run's data does not exist yet); after the step
// the weights are written through to the graph's own variables and workgroup 0
// publishes loss / accuracy / global_step and a done count to pinned memory.
#include "common.h"
#include "mlp_api.h"

#include <atomic>

#include <cstdlib>

namespace dtfk {
namespace mlpf {

typedef __attribute__((address_space(1))) unsigned gu32;

constexpr int DIN = 784, HID = 100, NCLS = 10;
constexpr int NJ = 7;              // hidden blocks of 16
constexpr int NQ = 4;              // feature slices: 13, 12, 12, 12 tiles of 16 features (49 = 784 / 16)
constexpr int NTW = 2;             // feature tiles per wave (local tiles w and w + 8)
constexpr int NBT = 7;             // batch tiles of 16 (B <= 112)
constexpr int BROWS = 16 * NBT;    // 112
constexpr int XTS = 128;           // batch rows padded to the weight gradient's K (4 chunks of 32)
constexpr int NCOMP = NJ * NQ;     // 28 compute workgroups: one XCD
constexpr int THREADS = 512;
constexpr int NCOP = 16;           // copier workgroups
constexpr int NCOPR = 14;          // RES: copiers of one record (8 batch rows each)
constexpr int RES_LR_BYTE = 124;   // RES: the run's lr rides in the record's label area (B <= 112)
constexpr int GRID_PACKED = 8 * NCOMP;
constexpr int GRID_SPREAD = NCOMP + NCOP;
__host__ __device__ constexpr int tile0(int q) { return q == 0 ? 0 : 13 + 12 * (q - 1); }
__host__ __device__ constexpr int ntile(int q) { return q == 0 ? 13 : 12; }
constexpr int OFF_W2 = 78400, OFF_B1 = 79400, OFF_B2 = 79500;

// device stage record of one step
// (no feature-major copy: the weight gradient's x^T fragments are transposing LDS
// reads of the row-major image, see read_xt)
constexpr long long XROW_BYTES = (long long)BROWS * DIN;   // [112][784] u8, rows >= B zero
constexpr long long REC = XROW_BYTES + 128;                // + labels [128]

// exchange buffer (bytes): every payload float travels as an 8-byte granule
// {value, tag} (the data is the flag: no separate flag word, no drain before a
// flag, one hop); a slot = 64 lanes x 4 granules = 2 KB.
// E1 [2][NJ][NQ][NBT] slots, E2 [2][NQ][NBT][NJ] slots
constexpr int GSLOT = 2048;
constexpr long long E1_OFF = 0;
constexpr long long E2_OFF = E1_OFF + 2LL * NJ * NQ * NBT * GSLOT;
constexpr long long HDR_OFF = E2_OFF + 2LL * NQ * NBT * NJ * GSLOT;   // [64] u64 placement census
constexpr long long XBUF_BYTES = HDR_OFF + 64 * 8;

// IPC buffer of one rank (N GPUs): [flags: workgroup c at byte 64c][2 parities][28 slots]
// slot: dW1 entries of wave w, lane l at 16 (w 64 + l) (bf16: both tiles' 4 bf16 in
// one 16-B entry, 8 B when the wave has one tile) or 16 ((2 w + k) 64 + l) (fp32:
// one entry per tile k) | dW2 64 lanes x 16 B at IPC_SMALL | db1 / db2 (16 + 10)
// fp32 behind it.  Lanes of padding units and the zero dW2 columns are never
// stored or loaded: the bytes read from a peer are the payload
// (scripts/exchange_cost_model.py, tests/test_exchange_model_cpu.py).
// Two-shot mode adds a reduced area of the same slot layout (the owner's sums:
// bf16 for a bf16 payload, rounded once by the owner) behind the slots, and a
// second flag per workgroup at byte 64c + 8.
constexpr int IPC_FLAGS = 4096;
constexpr int IPC_SMALL = 8 * NTW * 64 * 16;
constexpr int IPC_SLOT = IPC_SMALL + 1024 + 128;
constexpr long long IPC_RED = IPC_FLAGS + 2LL * NCOMP * IPC_SLOT;
constexpr long long IPC_BYTES = IPC_RED + 2LL * NCOMP * IPC_SLOT;

// LDS carve (compute); the copier reuses the same dynamic allocation
constexpr int LS = BROWS + 4;                          // [16][LS] fp32 images (float4-aligned rows)
constexpr int L_ZBUF = 0;                              // [8 waves][NBT][64] f32x4 forward partials  57344
constexpr int L_A2T = L_ZBUF + 8 * NBT * 64 * 16;      // [16 hidden][LS] a2
constexpr int L_DZ2T = L_A2T + 16 * LS * 4;            // [16 hidden][LS] dz2
constexpr int L_DZ3T = L_DZ2T + 16 * LS * 4;           // [16 class][LS] dz3
constexpr int L_W2 = L_DZ3T + 16 * LS * 4;             // [16 hidden][16 class] W2 of block j
constexpr int L_B1 = L_W2 + 1024;                      // [16]
constexpr int L_B2 = L_B1 + 64;                        // [16]
constexpr int L_RDB1 = L_B2 + 64;                      // [8][16]
constexpr int L_RDB2 = L_RDB1 + 512;                   // [8][16]
constexpr int L_RMET = L_RDB2 + 512;                   // [8][2]
constexpr int L_FLAG = L_RMET + 64;
// x operands of one step for this workgroup's feature slice, staged by wave 7
// with LDS-DMA (global_load_lds_dwordx4, lane-linear 1 KiB pieces) instead of
// fragment-shaped global loads in every wave (16 cache lines per instruction:
// those loads were TA-bound, ~2.5 us of every step)
constexpr int XF_ROW = 13 * 16;                        // [128 rows][13 tiles x 16 features] u8: rows < 112 staged,
constexpr int L_XF = L_FLAG + 64;                      // rows 112..127 zeroed once per launch (the weight
constexpr int XF_CHUNKS = BROWS * 13;                  // gradient's K = 128 batch rows); 1456 x 16 B staged
constexpr int L_LAB = L_XF + XTS * XF_ROW;             // [128] labels
constexpr int PS = XTS + 8;                            // split mode: bf16 plane row stride (elements)
constexpr int L_DZP = L_LAB + 128;                     // split mode: [3 pieces][16 hidden][PS] dz2 bf16
constexpr int L_HFLAG = L_DZP + 3 * 16 * PS * 2;       // [16] flags (step + 1): 0..6 head of batch tile v, 7 stage, 8..14 its partials
constexpr int L_DW2P = L_HFLAG + 64;                   // [7 batch tiles][64 lanes] f32x4 dW2 partials
constexpr int L_RLOSS = L_DW2P + NBT * 64 * 16;        // [2][128] per-row loss / correct of the step
constexpr int LDS_COMPUTE = L_RLOSS + 2 * 128 * 4;
static_assert(L_XF % 1024 == 0 && L_LAB % 16 == 0, "LDS-DMA bases");
static_assert(L_DW2P % 16 == 0, "dW2 partials: 16-B lanes");
constexpr int CROW = DIN + 16;                         // copier LDS row stride (800)
constexpr int LDS_COPIER = BROWS * CROW;               // 89600
constexpr int LDS_BYTES = LDS_COMPUTE > LDS_COPIER ? LDS_COMPUTE : LDS_COPIER;

struct Args {
  const uint8_t* stage;     // this chunk: nsteps records of REC bytes
  long long rec_h;          // host record bytes (B*785 rounded up to 16)
  int B, nsteps;
  float* params;            // flat fp32 master, TF variable order (read at start, written at end)
  const float* lr;
  float* metrics;
  int ring;
  int act, naive;
  long long* gstep;
  unsigned long long* seq;  // exchange sequence number (monotonic across launches)
  uint8_t* xbuf;            // granule exchange buffer (XBUF_BYTES, zeroed once)
  int* err;
  long long timeout;        // s_memrealtime ticks (100 MHz)
  long long* step_ts;       // optional: s_memrealtime at the start of every global step (ring)
  int ts_ring;
  const uint8_t* host_next; // device-visible pointer into pinned host memory
  int next_steps;
  uint8_t* stage_next;
  void* const* peer_base;   // N GPUs: IPC-mapped exchange buffers of every rank
  int W, rank;
  int gbf16;                // N GPUs: dW1 payload in bf16 (BASELINE config #2) instead of fp32
  int spread;               // placement: 0 packed on one XCD (default), 1 spread (several ranks per GPU)
  long long* phase_ts;      // optional phase stamps: [step < 64][workgroup 64][16] (wave 0 / wave 7, lane 0),
                            // then [64][workgroup 64][16] launch stamps (prologue / epilogue / copier)
  int xmode;                // N GPUs: 0 one-shot (every workgroup reads its slot from every peer),
                            // 1 two-shot (reduce-scatter by wave chunk, then all-gather of the sums)
  long long fault_step;     // fault injection (mlpf_set_fault(rank, step), tests of the bench's fallback):
  int fault_rank;           // that rank stops publishing its exchange flag from that global step on, a dead
                            // peer (-1: off; one skipped flag alone is absorbed: the flags are monotonic)
  // flat master layout: W1 at params[0..78400); W2 / b1 / b2 through their own
  // pointers (params + OFF_* for the flat trainer; a graph's own variables for the
  // resident Session engine)
  float* p_w2;
  float* p_b1;
  float* p_b2;
  // RESIDENT (Session engine, compat/resident.py): one launch serves many
  // Session.run calls.  Host -> device: a doorbell and 2 pinned record slots;
  // device -> host: metrics + a done count in pinned memory.  Exits by itself
  // after `idle` ticks without a doorbell (or on door < 0).
  const long long* door;    // pinned: runs made ready (run k ready when door > k); < 0: stop
  const uint8_t* host_recs; // pinned: 2 slots of rec_h bytes (B x 784 pixels, B labels)
  const float* host_lr;     // pinned: lr of each slot
  float* host_out;          // pinned: [loss, accuracy, global step] of the last run
  long long* host_done;     // pinned: runs completed
  long long* host_state;    // pinned: id of the launch that exited
  long long launch_id, run0, idle;
  unsigned census_tag;      // per-launch placement-census tag from the host (no device load in front of the census)
  void* gvar;               // the graph's global_step variable and its dtype code (csrc/gstep_kind.h)
  int gvar_kind;
  unsigned* dctr;           // device: [0] records staged, [8] runs released, [16] stop, [32] steps done
  long long* res_ts;        // profiling only (DTF_RESIDENT_STAMPS): [run % 64][8] resident per-run stamps
  int dbg;                  // profiling only (DTF_PERSIST_DBG): bit 0 = never stage the next step's x (wrong
                            // numerics; what the per-step LDS-DMA stage costs the hand-offs), bit 1 = head
                            // sub-phase stamps (slots 13-15, wave 0), bit 2 = wave 7 too prepares the next
                            // step's operands on the late path, after P2 (same bits as its early path:
                            // tests/test_mlp_persist_operand_prep_gpu.py), bit 3 = step-boundary stamps
                            // of every wave (PHB below; needs phase_ts), bit 4 = the weight-gradient
                            // chunks wait for the heads' second flag, behind the dW2 / db2 partial and
                            // workgroup 0's loss / hit rows (one flag's order, same bits:
                            // tests/test_mlp_persist_head_gpu.py)
};

// resident per-run stamp (s_memrealtime, 100 MHz) -- profiling only: 0 copier 0
// saw the doorbell, 1 copier 0 staged its rows, 2 compute workgroup 0 saw the
// whole record staged, 3 record in LDS / registers, 4 step math done, 5
// variables written through, 6 every workgroup arrived, 7 done count published
#define RTS(k, slot)                                                                             \
  if (a.res_ts != nullptr) a.res_ts[((k) & 63) * 8 + (slot)] = (long long)__builtin_amdgcn_s_memrealtime();
// the same in compute: instrumented instantiations only
#define RTSC(k, slot) \
  if constexpr (INS) { RTS(k, slot); }
// phase stamp ph of step st (s_memrealtime, 100 MHz) -- profiling only: compiled
// into the instrumented instantiations (INS) alone, absent from production code
#define PH(ph)                                                                                   \
  if constexpr (INS) {                                                                           \
    if (a.phase_ts != nullptr && lane == 0 && st < 64)                                           \
      a.phase_ts[((long long)st * 64 + c) * 16 + (ph)] = (long long)__builtin_amdgcn_s_memrealtime(); \
  }
// DTF_PERSIST_DBG bit 1: wave 0 stamps the head's sub-phases into slots 13-15 (wave 7's stamps off)
#define PHX(ph) \
  if ((dbg & 2) != 0) { PH(ph); }
#define PH7(ph) \
  if ((dbg & 2) == 0) { PH(ph); }
// DTF_PERSIST_DBG bit 3: step-boundary stamps of every wave, lane 0, in the 16
// slots of the unused workgroup row 32 + c (the rows of c keep wave 0's stamps):
// w = wave w arrives at barrier A, 8 + w = head wave w done (first flag set), 15 = wave
// 7's W2 / b1 / b2 updates stored.  Wave 7's slot 15 of row c is then its last
// chunk's MFMAs issued (not the stage landing)
#define PHB(slot)                                                                                \
  if constexpr (INS) {                                                                           \
    if ((dbg & 8) != 0 && a.phase_ts != nullptr && lane == 0 && st < 64)                         \
      a.phase_ts[((long long)st * 64 + 32 + c) * 16 + (slot)] = (long long)__builtin_amdgcn_s_memrealtime(); \
  }

// The exact three-way split v = hi + mid + lo by truncation, as fp32 bit
// patterns whose low 16 bits are zero: hi keeps v's top 8 significant bits, the
// remainder r = v - hi is exact (<= 16 bits), mid keeps its top 8, and r - mid
// has <= 8 significant bits, so lo is exact too (normal range).  4 VALU ops.
// (mlp_gemm.hip's split3 is another function: it rounds each piece to nearest, this one truncates.)
__device__ __forceinline__ void split3(float v, uint32_t& h, uint32_t& m, uint32_t& l) {
  h = __float_as_uint(v) & 0xffff0000u;
  const float r1 = v - __uint_as_float(h);
  m = __float_as_uint(r1) & 0xffff0000u;
  l = __float_as_uint(r1 - __uint_as_float(m));
}
// two split fp32 patterns -> one packed bf16 pair (upper halves)
__device__ __forceinline__ uint32_t hi2(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }
// 8 fp32 -> the three bf16x8 pieces
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& H, bf16x8& M, bf16x8& L) {
  u32x4 ph, pm, pl;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t h0, m0, l0, h1, m1, l1;
    split3(v[2 * k], h0, m0, l0);
    split3(v[2 * k + 1], h1, m1, l1);
    ph[k] = hi2(h0, h1);
    pm[k] = hi2(m0, m1);
    pl[k] = hi2(l0, l1);
  }
  H = __builtin_bit_cast(bf16x8, ph);
  M = __builtin_bit_cast(bf16x8, pm);
  L = __builtin_bit_cast(bf16x8, pl);
}
// 8 pixel bytes (two dwords) -> 8 bf16, exact (<= 8 significant bits): upper half of the f32
__device__ __forceinline__ bf16x8 px8(uint32_t w0, uint32_t w1) {
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t wd = k < 2 ? w0 : w1;
    const int sh = (k & 1) * 16;
    const float f0 = (float)((wd >> sh) & 0xffu), f1 = (float)((wd >> (sh + 8)) & 0xffu);
    o[k] = hi2(__float_as_uint(f0), __float_as_uint(f1));
  }
  return __builtin_bit_cast(bf16x8, o);
}

// launch-level stamp k of workgroup slot wg (compute c, copier NCOMP + cid), one lane
#define PRO(wg, k)                                                                             \
  if (a.phase_ts != nullptr)                                                                   \
    a.phase_ts[((long long)64 * 64 + (wg)) * 16 + (k)] = (long long)__builtin_amdgcn_s_memrealtime();
// the same in compute: instrumented instantiations only
#define PROC(wg, k) \
  if constexpr (INS) { PRO(wg, k); }

__device__ __forceinline__ float ub(uint32_t w, int e) { return (float)((w >> (8 * e)) & 0xffu); }

__device__ __forceinline__ void lds_barrier() {   // orders LDS only: no vmcnt(0) on in-flight prefetches
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// one lane-linear LDS-DMA piece: lane l's 16 bytes at gsrc land at lds + 16 l
__device__ __forceinline__ void glds16(const void* gsrc, uint8_t* lds) {
  __builtin_amdgcn_global_load_lds((gvoid*)(gsrc), (lvoid*)(lds), 16, 0, 0);
}

// Granule hand-off through a buffer resource over a wave-uniform region (one
// descriptor per edge and step; slot and lane go into the VGPR offset).
// Producer: 4 floats -> 4 granules {value, tag} in two 16-byte write-through
// (sc1) stores; consumer: two L1-bypassing (sc1) 16-byte loads, valid when all
// four tags match (8-byte halves of a 16-byte sc1 store are observed untorn on
// gfx950: MI355X_MICROARCH.md "Valid forms", R2).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t region_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
// l2_local: every consumer shares the producer's XCD (verified at launch) ->
// plain stores, the lines stay in that L2 where the consumers' sc1 loads hit;
// otherwise write-through (sc1) stores, visible to other XCDs' sc1 loads.
__device__ __forceinline__ void put_gran(__amdgpu_buffer_rsrc_t rs, int voff, f32x4 v, unsigned tag, bool l2_local) {
  const u32x4 lo = {__float_as_uint(v[0]), tag, __float_as_uint(v[1]), tag};
  const u32x4 hi = {__float_as_uint(v[2]), tag, __float_as_uint(v[3]), tag};
  if (l2_local) {
    __builtin_amdgcn_raw_buffer_store_b128(lo, rs, voff, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(hi, rs, voff + 16, 0, 0);
  } else {
    __builtin_amdgcn_raw_buffer_store_b128(lo, rs, voff, 0, 16);
    __builtin_amdgcn_raw_buffer_store_b128(hi, rs, voff + 16, 0, 16);
  }
}

// lane l <- lane l^16 / l^32 with gfx950's VALU row swaps
__device__ __forceinline__ float xor16(float v) {
  const auto p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(((threadIdx.x >> 4) & 1) ? p[0] : p[1]);
}
__device__ __forceinline__ float xor32(float v) {
  const auto p = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float((threadIdx.x & 32) ? p[0] : p[1]);
}

// Gather the N granule slots slot(k) (k != skip) of this lane until every tag
// matches; part[skip] = own (constant-index selects only: a runtime index would
// demote the array to scratch).  `need` false: this lane takes no data (zeros;
// it still joins the wave-wide exit test) and loads at an offset past the
// region's range, which the buffer unit answers with zeros and no traffic.
//
// A pass walks the slots in groups of GRP.  A group first issues both 16-byte
// sc1 loads of every slot that some lane of the wave still lacks (a scalar
// branch per slot: a slot the whole wave holds costs nothing in later passes),
// with no wait and no lane mask between the issues, and only then compares
// tags, so a group costs one L2 round trip plus issue, not one per slot.  A
// lane takes slot k in the pass in which all four tags of its two loads match,
// merged into part[k] under !have[k]; part[k] is not touched again (no order
// between a producer's lanes, so a later pass may see other bytes there).  A
// slot in flight is 8 VGPRs per lane: GRP bounds them.  Before this, the pass
// was `if (!have[k]) have[k] = get(...)` per lane, which compiled to one
// divergent region per slot with a vmcnt(0) in each: N serial round trips
// (scripts/probes/gather_pass_shape.py reads this off the generated code;
// tests/test_mlp_persist_gather_shape_cpu.py holds it).  false on timeout / error.
constexpr int OOB_OFF = 0x7ffffff0;   // a buffer offset past every region's range
// E2's group size: 7 slots, 6 of them live, as 4 + 3.  6 and 7 leave the resident
// instrumented instantiation with scratch; 4 measured 0.1 % above 5 and leaves
// the N-GPU kernels 8 VGPRs more (profiles/mlp_persist_f32_gather_inflight_ab.json)
constexpr int E2_GRP = 4;
template <int N, int GRP, typename SlotOff>
__device__ __forceinline__ bool gather_gran(__amdgpu_buffer_rsrc_t rs, SlotOff slot, int skip, bool need, unsigned tag,
                                            f32x4 own, f32x4 (&part)[N], int lane, const Args& a) {
  bool have[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    have[k] = (k == skip) || !need;
    part[k] = (k == skip) ? own : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // a lane that takes no data loads past the region's range (zeros, no traffic)
  const unsigned base = need ? 32u * (unsigned)lane : (unsigned)OOB_OFF;
  u32x4 lo[GRP] = {}, hi[GRP] = {};   // a group's raw granules: 8 VGPRs per slot in flight
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  // the clock and the error word are checked every 8th pass only
  for (int it = 1;; ++it) {
    asm volatile("" ::: "memory");   // re-load every pass (no loop-invariant hoisting)
    bool all = true;
#pragma unroll
    for (int g0 = 0; g0 < N; g0 += GRP) {
      bool go[GRP];
      // issue: every outstanding slot's two loads, no wait and no lane mask between them
#pragma unroll
      for (int i = 0; i < GRP; ++i) {
        const int k = g0 + i;
        go[i] = k < N && __any(!have[k < N ? k : 0]);
        if (go[i]) {
          const int voff = (int)(base + (unsigned)slot(k));
          lo[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 16);
          hi[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff + 16, 0, 16);
        }
      }
      // the registers as the loads left them, slot by slot, after the last issue:
      // the compiler neither sinks a load to its use nor regroups the group's
      // registers into one wide value with copies (and waits) between the issues
#pragma unroll
      for (int i = 0; i < GRP; ++i) asm volatile("" : "+v"(lo[i]), "+v"(hi[i]));
      // accept: all four tags of the lane's two loads match
#pragma unroll
      for (int i = 0; i < GRP; ++i) {
        const int k = g0 + i;
        if (k < N && go[i]) {
          const bool hit = lo[i][1] == tag && lo[i][3] == tag && hi[i][1] == tag && hi[i][3] == tag;
          const bool take = hit && !have[k];
          const f32x4 v = {__uint_as_float(lo[i][0]), __uint_as_float(lo[i][2]), __uint_as_float(hi[i][0]),
                           __uint_as_float(hi[i][2])};
#pragma unroll
          for (int c = 0; c < 4; ++c) part[k][c] = take ? v[c] : part[k][c];
          have[k] = have[k] || hit;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) all = all && have[k];
    if (__all(all)) return true;
    if ((it & 7) == 0 && ((long long)__builtin_amdgcn_s_memrealtime() - t0 > a.timeout ||
                          __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
      if (lane == 0) atomicOr(a.err, 1);
      return false;
    }
  }
}

// ------------------------------------------------------------------ N-GPU exchange loads
// Peer IPC buffers are read with 16-B (8-B / 4-B) system-scope loads (sc0 sc1:
// never served from a cache of this device) through a wave-uniform buffer
// resource per rank.  Loads of ranks outside `sel`, of ranks >= W and of
// masked lanes use an offset past the buffer's range: the buffer unit returns
// zero without touching memory, so the NW loads of a lane stay unconditional
// (no branch, no wait between them: all in flight at once) and only payload
// crosses the fabric.
constexpr int SYS = 1 | 16;            // sc0 | sc1
// one resource per rank, built once per launch in SGPRs (the table entry is read
// by one lane and broadcast: a per-use vector load of the pointer would turn
// every peer load into a waterfall loop behind a vmcnt(0))
template <int NW>
struct PeerRs {
  __amdgpu_buffer_rsrc_t r[NW];
};
template <int NW>
__device__ __forceinline__ PeerRs<NW> peer_rsrcs(void* const* peers, int W) {
  PeerRs<NW> o;
#pragma unroll
  for (int r = 0; r < NW; ++r) {
    const unsigned long long u = reinterpret_cast<unsigned long long>(peers[r < W ? r : 0]);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    void* pp = reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo);
    o.r[r] = __builtin_amdgcn_make_buffer_rsrc(pp, 0, (int)IPC_BYTES, 0x00020000);
  }
  return o;
}
__device__ __forceinline__ f32x4 unbf4(uint32_t lo, uint32_t hi) {
  return f32x4{__uint_as_float(lo << 16), __uint_as_float(lo & 0xffff0000u), __uint_as_float(hi << 16),
               __uint_as_float(hi & 0xffff0000u)};
}
__device__ __forceinline__ f32x4 round_bf16x4(f32x4 v) {
  const uint32_t lo = pack2bf(v[0], v[1]), hi = pack2bf(v[2], v[3]);
  return unbf4(lo, hi);
}
// Rank-order sum of this lane's dW1 entries over the W ranks (this rank's own
// term G0 / G1 from registers), GRP peer loads in flight per group.  BF: both
// tiles' bf16 in ONE 16-B entry at e0 (TWO false: the wave has one tile, 8 B);
// fp32: one 16-B entry per tile at e0 / e1.
template <int NW, int GRP, bool BF, bool TWO>
__device__ __forceinline__ void sum_entries(const PeerRs<NW>& prs, int W, int rank, int so, bool hv, int e0, int e1,
                                            f32x4& G0, f32x4& G1) {
  f32x4 S0 = {0.f, 0.f, 0.f, 0.f}, S1 = S0;
#pragma unroll
  for (int r0 = 0; r0 < NW; r0 += GRP) {
    if (r0 >= W) break;   // wave-uniform
    u32x4 v0[GRP], v1[GRP];
#pragma unroll
    for (int i = 0; i < GRP; ++i) {
      const int r = r0 + i;
      const bool on = r < W && r != rank && hv;
      const auto rs = prs.r[r];
      if constexpr (BF) {
        if constexpr (TWO) {
          v0[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, on ? so + e0 : OOB_OFF, 0, SYS);
        } else {
          const u32x2 h = __builtin_amdgcn_raw_buffer_load_b64(rs, on ? so + e0 : OOB_OFF, 0, SYS);
          v0[i] = u32x4{h[0], h[1], 0u, 0u};
        }
      } else {
        v0[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, on ? so + e0 : OOB_OFF, 0, SYS);
        if constexpr (TWO) v1[i] = __builtin_amdgcn_raw_buffer_load_b128(rs, on ? so + e1 : OOB_OFF, 0, SYS);
      }
    }
#pragma unroll
    for (int i = 0; i < GRP; ++i) {
      const int r = r0 + i;
      if (r >= W) break;
      const bool me = r == rank;
      f32x4 P0, P1 = {0.f, 0.f, 0.f, 0.f};
      if constexpr (BF) {
        P0 = unbf4(v0[i][0], v0[i][1]);
        if constexpr (TWO) P1 = unbf4(v0[i][2], v0[i][3]);
      } else {
        P0 = __builtin_bit_cast(f32x4, v0[i]);
        if constexpr (TWO) P1 = __builtin_bit_cast(f32x4, v1[i]);
      }
      S0 += me ? G0 : P0;
      S1 += me ? G1 : P1;
    }
  }
  G0 = S0;
  G1 = S1;
}
// wave 7's small part: rank-order sums of the dW2 entry (16 B, lanes with data)
// and db1 / db2 (4 B)
template <int NW>
__device__ __forceinline__ void sum_small(const PeerRs<NW>& prs, int W, int rank, int so, bool dlane, bool blane,
                                          int lane, f32x4& D, float& gb) {
  u32x4 d[NW];
  uint32_t b[NW];
#pragma unroll
  for (int r = 0; r < NW; ++r) {
    const bool on = r < W && r != rank;
    const auto rs = prs.r[r];
    d[r] = __builtin_amdgcn_raw_buffer_load_b128(rs, (on && dlane) ? so + lane * 16 : OOB_OFF, 0, SYS);
    b[r] = __builtin_amdgcn_raw_buffer_load_b32(rs, (on && blane) ? so + 1024 + lane * 4 : OOB_OFF, 0, SYS);
  }
  f32x4 SD = {0.f, 0.f, 0.f, 0.f};
  float SB = 0.f;
#pragma unroll
  for (int r = 0; r < NW; ++r) {
    if (r >= W) break;
    const bool me = r == rank;
    SD += me ? D : __builtin_bit_cast(f32x4, d[r]);
    SB += me ? gb : __uint_as_float(b[r]);
  }
  D = SD;
  gb = SB;
}

// ------------------------------------------------------------------ copier
// task = one step of the next chunk: 112 rows of 784 pixels from the pinned host
// record into LDS (rows >= B zero), then the row-major image and the labels
// into the device stage.
__device__ void copier(const Args& a, int cid, uint8_t* smem) {
  const int tid = threadIdx.x;
  const int B = a.B;
  if (tid == 0) { PRO(NCOMP + cid, 0); }
  for (int st = cid; st < a.next_steps; st += NCOP) {
    const uint8_t* src = a.host_next + (long long)st * a.rec_h;
    uint8_t* dst = a.stage_next + (long long)st * REC;
    constexpr int C16 = DIN / 16;   // 49
    for (int k = tid; k < BROWS * C16; k += THREADS) {
      const int row = k / C16, c = k % C16;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (row < B) v = reinterpret_cast<const uint4*>(src)[row * C16 + c];
      *reinterpret_cast<uint4*>(smem + row * CROW + 16 * c) = v;
    }
    if (tid < 128) dst[XROW_BYTES + tid] = tid < B ? src[(long long)B * DIN + tid] : (uint8_t)0;
    __syncthreads();
    for (int k = tid; k < BROWS * C16; k += THREADS) {
      const int row = k / C16, c = k % C16;
      reinterpret_cast<uint4*>(dst)[row * C16 + c] = *reinterpret_cast<const uint4*>(smem + row * CROW + 16 * c);
    }
    __syncthreads();
  }
  if (tid == 0) { PRO(NCOMP + cid, 1); }
}

// RES copier: copier 0 watches the doorbell (system-scope loads of pinned host
// memory) and releases run k to the others, or stops the launch after `idle`
// ticks without one (or on door < 0) and reports that to the host; copiers
// 0..13 each move 8 batch rows of the run's pinned record into device stage
// slot (st & 1): row-major image, labels + lr (copier 0); every store write-through (sc1), then
// every wave's vmcnt(0), the barrier and one agent add to the staged count.
__device__ void copier_res(const Args& a, int cid, uint8_t* smem) {
  if (cid >= NCOPR) return;
  const int tid = threadIdx.x;
  constexpr int RR = 8;                                   // rows per copier
  int* dec = reinterpret_cast<int*>(smem + RR * CROW);
  const int B = a.B;
  const int hb = (int)(2 * a.rec_h);
  const auto hrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.host_recs), 0, hb, 0x00020000);
  for (int st = 0;; ++st) {
    const long long k = a.run0 + st;
    if (tid == 0) {
      // every copier watches the doorbell (no second hop through a device flag);
      // copier 0 alone may stop the launch: its rows complete every record, so a
      // run it did not take never reaches the compute workgroups' staged count
      int d = 1;
      const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
      const long long lim = cid == 0 ? a.idle : a.idle + a.timeout;
      for (;;) {
        const long long v = __hip_atomic_load(a.door, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (v < 0) { d = 0; break; }
        if (v > k) break;
        if (cid != 0 && __hip_atomic_load(a.dctr + 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { d = 0; break; }
        if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > lim) { d = 0; break; }
        __builtin_amdgcn_s_sleep(1);
      }
      if (cid == 0 && !d) __hip_atomic_store(a.dctr + 16, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cid == 0 && d) { RTS(k, 0); }
      *dec = d;
    }
    __syncthreads();
    if (*dec == 0) break;
    const int slot = (int)(k & 1);
    const int hbase = slot * (int)a.rec_h;
    const int r0 = RR * cid;
    uint8_t* dst = const_cast<uint8_t*>(a.stage) + (long long)(st & 1) * REC;
    constexpr int C16 = DIN / 16;   // 49
    // pinned rows -> LDS (rows >= B zero): 16-B system-scope loads, a thread's
    // NLD loads all issued before the first LDS store (one host-memory round
    // trip, not NLD of them in series)
    constexpr int NLD = (RR * C16 + THREADS - 1) / THREADS;
    u32x4 hv[NLD];
    uint32_t lv = 0;   // copier 0, threads < 32: a label dword or the run's lr
    if (cid == 0 && tid < 32) {
      if (4 * tid == RES_LR_BYTE)
        lv = __float_as_uint(__hip_atomic_load(a.host_lr + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
      else
        lv = __builtin_amdgcn_raw_buffer_load_b32(hrs, 4 * tid < B ? hbase + B * DIN + 4 * tid : OOB_OFF, 0, SYS);
    }
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int t = tid + i * THREADS;
      const int rr = t / C16, cc = t % C16;
      const int row = r0 + rr;
      hv[i] = __builtin_amdgcn_raw_buffer_load_b128(hrs, (t < RR * C16 && row < B) ? hbase + row * DIN + 16 * cc : OOB_OFF,
                                                    0, SYS);
    }
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int t = tid + i * THREADS;
      if (t < RR * C16) *reinterpret_cast<u32x4*>(smem + (t / C16) * CROW + 16 * (t % C16)) = hv[i];
    }
    __syncthreads();
    for (int t = tid; t < RR * C16; t += THREADS) {
      const int rr = t / C16, cc = t % C16;
      const u32x4 v = *reinterpret_cast<const u32x4*>(smem + rr * CROW + 16 * cc);
      __builtin_amdgcn_raw_buffer_store_b128(v, region_rsrc(dst, (int)REC), (r0 + rr) * DIN + 16 * cc, 0, 16);
    }
    if (cid == 0 && tid < 32) {   // labels (dwords 0..27) and the run's lr (byte RES_LR_BYTE), loaded with the rows
      uint32_t v = lv;
      if (4 * tid != RES_LR_BYTE) {
        const int nv = B - 4 * tid;   // valid label bytes in this dword
        if (nv < 4) v = nv <= 0 ? 0u : (v & ((1u << (8 * nv)) - 1u));
      }
      __builtin_amdgcn_raw_buffer_store_b32(v, region_rsrc(dst, (int)REC), (int)XROW_BYTES + 4 * tid, 0, 16);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      __hip_atomic_fetch_add(a.dctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (cid == 0) { RTS(k, 1); }
    }
  }
  if (cid == 0 && tid == 0)   // no further run is taken by this launch
    __hip_atomic_store(a.host_state, a.launch_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------ compute
// ACT 0 sigmoid, 1 relu; MULTI: N-GPU gradient exchange; SPLIT: the two big
// GEMMs (forward x W1, weight gradient x^T dz2) on bf16 MFMA through the exact
// three-way split of their fp32 operand (pixels are exact in bf16), so every
// product is exact and accumulates in fp32 -- 16x16x32 bf16 MFMAs at 8x the
// f32-MFMA rate; the head stays on f32-input MFMA
// INS: the instrumented build (phase / per-run stamps, the DTF_PERSIST_DBG
// bits) -- production instantiations carry none of that code
template <int ACT, int NW, bool SPLIT, bool RES, bool INS = false>
__device__ void compute(const Args& a, const int j, const int q, uint8_t* smem) {
  const int dbg = INS ? a.dbg : 0;
  constexpr bool MULTI = NW > 1;
  // w through readfirstlane: the compiler then knows it is wave-uniform, so the
  // per-wave conditions (w == 7, w < NBT, the tile-valid flags) are scalar
  // branches, not 64-bit lane masks hoisted out of the step loop
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int c = j * NQ + q;
  const int B = a.B;
  f32x4* zbuf = reinterpret_cast<f32x4*>(smem + L_ZBUF);
  float* a2T = reinterpret_cast<float*>(smem + L_A2T);
  float* dz2T = reinterpret_cast<float*>(smem + L_DZ2T);
  float* dz3T = reinterpret_cast<float*>(smem + L_DZ3T);
  float* w2s = reinterpret_cast<float*>(smem + L_W2);
  float* b1s = reinterpret_cast<float*>(smem + L_B1);
  float* b2s = reinterpret_cast<float*>(smem + L_B2);
  float* rdb2 = reinterpret_cast<float*>(smem + L_RDB2);
  int* abort_flag = reinterpret_cast<int*>(smem + L_FLAG);
  int* census = abort_flag + 1;
  uint16_t* dzp = reinterpret_cast<uint16_t*>(smem + L_DZP);
  if (tid == 0) { PROC(c, 0); }

  // ---- load state: every global load of the prologue is issued first (the
  // master weights, the small parameters into registers, the step / sequence /
  // lr scalars); the LDS stores that consume them come after the LDS clears, so
  // no store waits on a load before the next load is even issued (~2 us of every
  // launch when the W2 / b loads fed LDS stores ahead of the W1 loads)
  const int hid = 16 * j + r;       // this lane's hidden unit in the W1 / dW1 layouts
  const bool hv = hid < HID;
  // wave w owns local feature tiles w and w + 8 of the slice (global tile ft[k])
  const int nt = ntile(q);
  // (constant-index scalars, not arrays a lambda captures: those would live in scratch)
  const bool tv0 = w < nt, tv1 = w + 8 < nt;
  const int ft0 = tile0(q) + w, ft1 = tile0(q) + (tv1 ? w + 8 : 0);
  auto tvk = [=](int k) { return k ? tv1 : tv0; };
  auto ftk = [=](int k) { return k ? ft1 : ft0; };
  // W1 slice: 16-byte loads of 4 consecutive hidden units of one feature row
  // (the 16 lanes of a lane group cover a 4-row x 16-unit block: 4 cache lines
  // per load), transposed across those lanes after the prologue's drain so lane
  // (r, g) holds unit 16j + r of rows 4g..4g+3 -- the accumulator layout of dW1.
  // (4-byte column loads touched 64 lines per wave instruction: ~2 us of issue
  // at the top of every launch.)
  // (RES keeps the column loads: the transposes' registers spill there, and its
  // prologue runs once per idle period, not once per timed launch)
  float Wt[NTW][4];
  f32x4 wld[NTW];
  if constexpr (RES) {
#pragma unroll
    for (int k = 0; k < NTW; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        Wt[k][e] = (tvk(k) && hv) ? a.params[(16 * ftk(k) + 4 * g + e) * HID + hid] : 0.f;
  } else if constexpr (MULTI) {   // (N GPUs: the branchy loads -- the unconditional ones below spill there)
    const int u0 = 16 * j + 4 * (r & 3);
#pragma unroll
    for (int k = 0; k < NTW; ++k)
      wld[k] = (tvk(k) && u0 < HID)
                   ? *reinterpret_cast<const f32x4*>(a.params + (16 * ftk(k) + 4 * g + (r >> 2)) * HID + u0)
                   : f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
    // unconditional buffer loads (an absent tile / padding unit reads past the
    // range: zero, no branch) -- a conditional load's result merged at the branch
    // end cost a vmcnt(0) right behind it, one serial HBM round trip per launch
    const int u0 = 16 * j + 4 * (r & 3);           // units 4(r&3)..+3 of block j, row 4g + (r >> 2)
    const auto rw1 = __builtin_amdgcn_make_buffer_rsrc(a.params, 0, DIN * HID * 4, 0x00020000);
#pragma unroll
    for (int k = 0; k < NTW; ++k)
      wld[k] = __builtin_bit_cast(
          f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                     rw1, (tvk(k) && u0 < HID) ? ((16 * ftk(k) + 4 * g + (r >> 2)) * HID + u0) * 4 : OOB_OFF, 0, 0));
  }
  // this thread's W2 / b1 / b2 entry (threads < 288): three unconditional loads,
  // at most one in range, OR-ed (the others read zero)
  float pv = 0.f;
  if constexpr (MULTI) {
    if (tid < 256) {
      const int n = tid >> 4, cl = tid & 15;
      const int hn = 16 * j + n;
      pv = (hn < HID && cl < NCLS) ? a.p_w2[hn * NCLS + cl] : 0.f;
    } else if (tid < 272) {
      const int hn = 16 * j + (tid - 256);
      pv = hn < HID ? a.p_b1[hn] : 0.f;
    } else if (tid < 288) {
      const int cl = tid - 272;
      pv = cl < NCLS ? a.p_b2[cl] : 0.f;
    }
  } else {
    const int n = tid >> 4, cl = tid & 15, hn = 16 * j + n, hb = 16 * j + (tid - 256), c2 = tid - 272;
    const auto rw2 = __builtin_amdgcn_make_buffer_rsrc(a.p_w2, 0, HID * NCLS * 4, 0x00020000);
    const auto rb1 = __builtin_amdgcn_make_buffer_rsrc(a.p_b1, 0, HID * 4, 0x00020000);
    const auto rb2 = __builtin_amdgcn_make_buffer_rsrc(a.p_b2, 0, NCLS * 4, 0x00020000);
    const uint32_t v0 =
        __builtin_amdgcn_raw_buffer_load_b32(rw2, (tid < 256 && hn < HID && cl < NCLS) ? (hn * NCLS + cl) * 4 : OOB_OFF, 0, 0);
    const uint32_t v1 =
        __builtin_amdgcn_raw_buffer_load_b32(rb1, (tid >= 256 && tid < 272 && hb < HID) ? hb * 4 : OOB_OFF, 0, 0);
    const uint32_t v2 =
        __builtin_amdgcn_raw_buffer_load_b32(rb2, (tid >= 272 && tid < 288 && c2 < NCLS) ? c2 * 4 : OOB_OFF, 0, 0);
    pv = __uint_as_float(v0 | v1 | v2);
  }
  // the step / sequence / lr scalars stay in VGPRs until the prologue's drain
  // (converted to SGPRs there): a readfirstlane right behind each load waited
  // for it, another serial round trip in front of the stage and census
  unsigned long long seq0 = *a.seq;
  long long gstep0 = *a.gstep;
  float lr = *a.lr;
  // the placement-census entry goes out before anything waits on a load: its
  // tag is the host's per-launch tag, not the device sequence counter (whose
  // load, with the lr / parameter waits ahead of the LDS stores, held every
  // workgroup's entry back ~2 us per launch)
  const unsigned xcc = __builtin_amdgcn_s_getreg((15 << 11) | (0 << 6) | 20) & 15u;
  unsigned long long* hdr = reinterpret_cast<unsigned long long*>(a.xbuf + HDR_OFF);
  const unsigned tag0 = a.census_tag;
  if (tid == 0)
    __hip_atomic_store(hdr + c, ((unsigned long long)tag0 << 32) | xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int k = tid; k < 3 * 16 * LS; k += THREADS) a2T[k] = 0.f;   // a2T, dz2T, dz3T (batch pad stays 0)
  if constexpr (SPLIT)
    for (int k = tid; k < 3 * 16 * PS; k += THREADS) dzp[k] = (uint16_t)0;   // dz2 planes (batch pad 0)
  // image rows 112..127: never staged, read by the weight gradient's last chunk
  for (int k = tid; k < (XTS - BROWS) * XF_ROW / 16; k += THREADS)
    *reinterpret_cast<u32x4*>(smem + L_XF + BROWS * XF_ROW + 16 * k) = u32x4{0u, 0u, 0u, 0u};
  const bool failed_in = __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;

  // x operands of the wave's feature tiles (registers, read from the LDS stage):
  //  xf[k][bt]: row 16bt+r, features 16ft+4g..+3 (forward B operand)
  //  xt[k][s] : feature 16ft+r, batch 16s+4g..+3 (weight-gradient A operand);
  //             SPLIT: dwords 2c, 2c+1 = batch 32c+8g..+7 (c < 4, batch >= 112 zero)
  //  lab      : label of batch row 16w+r (head, waves < 7)
  constexpr int XTN = SPLIT ? 8 : NBT;
  uint32_t xf[NTW][NBT], xt[NTW][XTN];
  int lab = 0;
  // PREP (one-GPU split engine): the byte -> bf16 conversions of both operand
  // sets are scheduled into the hand-off waits instead of in front of the MFMAs
  //  XF[bt]   : forward B operands of the step about to run, made from xf where the
  //             staged step is read: wave 7 right behind its own DMA wait (early
  //             path), a head wave after P2 (late path), the first step in the prologue
  //  XA[k][c] : weight-gradient A operands of this step, made from xt in the E1 window
  //  lab_n    : the next step's label until this step's head has used `lab`
  // P0 then starts with split8 and its MFMAs, and chunk() has only the dz2 piece
  // reads between a head flag and its MFMAs.  The head waves have no early path.
  // Since the transposing reads halved the stage it lands inside their E2 gather
  // (~0.4 us after the E2 publish), and preparing there between two polls, once
  // wave 7's flag is up, was built and measured: 18-36 % of the head waves took
  // it, every one found its granules there when it came back, and it gained
  // 0.5 % alone and nothing on top of MET_FAST below
  // (profiles/mlp_persist_f32_step_boundary_ab.json).  Converting in the idle
  // polls between chunks measured slower than the late path as well
  // (profiles/mlp_persist_f32_operand_prep_ab.json).
  // (the N-GPU split kernels sit at 225-227 VGPRs: not applied there)
  constexpr bool PREP = SPLIT && !RES && NW == 1;
  // MET_FAST (same engine): workgroup 0's loss / accuracy reduction sits in wave
  // 7's tail in front of barrier A, where it made workgroup 0 arrive ~0.5 us after
  // the other 27 at every step (profiles/mlp_persist_f32_step_boundary_ab.json) --
  // the same sums through VALU lane permutes instead of 12 LDS round trips, and a
  // 32-bit ring slot instead of a 64-bit modulo per step
  constexpr bool MET_FAST = PREP;
  bf16x8 XF[NBT], XA[NTW][4];
  int lab_n = 0;
  // an operand stays where it was made (the compiler neither sinks the
  // conversion to its MFMA nor hoists it to where its bytes were read)
  auto pin8 = [](bf16x8& v) {
    u32x4 t = __builtin_bit_cast(u32x4, v);
    asm volatile("" : "+v"(t));
    v = __builtin_bit_cast(bf16x8, t);
  };
  // local tile of k (an absent second tile reads local tile 0: staged, never used)
  auto tlk = [=](int k) { return k ? (tv1 ? w + 8 : 0) : w; };
  // wave 7: step st's slice -> LDS, lane-linear [row][13 tiles] (rows of 208 B:
  // conflict-free for the forward's dword reads and the weight gradient's
  // transposing reads alike).  One image serves both GEMMs.
  auto stage_x = [&](int st, int n0, int dn) {   // pieces n0, n0 + dn, ...
    const uint8_t* rec = a.stage + (long long)st * REC;
    const uint8_t* xr = rec + 16 * tile0(q);
#pragma unroll 1   // a rolled loop: unrolled, the 23 pieces' addresses get hoisted out of the step loop
    for (int n = n0; n < (XF_CHUNKS + 63) / 64; n += dn) {
      const int k = 64 * n + lane;
      // q = 3's 13th tile reads the next row's first 16 B (row 111: the first 16
      // label bytes; inside the record either way): unused
      if (k < XF_CHUNKS) glds16(xr + (k / 13) * DIN + 16 * (k % 13), smem + L_XF + 1024 * n);
    }
    if (n0 == 0 && lane < 8) glds16(rec + XROW_BYTES + 16 * lane, smem + L_LAB);
  };
  auto read_xf = [&](int& lb) {
#pragma unroll
    for (int k = 0; k < NTW; ++k)
#pragma unroll
      for (int b = 0; b < NBT; ++b)
        xf[k][b] = *reinterpret_cast<const uint32_t*>(smem + L_XF + (16 * b + r) * XF_ROW + 16 * tlk(k) + 4 * g);
    lb = smem[L_LAB + 16 * (w < NBT ? w : NBT - 1) + r];
  };
  // The x^T fragments come out of the row-major image through ds_read_b64_tr_b8:
  // per 16-lane group the 16 lanes' 8-byte pieces, in lane order, form an 8 x 16
  // byte block (lanes 2i, 2i + 1 = its row i, wherever they point), and lane i
  // gets column i, rows 0..7 in byte order (observed on MI355X with
  // scripts/probes/tr8_probe.hip, both modes).  Lane (r, g) supplies byte
  // 16 tile + 8 (r & 1) of a row picked so that the block's rows are the lane's K
  // order, and receives feature 16 tile + r of those 8 batch rows:
  //   SPLIT: row 32c + 8g + (r >> 1) -> batch 32c + 8g .. + 7.  Rows of 208 B = 52
  //     dwords: the 16 rows x 4 dwords of a 32-lane half fall on 64 distinct banks.
  //   else:  row 32c + 16 (r >> 3) + 4g + ((r >> 1) & 3) -> the lo dword is batch
  //     tile 2c's rows 4g .. + 3, the hi dword tile 2c + 1's (tile 7: zero rows,
  //     dropped); rows 16 apart share banks, a 2-way conflict on 8 reads a step.
  //     (The consecutive-row read + permlane exchange of the dwords between lane
  //     groups gave the same operands and cost this engine 0.9 us a step.)
  // Needs EXEC all ones: every call is wave-uniform.
  auto read_xt = [&]() {
    typedef int v2i __attribute__((ext_vector_type(2)));
    typedef __attribute__((address_space(3))) v2i lds_v2i;
    const int row = SPLIT ? 8 * g + (r >> 1) : 16 * (r >> 3) + 4 * g + ((r >> 1) & 3);
#pragma unroll
    for (int k = 0; k < NTW; ++k) {
      const uint8_t* blk = smem + L_XF + row * XF_ROW + 16 * tlk(k) + 8 * (r & 1);
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const v2i v = __builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_v2i*)(blk + 32 * cc * XF_ROW));
        xt[k][2 * cc] = (uint32_t)v.x;
        if (2 * cc + 1 < XTN) xt[k][2 * cc + 1] = (uint32_t)v.y;
      }
    }
  };
  // PREP: the staged step in LDS -> its forward operands XF and label, and its
  // raw x^T bytes (converted one window later, when the step runs)
  auto prep_fwd = [&](int& lb) {
    read_xf(lb);
#pragma unroll
    for (int b = 0; b < NBT; ++b) XF[b] = px8(xf[0][b], xf[1][b]);
#pragma unroll
    for (int b = 0; b < NBT; ++b) pin8(XF[b]);
    read_xt();
  };
  // PREP: this step's raw x^T bytes -> XA (wave 7, always one tile: a tile of
  // ones in the second slot gives db1)
  auto prep_xa = [&]() {
    if constexpr (SPLIT) {
#pragma unroll
      for (int k = 0; k < NTW; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(xt[k][i]));
#pragma unroll
      for (int ch = 0; ch < 4; ++ch) {
        XA[0][ch] = px8(xt[0][2 * ch], xt[0][2 * ch + 1]);
        XA[1][ch] = tv1 ? px8(xt[1][2 * ch], xt[1][2 * ch + 1]) : px8(0x01010101u, 0x01010101u);
      }
#pragma unroll
      for (int k = 0; k < NTW; ++k)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) pin8(XA[k][ch]);
    }
  };
  // Prologue, all latency overlapped (it was three serial phases, ~6 us per
  // launch): the census entry goes out first, the first step's x stage is
  // issued (LDS-DMA) while the parameter loads above are still in flight, and
  // wave 0 polls the census meanwhile; one drain + barrier then covers all three.
  if (tid == 0) { PROC(c, 4); }
  // ---- placement census: E1 group (the NQ slices of block j) and E2 group (the
  // NJ blocks of slice q) each on this workgroup's XCD -> that edge stays in one
  // L2 (plain stores).  Decided per launch from HW_REG_XCC_ID, never assumed.
  // (this workgroup's entry was stored above, right after the loads were issued)
  if constexpr (!RES) stage_x(0, w, 8);   // the first step's stage: every wave a share (RES: per run)
  if (w == 0) {   // lane cc watches workgroup cc's entry: all 28 polls in flight at once
    const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
    unsigned long long v = 0;
    bool seen = lane >= NCOMP, bad = false;
    for (;;) {
      if (!seen) {
        v = __hip_atomic_load(hdr + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        seen = (unsigned)(v >> 32) == tag0;
      }
      if (__all(seen)) break;
      if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > a.timeout) {
        if (lane == 0) atomicOr(a.err, 1);
        bad = true;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    const bool off = lane < NCOMP && (unsigned)v != xcc;   // workgroup `lane` on another XCD
    const bool e1 = !__any(off && lane / NQ == j);
    const bool e2 = !__any(off && lane % NQ == q);
    if (lane == 0) *census = bad ? -1 : ((e1 ? 1 : 0) | (e2 ? 2 : 0));
  }
  // the small parameters' LDS stores wait for their loads: placed after the
  // census entry and the stage DMA are out
  if (tid < 256) {
    w2s[tid] = pv;
  } else if (tid < 272) {
    b1s[tid - 256] = pv;
  } else if (tid < 288) {
    b2s[tid - 272] = pv;
  } else if (tid == 288) {
    *abort_flag = 0;
  } else if (tid >= 296 && tid < 312) {
    reinterpret_cast<int*>(smem + L_HFLAG)[tid - 296] = 0;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // parameter loads + the first stage landed
  if constexpr (!MULTI) {
    asm volatile("" : "+v"(seq0), "+v"(gstep0), "+v"(lr));
    seq0 = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(seq0 >> 32)) << 32) |
           __builtin_amdgcn_readfirstlane((unsigned)seq0);
    gstep0 = (long long)(((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)gstep0 >> 32))
                          << 32) |
                         __builtin_amdgcn_readfirstlane((unsigned)gstep0));
  }
  double gvar0 = 0.0;   // RES: the graph's global_step at launch
  if constexpr (RES) {
    if (a.gvar_kind == 1) gvar0 = *static_cast<const float*>(a.gvar);
    else if (a.gvar_kind == 2) gvar0 = (double)*static_cast<const long long*>(a.gvar);
    else if (a.gvar_kind == 3) gvar0 = *static_cast<const int*>(a.gvar);
    else if (a.gvar_kind == 4) gvar0 = *static_cast<const double*>(a.gvar);
    else gvar0 = (double)gstep0;
  }
  // the 4x4 transposes of the W1 blocks in 4 rounds of one lane permute:
  // in round t the lane that loaded row e_s offers component (e_s + t) & 3, and
  // lane r (unit 4b + m) takes row (m - t) & 3 from lane 4((m - t) & 3) + b --
  // which offers exactly component m
#pragma unroll
  for (int k = 0; k < NTW && !RES; ++k) {
    const int m = r & 3, b = r >> 2;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int cs = (b + t) & 3;          // as a source: this lane loaded row b (= r >> 2)
      const float v = cs == 0 ? wld[k][0] : (cs == 1 ? wld[k][1] : (cs == 2 ? wld[k][2] : wld[k][3]));
      const int e = (m - t) & 3;
      const float got = __shfl(v, 16 * g + 4 * e + b);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (q == e) Wt[k][q] = got;
    }
  }
  __syncthreads();
  float lrB = lr / (float)(B * (MULTI ? a.W : 1));   // RES: per run (the record's lr)
  float lrX = lrB * (1.f / 255.f);
  // an earlier launch failed (err set): nothing runs.  Checked only here, so the
  // wait for that load does not serialize the parameter loads behind it
  if (failed_in || *census < 0) return;
  const bool l2_e1 = (*census & 1) != 0;
  const bool l2_e2 = (*census & 2) != 0;
  if (tid == 0) { PROC(c, 1); }
  if constexpr (PREP) {
    prep_fwd(lab);   // the launch's first step is prepared here
  } else if constexpr (!RES) {
    read_xf(lab);
    read_xt();
  }
  if (tid == 0) { PROC(c, 2); }

  // RES: the run's record -> LDS at the top of every step.  The copiers stored it
  // write-through (sc1) and each added to the staged count after its waves'
  // vmcnt(0) + barrier; one lane polls that count with sc1 loads, the workgroup
  // barrier follows, and every load of the record is an sc1 load to registers
  // (MI355X_MICROARCH.md "Valid forms", first table row) -> the LDS layout of
  // stage_x.  false: stop (idle / door < 0 / error).
  auto res_stage = [&](int st) -> bool {
    int* rflag = abort_flag + 2;
    if (tid == 0) {
      const unsigned need = (unsigned)NCOPR * (unsigned)(st + 1);
      const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
      int v = 1;
      for (;;) {
        if (__hip_atomic_load(a.dctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need) break;
        if (__hip_atomic_load(a.dctr + 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) { v = 0; break; }
        if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > a.idle + a.timeout) {   // copiers gone: bounded
          atomicOr(a.err, 4);
          v = 0;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      *rflag = v;
    }
    __syncthreads();
    if (*rflag == 0) return false;
    if (c == 0 && tid == 0) { RTSC(a.run0 + st, 2); }
    const auto rs = region_rsrc(a.stage + (long long)(st & 1) * REC, (int)REC);
    const int xr0 = 16 * tile0(q);
#pragma unroll 4
    for (int k = tid; k < XF_CHUNKS; k += THREADS) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (k / 13) * DIN + 16 * (k % 13) + xr0, 0, 16);
      *reinterpret_cast<u32x4*>(smem + L_XF + 16 * k) = v;
    }
    if (tid < 8) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)XROW_BYTES + 16 * tid, 0, 16);
      *reinterpret_cast<u32x4*>(smem + L_LAB + 16 * tid) = v;
    }
    __syncthreads();
    read_xf(lab);
    read_xt();
    if (c == 0 && tid == 0) { RTSC(a.run0 + st, 3); }
    const float lr_run = *reinterpret_cast<const float*>(smem + L_LAB + RES_LR_BYTE);
    lrB = lr_run / (float)B;
    lrX = lrB * (1.f / 255.f);
    return true;
  };
  int st_done = 0;
  // fp32 master -> memory: W1 entries of this lane; W2 / b1 / b2 of block j from
  // the q == 0 workgroups, b2 from workgroup 0.  wt: write-through (sc1) stores
  // (RES: every step, read by torch kernels / copies between runs)
  auto write_params = [&](bool wt) {
    auto put = [wt](float* p, float v) {
      if (wt) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else *p = v;
    };
    if (hv) {
#pragma unroll
      for (int k = 0; k < NTW; ++k)
        if (tvk(k)) {
#pragma unroll
          for (int e = 0; e < 4; ++e) put(a.params + (16 * ftk(k) + 4 * g + e) * HID + hid, Wt[k][e]);
        }
    }
    if (q == 0) {
      if (tid < 256) {
        const int n = tid >> 4, cl = tid & 15;
        const int hn = 16 * j + n;
        if (hn < HID && cl < NCLS) put(a.p_w2 + hn * NCLS + cl, w2s[tid]);
      } else if (tid < 272) {
        const int hn = 16 * j + (tid - 256);
        if (hn < HID) put(a.p_b1 + hn, b1s[tid - 256]);
      }
    }
    if (c == 0 && tid >= 272 && tid < 272 + NCLS) put(a.p_b2 + (tid - 272), b2s[tid - 272]);
  };

  // MET_FAST: the metric ring slot of the launch's first step (workgroup 0), so a
  // step's slot is a 32-bit modulo (ring and the launch's steps are both < 2^31)
  unsigned mslot0 = 0u;
  if constexpr (MET_FAST) {
    if (c == 0) mslot0 = (unsigned)(gstep0 % a.ring);
  }

  const PeerRs<NW> prs = peer_rsrcs<NW>(a.peer_base, MULTI ? a.W : 1);
  bool aborted = false;
  for (int st = 0; st < a.nsteps; ++st) {
    if constexpr (RES) {
      if (!res_stage(st)) break;
    }
    // this workgroup's block / slice as opaque values per step: the gathers'
    // slot selects (k == skip) would otherwise be hoisted out of the step loop as
    // ten 64-bit lane masks held across it (SGPR spills, a v_readlane per use)
    int jq[2] = {j, q};
    asm volatile("" : "+s"(jq[0]), "+s"(jq[1]));
    const unsigned long long sq = seq0 + (unsigned long long)st + 1ull;
    const unsigned tag = (unsigned)sq;
    const int par = (int)(sq & 1ull);
    if (c == 0 && tid == 0 && a.step_ts != nullptr)
      a.step_ts[(gstep0 + st) % a.ts_ring] = (long long)__builtin_amdgcn_s_memrealtime();
    if (w == 0) { PH(0); }
    if (w == 7) { PH7(14); }

    // ---------------- P0: forward partial of the wave's tiles, all batch tiles
    {
      f32x4 acc[NBT];
#pragma unroll
      for (int b = 0; b < NBT; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (SPLIT) {
        // K = 32: k = 8g + i -> tile i >> 2, feature 4g + (i & 3) -- the A piece is this
        // lane's 8 master weights, the B operand its two x dwords (an absent second
        // tile has zero weights); pieces lo, mid, hi (small terms first)
        float wv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) wv[i] = Wt[i >> 2][i & 3];
        bf16x8 Ah, Am, Al;
        split8(wv, Ah, Am, Al);
        bf16x8 X[NBT];   // PREP: made ahead of the step, so split8 runs straight into the MFMAs
#pragma unroll
        for (int b = 0; b < NBT; ++b) {
          if constexpr (PREP) X[b] = XF[b];
          else X[b] = px8(xf[0][b], xf[1][b]);
        }
#pragma unroll
        for (int b = 0; b < NBT; ++b) acc[b] = mfma16x16x32(Al, X[b], acc[b]);
#pragma unroll
        for (int b = 0; b < NBT; ++b) acc[b] = mfma16x16x32(Am, X[b], acc[b]);
#pragma unroll
        for (int b = 0; b < NBT; ++b) acc[b] = mfma16x16x32(Ah, X[b], acc[b]);
      } else {
#pragma unroll
        for (int k = 0; k < NTW; ++k) {
          if (tvk(k)) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
              for (int b = 0; b < NBT; ++b) acc[b] = mfma4(Wt[k][e], ub(xf[k][b], e), acc[b]);
          }
        }
      }
#pragma unroll
      for (int b = 0; b < NBT; ++b) zbuf[(w * NBT + b) * 64 + lane] = acc[b];
    }
    if (w == 0) { PH(1); }
    PHB(w);
    lds_barrier();
    if (w == 0) { PH(2); }
    const bool more = !RES && st + 1 < a.nsteps;   // RES: the next run's record is staged at its top
    // everyone's reads of this step's stage retired at barrier A: wave 7 (idle
    // until P2) stages the next step while the others run the edges and the head
    // [0..6] head of batch tile v: dz2 pieces, dz3 / a2 rows in LDS; [7] stage landed;
    // [8..14] head of batch tile v: dW2 / db2 partial (workgroup 0: loss / hit rows) in LDS
    int* hflag = reinterpret_cast<int*>(smem + L_HFLAG);
    auto flags_up = [&](int f0) -> unsigned {   // bit v: flag f0 + v set this step
      const bool ok = lane < NBT && __hip_atomic_load(hflag + f0 + (lane < NBT ? lane : 0), __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_WORKGROUP) >= st + 1;
      return (unsigned)__ballot(ok) & ((1u << NBT) - 1u);
    };
    // a chunk waits for the first flag of its batch tiles (DTF_PERSIST_DBG bit 4: for
    // the second, the order in which one flag covered the partials as well)
    const int chunk_flag = (dbg & 16) != 0 ? 8 : 0;
    auto heads_done = [&]() -> unsigned { return flags_up(chunk_flag); };
    if (w == 7 && more && !(dbg & 1)) {
      stage_x(st + 1, 0, 1);
      // idle until the first head is done anyway: wait for the DMA here and tell the
      // other waves the next step's operands are in LDS
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if (lane == 0) __hip_atomic_store(hflag + 7, st + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if ((dbg & 8) == 0) { PH7(15); }
    } else if (w == 7 && more && lane == 0) {
      __hip_atomic_store(hflag + 7, st + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // PREP: true once this wave holds the next step's operands (XF, lab_n, raw xt)
    bool prepped = false;
    if constexpr (PREP) {
      if (w == 7) {
        // wave 7 has nothing to do until the first head is done: its own operands of
        // this step, and of the next one behind its own DMA wait
        prep_xa();
        if (more && !(dbg & 4)) {
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
          prep_fwd(lab_n);
          prepped = true;
        }
      }
    }

    // ---------------- E1 + P1 + E2 + head (wave w < 7: batch tile w)
    if (w < NBT) {
      const int bw = 16 * w + r;          // this lane's batch row
      const bool bv = bw < B;
      f32x4 zs = zbuf[w * 64 + lane];
#pragma unroll
      for (int v = 1; v < 8; ++v) zs += zbuf[(v * NBT + w) * 64 + lane];
      // publish the slice partial of (j, batch tile w) as granules; gather the others
      // E1 region of (parity, block j): [slice][batch tile] slots
      const auto r1 = region_rsrc(a.xbuf + E1_OFF + (long long)(par * NJ + j) * NQ * NBT * GSLOT, NQ * NBT * GSLOT);
      put_gran(r1, (q * NBT + w) * GSLOT + 32 * lane, zs, tag, l2_e1);
      if (w == 0) { PH(3); }
      // while the partial is in flight: this step's weight-gradient A operands
      // (chunk() then has only the dz2 piece reads between a head flag and its MFMAs)
      if constexpr (PREP) prep_xa();
      // this step's W2 / b1 / b2 operands of the lane, read from LDS while the
      // partial is in flight (their LDS latency off the E1 -> P1 -> E2 -> head chain)
      float w2p[4], w2d[4], b1v[4], b2v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        w2p[e] = w2s[(4 * g + e) * 16 + r];
        w2d[e] = w2s[r * 16 + 4 * g + e];
        b1v[e] = b1s[4 * g + e];
        b2v[e] = b2s[4 * g + e];
      }
      f32x4 part[NQ];
      bool ok = gather_gran<NQ, NQ>(r1, [&](int k) { return (k * NBT + w) * GSLOT; }, jq[1], true, tag, zs, part, lane, a);
      f32x4 z = part[0];
#pragma unroll
      for (int qq = 1; qq < NQ; ++qq) z += part[qq];
      if (w == 0) { PH(4); }
      if (w == 0) { PH(5); }
      // lane (batch r, g): hidden 16j+4g+i
      float a2[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int hl = 4 * g + i;
        const float zt = z[i] * (1.f / 255.f) + b1v[i];
        // v_exp_f32 / v_rcp_f32 (<= 2 ulp each, 1e-7 relative): ~20 instructions per
        // element less than IEEE expf + division on this single-wave critical path
        const float av = ACT == 0 ? __builtin_amdgcn_rcpf(1.f + __expf(-zt)) : fmaxf(zt, 0.f);
        a2[i] = (16 * j + hl < HID) ? av : 0.f;
      }
      // partial logits^T[class][batch] of block j: A = W2^T (lane: class r), B = a2^T
      f32x4 pl = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) pl = mfma4(w2p[e], a2[e], pl);
      // E2 region of (parity, slice q, batch tile w): [block] slots
      const auto r2 = region_rsrc(a.xbuf + E2_OFF + (long long)((par * NQ + q) * NBT + w) * NJ * GSLOT, NJ * GSLOT);
      if (g < 3) put_gran(r2, j * GSLOT + 32 * lane, pl, tag, l2_e2);
      if (w == 0) { PH(6); }
      // while the logits are in flight: a2 -> LDS (dW2)
#pragma unroll
      for (int i = 0; i < 4; ++i) a2T[(4 * g + i) * LS + bw] = a2[i];
      f32x4 lp[NJ];
      ok = gather_gran<NJ, E2_GRP>(r2, [&](int k) { return k * GSLOT; }, jq[0], g < 3, tag, pl, lp, lane, a) && ok;
      if (w == 0) { PH(7); }
      if (!ok && lane == 0) *abort_flag = 1;
      // logits and softmax -- identical in every workgroup.  Only what dz3 needs
      // (m, ssum, the label) sits on the chain to the dz2 stores; the row's loss and
      // hit come after the first head flag, in workgroup 0 alone
      float lg[4], ex[4];
      float m = -3.0e38f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = b2v[i];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) v += lp[jj][i];
        lg[i] = v;
        if (4 * g + i < NCLS) m = fmaxf(m, v);
      }
      if (w == 0) { PH(8); }
      m = fmaxf(m, xor16(m));
      m = fmaxf(m, xor32(m));
      const int y = lab < NCLS ? lab : 0;
      float ssum = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ex[i] = 4 * g + i < NCLS ? __expf(lg[i] - m) : 0.f;
        ssum += ex[i];
      }
      ssum += xor16(ssum); ssum += xor32(ssum);
      const float inv = __builtin_amdgcn_rcpf(ssum);
      if (w == 0) { PHX(13); }
      float pr[4], dz3[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cl = 4 * g + i;
        pr[i] = ex[i] * inv;
        // the rounded product, as when py summed it in front of dz3: not contracted
        // into an fma with the subtraction below (other bits in dz3)
        asm("" : "+v"(pr[i]));
        dz3[i] = (bv && cl < NCLS) ? pr[i] - (cl == y ? 1.f : 0.f) : 0.f;   // unscaled: 1/B at the update
      }
      // da2^T = W2 . dz3^T (A = W2, lane: hidden r), dz2 = da2 * act'(a2)
      f32x4 da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < 4; ++e) da = mfma4(w2d[e], dz3[e], da);
      if (w == 0) { PHX(14); }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = ACT == 0 ? da[i] * a2[i] * (1.f - a2[i]) : (a2[i] > 0.f ? da[i] : 0.f);
        if constexpr (SPLIT) {
          uint32_t ph, pm, pl;
          split3(d, ph, pm, pl);
          const int o = (4 * g + i) * PS + bw;
          dzp[o] = (uint16_t)(ph >> 16);
          dzp[16 * PS + o] = (uint16_t)(pm >> 16);
          dzp[32 * PS + o] = (uint16_t)(pl >> 16);
        } else {
          dz2T[(4 * g + i) * LS + bw] = d;
        }
        dz3T[(4 * g + i) * LS + bw] = dz3[i];
      }
      if (w == 0) { PHX(15); }
      // first head flag: the tile's dz2 pieces and its dz3 / a2 rows are in LDS --
      // all a weight-gradient chunk waits for
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if (lane == 0) __hip_atomic_store(hflag + w, st + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (w == 0) { PH(9); }
      PHB(8 + w);
      // the row's loss and hit, read by workgroup 0's wave 7 and by nobody else
      // (workgroup-uniform branch): zy and the argmax over the 4 lane groups, py =
      // the label's ex * inv product for the naive loss only -- the operands and the
      // order they had in front of dz3.  The label is laundered so its class masks
      // are compared again here and not carried in SGPRs across the MFMAs (the
      // kernel sits at its SGPR limit).
      if (c == 0) {
        int ym = y;
        asm volatile("" : "+v"(ym));
        float zy = 0.f, am = 1e9f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int cl = 4 * g + i;
          zy += (cl == ym) ? lg[i] : 0.f;
          if (cl < NCLS && lg[i] == m) am = fminf(am, (float)cl);
        }
        zy += xor16(zy); zy += xor32(zy);
        am = fminf(am, xor16(am)); am = fminf(am, xor32(am));
        float loss;
        if (a.naive) {
          float py = 0.f;
#pragma unroll
          for (int i = 0; i < 4; ++i) py += (4 * g + i == ym) ? pr[i] : 0.f;
          py += xor16(py); py += xor32(py);
          loss = -__logf(py);
        } else {
          loss = m + __logf(ssum) - zy;
        }
        if (g == 0) {
          float* rl = reinterpret_cast<float*>(smem + L_RLOSS);
          rl[bw] = bv ? loss : 0.f;
          rl[128 + bw] = (bv && (int)am == ym) ? 1.f : 0.f;
        }
      }
      // this tile's dW2 = a2^T dz3 and db2 = 1^T dz3 partials over its 16 rows (two
      // independent f32 MFMA chains; k = batch 4g + e, from the rows this wave just
      // wrote: LDS ops of one wave complete in order).  db1 rides along with wave
      // 7's weight-gradient MFMAs as a ones "feature" tile.
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      {
        const f32x4 av = *reinterpret_cast<const f32x4*>(a2T + r * LS + 16 * w + 4 * g);
        const f32x4 dv = *reinterpret_cast<const f32x4*>(dz3T + r * LS + 16 * w + 4 * g);
        const float one = r == 0 ? 1.f : 0.f;   // A = rows of ones at row 0
        f32x4 dp = {0.f, 0.f, 0.f, 0.f}, p2 = dp;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          dp = mfma4(av[e], dv[e], dp);
          p2 = mfma4(one, dv[e], p2);
        }
        reinterpret_cast<f32x4*>(smem + L_DW2P)[w * 64 + lane] = dp;
        if (g == 0) rdb2[w * 16 + r] = p2[0];   // D[0][class r]
      }
      // second head flag: the tile's dW2 / db2 partial (workgroup 0: its loss / hit
      // rows too) is in LDS -- what wave 7's fold and metric reduction wait for
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
      if (lane == 0) __hip_atomic_store(hflag + 8 + w, st + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // ---------------- P2 without a workgroup barrier: a wave multiplies the weight-
    // gradient chunk of batch rows 32cc..32cc+31 (one batch tile without SPLIT) as
    // soon as the heads of its batch tiles are done (LDS flags), chunks in order
    // (one accumulator chain: deterministic).  Barrier B used to wait for the LAST
    // head before any chunk started.  Reuse of everything the heads wrote is still
    // fenced by barrier A of the next step.
    f32x4 G[NTW];                        // dW1[16ft+4g+i][16j+r] (x 255 B)
    f32x4 G1[NTW];                       // !SPLIT: second accumulator chain
#pragma unroll
    for (int k = 0; k < NTW; ++k) G[k] = G1[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int NCH = SPLIT ? 4 : NBT;
    auto need_of = [](int ch) -> unsigned {
      return SPLIT ? ((1u << (2 * ch)) | (2 * ch + 1 < NBT ? 1u << (2 * ch + 1) : 0u)) : (1u << ch);
    };
    auto chunk = [&](int ch) {   // ch is a constant after unrolling (register operands)
      if constexpr (SPLIT) {
        // dW1 tile = x^T dz2 over K = 128 batch rows in 4 chunks: A = x^T bytes (exact),
        // B = the dz2 pieces; an absent second tile computes a zero-weight copy (unused)
        const uint16_t* bp = dzp + r * PS + 32 * ch + 8 * g;
        const bf16x8 Bh = *reinterpret_cast<const bf16x8*>(bp);
        const bf16x8 Bm = *reinterpret_cast<const bf16x8*>(bp + 16 * PS);
        const bf16x8 Bl = *reinterpret_cast<const bf16x8*>(bp + 32 * PS);
        bf16x8 X0, X1;   // PREP: finished operands from the E1 window
        if constexpr (PREP) X0 = XA[0][ch];
        else X0 = px8(xt[0][2 * ch], xt[0][2 * ch + 1]);
        if (tv1 || w == 7) {   // wave-uniform: waves without a second tile skip its MFMAs
          // wave 7 (always one tile) multiplies a tile of ones instead: G[1] = db1
          // (lane (r, g): hidden 16j + r, every i), exact like the rest
          if constexpr (PREP) X1 = XA[1][ch];
          else X1 = tv1 ? px8(xt[1][2 * ch], xt[1][2 * ch + 1]) : px8(0x01010101u, 0x01010101u);
          G[0] = mfma16x16x32(X0, Bl, G[0]);
          G[1] = mfma16x16x32(X1, Bl, G[1]);
          G[0] = mfma16x16x32(X0, Bm, G[0]);
          G[1] = mfma16x16x32(X1, Bm, G[1]);
          G[0] = mfma16x16x32(X0, Bh, G[0]);
          G[1] = mfma16x16x32(X1, Bh, G[1]);
        } else {
          G[0] = mfma16x16x32(X0, Bl, G[0]);
          G[0] = mfma16x16x32(X0, Bm, G[0]);
          G[0] = mfma16x16x32(X0, Bh, G[0]);
        }
      } else {
        const f32x4 bz = *reinterpret_cast<const f32x4*>(dz2T + r * LS + 16 * ch + 4 * g);
#pragma unroll
        for (int k = 0; k < NTW; ++k) {
          if (tvk(k)) {
            G[k] = mfma4(ub(xt[k][ch], 0), bz[0], G[k]);
            G1[k] = mfma4(ub(xt[k][ch], 1), bz[1], G1[k]);
            G[k] = mfma4(ub(xt[k][ch], 2), bz[2], G[k]);
            G1[k] = mfma4(ub(xt[k][ch], 3), bz[3], G1[k]);
          }
        }
        if (w == 7) {   // one tile: a ones tile in the second slot gives db1
          G[1] = mfma4(1.f, bz[0], G[1]);
          G1[1] = mfma4(1.f, bz[1], G1[1]);
          G[1] = mfma4(1.f, bz[2], G[1]);
          G1[1] = mfma4(1.f, bz[3], G1[1]);
        }
      }
    };
    {
      int cc = 0;   // next chunk
      for (;;) {
        const unsigned hm = heads_done();
        bool did = false;
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          if (ch == cc && (hm & need_of(ch)) == need_of(ch)) {   // wave-uniform
            if (!did) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
            if (cc == 0 && w == 0) { PH(10); }
            chunk(ch);
            ++cc;
            did = true;
          }
        }
        if (cc == NCH) break;
        if (!did) __builtin_amdgcn_s_sleep(0);
      }
    }
    if constexpr (!SPLIT) {
#pragma unroll
      for (int k = 0; k < NTW; ++k) G[k] = G[k] + G1[k];
    }
    // every head has set its first flag here.  Wave 7 waits for the seven second
    // flags, then sums the 7 head waves' dW2 / db2 partials and the per-row metrics
    // in fixed order (all loads in flight at once); one GPU: the W2 / b1 / b2
    // updates too (their readers, this step's heads, took them in the E1 window;
    // the next step's read them after barrier A)
    f32x4 D = {0.f, 0.f, 0.f, 0.f};      // wave 7: dW2[16j+4g+i][class r] (x B)
    float gb = 0.f;                      // wave 7: db1 (lanes < 16) / db2 (lanes 16..25) (x B)
    if (w == 7) {
      if constexpr (INS) {
        if ((dbg & 8) != 0) { PH7(15); }
      }
      // its own chunks are multiplied: now the seven second flags
      while (flags_up(8) != (1u << NBT) - 1u) __builtin_amdgcn_s_sleep(0);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
      // lanes 16..25: db2 column lane - 16 (lanes < 16 take db1 from the ones tile)
      const float* gsrc = rdb2 + (lane >= 16 && lane < 16 + NCLS ? lane - 16 : 0);
      const f32x4* dw2p = reinterpret_cast<const f32x4*>(smem + L_DW2P);
#pragma unroll
      for (int v = 0; v < NBT; ++v) {
        D += dw2p[v * 64 + lane];
        gb += gsrc[v * 16];
      }
      if (lane < 16) gb = G[1][0];   // db1 of hidden 16j + lane from the ones tile
      if (lane >= 16 + NCLS) gb = 0.f;
      PH7(13);
      if (c == 0) {   // loss / accuracy of the batch: per-row values, fixed reduction order
        const float* rl = reinterpret_cast<const float*>(smem + L_RLOSS);
        const bool hi = lane + 64 < BROWS;
        // MET_FAST: wave_sum's butterfly (lane ^ 32, 16, 8, 4, 2, 1) without its LDS
        // round trips.  After the ^32 and ^16 steps a row's rotation by 8 is its ^8
        // partner, and from then on the values repeat with the period of the next
        // partner distance, so the rotations by 4, 2, 1 fetch what ^4, ^2, ^1 would:
        // the same additions, the same bits in every lane
        auto wsum = [&](float v) {
          if constexpr (MET_FAST) {
            v += xor32(v);
            v += xor16(v);
            return row16_sum(v);
          } else {
            return wave_sum(v);
          }
        };
        const float ls = wsum(rl[lane] + (hi ? rl[lane + 64] : 0.f));
        const float cr = wsum(rl[128 + lane] + (hi ? rl[128 + lane + 64] : 0.f));
        if (lane == 63) {
          const int sl = MET_FAST ? (int)((mslot0 + (unsigned)st) % (unsigned)a.ring) : (int)((gstep0 + st) % a.ring);
          if constexpr (RES) {   // workgroup 0 publishes them (LDS), the ring keeps them too
            reinterpret_cast<float*>(abort_flag)[4] = ls / (float)B;
            reinterpret_cast<float*>(abort_flag)[5] = cr / (float)B;
            __hip_atomic_store(a.metrics + 2 * sl, ls / (float)B, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.metrics + 2 * sl + 1, cr / (float)B, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          } else {
            a.metrics[2 * sl] = ls / (float)B;
            a.metrics[2 * sl + 1] = cr / (float)B;
          }
        }
      }
      if constexpr (!MULTI) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (16 * j + 4 * g + i < HID && r < NCLS) w2s[(4 * g + i) * 16 + r] -= lrB * D[i];
        if (lane < 16) {
          if (16 * j + lane < HID) b1s[lane] -= lrB * gb;
        } else if (lane < 16 + NCLS) {
          b2s[lane - 16] -= lrB * gb;
        }
      }
      PHB(15);
    }
    if (*abort_flag) { aborted = true; break; }   // final for this step: every head has reported
    if (more && !prepped) {
      // next step's operands (this step's are consumed): x rows + label once wave 7
      // saw the stage land, x^T.  PREP: the late path of the head waves, conversions
      // included (DTF_PERSIST_DBG bit 2: wave 7 too)
      while (__hip_atomic_load(hflag + 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < st + 1)
        __builtin_amdgcn_s_sleep(1);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
      if constexpr (PREP) {
        prep_fwd(lab_n);
      } else {
        read_xf(lab);
        read_xt();
      }
    }
    if constexpr (PREP) lab = lab_n;   // this step's head is done with its label
    if (w == 0) { PH(11); }
    if constexpr (MULTI) {
      // ---- exchange of this workgroup's gradient with the same workgroup on
      // every peer GPU (uncached IPC buffers: completion == visibility); sums in
      // rank order keep the replicas bit-identical.  Only payload crosses the
      // fabric: bf16 packs a lane's two tiles into ONE 16-B entry (8 B when the
      // wave has one tile), hidden-padding lanes (unit >= 100) and the zero
      // columns of dW2 (class >= 10) neither store nor load, and every peer is
      // read with single 16-B system-scope loads, all NW of them in flight
      // (absent peers / masked lanes read out of the buffer's range: zero, no
      // memory traffic).
      const bool pk = a.gbf16 != 0;
      const size_t soff = IPC_FLAGS + (size_t)(par * NCOMP + c) * IPC_SLOT;
      char* own = static_cast<char*>(a.peer_base[a.rank]) + soff;
      const int eb = (w * 64 + lane) * 16;                       // bf16: both tiles
      const int ef0 = ((w * NTW + 0) * 64 + lane) * 16;          // fp32: tile 0
      const int ef1 = ((w * NTW + 1) * 64 + lane) * 16;          // fp32: tile 1
      const bool dlane = r < NCLS && 16 * j + 4 * g < HID;       // wave 7: dW2 entry carries data
      const bool blane = lane < 16 ? 16 * j + lane < HID : lane < 16 + NCLS;   // wave 7: db1 / db2
      if (hv) {
        if (pk) {
          const uint32_t p0 = pack2bf(G[0][0], G[0][1]), p1 = pack2bf(G[0][2], G[0][3]);
          const uint32_t p2 = pack2bf(G[1][0], G[1][1]), p3 = pack2bf(G[1][2], G[1][3]);
          if (tv1) *reinterpret_cast<uint4*>(own + eb) = make_uint4(p0, p1, p2, p3);
          else if (tv0) *reinterpret_cast<uint2*>(own + eb) = make_uint2(p0, p1);
        } else {
          if (tv0) *reinterpret_cast<f32x4*>(own + ef0) = G[0];
          if (tv1) *reinterpret_cast<f32x4*>(own + ef1) = G[1];
        }
      }
      if (pk) {   // this rank's own term, as every peer sees it
        G[0] = round_bf16x4(G[0]);
        G[1] = round_bf16x4(G[1]);
      }
      if (w == 7) {
        if (dlane) *reinterpret_cast<f32x4*>(own + IPC_SMALL + lane * 16) = D;
        if (blane) *reinterpret_cast<float*>(own + IPC_SMALL + 1024 + lane * 4) = gb;
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every wave: its slot stores landed
      lds_barrier();
      char* flags = static_cast<char*>(a.peer_base[a.rank]);
      // wave 0 waits until every peer's flag word `fo` of this workgroup reached `tag`
      auto wait_peers = [&](int fo) {
        if (w == 0) {
          const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
          for (;;) {
            bool ok = true;
            if (lane < a.W && lane != a.rank) {
              const unsigned v = __hip_atomic_load(
                  reinterpret_cast<const unsigned*>(static_cast<const char*>(a.peer_base[lane]) + 64 * c + fo),
                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
              ok = (int)(v - tag) >= 0;
            }
            if (__all(ok)) break;
            if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > a.timeout ||
                __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
              if (lane == 0) {
                atomicOr(a.err, 2);
                *abort_flag = 1;
              }
              break;
            }
            __builtin_amdgcn_s_sleep(1);
          }
        }
        lds_barrier();
        asm volatile("" ::: "memory");   // no peer-slot load hoisted above the flag match
      };
      if (tid == 0 && !(a.rank == a.fault_rank && gstep0 + st >= a.fault_step))
        __hip_atomic_store(reinterpret_cast<unsigned*>(flags + 64 * c), tag, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
      wait_peers(0);
      if (*abort_flag) { aborted = true; break; }
      // rank-order sums of this lane's entries at slot offset `so` over all ranks
      auto sum_ranks = [&](size_t so) {
        constexpr int GF = NW < 4 ? NW : 4;   // fp32 payload: 4 peers in flight per group (registers)
        if (pk) {
          if (tv1) sum_entries<NW, NW, true, true>(prs, a.W, a.rank, (int)so, hv, eb, eb, G[0], G[1]);
          else sum_entries<NW, NW, true, false>(prs, a.W, a.rank, (int)so, hv, eb, eb, G[0], G[1]);
        } else {
          if (tv1) sum_entries<NW, GF, false, true>(prs, a.W, a.rank, (int)so, hv, ef0, ef1, G[0], G[1]);
          else sum_entries<NW, GF, false, false>(prs, a.W, a.rank, (int)so, hv, ef0, ef1, G[0], G[1]);
        }
        if (w == 7) sum_small<NW>(prs, a.W, a.rank, (int)so + IPC_SMALL, dlane, blane, lane, D, gb);
      };
      if (a.xmode == 0) {
        // one-shot: every wave sums its entries over all ranks
        sum_ranks(soff);
      } else {
        // two-shot: wave w's entries form chunk w % W, reduced (rank order) by
        // that rank only, then every rank reads each chunk's sums from its owner:
        // 2 (W-1)/W of a slot crosses the fabric per GPU instead of (W-1) slots.
        // bf16 payload: the owner rounds the sum to bf16 once and uses the rounded
        // value itself, so the all-gather moves bf16 too and replicas stay identical
        const int own_chunk = w % a.W;
        const size_t roff = IPC_RED + (size_t)(par * NCOMP + c) * IPC_SLOT;
        char* ored = static_cast<char*>(a.peer_base[a.rank]) + roff;
        if (own_chunk == a.rank) {
          sum_ranks(soff);
          if (hv) {
            if (pk) {
              const uint32_t p0 = pack2bf(G[0][0], G[0][1]), p1 = pack2bf(G[0][2], G[0][3]);
              const uint32_t p2 = pack2bf(G[1][0], G[1][1]), p3 = pack2bf(G[1][2], G[1][3]);
              if (tv1) *reinterpret_cast<uint4*>(ored + eb) = make_uint4(p0, p1, p2, p3);
              else if (tv0) *reinterpret_cast<uint2*>(ored + eb) = make_uint2(p0, p1);
              G[0] = round_bf16x4(G[0]);
              G[1] = round_bf16x4(G[1]);
            } else {
              if (tv0) *reinterpret_cast<f32x4*>(ored + ef0) = G[0];
              if (tv1) *reinterpret_cast<f32x4*>(ored + ef1) = G[1];
            }
          }
          if (w == 7) {
            if (dlane) *reinterpret_cast<f32x4*>(ored + IPC_SMALL + lane * 16) = D;
            if (blane) *reinterpret_cast<float*>(ored + IPC_SMALL + 1024 + lane * 4) = gb;
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the reduced chunk landed
        lds_barrier();
        if (tid == 0)
          __hip_atomic_store(reinterpret_cast<unsigned*>(flags + 64 * c + 8), tag, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_SYSTEM);
        wait_peers(8);
        if (*abort_flag) { aborted = true; break; }
        if (own_chunk != a.rank) {
          // all-gather: this wave's chunk sums from their owner
          __amdgpu_buffer_rsrc_t rs = prs.r[0];
#pragma unroll
          for (int rr = 1; rr < NW; ++rr)
            if (rr == own_chunk) rs = prs.r[rr];   // wave-uniform
          const int ro = (int)roff;
          if (pk) {
            if (tv1) {
              const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, hv ? ro + eb : OOB_OFF, 0, SYS);
              G[0] = unbf4(v[0], v[1]);
              G[1] = unbf4(v[2], v[3]);
            } else {
              const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, hv ? ro + eb : OOB_OFF, 0, SYS);
              G[0] = unbf4(v[0], v[1]);
            }
          } else {
            G[0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, hv ? ro + ef0 : OOB_OFF, 0, SYS));
            if (tv1)
              G[1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, hv ? ro + ef1 : OOB_OFF, 0, SYS));
          }
          if (w == 7) {
            D = __builtin_bit_cast(
                f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, dlane ? ro + IPC_SMALL + lane * 16 : OOB_OFF, 0, SYS));
            gb = __uint_as_float(
                __builtin_amdgcn_raw_buffer_load_b32(rs, blane ? ro + IPC_SMALL + 1024 + lane * 4 : OOB_OFF, 0, SYS));
          }
        }
      }
    }
    // ---------------- updates (lr / (W B), 1/255 for the pixel scale)
    if (hv) {   // an absent second tile keeps its zero weights (wave 7's G[1] is db1)
#pragma unroll
      for (int k = 0; k < NTW; ++k)
#pragma unroll
        for (int i = 0; i < 4; ++i) Wt[k][i] -= (k == 0 || tv1) ? lrX * G[k][i] : 0.f;
    }
    if (w == 0) { PH(12); }
    if (MULTI && w == 7) {   // N GPUs: with the rank sums of dW2 / db1 / db2
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (16 * j + 4 * g + i < HID && r < NCLS) w2s[(4 * g + i) * 16 + r] -= lrB * D[i];
      if (lane < 16) {
        if (16 * j + lane < HID) b1s[lane] -= lrB * gb;
      } else if (lane < 16 + NCLS) {
        b2s[lane - 16] -= lrB * gb;
      }
    }
    st_done = st + 1;
    if constexpr (RES) {
      // the run is complete once every compute workgroup's parameters are in
      // memory: write-through stores, every wave's vmcnt(0), barrier, one agent add;
      // the last arriver (its add's return value says so) publishes the metrics,
      // global_step and the done count to pinned host memory
      __syncthreads();   // wave 7's LDS updates of W2 / b1 / b2 (and workgroup 0's metrics)
      if (c == 0 && tid == 0) { RTSC(a.run0 + st, 4); }
      write_params(true);
      // the graph's global_step: counted here (anything else that writes it stops
      // the engine first), stored write-through by workgroup 0
      const double gsv = gvar0 + (double)(st + 1);
      if (c == 0 && tid == 0) {
        if (a.gvar_kind == 1) __hip_atomic_store(static_cast<float*>(a.gvar), (float)gsv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (a.gvar_kind == 2) __hip_atomic_store(static_cast<long long*>(a.gvar), (long long)gsv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (a.gvar_kind == 3) __hip_atomic_store(static_cast<int*>(a.gvar), (int)gsv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (a.gvar_kind == 4) __hip_atomic_store(static_cast<double*>(a.gvar), gsv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) {
        if (c == 0) { RTSC(a.run0 + st, 5); }
        __hip_atomic_fetch_add(a.dctr + 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == 0) {
          // workgroup 0 (it holds the metrics) publishes once all 28 have arrived
          const unsigned need = (unsigned)NCOMP * (unsigned)(st + 1);
          const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
          while (__hip_atomic_load(a.dctr + 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
            if ((long long)__builtin_amdgcn_s_memrealtime() - t0 > a.timeout) {
              atomicOr(a.err, 8);
              break;
            }
          }
          RTSC(a.run0 + st, 6);
          const float* mf = reinterpret_cast<const float*>(abort_flag);
          __hip_atomic_store(a.host_out, mf[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(a.host_out + 1, mf[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          __hip_atomic_store(a.host_out + 2, (float)gsv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __hip_atomic_store(a.host_done, a.run0 + st + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
          RTSC(a.run0 + st, 7);
        }
      }
    }
  }
  if (aborted) return;
  __syncthreads();   // wave 7's last small-parameter update
  if (tid == 0) { PROC(c, 3); }

  // ---- write back (fp32 master), global step, exchange sequence, end stamp
  // (RES: the steps that ran -- the sequence never falls behind the tags in use)
  write_params(false);
  if (c == 0 && tid == 300) {
    *a.gstep = gstep0 + st_done;
    *a.seq = seq0 + (unsigned long long)st_done;
    if (a.step_ts != nullptr)
      a.step_ts[(gstep0 + st_done) % a.ts_ring] = (long long)__builtin_amdgcn_s_memrealtime();
  }
  if (tid == 0) { PROC(c, 5); }
}

// packed placement (a.spread == 0): compute workgroup c runs as blockIdx 8c, so
// under the observed round-robin dispatch all 28 share ONE XCD (both edges in one
// L2); the first NCOP other blocks copy, the rest exit.  spread (several ranks on
// one GPU, tests): compute = blocks 0..27, copiers = 28..43.  Placement is speed
// only: the census above decides each edge's store flavour.
template <int ACT, int NW, bool SPLIT, bool RES = false, bool INS = false>
__global__ __launch_bounds__(THREADS, 1) void mlp_persist_f32(Args a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int b = blockIdx.x;
  int c = -1, cid = -1;
  if (a.spread) {
    if (b < NCOMP) c = b; else cid = b - NCOMP;
  } else {
    if ((b & 7) == 0) c = b >> 3; else cid = b - (b >> 3) - 1;
  }
  if (c >= 0) {
    if (a.nsteps > 0) compute<ACT, NW, SPLIT, RES, INS>(a, c / NQ, c % NQ, smem);
    return;
  }
  if constexpr (RES) copier_res(a, cid, smem);
  else if (cid < NCOP) copier(a, cid, smem);
}

// ------------------------------------------------------------------ host launch
// fault injection (tests of the bench's in-process fallback): rank `rank` stops
// publishing its exchange flag from global step `step` on; rank -1 = off
static int g_fault_rank = -1;
static long long g_fault_step = -1;

// Placement-census tags: unique per launch within the process (the census
// buffer lives in a runner's exchange buffer, zeroed once; tag 0 never matches)
static unsigned next_census_tag() {
  static std::atomic<unsigned> ctr{0};
  unsigned t = ctr.fetch_add(1u, std::memory_order_relaxed) + 1u;
  return t == 0u ? ctr.fetch_add(1u, std::memory_order_relaxed) + 1u : t;
}

// DTF_PERSIST_DBG (profiling, flat launches), read once per process: a getenv per
// launch is host time inside a short timed run
static int persist_dbg() {
  static const int dbg = [] {
    const char* db = getenv("DTF_PERSIST_DBG");
    return db ? atoi(db) : 0;
  }();
  return dbg;
}

// The kernel's arguments of one launch: every field from `p` or zero.
static Args make_args(const Launch& p) {
  const bool res = p.door != nullptr;
  Args a{};
  a.stage = static_cast<const uint8_t*>(p.stage);
  a.rec_h = p.rec_h;
  a.B = p.B;
  a.nsteps = res ? 0x7fffffff : p.nsteps;   // resident: bounded by the doorbell / idle exit
  a.params = p.params;
  a.lr = p.lr;
  a.metrics = p.metrics;
  a.ring = p.ring;
  a.act = p.act;
  a.naive = p.naive;
  a.gstep = p.gstep;
  a.seq = p.seq;
  a.xbuf = static_cast<uint8_t*>(p.xbuf);
  a.err = p.err;
  a.timeout = p.timeout;
  a.step_ts = p.step_ts;
  a.ts_ring = p.ts_ring > 0 ? p.ts_ring : 1;
  a.host_next = static_cast<const uint8_t*>(p.host_next);
  a.next_steps = p.next_steps;
  a.stage_next = static_cast<uint8_t*>(p.stage_next);
  a.peer_base = p.peer_base;
  a.W = p.W;
  a.rank = p.rank;
  a.gbf16 = p.gbf16;
  a.spread = p.spread;
  a.phase_ts = p.phase_ts;
  a.xmode = p.xmode;
  a.fault_step = g_fault_step;
  a.fault_rank = g_fault_rank;
  a.p_w2 = p.W2 != nullptr ? p.W2 : p.params + OFF_W2;
  a.p_b1 = p.b1 != nullptr ? p.b1 : p.params + OFF_B1;
  a.p_b2 = p.b2 != nullptr ? p.b2 : p.params + OFF_B2;
  a.door = p.door;
  a.host_recs = static_cast<const uint8_t*>(p.host_recs);
  a.host_lr = p.host_lr;
  a.host_out = p.host_out;
  a.host_done = p.host_done;
  a.host_state = p.host_state;
  a.launch_id = p.launch_id;
  a.run0 = p.run0;
  a.idle = p.idle;
  a.census_tag = next_census_tag();
  a.gvar = p.gvar;
  a.gvar_kind = p.gvar_kind;
  a.dctr = p.dctr;
  a.res_ts = p.res_ts;
  a.dbg = res ? 0 : persist_dbg();
  return a;
}

typedef void (*Kern)(Args);
// every instantiation the launcher can pick: [0, 16) production, act + 2 nwi + 8 split
// (NW, the peer-table width the exchange is unrolled for: 1, 2, 4, 8); [16, 20)
// instrumented, act + 2 split; [20, 24) resident, act + 2 instrumented
static const Kern kKernels[24] = {
    mlp_persist_f32<0, 1, false>, mlp_persist_f32<1, 1, false>, mlp_persist_f32<0, 2, false>,
    mlp_persist_f32<1, 2, false>, mlp_persist_f32<0, 4, false>, mlp_persist_f32<1, 4, false>,
    mlp_persist_f32<0, 8, false>, mlp_persist_f32<1, 8, false>, mlp_persist_f32<0, 1, true>,
    mlp_persist_f32<1, 1, true>,  mlp_persist_f32<0, 2, true>,  mlp_persist_f32<1, 2, true>,
    mlp_persist_f32<0, 4, true>,  mlp_persist_f32<1, 4, true>,  mlp_persist_f32<0, 8, true>,
    mlp_persist_f32<1, 8, true>,
    mlp_persist_f32<0, 1, false, false, true>, mlp_persist_f32<1, 1, false, false, true>,
    mlp_persist_f32<0, 1, true, false, true>,  mlp_persist_f32<1, 1, true, false, true>,
    mlp_persist_f32<0, 1, true, true>,         mlp_persist_f32<1, 1, true, true>,
    mlp_persist_f32<0, 1, true, true, true>,   mlp_persist_f32<1, 1, true, true, true>};

// The instantiation for (activation, NW index, split, resident, instrumented);
// nullptr where none exists: the instrumented build is one-GPU only, the
// resident engine split and one-GPU only.
static Kern select_kernel(int act, int nwi, bool split, bool res, bool ins) {
  const int ai = act == 0 ? 0 : 1;
  if (res) return (split && nwi == 0) ? kKernels[20 + ai + (ins ? 2 : 0)] : nullptr;
  if (ins) return nwi == 0 ? kKernels[16 + ai + (split ? 2 : 0)] : nullptr;
  return kKernels[ai + 2 * nwi + (split ? 8 : 0)];
}

}  // namespace mlpf
}  // namespace dtfk

extern "C" {

void dtfk_mlpf_set_fault(int rank, long long step) {
  dtfk::mlpf::g_fault_rank = rank;
  dtfk::mlpf::g_fault_step = step;
}

long long dtfk_mlpf_stage_rec() { return dtfk::mlpf::REC; }
long long dtfk_mlpf_xbuf_bytes() { return dtfk::mlpf::XBUF_BYTES; }
long long dtfk_mlpf_ipc_bytes() { return dtfk::mlpf::IPC_BYTES; }
int dtfk_mlpf_max_batch() { return dtfk::mlpf::BROWS; }

// One launch of the engine.  Flat (p->door == nullptr): `nsteps` SGD steps of the
// chunk in `stage` on the flat master and, in the same launch, `next_steps` host
// records into `stage_next`.  Resident (compat/resident.py, csrc/bind_mlp.cpp
// ResidentMLPPlan): ONE launch serves Session.run calls until `idle` ticks pass
// without a doorbell or the host writes door < 0 -- one GPU, the reference's
// precision (SPLIT), packed placement; the graph's own W1 / W2 / b1 / b2 tensors
// and global_step variable are read at launch and written through every step.
// Instrumented instantiations (profiling): flat with phase stamps or
// DTF_PERSIST_DBG, resident with per-run stamps.
hipError_t dtfk_mlp_persist_f32_launch(const dtfk::mlpf::Launch* p, hipStream_t stream) {
  using namespace dtfk::mlpf;
  const bool res = p->door != nullptr;
  if (p->B < 1 || p->B > BROWS || p->rec_h < (long long)p->B * (DIN + 1) || p->gvar_kind < 0 || p->gvar_kind > 4 ||
      (p->gvar_kind != 0 && p->gvar == nullptr))
    return hipErrorInvalidValue;
  if (p->W < 1 || p->W > 8 || p->rank < 0 || p->rank >= p->W) return hipErrorInvalidValue;
  if (res && p->spread) return hipErrorInvalidValue;
  static bool attr_set = false;
  if (!attr_set) {
    for (Kern k : kKernels) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BYTES);
      if (e != hipSuccess) return e;
    }
    attr_set = true;
  }
  const Args a = make_args(*p);
  const int nwi = p->W <= 1 ? 0 : (p->W <= 2 ? 1 : (p->W <= 4 ? 2 : 3));
  const bool ins = res ? p->res_ts != nullptr : (p->phase_ts != nullptr || a.dbg != 0);
  const Kern k = select_kernel(p->act, nwi, p->split != 0, res, ins);
  if (k == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k, dim3(p->spread ? GRID_SPREAD : GRID_PACKED), dim3(THREADS), LDS_BYTES, stream, a);
  return hipGetLastError();
}

}  // extern "C"
