// The host entry points of the MLP kernel files (mlp_step.hip, mlp_gemm.hip,
// mlp_persist_f32.hip, graph_mlp.hip, mlp_eval.hip), declared once: csrc/bind_mlp.cpp calls
// through these declarations and every defining file includes them, so a
// definition that disagrees with its declaration does not compile.  Host-only:
// no device code here.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

namespace dtfk {
namespace mlpf {

// One launch of the fp32 persistent engine (mlp_persist_f32.hip).  Value-
// initialise it (`Launch p{}`) and set what the mode needs; everything else
// stays null / zero.
struct Launch {
  const void* stage;        // flat: this chunk, nsteps records; resident: 2 device record slots
  long long rec_h;          // host record bytes (B * 785 rounded up to 16)
  int B, nsteps;            // nsteps: flat only (0: copy only); a resident launch runs until its doorbell stops it
  float* params;            // W1, the front of the flat fp32 master
  float* W2;                // null: the flat master's own (params + OFF_W2 / OFF_B1 / OFF_B2);
  float* b1;                //   resident: the graph's variables
  float* b2;
  const float* lr;
  float* metrics;
  int ring;                 // metrics ring: [ring][2]
  int act, naive;
  long long* gstep;
  unsigned long long* seq;  // exchange sequence number (monotonic across launches)
  void* xbuf;               // granule exchange buffer (dtfk_mlpf_xbuf_bytes(), zeroed once)
  int* err;
  long long timeout;        // s_memrealtime ticks (100 MHz)
  long long* step_ts;       // optional per-step stamp ring of ts_ring entries
  int ts_ring;
  const void* host_next;    // next chunk: next_steps host records (device-visible pinned memory) -> stage_next
  int next_steps;
  void* stage_next;
  void* const* peer_base;   // N GPUs: IPC-mapped exchange buffers of every rank
  int W, rank;              // 1 <= W <= 8 (1: one GPU), 0 <= rank < W
  int gbf16, spread, xmode; // dW1 payload in bf16; spread placement; 1: two-shot exchange
  int split;                // 1: the big GEMMs as exact 3-way bf16 splits, 0: f32-input MFMA
  long long* phase_ts;      // profiling: [65][64][16] phase stamps -> the instrumented build (one GPU)
  // resident mode (door != nullptr): the Session engine's pinned mailbox
  const long long* door;
  const void* host_recs;
  const float* host_lr;
  float* host_out;
  long long* host_done;
  long long* host_state;
  long long launch_id, run0, idle;
  void* gvar;               // the graph's global_step variable and its dtype code (csrc/gstep_kind.h)
  int gvar_kind;
  unsigned* dctr;
  long long* res_ts;        // profiling: [64][8] per-run stamps -> the instrumented resident build
};

}  // namespace mlpf

namespace gmlp {

// One step of the compat Session's lowered MLP graph (graph_mlp.hip).  Value-
// initialise it (`Step p{}`) and set what the mode needs; everything else
// stays null / zero.
struct Step {
  const float* x;           // feed [B][K] fp32 ...
  const uint8_t* xu;        //   ... or, when non-null, uint8 pixels instead (K % 4 == 0, 4-byte aligned)
  const float* ylab;        // labels [B][C]
  float* W1;                // the graph's variables: [K][H], [H], [H][C], [C]
  float* b1;
  float* W2;
  float* b2;
  float* a2;                // scratch [BP][HP] each (BP = B, HP = H + 1, rounded up to 16)
  float* dz2;
  float* part;              // scratch of dtfk_graph_mlp_part_floats(B, H) floats, ZERO when first used
  float* gW1;               // sgd == 0: gradient outputs, the variables' shapes
  float* gb1;
  float* gW2;
  float* gb2;
  float* metrics;           // [3] loss, accuracy, global_step after the step
  float* host_metrics;      // the same three stored into pinned host memory by the last kernel, or null
  void* gstep;              // the graph's global_step variable (gstep_kind.h), bumped once
  int gstep_kind;
  const float* lr;          // device learning rate (a captured step reads the current one)
  int B, K, H, C;           // B <= 256, H <= 128, C <= 16, BP * HP <= 16384
  int act, naive;           // act 0 sigmoid, 1 relu; naive: loss as -sum(y_ log softmax), else the stable form
  int sgd;                  // 1: variables updated in place with lr; 0: gradients into g*
};

}  // namespace gmlp

namespace mlpe {

// What an evaluation accumulates on the device (mlp_eval.hip): 24 bytes, 8-byte aligned.
struct Record {
  double loss_sum;          // sum of the per-row losses
  long long correct;        // rows whose argmax(z3) is the label
  long long rows;
};

// One forward-only evaluation of N rows (mlp_eval.hip).  Value-initialise it
// (`Eval p{}`) and set what the call needs; everything else stays null / zero.
struct Eval {
  const float* x;           // rows [N][K] fp32 ...
  const uint8_t* xu;        //   ... or uint8 pixels instead (K % 4 == 0, 4-byte aligned); exactly one is non-null
  const void* labels;       // label_kind 0: uint8 class ids [N], 1: int32 ids [N], 2: fp32 one-hot [N][C]
  int label_kind;
  const float* W1;          // [K][H], [H], [H][C], [C]: the flat master's slices or the Session's variables
  const float* b1;
  const float* W2;
  const float* b2;
  float* part;              // scratch of dtfk_mlp_eval_part_words(N) 4-byte words
  Record* rec;              // accumulated into; reset != 0: started over by this call
  int reset;
  int* pred;                // optional [N] argmax(z3)
  float* logits;            // optional [N][C] z3
  int N, K, H, C;           // N >= 1, K >= 1, H <= 128, C <= 16
  int act, naive;           // act 0 sigmoid, 1 relu; naive: loss as -sum(y_ log softmax), else the stable form
};

}  // namespace mlpe
}  // namespace dtfk

extern "C" {
// ---- mlp_step.hip
int dtfk_mlp_ksplit();
hipError_t dtfk_mlp_l1_fwd(const void* x, int x_kind, int B, const void* W1T, float* z2p, long long* ts,
                           hipStream_t stream);
hipError_t dtfk_mlp_head_bwd(const float* z2p, const void* labels, int B, const void* W2T, const void* W2N,
                             const float* params, void* dz2T, int BP, float* partials, float inv_batch, int act,
                             int naive_loss, long long* gstep, long long* ts, hipStream_t stream);
hipError_t dtfk_mlp_wgrad(const void* x, int x_kind, const void* dz2T, int BP, int B, const float* partials,
                          float* params, void* W1T, void* W2T, void* W2N, void* grads, int grad_kind, const float* lr,
                          float* metrics, long long* gstep, int ring, long long* ts, void* const* ipc_table, int ipc_W,
                          int ipc_rank, int ipc_parity, long long ipc_slot_bytes, int* ipc_err, long long ipc_timeout,
                          hipStream_t stream);
hipError_t dtfk_mlp_apply_flat(float* params, const void* grads, int grad_kind, const float* lr, float scale,
                               void* W1T, void* W2T, void* W2N, hipStream_t stream);
int dtfk_mlp_ipc_flag_bytes();
hipError_t dtfk_mlp_ipc_reduce_apply(float* params, void* const* peer_table, int W, int rank, int parity,
                                     long long slot_bytes, const long long* gstep, const float* lr, float scale,
                                     void* W1T, void* W2T, void* W2N, int* err, long long timeout_ticks,
                                     hipStream_t stream);
// ---- mlp_gemm.hip
int dtfk_mlpg_p1_floats();
hipError_t dtfk_mlpg_fwd(const void* x, const void* labels, int B, int BP, const void* W1F, const float* params,
                         float* a2g, float* P1, void* dz2F, int act, int naive, float gscale, hipStream_t s);
int dtfk_mlpg_wchunk(int B);
int dtfk_mlpg_p2_floats();
hipError_t dtfk_mlpg_wgrad(const void* x, int B, const void* dz2F, float* P2, int nchunk, hipStream_t s);
hipError_t dtfk_mlpg_apply(float* params, const float* P1, int n1, const float* P2, int n2, const float* gin,
                           float* gout, const float* lr, float scale, void* W1S, float* metrics, int ring,
                           long long* gstep, int B, int mode, hipStream_t s);
// ---- mlp_persist_f32.hip
void dtfk_mlpf_set_fault(int rank, long long step);
long long dtfk_mlpf_stage_rec();
long long dtfk_mlpf_xbuf_bytes();
long long dtfk_mlpf_ipc_bytes();
int dtfk_mlpf_max_batch();
hipError_t dtfk_mlp_persist_f32_launch(const dtfk::mlpf::Launch* p, hipStream_t stream);
// ---- graph_mlp.hip
long long dtfk_graph_mlp_part_floats(int B, int H);
hipError_t dtfk_graph_mlp_step(const dtfk::gmlp::Step* p, hipStream_t stream);
// ---- mlp_eval.hip
long long dtfk_mlp_eval_part_words(long long N);
hipError_t dtfk_mlp_eval(const dtfk::mlpe::Eval* p, hipStream_t stream);
}
