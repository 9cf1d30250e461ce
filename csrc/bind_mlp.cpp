// Python bindings for the fused MLP step kernels (csrc/kernels/mlp_step.hip)
// and the pinned-host -> device batch copy used by the input pipeline.
#include "bind_common.h"
#include "comm/ipc_coll_host.h"
#include "gstep_host.h"
#include "kernels/mlp_api.h"

#include <pybind11/numpy.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <cstring>
#include <stdexcept>
#include <string>

namespace dtf {

constexpr int kNParam = 79510;

static long long* ts_ptr(const c10::optional<at::Tensor>& ts, int64_t need_numel) {
  if (!ts.has_value()) return nullptr;
  need(*ts, at::kLong, need_numel, "ts");
  return reinterpret_cast<long long*>(ts->data_ptr<int64_t>());
}

// device-visible address of `nbytes` of pinned host memory at `off`
static const void* pinned_device_ptr(const c10::optional<at::Tensor>& host, int64_t off, int64_t nbytes) {
  if (!host.has_value()) throw std::runtime_error("next chunk needs the pinned host epoch");
  const at::Tensor& h = *host;
  if (h.is_cuda() || !h.is_pinned()) throw std::runtime_error("host must be pinned host memory");
  if (off < 0 || off % 16 != 0 || off + nbytes > (int64_t)(h.numel() * h.element_size()))
    throw std::runtime_error("host range out of bounds");
  void* dp = nullptr;
  char* hp = reinterpret_cast<char*>(h.data_ptr()) + off;
  if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess || dp == nullptr) {
    (void)hipGetLastError();
    dp = hp;   // unified addressing: the host address is device-visible
  }
  if (reinterpret_cast<uintptr_t>(dp) % 16 != 0) throw std::runtime_error("pinned host pointer not aligned");
  return dp;
}

static int bp_of(int B) { return ((B + 31) / 32) * 32; }

// x_kind: 0 u8 pixels (/255), 1 fp32, 2 bf16; rows of 784 features.
static const char* x_ptr(const at::Tensor& x, int64_t off, int x_kind, int B) {
  const int64_t esz = x_kind == 0 ? 1 : (x_kind == 1 ? 4 : 2);
  if (x_kind < 0 || x_kind > 2) throw std::runtime_error("bad x_kind");
  if (!x.is_cuda() || !x.is_contiguous()) throw std::runtime_error("x must be a contiguous GPU tensor");
  if ((int64_t)x.numel() * x.element_size() < off + (int64_t)B * 784 * esz)
    throw std::runtime_error("x buffer too small");
  if (off % 16 != 0 || (reinterpret_cast<uintptr_t>(x.data_ptr()) % 16) != 0)
    throw std::runtime_error("x must be 16-byte aligned");
  return reinterpret_cast<const char*>(x.data_ptr()) + off;
}

// z2p: per-K-half partial pre-activations [ksplit][nb*16][112] fp32
void mlp_l1_fwd(at::Tensor x, int64_t x_off, int x_kind, int B, at::Tensor W1T, at::Tensor z2p,
                c10::optional<at::Tensor> ts) {
  if (B <= 0) throw std::runtime_error("B must be positive");
  const int nb = (B + 15) / 16;
  const char* xb = x_ptr(x, x_off, x_kind, B);
  need(W1T, at::kBFloat16, 112 * 800, "W1T");
  need(z2p, at::kFloat, (int64_t)dtfk_mlp_ksplit() * nb * 16 * 112, "z2p");
  hip_check(dtfk_mlp_l1_fwd(xb, x_kind, B, W1T.data_ptr(), z2p.data_ptr<float>(),
                            ts_ptr(ts, (int64_t)nb * 7 * dtfk_mlp_ksplit() * 16), cur_stream()),
            "mlp_l1_fwd");
}

void mlp_head_bwd(at::Tensor z2p, at::Tensor labels, int64_t labels_off, int B, at::Tensor W2T,
                  at::Tensor W2N, at::Tensor params, at::Tensor dz2T, at::Tensor partials, double inv_batch, int act,
                  bool naive_loss, at::Tensor gstep, c10::optional<at::Tensor> ts) {
  const int nb = (B + 15) / 16, BP = bp_of(B);
  need(z2p, at::kFloat, (int64_t)dtfk_mlp_ksplit() * nb * 16 * 112, "z2p");
  if (!labels.is_cuda() || labels.scalar_type() != at::kByte)
    throw std::runtime_error("labels must be a uint8 GPU tensor");
  if (labels.numel() < labels_off + B) throw std::runtime_error("labels buffer too small");
  need(W2T, at::kBFloat16, 16 * 128, "W2T");
  need(W2N, at::kBFloat16, 112 * 32, "W2N");
  need(params, at::kFloat, kNParam, "params");
  need(dz2T, at::kBFloat16, (int64_t)112 * BP, "dz2T");
  need(partials, at::kFloat, (int64_t)nb * 1112, "partials");
  hip_check(dtfk_mlp_head_bwd(z2p.data_ptr<float>(),
                              reinterpret_cast<const uint8_t*>(labels.data_ptr()) + labels_off, B,
                              W2T.data_ptr(), W2N.data_ptr(), params.data_ptr<float>(), dz2T.data_ptr(), BP,
                              partials.data_ptr<float>(), (float)inv_batch, act, naive_loss ? 1 : 0,
                              reinterpret_cast<long long*>(gstep.data_ptr<int64_t>()),
                              ts_ptr(ts, (int64_t)nb * 16), cur_stream()),
            "mlp_head_bwd");
}

// grad_kind: 0 fused SGD (grads ignored), 1 fp32 grads, 2 bf16 grads
void mlp_wgrad(at::Tensor x, int64_t x_off, int x_kind, at::Tensor dz2T, int B,
               at::Tensor partials, at::Tensor params, at::Tensor W1T, at::Tensor W2T,
               at::Tensor W2N, c10::optional<at::Tensor> grads, int grad_kind, at::Tensor lr, at::Tensor metrics,
               at::Tensor gstep, c10::optional<at::Tensor> ts, int64_t ipc_table, int ipc_W, int ipc_rank,
               int ipc_parity, int64_t ipc_slot_bytes, c10::optional<at::Tensor> ipc_err, double ipc_timeout_s) {
  const int nb = (B + 15) / 16, BP = bp_of(B);
  if (BP > 4096) throw std::runtime_error("per-GPU batch > 4096 not supported by mlp_wgrad");
  const char* xb = x_ptr(x, x_off, x_kind, B);
  need(dz2T, at::kBFloat16, (int64_t)112 * BP, "dz2T");
  need(partials, at::kFloat, (int64_t)nb * 1112, "partials");
  need(params, at::kFloat, kNParam, "params");
  need(W1T, at::kBFloat16, 112 * 800, "W1T");
  need(W2T, at::kBFloat16, 16 * 128, "W2T");
  need(W2N, at::kBFloat16, 112 * 32, "W2N");
  need(lr, at::kFloat, 1, "lr");
  need(metrics, at::kFloat, 2, "metrics");
  need(gstep, at::kLong, 1, "global_step");
  void* g = nullptr;
  int* errp = nullptr;
  if (grad_kind == 3) {
    if (ipc_table == 0 || ipc_W < 2 || ipc_rank < 0 || ipc_rank >= ipc_W || ipc_W > 64 || (ipc_parity & ~1) ||
        ipc_slot_bytes < kNParam * 2 || !ipc_err.has_value())
      throw std::runtime_error("mlp_wgrad: bad IPC arguments");
    if (!ipc_err->is_cuda() || ipc_err->scalar_type() != at::kInt) throw std::runtime_error("ipc_err: GPU int32");
    errp = ipc_err->data_ptr<int>();
  } else if (grad_kind != 0) {
    if (!grads.has_value()) throw std::runtime_error("grads required");
    need(*grads, grad_kind == 1 ? at::kFloat : at::kBFloat16, kNParam, "grads");
    g = grads->data_ptr();
  }
  const int ring = (int)(metrics.numel() / 2);
  hip_check(dtfk_mlp_wgrad(xb, x_kind, dz2T.data_ptr(), BP, B, partials.data_ptr<float>(),
                           params.data_ptr<float>(), W1T.data_ptr(), W2T.data_ptr(),
                           W2N.data_ptr(), g, grad_kind,
                           lr.data_ptr<float>(), metrics.data_ptr<float>(),
                           reinterpret_cast<long long*>(gstep.data_ptr<int64_t>()), ring,
                           ts_ptr(ts, (int64_t)(49 * 7 + 4) * 16), reinterpret_cast<void* const*>(ipc_table),
                           grad_kind == 3 ? ipc_W : 0, ipc_rank, ipc_parity, ipc_slot_bytes, errp,
                           (long long)(ipc_timeout_s * 1.0e8), cur_stream()),
            "mlp_wgrad");
}

// one-shot IPC all-reduce fused with SGD apply (see mlp_step.hip); peer_table is the
// device address of IpcPeerBuffers.table_ptr(); err: int32[1] device flag
void mlp_ipc_reduce_apply(at::Tensor params, int64_t peer_table, int W, int rank, int parity, int64_t slot_bytes,
                          at::Tensor gstep, at::Tensor lr, double scale, at::Tensor W1T, at::Tensor W2T,
                          at::Tensor W2N, at::Tensor err, double timeout_s) {
  need(params, at::kFloat, kNParam, "params");
  need(W1T, at::kBFloat16, 112 * 800, "W1T");
  need(W2T, at::kBFloat16, 16 * 128, "W2T");
  need(W2N, at::kBFloat16, 112 * 32, "W2N");
  if (!err.is_cuda() || err.scalar_type() != at::kInt) throw std::runtime_error("err must be a GPU int32 tensor");
  if (peer_table == 0 || W < 2 || rank < 0 || rank >= W || (parity & ~1) || slot_bytes < kNParam * 2)
    throw std::runtime_error("mlp_ipc_reduce_apply: bad arguments");
  const long long ticks = (long long)(timeout_s * 1.0e8);  // s_memrealtime runs at 100 MHz
  hip_check(dtfk_mlp_ipc_reduce_apply(params.data_ptr<float>(), reinterpret_cast<void* const*>(peer_table), W, rank, parity,
                               slot_bytes, reinterpret_cast<const long long*>(gstep.data_ptr<int64_t>()), lr.data_ptr<float>(), (float)scale,
                               W1T.data_ptr(), W2T.data_ptr(), W2N.data_ptr(), err.data_ptr<int>(), ticks, cur_stream()),
     "mlp_ipc_reduce_apply");
}

void mlp_apply_flat(at::Tensor params, c10::optional<at::Tensor> grads, at::Tensor lr,
                    double scale, at::Tensor W1T, at::Tensor W2T, at::Tensor W2N) {
  need(W2N, at::kBFloat16, 112 * 32, "W2N");
  need(params, at::kFloat, kNParam, "params");
  need(lr, at::kFloat, 1, "lr");
  need(W1T, at::kBFloat16, 112 * 800, "W1T");
  need(W2T, at::kBFloat16, 16 * 128, "W2T");
  const void* g = nullptr;
  int kind = 1;
  if (grads.has_value()) {
    if (grads->scalar_type() == at::kFloat) kind = 1;
    else if (grads->scalar_type() == at::kBFloat16) kind = 2;
    else throw std::runtime_error("grads must be fp32 or bf16");
    need(*grads, grads->scalar_type(), kNParam, "grads");
    g = grads->data_ptr();
  }
  hip_check(dtfk_mlp_apply_flat(params.data_ptr<float>(), g, kind, lr.data_ptr<float>(),
                                (float)scale, W1T.data_ptr(), W2T.data_ptr(), W2N.data_ptr(),
                                cur_stream()),
            "mlp_apply_flat");
}

// ---- large-batch GEMM step (kernels/mlp_gemm.hip); x / labels: u8 stage at a byte offset
static const uint8_t* stage_ptr(const at::Tensor& st, int64_t off, int64_t nbytes, const char* name) {
  need(st, at::kByte, -1, name);
  if (off < 0 || off + nbytes > st.numel()) throw std::runtime_error(std::string(name) + ": offset out of range");
  return st.data_ptr<uint8_t>() + off;
}

static int64_t mlpg_bp(int B) { return ((int64_t)B + 63) / 64 * 64; }
static int64_t mlpg_bp2(int B) {
  const int64_t c = dtfk_mlpg_wchunk(B);
  return ((int64_t)B + c - 1) / c * c;
}


void mlpg_fwd(at::Tensor x, int64_t x_off, at::Tensor labels, int64_t labels_off, int B, at::Tensor W1F,
              at::Tensor params, at::Tensor a2, at::Tensor P1, at::Tensor dz2F, int act, bool naive, double gscale) {
  const int64_t BP = mlpg_bp(B);
  if (B < 1) throw std::runtime_error("mlpg_fwd: B >= 1");
  const uint8_t* px = stage_ptr(x, x_off, (int64_t)B * 784, "x");
  if (reinterpret_cast<uintptr_t>(px) & 15) throw std::runtime_error("mlpg_fwd: x must be 16-byte aligned");
  const uint8_t* pl = stage_ptr(labels, labels_off, B, "labels");
  need(W1F, at::kBFloat16, 3 * 112 * 800, "W1F");
  need(params, at::kFloat, kNParam, "params");
  need(a2, at::kFloat, BP * 112, "a2");
  need(P1, at::kFloat, BP / 16 * dtfk_mlpg_p1_floats(), "P1");
  need(dz2F, at::kBFloat16, 3 * 112 * mlpg_bp2(B), "dz2F");
  hip_check(dtfk_mlpg_fwd(px, pl, B, (int)BP, W1F.data_ptr(), params.data_ptr<float>(), a2.data_ptr<float>(),
                          P1.data_ptr<float>(), dz2F.data_ptr(), act, naive ? 1 : 0, (float)gscale, cur_stream()),
            "mlpg_fwd");
}

void mlpg_wgrad(at::Tensor x, int64_t x_off, int B, at::Tensor dz2F, at::Tensor P2, int nchunk) {
  const int64_t BP2 = mlpg_bp2(B);
  const uint8_t* px = stage_ptr(x, x_off, (int64_t)B * 784, "x");
  if (reinterpret_cast<uintptr_t>(px) & 15) throw std::runtime_error("mlpg_wgrad: x must be 16-byte aligned");
  if (nchunk != BP2 / dtfk_mlpg_wchunk(B)) throw std::runtime_error("mlpg_wgrad: nchunk must be ceil(B / chunk)");
  need(dz2F, at::kBFloat16, 3 * 112 * BP2, "dz2F");
  need(P2, at::kFloat, (int64_t)nchunk * dtfk_mlpg_p2_floats(), "P2");
  hip_check(dtfk_mlpg_wgrad(px, B, dz2F.data_ptr(), P2.data_ptr<float>(), nchunk, cur_stream()), "mlpg_wgrad");
}

void mlpg_apply(at::Tensor params, at::Tensor P1, at::Tensor P2, int nchunk, c10::optional<at::Tensor> gin,
                c10::optional<at::Tensor> gout, at::Tensor lr, double scale, at::Tensor W1S, at::Tensor metrics,
                at::Tensor gstep, int B, int mode) {
  const int64_t BP = mlpg_bp(B);
  if (mode < 0 || mode > 3) throw std::runtime_error("mlpg_apply: mode 0..3");
  need(params, at::kFloat, kNParam, "params");
  need(P1, at::kFloat, BP / 16 * dtfk_mlpg_p1_floats(), "P1");
  need(P2, at::kFloat, (int64_t)nchunk * dtfk_mlpg_p2_floats(), "P2");
  if (mode == 2 && !gin.has_value()) throw std::runtime_error("mlpg_apply: mode 2 needs gin");
  if (mode == 1 && !gout.has_value()) throw std::runtime_error("mlpg_apply: mode 1 needs gout");
  if (gin.has_value()) need(*gin, at::kFloat, kNParam, "gin");
  if (gout.has_value()) need(*gout, at::kFloat, kNParam, "gout");
  need(lr, at::kFloat, 1, "lr");
  need(W1S, at::kBFloat16, 3 * 112 * 800, "W1S");
  need(metrics, at::kFloat, 2, "metrics");
  need(gstep, at::kLong, 1, "gstep");
  hip_check(dtfk_mlpg_apply(params.data_ptr<float>(), P1.data_ptr<float>(), (int)(BP / 16), P2.data_ptr<float>(),
                            nchunk, gin.has_value() ? gin->data_ptr<float>() : nullptr,
                            gout.has_value() ? gout->data_ptr<float>() : nullptr, lr.data_ptr<float>(), (float)scale,
                            W1S.data_ptr(), metrics.data_ptr<float>(), (int)(metrics.numel() / 2),
                            reinterpret_cast<long long*>(gstep.data_ptr<int64_t>()), B, mode, cur_stream()),
            "mlpg_apply");
}

// hipMemcpyAsync host(pinned) -> device on the *current* stream (graph-capturable).
void memcpy_h2d_async(at::Tensor dst, int64_t dst_offset, at::Tensor src, int64_t src_offset,
                      int64_t nbytes) {
  if (!dst.is_cuda()) throw std::runtime_error("dst must be a GPU tensor");
  if (src.is_cuda()) throw std::runtime_error("src must be a host tensor");
  if (!src.is_pinned()) throw std::runtime_error("src must be pinned host memory");
  if (dst_offset + nbytes > (int64_t)(dst.numel() * dst.element_size()) ||
      src_offset + nbytes > (int64_t)(src.numel() * src.element_size()))
    throw std::runtime_error("memcpy_h2d_async out of range");
  hip_check(hipMemcpyAsync(reinterpret_cast<char*>(dst.data_ptr()) + dst_offset,
                           reinterpret_cast<const char*>(src.data_ptr()) + src_offset, nbytes,
                           hipMemcpyHostToDevice, cur_stream()),
            "hipMemcpyAsync");
}

// A prepared launcher for the fp32 persistent engine (csrc/kernels/mlp_persist_f32.hip;
// mfma_split: the big GEMMs as exact 3-way bf16 splits, else f32-input MFMA):
// every tensor checked and every pointer resolved once into the launch struct,
// so a launch from Python is a call with 5 ints that patches the per-launch
// fields (per-call tensor arguments and checks cost ~10 us of host time on a
// 20-step run: scripts/probes/launch_overhead.py).
struct PersistF32Plan {
  at::Tensor stage0, stage1, params, lr, metrics, gstep, seq, xbuf, err, step_ts, host, phase_ts;
  void* st[2];
  const char* host_dev = nullptr;
  int64_t host_bytes = 0, rec_s = 0;
  dtfk::mlpf::Launch p{};

  PersistF32Plan(at::Tensor s0, at::Tensor s1, int64_t rec_h, int B, at::Tensor params_, at::Tensor lr_,
                 at::Tensor metrics_, at::Tensor gstep_, at::Tensor seq_, at::Tensor xbuf_, at::Tensor err_,
                 double timeout_s, int act, int naive, at::Tensor host_, at::Tensor step_ts_, int64_t ipc_table,
                 int ipc_W, int ipc_rank, bool grad_bf16, bool spread, bool two_shot, bool mfma_split)
      : stage0(s0), stage1(s1), params(params_), lr(lr_), metrics(metrics_), gstep(gstep_), seq(seq_), xbuf(xbuf_),
        err(err_), step_ts(step_ts_), host(host_) {
    if (ipc_W > 1 && (ipc_table == 0 || ipc_rank < 0 || ipc_rank >= ipc_W || ipc_W > 64))
      throw std::runtime_error("PersistF32Plan: N-GPU exchange needs the IPC peer table");
    if (B <= 0 || B > dtfk_mlpf_max_batch()) throw std::runtime_error("PersistF32Plan: B out of range");
    if (rec_h < (int64_t)B * 785 || rec_h % 16 != 0) throw std::runtime_error("PersistF32Plan: bad record size");
    rec_s = dtfk_mlpf_stage_rec();
    need(stage0, at::kByte, rec_s, "stage0");
    need(stage1, at::kByte, rec_s, "stage1");
    need(params, at::kFloat, kNParam, "params");
    need(lr, at::kFloat, 1, "lr");
    need(metrics, at::kFloat, 2, "metrics");
    need(gstep, at::kLong, 1, "gstep");
    need(seq, at::kLong, 1, "seq");
    need(xbuf, at::kByte, dtfk_mlpf_xbuf_bytes(), "xbuf");
    need(err, at::kInt, 1, "err");
    need(step_ts, at::kLong, 2, "step_ts");
    st[0] = stage0.data_ptr();
    st[1] = stage1.data_ptr();
    if ((((uintptr_t)st[0]) | ((uintptr_t)st[1]) | (uintptr_t)xbuf.data_ptr()) % 16 != 0)
      throw std::runtime_error("PersistF32Plan: stage / xbuf must be 16-byte aligned");
    host_bytes = host.numel() * host.element_size();
    host_dev = static_cast<const char*>(pinned_device_ptr(host, 0, host_bytes));
    p.rec_h = rec_h;
    p.B = B;
    p.params = params.data_ptr<float>();
    p.lr = lr.data_ptr<float>();
    p.metrics = metrics.data_ptr<float>();
    p.ring = (int)(metrics.numel() / 2);
    p.act = act;
    p.naive = naive;
    p.gstep = reinterpret_cast<long long*>(gstep.data_ptr<int64_t>());
    p.seq = reinterpret_cast<unsigned long long*>(seq.data_ptr<int64_t>());
    p.xbuf = xbuf.data_ptr();
    p.err = err.data_ptr<int>();
    p.timeout = (long long)(timeout_s * 1e8);   // s_memrealtime: 100 MHz
    p.step_ts = reinterpret_cast<long long*>(step_ts.data_ptr<int64_t>());
    p.ts_ring = (int)step_ts.numel();
    p.peer_base = reinterpret_cast<void* const*>(ipc_table);
    p.W = ipc_W > 1 ? ipc_W : 1;
    p.rank = ipc_W > 1 ? ipc_rank : 0;
    p.gbf16 = grad_bf16 ? 1 : 0;
    p.spread = spread ? 1 : 0;
    p.xmode = two_shot ? 1 : 0;
    p.split = mfma_split ? 1 : 0;
  }

  // profiling: phase stamps [65][64][16] on (the instrumented build, one GPU) / off (None)
  void set_phase_ts(c10::optional<at::Tensor> ts) {
    p.phase_ts = ts_ptr(ts, 65 * 64 * 16);
    phase_ts = ts.has_value() ? *ts : at::Tensor();
  }

  // nsteps steps from stage `par` at step offset `off` (records of mlpf_stage_rec()
  // bytes) and, in the same launch, next_steps host records from byte host_off of
  // the pinned epoch into stage par ^ 1.  nsteps = 0: copy only.
  void launch(int par, int64_t off, int nsteps, int64_t host_off, int next_steps) {
    if ((par & ~1) != 0 || nsteps < 0 || next_steps < 0 || off < 0) throw std::runtime_error("PersistF32Plan: args");
    const at::Tensor& cur = par ? stage1 : stage0;
    const at::Tensor& nxt = par ? stage0 : stage1;
    if ((off + std::max(nsteps, 1)) * rec_s > cur.numel()) throw std::runtime_error("PersistF32Plan: stage overrun");
    p.host_next = nullptr;
    p.stage_next = nullptr;
    if (next_steps > 0) {
      if ((int64_t)next_steps * rec_s > nxt.numel()) throw std::runtime_error("PersistF32Plan: next stage too small");
      if (host_off < 0 || host_off % 16 != 0 || host_off + (int64_t)next_steps * p.rec_h > host_bytes)
        throw std::runtime_error("PersistF32Plan: host range out of bounds");
      p.host_next = host_dev + host_off;
      p.stage_next = st[par ^ 1];
    }
    p.stage = static_cast<const char*>(st[par]) + off * rec_s;
    p.nsteps = nsteps;
    p.next_steps = next_steps;
    hip_check(dtfk_mlp_persist_f32_launch(&p, cur_stream()), "PersistF32Plan.launch");
  }
};

// "<who>: fp32 contiguous device <what> expected" unless every tensor is one
static void need_f32_device(const char* who, std::initializer_list<const at::Tensor*> ts,
                            const char* what = "parameters") {
  for (const at::Tensor* t : ts)
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous(), who,
                ": fp32 contiguous device ", what, " expected");
}

// The compat graph's matched MLP training step (csrc/kernels/graph_mlp.hip).
// sgd: W/b updated in place with lr; else gradients into g* (same shapes).
void graph_mlp_step(at::Tensor x, at::Tensor ylab, at::Tensor W1, at::Tensor b1, at::Tensor W2, at::Tensor b2,
                    at::Tensor a2buf, at::Tensor dz2buf, c10::optional<std::vector<at::Tensor>> grads,
                    at::Tensor metrics,
                    c10::optional<at::Tensor> gstep, double lr, int act, bool naive, bool sgd) {
  need_f32_device("graph_mlp_step", {&x, &ylab, &W1, &b1, &W2, &b2, &a2buf, &dz2buf, &metrics}, "tensors");
  TORCH_CHECK(x.dim() == 2 && W1.dim() == 2 && W2.dim() == 2, "graph_mlp_step: 2-D x, W1, W2");
  const int B = (int)x.size(0), K = (int)x.size(1), H = (int)W1.size(1), C = (int)W2.size(1);
  TORCH_CHECK(W1.size(0) == K && W2.size(0) == H && b1.numel() == H && b2.numel() == C &&
                  ylab.numel() == (int64_t)B * C,
              "graph_mlp_step: shape mismatch");
  const int HP = (H + 16) & ~15, BP = (B + 15) & ~15;
  TORCH_CHECK(a2buf.numel() >= (int64_t)BP * HP && dz2buf.numel() >= (int64_t)BP * HP && metrics.numel() >= 3,
              "graph_mlp_step: scratch too small");
  dtfk::gmlp::Step p{};
  if (!sgd) {
    TORCH_CHECK(grads.has_value() && grads->size() == 4, "graph_mlp_step: gradients [dW1, db1, dW2, db2] expected");
    const int64_t n[4] = {(int64_t)K * H, H, (int64_t)H * C, C};
    float** dst[4] = {&p.gW1, &p.gb1, &p.gW2, &p.gb2};
    for (int i = 0; i < 4; ++i) {
      const at::Tensor& g = (*grads)[i];
      TORCH_CHECK(g.is_cuda() && g.scalar_type() == at::kFloat && g.is_contiguous() && g.numel() == n[i],
                  "graph_mlp_step: bad gradient tensor ", i);
      *dst[i] = g.data_ptr<float>();
    }
  }
  const GstepRef gs = gstep_ref(gstep, "graph_mlp_step");
  // L2's partials + the learning rate on the device (scratch from the caching allocator)
  at::Tensor part = at::zeros({dtfk_graph_mlp_part_floats(B, H) + 1}, x.options());
  part.narrow(0, 0, 1).fill_(lr);
  p.x = x.data_ptr<float>();
  p.ylab = ylab.data_ptr<float>();
  p.W1 = W1.data_ptr<float>();
  p.b1 = b1.data_ptr<float>();
  p.W2 = W2.data_ptr<float>();
  p.b2 = b2.data_ptr<float>();
  p.a2 = a2buf.data_ptr<float>();
  p.dz2 = dz2buf.data_ptr<float>();
  p.part = part.data_ptr<float>() + 1;
  p.metrics = metrics.data_ptr<float>();
  p.gstep = gs.ptr;
  p.gstep_kind = gs.kind;
  p.lr = part.data_ptr<float>();
  p.B = B, p.K = K, p.H = H, p.C = C;
  p.act = act, p.naive = naive ? 1 : 0, p.sgd = sgd ? 1 : 0;
  hip_check(dtfk_graph_mlp_step(&p, cur_stream()), "graph_mlp_step");
}

// Forward-only evaluation of N rows (csrc/kernels/mlp_eval.hip): loss sum,
// correct count and rows accumulated into `out` (int64[3] holding a
// dtfk::mlpe::Record: [0] is the fp64 loss sum's bits), started over when
// `reset`.  x: fp32 or uint8 [N, K]; labels: uint8 / int32 class ids [N] or an
// fp32 one-hot [N, C]; the parameters are any four fp32 tensors (slices of a
// flat master or separate variables).  Optional pred int32 [N], logits fp32 [N, C].
void mlp_eval(at::Tensor x, at::Tensor labels, at::Tensor W1, at::Tensor b1, at::Tensor W2, at::Tensor b2, int act,
              bool naive, at::Tensor out, bool reset, c10::optional<at::Tensor> pred,
              c10::optional<at::Tensor> logits) {
  need_f32_device("mlp_eval", {&W1, &b1, &W2, &b2});
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2 &&
                  (x.scalar_type() == at::kFloat || x.scalar_type() == at::kByte),
              "mlp_eval: x must be a contiguous 2-D fp32 or uint8 device tensor");
  TORCH_CHECK(W1.dim() == 2 && W2.dim() == 2, "mlp_eval: 2-D W1, W2");
  const int64_t N = x.size(0), K = x.size(1), H = W1.size(1), C = W2.size(1);
  TORCH_CHECK(N >= 1 && N <= INT32_MAX, "mlp_eval: N >= 1 rows expected, got ", N);
  TORCH_CHECK(W1.size(0) == K && W2.size(0) == H && b1.numel() == H && b2.numel() == C, "mlp_eval: shape mismatch");
  TORCH_CHECK(K >= 1 && K <= INT32_MAX && H >= 1 && H <= 128 && C >= 1 && C <= 16,
              "mlp_eval: shapes outside the kernel's gate (K >= 1, H <= 128, C <= 16)");
  TORCH_CHECK(act == 0 || act == 1, "mlp_eval: act must be 0 (sigmoid) or 1 (relu)");
  TORCH_CHECK(labels.is_cuda() && labels.is_contiguous(), "mlp_eval: labels must be a contiguous device tensor");
  dtfk::mlpe::Eval p{};
  if (labels.scalar_type() == at::kFloat) {
    TORCH_CHECK(labels.dim() == 2 && labels.size(0) == N && labels.size(1) == C,
                "mlp_eval: one-hot labels must be fp32 [N, C]");
    p.label_kind = 2;
  } else {
    TORCH_CHECK((labels.scalar_type() == at::kByte || labels.scalar_type() == at::kInt) && labels.numel() == N,
                "mlp_eval: class ids must be uint8 or int32 [N]");
    p.label_kind = labels.scalar_type() == at::kByte ? 0 : 1;
  }
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.scalar_type() == at::kLong && out.numel() >= 3,
              "mlp_eval: out must be an int64[3] device tensor");
  if (x.scalar_type() == at::kByte) {
    TORCH_CHECK(K % 4 == 0 && reinterpret_cast<uintptr_t>(x.data_ptr()) % 4 == 0,
                "mlp_eval: uint8 x needs K % 4 == 0 and 4-byte aligned rows");
    p.xu = x.data_ptr<uint8_t>();
  } else {
    p.x = x.data_ptr<float>();
  }
  if (pred.has_value()) {
    TORCH_CHECK(pred->is_cuda() && pred->is_contiguous() && pred->scalar_type() == at::kInt && pred->numel() == N,
                "mlp_eval: pred must be an int32 [N] device tensor");
    p.pred = pred->data_ptr<int>();
  }
  if (logits.has_value()) {
    TORCH_CHECK(logits->is_cuda() && logits->is_contiguous() && logits->scalar_type() == at::kFloat &&
                    logits->numel() == N * C,
                "mlp_eval: logits must be an fp32 [N, C] device tensor");
    p.logits = logits->data_ptr<float>();
  }
  // per-tile {loss, correct} (scratch from the caching allocator, this stream's)
  at::Tensor part = at::empty({dtfk_mlp_eval_part_words(N)}, W1.options());
  p.labels = labels.data_ptr();
  p.W1 = W1.data_ptr<float>();
  p.b1 = b1.data_ptr<float>();
  p.W2 = W2.data_ptr<float>();
  p.b2 = b2.data_ptr<float>();
  p.part = part.data_ptr<float>();
  p.rec = reinterpret_cast<dtfk::mlpe::Record*>(out.data_ptr<int64_t>());
  p.reset = reset ? 1 : 0;
  p.N = (int)N, p.K = (int)K, p.H = (int)H, p.C = (int)C;
  p.act = act, p.naive = naive ? 1 : 0;
  hip_check(dtfk_mlp_eval(&p, cur_stream()), "mlp_eval");
}

// The lowered Session.run of the reference's training graph as ONE host call
// (compat/lowering.py, in-kernel SGD): the numpy feeds x [B,K] / y_ [B,C] and the
// learning rate go into a pinned staging slot (one memcpy, GIL released), ONE
// host-to-device copy, then L1 / L2 / L3 launched on the caller's stream (the
// last kernel stores loss / accuracy / global_step into pinned host memory) or,
// with `use_graph`, replayed with a metrics copy-back from a captured hipGraph
// on the plan's own stream; with `sync` the call returns after the step (the
// reference fetches the loss every step).
class GraphStepPlan {
 public:
  GraphStepPlan(at::Tensor W1, at::Tensor b1, at::Tensor W2, at::Tensor b2, c10::optional<at::Tensor> gstep, int B,
                int act, bool naive, bool use_graph)
      : W1_(W1), b1_(b1), W2_(W2), b2_(b2), use_graph_(use_graph) {
    need_f32_device("GraphStepPlan", {&W1, &b1, &W2, &b2});
    const int K = (int)W1.size(0), H = (int)W1.size(1), C = (int)W2.size(1);
    TORCH_CHECK(W2.size(0) == H && b1.numel() == H && b2.numel() == C, "GraphStepPlan: shape mismatch");
    const int HP = (H + 16) & ~15, BP = (B + 15) & ~15;
    gs_ = gstep_ref(gstep, "GraphStepPlan");
    if (gstep.has_value()) gstep_ = *gstep;
    const int64_t nfeed = ((int64_t)B * K + (int64_t)B * C + 1 + 3) / 4 * 4;   // x | y | lr, padded to 16 bytes
    auto fo = W1.options();
    dev_ = at::empty({nfeed}, fo);
    a2_ = at::empty({(int64_t)BP * HP}, fo);
    dz2_ = at::empty({(int64_t)BP * HP}, fo);
    part_ = at::zeros({dtfk_graph_mlp_part_floats(B, H)}, fo);
    metrics_ = at::zeros({4}, fo);
    auto ho = at::TensorOptions().dtype(at::kFloat).pinned_memory(true);
    for (int i = 0; i < 2; ++i) stage_[i] = at::empty({nfeed}, ho);
    host_metrics_ = at::zeros({4}, ho);
    for (int i = 0; i < 2; ++i) hip_check(hipEventCreateWithFlags(&ev_[i], hipEventDisableTiming), "hipEventCreate");
    hip_check(hipEventCreateWithFlags(&in_ev_, hipEventDisableTiming), "hipEventCreate");
    hip_check(hipEventCreateWithFlags(&out_ev_, hipEventDisableTiming), "hipEventCreate");
    // its own stream: graph capture needs one that is not the legacy default stream
    hip_check(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking), "hipStreamCreate");
    // everything of the step but the feed pointers (launch_step sets them per launch)
    step_.W1 = W1.data_ptr<float>();
    step_.b1 = b1.data_ptr<float>();
    step_.W2 = W2.data_ptr<float>();
    step_.b2 = b2.data_ptr<float>();
    step_.a2 = a2_.data_ptr<float>();
    step_.dz2 = dz2_.data_ptr<float>();
    step_.part = part_.data_ptr<float>();
    step_.metrics = metrics_.data_ptr<float>();
    // direct launches: the last kernel stores the metrics into the pinned buffer;
    // a captured graph copies them back instead
    step_.host_metrics = use_graph_ ? nullptr : host_metrics_.data_ptr<float>();
    step_.gstep = gs_.ptr;
    step_.gstep_kind = gs_.kind;
    step_.B = B, step_.K = K, step_.H = H, step_.C = C;
    step_.act = act, step_.naive = naive ? 1 : 0, step_.sgd = 1;
  }
  ~GraphStepPlan() {
    if (exec_) (void)hipGraphExecDestroy(exec_);
    if (graph_) (void)hipGraphDestroy(graph_);
    for (auto& e : ev_)
      if (e) (void)hipEventDestroy(e);
    if (in_ev_) (void)hipEventDestroy(in_ev_);
    if (out_ev_) (void)hipEventDestroy(out_ev_);
    if (st_) (void)hipStreamDestroy(st_);
  }

  at::Tensor host_metrics() const { return host_metrics_; }

  // Synchronous data parallelism over the node's IPC data plane: the step's
  // kernels write this worker's gradients (flat [W1 | b1 | W2 | b2], fp32) and
  // ONE more kernel all-reduces them with every worker's in rank order, applies
  // p -= lr / W * sum on the graph's variables and bumps global_step
  // (csrc/kernels/ipc_coll.hip reduce_sgd_k) -- no RCCL, no host round trip.
  // Direct launches only (the collective's sequence number lives on the device,
  // but the plan's own graph capture is single-worker).
  void attach_ipc(py::object coll) {
    TORCH_CHECK(!use_graph_, "GraphStepPlan.attach_ipc: direct-launch plans only");
    ipc_obj_ = coll;
    ipc_ = coll.cast<IpcColl*>();
    const int64_t nW1 = (int64_t)step_.K * step_.H, nW2 = (int64_t)step_.H * step_.C;
    grad_ = at::zeros({(nW1 + step_.H + nW2 + step_.C + 1) & ~1LL}, W1_.options());
    // gradients out (flat, variable order); the reduce + SGD kernel bumps global_step
    step_.gW1 = grad_.data_ptr<float>();
    step_.gb1 = step_.gW1 + nW1;
    step_.gW2 = step_.gb1 + step_.H;
    step_.gb2 = step_.gW2 + nW2;
    step_.sgd = 0;
    step_.gstep = nullptr;
    step_.gstep_kind = dtfk::GSTEP_NONE;
  }
  bool has_ipc() const { return ipc_ != nullptr; }

  // One training step.  x, y: C-contiguous float32 numpy arrays of the plan's
  // shapes.  Returns after the step when `sync` (host_metrics() then holds
  // loss, accuracy, global_step after the step).
  void run(py::array x, py::array y, double lr, bool sync) {
    TORCH_CHECK(x.dtype().is(py::dtype::of<float>()) && y.dtype().is(py::dtype::of<float>()),
                "GraphStepPlan.run: float32 feeds expected");
    TORCH_CHECK((x.flags() & py::array::c_style) && (y.flags() & py::array::c_style),
                "GraphStepPlan.run: C-contiguous feeds expected");
    TORCH_CHECK(x.size() == nx() && y.size() == ny(), "GraphStepPlan.run: feed shapes differ from the plan's");
    step(x.data(), static_cast<const float*>(y.data()), lr, false, sync);
  }
  // The same step fed uint8 pixels (the MNIST loader's source bytes of a float
  // batch x = u8 / 255, data/mnist.py): a 4x smaller staging copy and transfer;
  // the kernels convert with the loader's exact float32 division, so the step is
  // bit-identical to run() with that float batch.  Direct launches only.
  void run_u8(py::array xu8, py::array y, double lr, bool sync) {
    TORCH_CHECK(!use_graph_, "GraphStepPlan.run_u8: direct-launch plans only");
    TORCH_CHECK(xu8.dtype().is(py::dtype::of<uint8_t>()) && y.dtype().is(py::dtype::of<float>()),
                "GraphStepPlan.run_u8: uint8 x and float32 y_ expected");
    TORCH_CHECK((xu8.flags() & py::array::c_style) && (y.flags() & py::array::c_style),
                "GraphStepPlan.run_u8: C-contiguous feeds expected");
    TORCH_CHECK(xu8.size() == nx() && y.size() == ny(), "GraphStepPlan.run_u8: feed shapes differ from the plan's");
    TORCH_CHECK(step_.K % 4 == 0, "GraphStepPlan.run_u8: K % 4 == 0 expected");
    step(xu8.data(), static_cast<const float*>(y.data()), lr, true, sync);
  }
  int64_t steps() const { return steps_; }
  bool use_graph() const { return use_graph_; }
  // host-side split of the calls so far, us per call: feed copy into the
  // staging slot, everything up to the last enqueue, the final wait
  py::dict timing() const {
    py::dict d;
    const double n = steps_ > 0 ? (double)steps_ : 1.0;
    d["feed_memcpy_us"] = t_[0] / n;
    d["enqueue_us"] = t_[1] / n;
    d["sync_us"] = t_[2] / n;
    d["calls"] = steps_;
    return d;
  }

 private:
  int64_t nx() const { return (int64_t)step_.B * step_.K; }
  int64_t ny() const { return (int64_t)step_.B * step_.C; }
  // floats x occupies at the front of the feed buffer: [x | y_ | lr], uint8 x padded to 16 bytes
  int64_t x_floats(bool u8) const { return u8 ? (nx() + 15) / 16 * 4 : nx(); }

  // The one run path.  xp: nx() floats, or bytes when `u8`.  Take the other
  // staging slot (waiting for the copy an unsynchronized call left in flight on
  // it), pack x | y_ | lr into it, ONE host-to-device copy, the step.  Direct
  // launches go on the caller's stream: no cross-stream events, no replay floor.
  // A captured plan runs on its own stream, after whatever the caller's stream
  // queued (variable init, eager updates) and, when not syncing, before what it
  // queues next.
  void step(const void* xp, const float* yp, double lr, bool u8, bool sync) {
    using clk = std::chrono::steady_clock;
    const int64_t xf = x_floats(u8), nyf = ny();
    hipStream_t cur = cur_stream(), st = use_graph_ ? st_ : cur;
    const int slot = slot_ ^= 1;
    py::gil_scoped_release nogil;
    const auto t0 = clk::now();
    if (pending_[slot]) hip_check(hipEventSynchronize(ev_[slot]), "GraphStepPlan: staging slot");
    pending_[slot] = false;
    float* h = stage_[slot].data_ptr<float>();
    std::memcpy(h, xp, u8 ? (size_t)nx() : sizeof(float) * nx());
    std::memcpy(h + xf, yp, sizeof(float) * nyf);
    h[xf + nyf] = (float)lr;
    t_[0] += std::chrono::duration<double, std::micro>(clk::now() - t0).count();
    if (use_graph_) {
      hip_check(hipEventRecord(in_ev_, cur), "GraphStepPlan: event");
      hip_check(hipStreamWaitEvent(st, in_ev_, 0), "GraphStepPlan: wait");
    }
    hip_check(hipMemcpyAsync(dev_.data_ptr<float>(), h, sizeof(float) * (xf + nyf + 1), hipMemcpyHostToDevice, st),
              "GraphStepPlan: feed copy");
    if (!sync) {   // a synchronizing call leaves no copy in flight: no event at all
      hip_check(hipEventRecord(ev_[slot], st), "GraphStepPlan: event");
      pending_[slot] = true;
    }
    if (use_graph_) {
      if (exec_ == nullptr) capture(st);
      hip_check(hipGraphLaunch(exec_, st), "GraphStepPlan: graph launch");
      if (!sync) {   // later work on the caller's stream sees the updated variables
        hip_check(hipEventRecord(out_ev_, st), "GraphStepPlan: event");
        hip_check(hipStreamWaitEvent(cur, out_ev_, 0), "GraphStepPlan: wait");
      }
    } else {
      hip_check(launch_step(st, u8), "GraphStepPlan: launch");
    }
    const auto t2 = clk::now();
    t_[1] += std::chrono::duration<double, std::micro>(t2 - t0).count();
    if (sync) {
      hip_check(hipStreamSynchronize(st), "GraphStepPlan: sync");
      pending_[0] = pending_[1] = false;
    }
    t_[2] += std::chrono::duration<double, std::micro>(clk::now() - t2).count();
    ++steps_;
  }

  // the step's kernels on stream st, fed from dev_; with IPC the reduce + SGD
  // kernel follows; a captured graph ends with the metrics copy-back
  hipError_t launch_step(hipStream_t st, bool u8) {
    float* d = dev_.data_ptr<float>();
    step_.x = u8 ? nullptr : d;
    step_.xu = u8 ? reinterpret_cast<const uint8_t*>(d) : nullptr;
    step_.ylab = d + x_floats(u8);
    step_.lr = step_.ylab + ny();
    hipError_t e = dtfk_graph_mlp_step(&step_, st);
    if (e == hipSuccess && ipc_ != nullptr) {
      (void)ipc_->begin();   // (throws on a failed earlier collective; chains streams like every IPC call)
      const int64_t nW1 = (int64_t)step_.K * step_.H, nW2 = (int64_t)step_.H * step_.C;
      ipc_->reduce_sgd_raw(grad_.data_ptr<float>(), nW1 + step_.H + nW2 + step_.C,
                           {step_.W1, step_.b1, step_.W2, step_.b2}, {nW1, (int64_t)step_.H, nW2, (int64_t)step_.C},
                           step_.lr, 0.f, 1.f / (float)ipc_->world_size(), gs_.ptr, gs_.kind, step_.metrics,
                           step_.host_metrics, st);
    }
    if (e == hipSuccess && use_graph_)
      e = hipMemcpyAsync(host_metrics_.data_ptr<float>(), step_.metrics, 3 * sizeof(float), hipMemcpyDeviceToHost, st);
    return e;
  }

  void capture(hipStream_t st) {
    if (graph_) { (void)hipGraphDestroy(graph_); graph_ = nullptr; }   // left by a failed instantiate
    hip_check(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal), "GraphStepPlan: begin capture");
    const hipError_t e = launch_step(st, false);
    hipGraph_t g = nullptr;
    const hipError_t e2 = hipStreamEndCapture(st, &g);
    hip_check(e, "GraphStepPlan: captured launches");
    hip_check(e2, "GraphStepPlan: end capture");
    graph_ = g;
    hip_check(hipGraphInstantiate(&exec_, graph_, nullptr, nullptr, 0), "GraphStepPlan: instantiate");
  }

  at::Tensor W1_, b1_, W2_, b2_, gstep_, dev_, a2_, dz2_, part_, metrics_, host_metrics_, grad_;
  at::Tensor stage_[2];
  py::object ipc_obj_;
  IpcColl* ipc_ = nullptr;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  hipEvent_t in_ev_ = nullptr, out_ev_ = nullptr;
  hipGraph_t graph_ = nullptr;
  hipGraphExec_t exec_ = nullptr;
  hipStream_t st_ = nullptr;
  dtfk::gmlp::Step step_{};   // filled at construction / attach_ipc; launch_step sets the feed pointers
  GstepRef gs_;               // the graph's global_step (with IPC the reduce + SGD kernel bumps it)
  bool use_graph_;
  int slot_ = 0;
  int64_t steps_ = 0;
  bool pending_[2] = {false, false};   // an event on the staging slot's copy may still be in flight
  double t_[3] = {0, 0, 0};
};

// The resident Session engine (compat/resident.py): the persistent fp32 kernel
// (csrc/kernels/mlp_persist_f32.hip, RES) stays launched across Session.run
// calls of the reference's training graph and is driven through pinned host
// memory -- per run the host writes the uint8 batch, its labels and lr into a
// record slot and bumps a doorbell; the kernel stages, trains one step on the
// graph's own W1 / b1 / W2 / b2 (written through every step, so other readers
// see current values), bumps global_step and stores loss / accuracy /
// global_step and a done count back into pinned memory.  No launch, no
// completion, no copy-engine op per run.  The launch exits by itself after
// `idle_s` without a doorbell (relaunched on the next run) or when stop() rings
// door = -1; either way every wave reaches the exit.
class ResidentMLPPlan {
 public:
  ResidentMLPPlan(at::Tensor W1, at::Tensor b1, at::Tensor W2, at::Tensor b2, c10::optional<at::Tensor> gstep, int B,
                  int act, bool naive, double idle_s, double timeout_s)
      : W1_(W1), b1_(b1), W2_(W2), b2_(b2), B_(B), act_(act), naive_(naive) {
    need_f32_device("ResidentMLPPlan", {&W1, &b1, &W2, &b2});
    TORCH_CHECK(W1.dim() == 2 && W1.size(0) == 784 && W1.size(1) == 100 && b1.numel() == 100 && W2.dim() == 2 &&
                    W2.size(0) == 100 && W2.size(1) == 10 && b2.numel() == 10,
                "ResidentMLPPlan: the reference's 784-100-10 shapes expected");
    TORCH_CHECK(B >= 1 && B <= dtfk_mlpf_max_batch(), "ResidentMLPPlan: batch must be in [1, ",
                dtfk_mlpf_max_batch(), "]");
    gkind_ = gstep_ref(gstep, "ResidentMLPPlan").kind;
    if (gstep.has_value()) gstep_ = *gstep;
    rec_h_ = ((int64_t)B * 785 + 15) / 16 * 16;
    const size_t bytes = 512 + 2 * (size_t)rec_h_;
    hip_check(hipHostMalloc(&mail_, bytes, hipHostMallocMapped | hipHostMallocCoherent), "ResidentMLPPlan: mailbox");
    std::memset(mail_, 0, bytes);
    char* m = static_cast<char*>(mail_);
    door_ = reinterpret_cast<long long*>(m);
    done_ = reinterpret_cast<long long*>(m + 64);
    state_ = reinterpret_cast<long long*>(m + 128);
    out_ = reinterpret_cast<float*>(m + 192);
    lr_ = reinterpret_cast<float*>(m + 256);
    recs_ = reinterpret_cast<uint8_t*>(m + 512);
    void* dp = nullptr;   // device-visible alias of the mailbox (unified addressing: the same address)
    if (hipHostGetDevicePointer(&dp, mail_, 0) != hipSuccess || dp == nullptr) {
      (void)hipGetLastError();
      dp = mail_;
    }
    dmail_ = static_cast<char*>(dp);
    auto o8 = W1.options().dtype(at::kByte);
    stage_ = at::zeros({2 * dtfk_mlpf_stage_rec()}, o8);
    xbuf_ = at::zeros({dtfk_mlpf_xbuf_bytes()}, o8);
    seq_ = at::zeros({1}, W1.options().dtype(at::kLong));
    kgstep_ = at::zeros({1}, W1.options().dtype(at::kLong));
    err_ = at::zeros({1}, W1.options().dtype(at::kInt));
    lrdev_ = at::zeros({1}, W1.options());
    metrics_ = at::zeros({2 * kRing}, W1.options());
    dctr_ = at::zeros({64}, W1.options().dtype(at::kInt));
    const char* rs = std::getenv("DTF_RESIDENT_STAMPS");   // profiling: per-run device stamps
    if (rs != nullptr && rs[0] == '1') res_ts_ = at::zeros({64 * 8}, W1.options().dtype(at::kLong));
    idle_ = (long long)(idle_s * 1e8);            // s_memrealtime: 100 MHz
    timeout_ = (long long)(timeout_s * 1e8);
    wait_s_ = std::max(5.0, 4.0 * idle_s + timeout_s);
    // The launch stays resident between runs, so no other work may queue behind
    // it: HIP maps streams onto GPU_MAX_HW_QUEUES (4) hardware queues round-robin,
    // and a stream sharing the resident kernel's queue (e.g. torch's, reading a
    // variable) waits until the idle exit.  DTF_RESIDENT_STREAM: "priority"
    // (default: a non-blocking high-priority stream -- its own queue as long as no
    // other high-priority stream exists), "cumask" (a CU-masked stream: its own
    // queue, but BLOCKING -- legacy-default-stream work waits for it; measured:
    // every variable read waited out the idle bound,
    // scripts/probes/resident_relaunch.py) or "plain".
    const char* sk = std::getenv("DTF_RESIDENT_STREAM");
    const std::string want = sk != nullptr ? sk : "priority";
    bool made = false;
    if (want == "cumask") {
      int ncu = 0;
      (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, W1.get_device());
      std::vector<uint32_t> mask((size_t)std::max(1, (ncu + 31) / 32), 0xffffffffu);
      made = ncu > 0 && hipExtStreamCreateWithCUMask(&st_, (uint32_t)mask.size(), mask.data()) == hipSuccess;
      if (made) stream_kind_ = "CU-masked (blocking) stream";
    } else if (want != "plain") {
      int lo = 0, hi = 0;
      made = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess &&
             hipStreamCreateWithPriority(&st_, hipStreamNonBlocking, hi) == hipSuccess;
      if (made) stream_kind_ = "high-priority non-blocking stream";
    }
    if (!made) {
      (void)hipGetLastError();
      hip_check(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking), "hipStreamCreate");
      stream_kind_ = "plain non-blocking stream";
    }
    hip_check(hipEventCreateWithFlags(&ev_, hipEventDisableTiming), "hipEventCreate");
  }
  ~ResidentMLPPlan() {
    try {
      stop();
    } catch (...) {
    }
    if (ev_) (void)hipEventDestroy(ev_);
    if (st_) (void)hipStreamDestroy(st_);
    if (mail_) (void)hipHostFree(mail_);
  }

  // One training step from the MNIST loader's uint8 batch [B, 784] and one-hot
  // float32 labels [B, 10].  False (nothing ran) when y_ is not exactly one-hot:
  // the caller takes the general plan.  Returns after the step; host_metrics()
  // then holds loss, accuracy, global_step (pre-update loss / accuracy, as the
  // graph evaluates them in the same run).
  bool run_u8(py::array xu8, py::array y, double lr) {
    TORCH_CHECK(xu8.dtype().is(py::dtype::of<uint8_t>()) && y.dtype().is(py::dtype::of<float>()),
                "ResidentMLPPlan.run_u8: uint8 x and float32 y_ expected");
    TORCH_CHECK((xu8.flags() & py::array::c_style) && (y.flags() & py::array::c_style),
                "ResidentMLPPlan.run_u8: C-contiguous feeds expected");
    TORCH_CHECK(xu8.size() == (int64_t)B_ * 784 && y.size() == (int64_t)B_ * 10,
                "ResidentMLPPlan.run_u8: feed shapes differ from the plan's");
    const uint8_t* xp = static_cast<const uint8_t*>(xu8.data());
    const float* yp = static_cast<const float*>(y.data());
    uint8_t lab[128];
    for (int b = 0; b < B_; ++b) {   // class ids; anything but an exact one-hot row -> general plan
      int hot = -1;
      for (int c = 0; c < 10; ++c) {
        const float v = yp[b * 10 + c];
        if (v == 1.0f && hot < 0) hot = c;
        else if (v != 0.0f) return false;
      }
      if (hot < 0) return false;
      lab[b] = (uint8_t)hot;
    }
    {
      py::gil_scoped_release nogil;
      using clk = std::chrono::steady_clock;
      const auto t0 = clk::now();
      if (alive_ && __atomic_load_n(state_, __ATOMIC_ACQUIRE) == launch_id_) {   // exited while idle
        reap();
        ++idle_exits_;
      }
      if (!alive_) launch();
      const int slot = (int)(runs_ & 1);
      uint8_t* rec = recs_ + slot * rec_h_;
      std::memcpy(rec, xp, (size_t)B_ * 784);
      std::memcpy(rec + (size_t)B_ * 784, lab, (size_t)B_);
      lr_[slot] = (float)lr;
      std::atomic_thread_fence(std::memory_order_seq_cst);
      __atomic_store_n(door_, runs_ + 1, __ATOMIC_RELEASE);
      const auto t1 = clk::now();
      t_[0] += std::chrono::duration<double, std::micro>(t1 - t0).count();
      long long spins = 0;
      while (__atomic_load_n(done_, __ATOMIC_ACQUIRE) < runs_ + 1) {
        if ((++spins & 1023) == 0) {
          if (__atomic_load_n(state_, __ATOMIC_ACQUIRE) == launch_id_ &&
              __atomic_load_n(done_, __ATOMIC_ACQUIRE) < runs_ + 1) {
            // the launch stopped (idle) without taking this run: start another
            reap();
            ++idle_exits_;
            launch();
          }
          if (std::chrono::duration<double>(clk::now() - t1).count() > wait_s_) {
            dead_ = true;
            throw std::runtime_error("ResidentMLPPlan: no completion within the wait bound");
          }
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
      }
      const double waited = std::chrono::duration<double, std::micro>(clk::now() - t1).count();
      host_wait_[runs_ & 63] = waited;
      ++runs_;
      t_[1] += waited;
    }
    return true;
  }

  // door = -1, then wait for the launch to finish (the variables hold the
  // trained values either way: every step writes them through)
  void stop() {
    if (!alive_) return;
    ++stops_;
    __atomic_store_n(door_, -1LL, __ATOMIC_RELEASE);
    reap();
  }

  bool alive() const { return alive_; }
  int64_t runs() const { return runs_; }
  int64_t launches() const { return launch_id_; }
  // profiling (DTF_RESIDENT_STAMPS=1): device stamps [run % 64][8] and the host's
  // door -> done wait of the same runs (us)
  py::object stamps() const {
    if (!res_ts_.defined()) return py::none();
    return py::make_tuple(res_ts_.cpu(), at::from_blob(const_cast<double*>(host_wait_), {64},
                                                       at::TensorOptions().dtype(at::kDouble)).clone());
  }
  at::Tensor host_metrics() const {
    return at::from_blob(out_, {3}, at::TensorOptions().dtype(at::kFloat));
  }
  py::dict timing() const {
    py::dict d;
    const double n = runs_ > 0 ? (double)runs_ : 1.0;
    d["feed_us"] = t_[0] / n;
    d["wait_us"] = t_[1] / n;
    d["runs"] = runs_;
    d["launches"] = launch_id_;
    d["stream"] = stream_kind_;
    d["stops"] = stops_;             // host-requested (quiesce / close)
    d["idle_exits"] = idle_exits_;   // the launch left by itself (idle bound)
    return d;
  }

 private:
  static constexpr int kRing = 64;

  void reap() {
    const hipError_t e = hipStreamSynchronize(st_);
    alive_ = false;
    hip_check(e, "ResidentMLPPlan: launch");
    int err = 0;
    hip_check(hipMemcpy(&err, err_.data_ptr(), sizeof(int), hipMemcpyDeviceToHost), "ResidentMLPPlan: err");
    if (err != 0) {
      dead_ = true;
      throw std::runtime_error("ResidentMLPPlan: the resident kernel reported error " + std::to_string(err));
    }
  }

  void launch() {
    TORCH_CHECK(!dead_, "ResidentMLPPlan: failed earlier");
    // whatever the caller's stream queued (initialisation, restores) lands first
    hip_check(hipEventRecord(ev_, cur_stream()), "ResidentMLPPlan: event");
    hip_check(hipStreamWaitEvent(st_, ev_, 0), "ResidentMLPPlan: wait");
    hip_check(hipMemsetAsync(dctr_.data_ptr(), 0, dctr_.numel() * sizeof(int), st_), "ResidentMLPPlan: counters");
    if (__atomic_load_n(door_, __ATOMIC_ACQUIRE) < 0) __atomic_store_n(door_, runs_, __ATOMIC_RELEASE);   // after stop()
    ++launch_id_;
    dtfk::mlpf::Launch p{};
    p.stage = stage_.data_ptr();
    p.rec_h = rec_h_;
    p.B = B_;
    p.params = W1_.data_ptr<float>();
    p.W2 = W2_.data_ptr<float>();
    p.b1 = b1_.data_ptr<float>();
    p.b2 = b2_.data_ptr<float>();
    p.lr = lrdev_.data_ptr<float>();
    p.metrics = metrics_.data_ptr<float>();
    p.ring = kRing;
    p.act = act_;
    p.naive = naive_ ? 1 : 0;
    p.gstep = reinterpret_cast<long long*>(kgstep_.data_ptr<int64_t>());
    p.seq = reinterpret_cast<unsigned long long*>(seq_.data_ptr<int64_t>());
    p.xbuf = xbuf_.data_ptr();
    p.err = err_.data_ptr<int>();
    p.timeout = timeout_;
    p.W = 1;
    p.split = 1;
    p.door = reinterpret_cast<const long long*>(dmail_);
    p.host_recs = dmail_ + 512;
    p.host_lr = reinterpret_cast<const float*>(dmail_ + 256);
    p.host_out = reinterpret_cast<float*>(dmail_ + 192);
    p.host_done = reinterpret_cast<long long*>(dmail_ + 64);
    p.host_state = reinterpret_cast<long long*>(dmail_ + 128);
    p.launch_id = launch_id_;
    p.run0 = runs_;
    p.idle = idle_;
    p.gvar = gkind_ ? gstep_.data_ptr() : nullptr;
    p.gvar_kind = gkind_;
    p.dctr = reinterpret_cast<unsigned*>(dctr_.data_ptr<int>());
    p.res_ts = res_ts_.defined() ? reinterpret_cast<long long*>(res_ts_.data_ptr<int64_t>()) : nullptr;
    hip_check(dtfk_mlp_persist_f32_launch(&p, st_), "ResidentMLPPlan: launch");
    alive_ = true;
  }

  at::Tensor W1_, b1_, W2_, b2_, gstep_, stage_, xbuf_, seq_, kgstep_, err_, lrdev_, metrics_, dctr_, res_ts_;
  double host_wait_[64] = {0};
  int B_, act_, gkind_ = 0;
  bool naive_;
  int64_t rec_h_ = 0;
  const char* stream_kind_ = "";
  int64_t stops_ = 0, idle_exits_ = 0;
  void* mail_ = nullptr;
  char* dmail_ = nullptr;
  long long* door_ = nullptr;
  long long* done_ = nullptr;
  long long* state_ = nullptr;
  float* out_ = nullptr;
  float* lr_ = nullptr;
  uint8_t* recs_ = nullptr;
  long long idle_ = 0, timeout_ = 0;
  double wait_s_ = 5.0;
  hipStream_t st_ = nullptr;
  hipEvent_t ev_ = nullptr;
  bool alive_ = false, dead_ = false;
  long long runs_ = 0, launch_id_ = 0;
  double t_[2] = {0, 0};
};

void init_mlp(py::module& m) {
  py::class_<ResidentMLPPlan>(m, "ResidentMLPPlan")
      .def(py::init<at::Tensor, at::Tensor, at::Tensor, at::Tensor, c10::optional<at::Tensor>, int, int, bool, double,
                    double>(),
           py::arg("W1"), py::arg("b1"), py::arg("W2"), py::arg("b2"), py::arg("gstep"), py::arg("B"), py::arg("act"),
           py::arg("naive"), py::arg("idle_s") = 0.002, py::arg("timeout_s") = 10.0)
      .def("run_u8", &ResidentMLPPlan::run_u8, py::arg("xu8"), py::arg("y"), py::arg("lr"))
      .def("stop", &ResidentMLPPlan::stop)
      .def("alive", &ResidentMLPPlan::alive)
      .def("runs", &ResidentMLPPlan::runs)
      .def("launches", &ResidentMLPPlan::launches)
      .def("host_metrics", &ResidentMLPPlan::host_metrics)
      .def("timing", &ResidentMLPPlan::timing)
      .def("stamps", &ResidentMLPPlan::stamps);
  py::class_<GraphStepPlan>(m, "GraphStepPlan")
      .def(py::init<at::Tensor, at::Tensor, at::Tensor, at::Tensor, c10::optional<at::Tensor>, int, int, bool, bool>(),
           py::arg("W1"), py::arg("b1"), py::arg("W2"), py::arg("b2"), py::arg("gstep"), py::arg("B"), py::arg("act"),
           py::arg("naive"), py::arg("use_graph") = false)
      .def("use_graph", &GraphStepPlan::use_graph)
      .def("run", &GraphStepPlan::run, py::arg("x"), py::arg("y"), py::arg("lr"), py::arg("sync"))
      .def("run_u8", &GraphStepPlan::run_u8, py::arg("xu8"), py::arg("y"), py::arg("lr"), py::arg("sync"))
      .def("host_metrics", &GraphStepPlan::host_metrics)
      .def("attach_ipc", &GraphStepPlan::attach_ipc)
      .def("has_ipc", &GraphStepPlan::has_ipc)
      .def("steps", &GraphStepPlan::steps)
      .def("timing", &GraphStepPlan::timing);
  m.def("graph_mlp_step", &graph_mlp_step, py::arg("x"), py::arg("ylab"), py::arg("W1"), py::arg("b1"),
        py::arg("W2"), py::arg("b2"), py::arg("a2buf"), py::arg("dz2buf"), py::arg("grads"), py::arg("metrics"),
        py::arg("gstep"), py::arg("lr"), py::arg("act"), py::arg("naive"), py::arg("sgd"));
  m.def("mlp_eval", &mlp_eval, py::arg("x"), py::arg("labels"), py::arg("W1"), py::arg("b1"), py::arg("W2"),
        py::arg("b2"), py::arg("act"), py::arg("naive"), py::arg("out"), py::arg("reset"),
        py::arg("pred") = py::none(), py::arg("logits") = py::none());
  py::class_<PersistF32Plan>(m, "PersistF32Plan")
      .def(py::init<at::Tensor, at::Tensor, int64_t, int, at::Tensor, at::Tensor, at::Tensor, at::Tensor,
                    at::Tensor, at::Tensor, at::Tensor, double, int, int, at::Tensor, at::Tensor, int64_t, int, int,
                    bool, bool, bool, bool>())
      .def("set_phase_ts", &PersistF32Plan::set_phase_ts, py::arg("phase_ts"))
      .def("launch", &PersistF32Plan::launch);
  m.def("mlpf_stage_rec", &dtfk_mlpf_stage_rec);
  m.def("mlpf_set_fault", &dtfk_mlpf_set_fault, py::arg("rank"), py::arg("step"));
  m.def("mlpf_xbuf_bytes", &dtfk_mlpf_xbuf_bytes);
  m.def("mlpf_ipc_bytes", &dtfk_mlpf_ipc_bytes);
  m.def("mlpf_max_batch", &dtfk_mlpf_max_batch);
  m.def("mlp_ksplit", &dtfk_mlp_ksplit);
  m.def("mlp_l1_fwd", &mlp_l1_fwd, py::arg("x"), py::arg("x_offset"), py::arg("x_kind"),
        py::arg("B"), py::arg("W1T"), py::arg("z2p"), py::arg("ts") = py::none());
  m.def("mlp_head_bwd", &mlp_head_bwd, py::arg("z2p"), py::arg("labels"), py::arg("labels_offset"),
        py::arg("B"), py::arg("W2T"), py::arg("W2N"), py::arg("params"), py::arg("dz2T"),
        py::arg("partials"),
        py::arg("inv_batch"), py::arg("act"), py::arg("naive_loss"), py::arg("gstep"), py::arg("ts") = py::none());
  m.def("mlp_wgrad", &mlp_wgrad, py::arg("x"), py::arg("x_offset"), py::arg("x_kind"),
        py::arg("dz2T"), py::arg("B"), py::arg("partials"), py::arg("params"), py::arg("W1T"),
        py::arg("W2T"), py::arg("W2N"), py::arg("grads"), py::arg("grad_kind"), py::arg("lr"),
        py::arg("metrics"),
        py::arg("gstep"), py::arg("ts") = py::none(), py::arg("ipc_table") = 0, py::arg("ipc_W") = 0,
        py::arg("ipc_rank") = 0, py::arg("ipc_parity") = 0, py::arg("ipc_slot_bytes") = 0,
        py::arg("ipc_err") = py::none(), py::arg("ipc_timeout_s") = 5.0);
  m.def("mlp_apply_flat", &mlp_apply_flat);
  m.def("mlp_ipc_reduce_apply", &mlp_ipc_reduce_apply);
  m.def("mlp_ipc_flag_bytes", &dtfk_mlp_ipc_flag_bytes);
  m.def("memcpy_h2d_async", &memcpy_h2d_async);
  m.def("mlpg_fwd", &mlpg_fwd, py::arg("x"), py::arg("x_offset"), py::arg("labels"), py::arg("labels_offset"),
        py::arg("B"), py::arg("W1F"), py::arg("params"), py::arg("a2"), py::arg("P1"), py::arg("dz2F"), py::arg("act"),
        py::arg("naive"), py::arg("gscale"));
  m.def("mlpg_wgrad", &mlpg_wgrad, py::arg("x"), py::arg("x_offset"), py::arg("B"), py::arg("dz2S"), py::arg("P2"),
        py::arg("nchunk"));
  m.def("mlpg_apply", &mlpg_apply, py::arg("params"), py::arg("P1"), py::arg("P2"), py::arg("nchunk"),
        py::arg("gin"), py::arg("gout"), py::arg("lr"), py::arg("scale"), py::arg("W1S"), py::arg("metrics"),
        py::arg("gstep"), py::arg("B"), py::arg("mode"));
  m.def("mlpg_p1_floats", &dtfk_mlpg_p1_floats);
  m.def("mlpg_wchunk", &dtfk_mlpg_wchunk);
  m.def("mlpg_p2_floats", &dtfk_mlpg_p2_floats);
}

}  // namespace dtf
