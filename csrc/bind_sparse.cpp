// The one-GPU sparse logistic-regression step of lr2.py as ONE host call
// (csrc/kernels/sparse_lr.hip).  SparseLRPlan.run takes lr2.py's own feed
// arrays -- labels y [B, 1], SparseTensor indices [nnz, 2] (row, column),
// feature ids [nnz], values [nnz] (lr2.py:440-446) -- builds the CSR row
// offsets (a stable counting sort when the COO entries are not in row order),
// packs ids | offsets | values | labels into a pinned staging slot (mapped,
// coherent host memory) with the GIL released and issues the two step kernels
// on the caller's stream: the forward kernel reads the slot in place and leaves
// device copies of ids / offsets / values for the apply kernel (DTF_SLR_FEED=
// stage: a staging kernel copies the slot first; =dma: an SDMA hipMemcpyAsync,
// which ran as a 36 us blit and cost ~40 us of host time per call on MI355X --
// profiles/lr2_compat_r5.json).  Returns without waiting (staging slots are
// double buffered behind events).  SparseLRPlan.step runs the same kernels on device
// tensors (models/sparse_lr.py, one worker).  SparseLRPlan.set_ftrl switches
// both entry points from scatter-SGD to the FTRL-Proximal update (slr_fwd + the
// three slr_ftrl_* kernels); a plan without it runs what it always ran.
// SparseLRPlan.evaluate / eval_csr / eval_coo are the forward-only evaluation
// (slr_eval_rows + the record's reduce, eval_record.hip) of device tensors /
// the same host feeds: packing, int32 ids and the two staging slots are the training step's
// (submit_), the kernels read W and b only and add the batch to a device record.
#include "bind_common.h"
#include "eval_record_host.h"
#include "gstep_host.h"
#include "kernels/sparse_lr_api.h"

#include <pybind11/numpy.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace dtf {

static int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

class SparseLRPlan {
 public:
  SparseLRPlan(at::Tensor W, at::Tensor bias, c10::optional<at::Tensor> gstep) : W_(W), bias_(bias) {
    TORCH_CHECK(W.is_cuda() && W.scalar_type() == at::kFloat && W.is_contiguous() &&
                    (W.dim() == 1 || (W.dim() == 2 && W.size(1) == 1)),
                "SparseLRPlan: W must be a contiguous fp32 [F, 1] GPU table");
    TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == at::kFloat && bias.numel() == 1 && bias.is_contiguous(),
                "SparseLRPlan: bias must be one fp32 GPU value");
    F_ = W.size(0);
    gs_ = gstep_ref(gstep, "SparseLRPlan");
    if (gstep.has_value()) gstep_ = *gstep;   // keeps gs_.ptr alive
    auto fo = W.options();
    loss_ = at::zeros({1}, fo);
    bad_ = at::zeros({1}, fo.dtype(at::kInt));
    for (int i = 0; i < 2; ++i) hip_check(hipEventCreateWithFlags(&ev_[i], hipEventDisableTiming), "hipEventCreate");
    const char* fe = std::getenv("DTF_SLR_FEED");
    const std::string f = fe != nullptr ? fe : "direct";
    feed_ = f == "dma" ? 2 : (f == "stage" ? 1 : (f == "overlap" ? 3 : 0));
    const char* rp = std::getenv("DTF_SLR_RPW");
    dtfk_slr_set_rows_per_wg(rp != nullptr ? std::atoi(rp) : 32);
    if (feed_ == 3) {
      // the next batch's staging copy runs on a queue of its own, under the
      // current step's kernels (a CU mask is a queue property: a CU-masked stream
      // does not share a hardware queue with the compute stream)
      int ncu = 0;
      (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, W.get_device());
      std::vector<uint32_t> mask((size_t)std::max(1, (ncu + 31) / 32), 0xffffffffu);
      if (ncu <= 0 || hipExtStreamCreateWithCUMask(&side_, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
        (void)hipGetLastError();
        hip_check(hipStreamCreateWithFlags(&side_, hipStreamNonBlocking), "SparseLRPlan: side stream");
      }
      for (int i = 0; i < 2; ++i) hip_check(hipEventCreateWithFlags(&evs_[i], hipEventDisableTiming), "hipEventCreate");
    }
  }
  ~SparseLRPlan() {
    for (int i = 0; i < 2; ++i) {
      if (pending_[i]) (void)hipEventSynchronize(ev_[i]);
      if (ev_[i]) (void)hipEventDestroy(ev_[i]);
      if (hbuf_[i]) (void)hipHostFree(hbuf_[i]);
      if (evs_[i]) (void)hipEventDestroy(evs_[i]);
    }
    if (side_) (void)hipStreamDestroy(side_);
  }

  // From now on the step applies FTRL-Proximal instead of scatter-SGD.  accum /
  // linear: W's slots (same shape); bias_slots: {bias accum, bias linear}.  The
  // plan adds the dense gradient accumulator (W's size, zero between steps):
  // memory is W + 3 arrays of W's size.
  void set_ftrl(at::Tensor accum, at::Tensor linear, at::Tensor bias_slots, double lr_power, double l1, double l2,
                double l2_shrinkage) {
    for (const at::Tensor* t : {&accum, &linear})
      TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == F_ &&
                      t->get_device() == W_.get_device(),
                  "SparseLRPlan.set_ftrl: accum / linear must be contiguous fp32 GPU tensors of W's size");
    TORCH_CHECK(bias_slots.is_cuda() && bias_slots.scalar_type() == at::kFloat && bias_slots.is_contiguous() &&
                    bias_slots.numel() == 2,
                "SparseLRPlan.set_ftrl: bias_slots must be two fp32 GPU values");
    TORCH_CHECK(lr_power <= 0 && l1 >= 0 && l2 >= 0 && l2_shrinkage >= 0,
                "SparseLRPlan.set_ftrl: learning_rate_power <= 0 and l1, l2, l2_shrinkage >= 0");
    acc_ = accum;
    lin_ = linear;
    bslots_ = bias_slots;
    gsum_ = at::zeros({F_}, W_.options());
    hp_[0] = (float)lr_power, hp_[1] = (float)l1, hp_[2] = (float)l2, hp_[3] = (float)l2_shrinkage;
    ftrl_ = true;
  }
  bool ftrl() const { return ftrl_; }
  // the FTRL step's gradient accumulator (all 0.0 between steps)
  at::Tensor grad_accumulator() const {
    TORCH_CHECK(ftrl_, "SparseLRPlan.grad_accumulator: not an FTRL plan");
    return gsum_;
  }

  // lr2.py's feeds (numpy).  False: not applicable (dtypes, shapes, a row index
  // outside [0, B)) -- nothing ran, the caller takes the general path.
  bool run(py::array y, py::array idx, py::array ids, py::array vals, double lr) {
    return coo_(y, idx, ids, vals, true, [&](const Feed& f, hipStream_t st) { train_go_(f, lr, st); });
  }

  // A host CSR batch (the native trainer's own layout: labels [B] / [B, 1] f32,
  // offsets [B + 1] i64, ids [nnz] i64, vals [nnz] f32 or None) through the same
  // packed feed.  False: not applicable (dtypes / shapes / offsets not a CSR of nnz).
  bool run_csr(py::array y, py::array offsets, py::array ids, py::object vals_o, double lr) {
    return csr_(y, offsets, ids, vals_o, true, [&](const Feed& f, hipStream_t st) { train_go_(f, lr, st); });
  }

  // Forward-only evaluation of host feeds (run's / run_csr's arrays, packing
  // and staging slots): the batch's loss sum, row count, out-of-range ids and
  // streaming_auc histograms are added to `record` (kernels/eval_record.h, on
  // the device; reset: start it over).
  // pred / logits: optional [B] fp32 outputs (sigmoid(z), z).  Nothing of the
  // training state changes.  False: a feed run / run_csr would refuse, nothing ran.
  // The record and the outputs are checked first: a wrong record / pred / logits
  // raises whatever the feed is.
  bool eval_coo(py::array y, py::array idx, py::array ids, py::array vals, at::Tensor record, bool reset,
                c10::optional<at::Tensor> pred, c10::optional<at::Tensor> logits) {
    const EvalOut o = eval_out("SparseLRPlan", W_.get_device(), y.size(), record, reset, pred, logits);
    return coo_(y, idx, ids, vals, false, [&](const Feed& f, hipStream_t st) { eval_go_(f, o, st); });
  }
  bool eval_csr(py::array y, py::array offsets, py::array ids, py::object vals_o, at::Tensor record, bool reset,
                c10::optional<at::Tensor> pred, c10::optional<at::Tensor> logits) {
    const EvalOut o = eval_out("SparseLRPlan", W_.get_device(), y.size(), record, reset, pred, logits);
    return csr_(y, offsets, ids, vals_o, false, [&](const Feed& f, hipStream_t st) { eval_go_(f, o, st); });
  }

 private:
  // one packed feed in its staging slot: h the pinned host slot, hd its device
  // view, d the device copy; byte offsets of ids | offsets | values | labels
  struct Feed {
    char* h;
    const char* hd;
    char* d;
    int64_t o_ids, o_off, o_val, o_lab, total;
    int B, slot;
    bool i32;
  };

  template <typename Go>
  bool coo_(py::array y, py::array idx, py::array ids, py::array vals, bool train, Go&& go) {
    if (!y.dtype().is(py::dtype::of<float>()) || !idx.dtype().is(py::dtype::of<int64_t>()) ||
        !ids.dtype().is(py::dtype::of<int64_t>()) || !vals.dtype().is(py::dtype::of<float>()))
      return false;
    const int64_t B = y.size(), n = ids.size();
    if (B < 1 || B > (1 << 30) || vals.size() != n || (n > 0 && (idx.ndim() != 2 || idx.shape(0) != n || idx.shape(1) < 2)))
      return false;
    // strided views are fine: read through the numpy strides
    const char* yb = static_cast<const char*>(y.data());
    const char* ib = static_cast<const char*>(idx.data());
    const char* fb = static_cast<const char*>(ids.data());
    const char* vb = static_cast<const char*>(vals.data());
    const int64_t ys = y.ndim() >= 1 ? y.strides(0) : 4;
    const int64_t is0 = n > 0 ? idx.strides(0) : 0;
    const int64_t fs = ids.ndim() >= 1 ? ids.strides(0) : 8, vs = vals.ndim() >= 1 ? vals.strides(0) : 4;
    if (y.ndim() > 2 || ids.ndim() > 1 || vals.ndim() > 1 || (y.ndim() == 2 && y.shape(1) != 1 && y.shape(0) != 1))
      return false;
    const int64_t ys_el = (y.ndim() == 2 && y.shape(0) == 1) ? y.strides(1) : ys;
    return submit_(B, n, train, [&](int64_t* hoff, int64_t* hid, int32_t* hid32, float* hval, float* hlab, bool i32) {
      // rows -> CSR offsets: in row order (lr2.py's own feeds, as_tf_feed) the
      // offsets are the row boundaries, found in one pass; otherwise a stable
      // counting sort by row (the same bags: the 'sum' combiner)
      bool ok = true, sorted = true;
      auto row = [&](int64_t j) { return *reinterpret_cast<const int64_t*>(ib + j * is0); };
      // one pass: row range, order and (in order) the CSR boundaries -- the
      // common case, lr2.py's own row-major feeds (as_tf_feed); a row out of
      // order sends the batch to the stable counting sort below
      int64_t prev = n > 0 ? row(0) : B;
      if (n > 0 && (prev < 0 || prev >= B)) return false;
      for (int64_t b = 0; b <= prev && b <= B; ++b) hoff[b] = 0;
      for (int64_t j = 1; j < n; ++j) {
        const int64_t r = row(j);
        if (r != prev) {
          if (r < prev || r >= B) {
            sorted = false;
            break;
          }
          for (int64_t b = prev + 1; b <= r; ++b) hoff[b] = j;
          prev = r;
        }
      }
      if (sorted) {
        for (int64_t b = prev + 1; b <= B; ++b) hoff[b] = n;
      } else {
        for (int64_t j = 0; j < n && ok; ++j) {
          const int64_t r = row(j);
          ok = r >= 0 && r < B;
        }
      }
      if (!ok) return false;
      if (sorted) {
        pack_ids_(hid, hid32, i32, fb, fs, n);
        if (vs == 4) std::memcpy(hval, vb, 4 * (size_t)n);
        else for (int64_t j = 0; j < n; ++j) hval[j] = *reinterpret_cast<const float*>(vb + j * vs);
      } else {
        std::vector<int64_t>& cnt = cnt_;
        cnt.assign((size_t)B + 1, 0);
        for (int64_t j = 0; j < n; ++j) ++cnt[(size_t)row(j) + 1];
        for (int64_t b = 0; b < B; ++b) cnt[(size_t)b + 1] += cnt[(size_t)b];
        std::memcpy(hoff, cnt.data(), sizeof(int64_t) * (size_t)(B + 1));
        const int64_t F = F_;
        for (int64_t j = 0; j < n; ++j) {
          const int64_t dd = cnt[(size_t)row(j)]++;
          const int64_t id = *reinterpret_cast<const int64_t*>(fb + j * fs);
          if (i32) hid32[dd] = ((uint64_t)id < (uint64_t)F) ? (int32_t)id : -1;
          else hid[dd] = id;
          hval[dd] = *reinterpret_cast<const float*>(vb + j * vs);
        }
      }
      for (int64_t b = 0; b < B; ++b) hlab[b] = *reinterpret_cast<const float*>(yb + b * ys_el);
      return true;
    }, go);
  }

  template <typename Go>
  bool csr_(py::array y, py::array offsets, py::array ids, py::object vals_o, bool train, Go&& go) {
    if (!y.dtype().is(py::dtype::of<float>()) || !offsets.dtype().is(py::dtype::of<int64_t>()) ||
        !ids.dtype().is(py::dtype::of<int64_t>()))
      return false;
    py::array vals;
    const bool has_v = !vals_o.is_none();
    if (has_v) {
      vals = py::array::ensure(vals_o);
      if (!vals || !vals.dtype().is(py::dtype::of<float>()) || vals.ndim() != 1 || vals.size() != ids.size()) return false;
    }
    const int64_t B = y.size(), n = ids.size();
    if (B < 1 || B > (1 << 30) || offsets.ndim() != 1 || offsets.size() != B + 1 || ids.ndim() != 1) return false;
    const char* yb = static_cast<const char*>(y.data());
    const char* ob = static_cast<const char*>(offsets.data());
    const char* fb = static_cast<const char*>(ids.data());
    const char* vb = has_v ? static_cast<const char*>(vals.data()) : nullptr;
    const int64_t ys = (y.ndim() == 2 && y.shape(0) == 1) ? y.strides(1) : (y.ndim() >= 1 ? y.strides(0) : 4);
    const int64_t os = offsets.strides(0), fs = ids.strides(0), vs = has_v ? vals.strides(0) : 4;
    if (y.ndim() > 2 || (y.ndim() == 2 && y.shape(1) != 1 && y.shape(0) != 1)) return false;
    return submit_(B, n, train, [&](int64_t* hoff, int64_t* hid, int32_t* hid32, float* hval, float* hlab, bool i32) {
      int64_t prev = 0;
      for (int64_t b = 0; b <= B; ++b) {
        const int64_t o = *reinterpret_cast<const int64_t*>(ob + b * os);
        if (o < prev || o > n || (b == 0 && o != 0)) return false;
        hoff[b] = prev = o;
      }
      if (hoff[B] != n) return false;
      pack_ids_(hid, hid32, i32, fb, fs, n);
      if (!has_v) for (int64_t j = 0; j < n; ++j) hval[j] = 1.f;
      else if (vs == 4) std::memcpy(hval, vb, 4 * (size_t)n);
      else for (int64_t j = 0; j < n; ++j) hval[j] = *reinterpret_cast<const float*>(vb + j * vs);
      for (int64_t b = 0; b < B; ++b) hlab[b] = *reinterpret_cast<const float*>(yb + b * ys);
      return true;
    }, go);
  }

  // out-of-range ids are kept as such (the kernels count and skip them): in
  // int32 form anything outside [0, F) becomes -1
  void pack_ids_(int64_t* hid, int32_t* hid32, bool i32, const char* fb, int64_t fs, int64_t n) const {
    const int64_t F = F_;
    if (i32 && fs == 8) {
      const int64_t* f = reinterpret_cast<const int64_t*>(fb);
      for (int64_t j = 0; j < n; ++j) hid32[j] = ((uint64_t)f[j] < (uint64_t)F) ? (int32_t)f[j] : -1;
    } else if (!i32 && fs == 8) {
      std::memcpy(hid, fb, 8 * (size_t)n);
    } else {
      for (int64_t j = 0; j < n; ++j) {
        const int64_t id = *reinterpret_cast<const int64_t*>(fb + j * fs);
        if (i32) hid32[j] = ((uint64_t)id < (uint64_t)F) ? (int32_t)id : -1;
        else hid[j] = id;
      }
    }
  }

  // Packs one batch (fill writes the CSR offsets, ids, values and labels into
  // the pinned slot) with the GIL released, then go(feed, stream) moves it to the
  // device and launches the kernels -- the training step or the evaluation:
  // both share the slots, their events and the device copy.  False when fill
  // refused the batch (nothing was launched).  Only a training run counts in
  // runs() / timing().
  template <typename Fill, typename Go>
  bool submit_(int64_t B, int64_t n, bool train, Fill&& fill, Go&& go) {
    // ids travel as int32 when the table has < 2^31 rows (lr2's F = 1e9 does): half the bytes
    const bool i32 = F_ < (1LL << 31);
    const int64_t isz = i32 ? 4 : 8;
    Feed f;
    f.i32 = i32;
    f.B = (int)B;
    f.o_ids = 0, f.o_off = align16(isz * n), f.o_val = f.o_off + align16(8 * (B + 1));
    f.o_lab = f.o_val + align16(4 * n), f.total = f.o_lab + align16(4 * B);
    const int64_t total = f.total;
    const int slot = f.slot = slot_ ^ 1;
    bool ok = true;
    if (train) ensure_rows_(B);
    else esc_.ensure(B, W_.options());
    at::Tensor& dvb = feed_ == 3 ? dev2_[slot] : dev_;   // overlap: one device copy per slot
    if (dvb.numel() < total) dvb = at::empty({std::max<int64_t>(total, 1 << 20)}, W_.options().dtype(at::kByte));
    hipStream_t st = cur_stream();
    f.d = static_cast<char*>(dvb.data_ptr());
    {
      py::gil_scoped_release nogil;
      using clk = std::chrono::steady_clock;
      const auto t0 = clk::now();
      if (pending_[slot]) hip_check(hipEventSynchronize(ev_[slot]), "SparseLRPlan: staging slot");
      pending_[slot] = false;
      if (hcap_[slot] < total) {   // mapped + coherent: the staging kernel reads it in place
        if (hbuf_[slot]) hip_check(hipHostFree(hbuf_[slot]), "hipHostFree");
        hbuf_[slot] = nullptr;
        const int64_t cap = std::max<int64_t>(total, 1 << 20);
        hip_check(hipHostMalloc(&hbuf_[slot], (size_t)cap, hipHostMallocMapped | hipHostMallocCoherent),
                  "SparseLRPlan: pinned staging slot");
        hip_check(hipHostGetDevicePointer(&hdev_[slot], hbuf_[slot], 0), "SparseLRPlan: staging slot device view");
        hcap_[slot] = cap;
      }
      const auto tw = clk::now();   // slot wait (+ first-use allocation) | packing
      char* h = f.h = static_cast<char*>(hbuf_[slot]);
      f.hd = static_cast<const char*>(hdev_[slot]);
      ok = fill(reinterpret_cast<int64_t*>(h + f.o_off), reinterpret_cast<int64_t*>(h + f.o_ids),
                reinterpret_cast<int32_t*>(h + f.o_ids), reinterpret_cast<float*>(h + f.o_val),
                reinterpret_cast<float*>(h + f.o_lab), i32);
      if (ok) {
        slot_ = slot;
        const auto t1 = clk::now();
        go(f, st);
        if (train) {
          t_[2] += std::chrono::duration<double, std::micro>(tw - t0).count();
          t_[0] += std::chrono::duration<double, std::micro>(t1 - tw).count();
          t_[1] += std::chrono::duration<double, std::micro>(clk::now() - t1).count();
        }
      }
    }
    if (!ok) return false;
    if (train) ++runs_;
    else ++eval_runs_;
    return true;
  }

  // the training step on a packed feed (the feed modes of DTF_SLR_FEED)
  void train_go_(const Feed& f, double lr, hipStream_t st) {
    const int slot = f.slot;
    const int64_t o_ids = f.o_ids, o_off = f.o_off, o_val = f.o_val, o_lab = f.o_lab, total = f.total;
    const bool i32 = f.i32;
    const int B = f.B;
    char* d = f.d;
    if (feed_ == 0) {
      // the forward kernel reads the slot in place and leaves device copies for the apply
      const char* hd = f.hd;
      if (ftrl_) {
        hip_check(dtfk_slr_ftrl_step_direct(W_.data_ptr<float>(), (long long)F_, hd + o_ids, i32 ? 1 : 0,
                                            reinterpret_cast<const long long*>(hd + o_off),
                                            reinterpret_cast<const float*>(hd + o_val),
                                            reinterpret_cast<const float*>(hd + o_lab), d + o_ids,
                                            reinterpret_cast<long long*>(d + o_off),
                                            reinterpret_cast<float*>(d + o_val), bias_.data_ptr<float>(), B, (float)lr,
                                            dz_.data_ptr<float>(), lrow_.data_ptr<float>(), loss_.data_ptr<float>(),
                                            bad_.data_ptr<int>(), gs_.ptr, gs_.kind, acc_.data_ptr<float>(),
                                            lin_.data_ptr<float>(), gsum_.data_ptr<float>(), bslots_.data_ptr<float>(),
                                            hp_[0], hp_[1], hp_[2], hp_[3], st),
                  "SparseLRPlan: FTRL step");
      } else {
        hip_check(dtfk_slr_step_direct(W_.data_ptr<float>(), (long long)F_, hd + o_ids, i32 ? 1 : 0,
                                       reinterpret_cast<const long long*>(hd + o_off),
                                       reinterpret_cast<const float*>(hd + o_val),
                                       reinterpret_cast<const float*>(hd + o_lab), d + o_ids,
                                       reinterpret_cast<long long*>(d + o_off), reinterpret_cast<float*>(d + o_val),
                                       bias_.data_ptr<float>(), B, (float)lr, dz_.data_ptr<float>(),
                                       lrow_.data_ptr<float>(), loss_.data_ptr<float>(), bad_.data_ptr<int>(), gs_.ptr,
                                       gs_.kind, st),
                  "SparseLRPlan: step");
      }
      hip_check(hipEventRecord(ev_[slot], st), "SparseLRPlan: event");
      pending_[slot] = true;
    } else if (feed_ == 3) {
      hip_check(dtfk_slr_stage(f.hd, d, total, side_), "SparseLRPlan: feed staging");
      hip_check(hipEventRecord(evs_[slot], side_), "SparseLRPlan: event");
      hip_check(hipStreamWaitEvent(st, evs_[slot], 0), "SparseLRPlan: wait staging");
      launch(d + o_ids, i32, reinterpret_cast<const long long*>(d + o_off), reinterpret_cast<const float*>(d + o_val),
             reinterpret_cast<const float*>(d + o_lab), B, (float)lr, st);
      hip_check(hipEventRecord(ev_[slot], st), "SparseLRPlan: event");   // host + device slot free after the step
      pending_[slot] = true;
    } else {
      if (feed_ == 2)
        hip_check(hipMemcpyAsync(d, f.h, (size_t)total, hipMemcpyHostToDevice, st), "SparseLRPlan: feed copy");
      else hip_check(dtfk_slr_stage(f.hd, d, total, st), "SparseLRPlan: feed staging");
      hip_check(hipEventRecord(ev_[slot], st), "SparseLRPlan: event");
      pending_[slot] = true;
      launch(d + o_ids, i32, reinterpret_cast<const long long*>(d + o_off), reinterpret_cast<const float*>(d + o_val),
             reinterpret_cast<const float*>(d + o_lab), B, (float)lr, st);
    }
  }

  // the evaluation on a packed feed: read in place from the pinned slot (the
  // default feed mode; no staging copy), else staged on the caller's stream first
  void eval_go_(const Feed& f, const EvalOut& o, hipStream_t st) {
    const bool direct = feed_ == 0;
    if (feed_ == 2)
      hip_check(hipMemcpyAsync(f.d, f.h, (size_t)f.total, hipMemcpyHostToDevice, st), "SparseLRPlan: feed copy");
    else if (!direct) hip_check(dtfk_slr_stage(f.hd, f.d, f.total, st), "SparseLRPlan: feed staging");
    const char* src = direct ? f.hd : f.d;
    eval_launch_(src + f.o_ids, f.i32, reinterpret_cast<const long long*>(src + f.o_off),
                 reinterpret_cast<const float*>(src + f.o_val), reinterpret_cast<const float*>(src + f.o_lab), direct,
                 f.B, o, st);
    // slot (and device copy) free after the kernels
    hip_check(hipEventRecord(ev_[f.slot], st), "SparseLRPlan: event");
    pending_[f.slot] = true;
  }

  void eval_launch_(const void* ids, bool i32, const long long* offs, const float* vals, const float* labels,
                    bool direct, int B, const EvalOut& o, hipStream_t st) {
    // the scratch's quarters: lrow | prow | labels | bad ids per row (int)
    hip_check(dtfk_slr_eval(W_.data_ptr<float>(), (long long)F_, ids, i32 ? 1 : 0, offs, vals, labels, esc_.part(2),
                            direct ? 1 : 0, bias_.data_ptr<float>(), B, esc_.part(0), esc_.part(1),
                            reinterpret_cast<int*>(esc_.part(3)), bad_.data_ptr<int>(), o.logits, o.pred, o.T, o.reset,
                            o.rec, st),
              "SparseLRPlan: evaluation");
  }

  void ensure_rows_(int64_t B) {
    if (dz_.numel() < B) {
      dz_ = at::empty({std::max<int64_t>(B, 1024)}, W_.options());
      lrow_ = at::empty({std::max<int64_t>(B, 1024)}, W_.options());
    }
  }

 public:
  // device tensors (labels [B] / [B,1] f32, offsets [B+1] i64, ids [nnz] i64, vals [nnz] f32 or None)
  at::Tensor step(at::Tensor labels, at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals, double lr) {
    TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kFloat && labels.is_contiguous(), "labels");
    TORCH_CHECK(offsets.is_cuda() && offsets.scalar_type() == at::kLong && offsets.is_contiguous(), "offsets");
    TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kLong && ids.is_contiguous(), "ids");
    const int64_t B = labels.numel();
    TORCH_CHECK(offsets.numel() == B + 1, "SparseLRPlan.step: offsets must hold B + 1 entries");
    const float* vp = nullptr;
    if (vals.has_value()) {
      TORCH_CHECK(vals->is_cuda() && vals->scalar_type() == at::kFloat && vals->is_contiguous() &&
                      vals->numel() == ids.numel(), "vals");
      vp = vals->data_ptr<float>();
    }
    ensure_rows_(B);
    launch(ids.data_ptr(), false, reinterpret_cast<const long long*>(offsets.data_ptr<int64_t>()), vp,
           labels.data_ptr<float>(), (int)B, (float)lr, cur_stream());
    ++runs_;
    return loss();
  }

  // Forward-only evaluation of a device batch (step's tensors, csr_batch's
  // checks) into `record` (see eval_csr); W, b, the optimizer's slots,
  // global_step, runs() and loss() are not touched.  Capturable in a hipGraph (no
  // host read-back, no memset node): the capture holds the tensors' and the
  // scratch's addresses.
  void evaluate(at::Tensor labels, at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals,
                at::Tensor record, bool reset, c10::optional<at::Tensor> pred, c10::optional<at::Tensor> logits) {
    const int dev = W_.get_device();
    const CsrBatch in = csr_batch("SparseLRPlan.evaluate", dev, labels, offsets, ids, vals);
    const EvalOut o = eval_out("SparseLRPlan", dev, in.B, record, reset, pred, logits);
    esc_.ensure(in.B, W_.options());
    eval_launch_(in.ids, false, in.offsets, in.vals, in.labels, false, (int)in.B, o,
                 cur_stream());
    ++eval_runs_;
  }
  int64_t eval_runs() const { return eval_runs_; }

  at::Tensor loss() const { return loss_.select(0, 0); }   // the last run's mean loss (0-d, device)
  // host time per run() call, us: waiting for the staging slot (the GPU two
  // steps behind), feed packing (CSR build + copies into the pinned slot), then
  // the feed transfer + two launches
  py::dict timing() const {
    py::dict dd;
    const double k = runs_ > 0 ? (double)runs_ : 1.0;
    dd["pack_us"] = t_[0] / k;
    dd["enqueue_us"] = t_[1] / k;
    dd["slot_wait_us"] = t_[2] / k;
    dd["runs"] = runs_;
    dd["feed"] = feed_ == 2 ? "dma" : (feed_ == 1 ? "staging kernel" : (feed_ == 3 ? "overlapped staging" : "direct"));
    return dd;
  }
  int64_t runs() const { return runs_; }
  int64_t bad_ids() const { return bad_.item<int>(); }

 private:
  void launch(const void* ids, bool i32, const long long* offs, const float* vals, const float* labels, int B,
              float lr, hipStream_t st) {
    if (ftrl_) {
      hip_check(dtfk_slr_ftrl_step(W_.data_ptr<float>(), (long long)F_, ids, i32 ? 1 : 0, offs, vals, labels,
                                   bias_.data_ptr<float>(), B, nullptr, lr, dz_.data_ptr<float>(),
                                   lrow_.data_ptr<float>(), loss_.data_ptr<float>(), bad_.data_ptr<int>(), gs_.ptr,
                                   gs_.kind, acc_.data_ptr<float>(), lin_.data_ptr<float>(), gsum_.data_ptr<float>(),
                                   bslots_.data_ptr<float>(), hp_[0], hp_[1], hp_[2], hp_[3], st),
                "SparseLRPlan: FTRL step");
      return;
    }
    hip_check(dtfk_slr_step(W_.data_ptr<float>(), (long long)F_, ids, i32 ? 1 : 0, offs, vals, labels,
                            bias_.data_ptr<float>(), B, nullptr, lr, dz_.data_ptr<float>(), lrow_.data_ptr<float>(),
                            loss_.data_ptr<float>(), bad_.data_ptr<int>(), gs_.ptr, gs_.kind, st),
              "SparseLRPlan: step");
  }

  at::Tensor W_, bias_, gstep_, loss_, bad_, dev_, dz_, lrow_;
  EvalScratch esc_{4};   // the evaluation's per-row scratch
  at::Tensor acc_, lin_, bslots_, gsum_;   // set_ftrl: W's slots, the bias's two, the gradient accumulator
  bool ftrl_ = false;
  float hp_[4] = {-0.5f, 0.f, 0.f, 0.f};   // learning_rate_power, l1, l2, l2_shrinkage
  void* hbuf_[2] = {nullptr, nullptr};
  void* hdev_[2] = {nullptr, nullptr};
  int64_t hcap_[2] = {0, 0};
  int feed_ = 0;   // 0 direct (the forward reads the pinned slot), 1 staging kernel, 2 SDMA copy, 3 staging on a side queue
  hipStream_t side_ = nullptr;
  hipEvent_t evs_[2] = {nullptr, nullptr};
  at::Tensor dev2_[2];
  std::vector<int64_t> cnt_;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  bool pending_[2] = {false, false};
  GstepRef gs_;
  int slot_ = 0;
  int64_t F_ = 0, runs_ = 0, eval_runs_ = 0;
  double t_[3] = {0, 0, 0};
};

void init_sparse(py::module& m) {
  py::class_<SparseLRPlan>(m, "SparseLRPlan")
      .def(py::init<at::Tensor, at::Tensor, c10::optional<at::Tensor>>(), py::arg("W"), py::arg("bias"),
           py::arg("gstep") = py::none())
      .def("run", &SparseLRPlan::run, py::arg("y"), py::arg("indices"), py::arg("ids"), py::arg("vals"), py::arg("lr"))
      .def("run_csr", &SparseLRPlan::run_csr, py::arg("y"), py::arg("offsets"), py::arg("ids"), py::arg("vals"),
           py::arg("lr"))
      .def("step", &SparseLRPlan::step, py::arg("labels"), py::arg("offsets"), py::arg("ids"), py::arg("vals"),
           py::arg("lr"))
      .def("evaluate", &SparseLRPlan::evaluate, py::arg("labels"), py::arg("offsets"), py::arg("ids"), py::arg("vals"),
           py::arg("record"), py::arg("reset"), py::arg("pred") = py::none(), py::arg("logits") = py::none())
      .def("eval_csr", &SparseLRPlan::eval_csr, py::arg("y"), py::arg("offsets"), py::arg("ids"), py::arg("vals"),
           py::arg("record"), py::arg("reset"), py::arg("pred") = py::none(), py::arg("logits") = py::none())
      .def("eval_coo", &SparseLRPlan::eval_coo, py::arg("y"), py::arg("indices"), py::arg("ids"), py::arg("vals"),
           py::arg("record"), py::arg("reset"), py::arg("pred") = py::none(), py::arg("logits") = py::none())
      .def("eval_runs", &SparseLRPlan::eval_runs)
      .def("set_ftrl", &SparseLRPlan::set_ftrl, py::arg("accum"), py::arg("linear"), py::arg("bias_slots"),
           py::arg("lr_power") = -0.5, py::arg("l1") = 0.0, py::arg("l2") = 0.0, py::arg("l2_shrinkage") = 0.0)
      .def("ftrl", &SparseLRPlan::ftrl)
      .def("grad_accumulator", &SparseLRPlan::grad_accumulator)
      .def("loss", &SparseLRPlan::loss)
      .def("runs", &SparseLRPlan::runs)
      .def("timing", &SparseLRPlan::timing)
      .def("bad_ids", &SparseLRPlan::bad_ids);
}

}  // namespace dtf
