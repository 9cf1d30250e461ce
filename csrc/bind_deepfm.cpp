// One-GPU DeepFM as host calls (csrc/kernels/deepfm.hip, deepfm_fields.hip).
// DeepFMPlan holds the model's tensors themselves, not copies: w [F], V [F, K], the
// tower's layers [W_0, b_0, ..., w_last, b_last] and the bias.  A training step is
// rows() (dfm_rows<TM, true>: z, loss, dz, act, dzl, demb), sums()
// (wide_deep_train.hip's fixed-order reduce) and update() (fm.hip's one-writer table
// update with this plan's dz and demb); the tower's weight gradients are the caller's
// gemm / col_sum launches over act() and dzl().  An evaluation is dfm_rows<TM, false>
// plus eval_record.hip's reduce.  Every refusal raises before anything is launched; no
// host read-back and no memset node, so a step can be captured in a hipGraph.
//
// Two forms.  num_fields = 0: CSR rows (offsets [B + 1]), the tower reads the pooled
// factors S_r, K wide.  num_fields = P >= 1: (row, field) bags (offsets [B P + 1]), the
// tower reads the concatenation of the P per-field sums, P K wide (dfmf_rows); demb is
// [B, P K], which update() hands to the same table update as [B P, K] over B P bags,
// with dz once per bag.
//
// Scratch (step_scratch.h), one tensor of `capacity` rows per part, grown only when
// a batch exceeds it and never inside a stream capture (an outgrown tensor is kept
// alive for the graphs that hold it):
//   rows:   act[0 .. nl-1] [cap, dims[l]] | dzl[1 .. nl-1] [cap, dims[l]] | demb [cap, dims[0]] | dz | lrow | brow (int) | z [cap]
//           with fields also: S [cap, K] | dz per bag [cap, P]
//   update: bag_of [ids cap] (int) | part (table_update.h)
// An evaluation has per-row arrays of its own (EvalScratch: lrow | prow | brow).
#include "bind_common.h"
#include "eval_record_host.h"
#include "kernels/deepfm.h"
#include "kernels/deepfm_fields.h"
#include "kernels/fm.h"
#include "step_scratch.h"
#include "table_update_host.h"

#include <algorithm>
#include <vector>

namespace dtf {

class DeepFMPlan {
 public:
  DeepFMPlan(at::Tensor w, at::Tensor V, std::vector<at::Tensor> layers, at::Tensor bias, int64_t num_fields)
      : w_(w), V_(V), bias_(bias), layers_(std::move(layers)), P_(num_fields) {
    const char* who = "DeepFMPlan";
    TORCH_CHECK(V.is_cuda() && V.scalar_type() == at::kFloat && V.is_contiguous() && V.dim() == 2, who,
                ": V must be a contiguous fp32 [F, K] GPU table");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(V.data_ptr()) & 15) == 0, who, ": V must be 16-byte aligned");
    const int dev = V.get_device();
    F_ = V.size(0);
    const int64_t K = V.size(1);
    TORCH_CHECK(on_device(w, dev, at::kFloat) && w.numel() == F_, who, ": w must be a contiguous fp32 [F] GPU table on V's device");
    TORCH_CHECK(on_device(bias, dev, at::kFloat) && bias.numel() == 1, who, ": bias must be one fp32 GPU value");
    TORCH_CHECK(F_ >= 1 && K <= dtfk::wde::MAXD && layers_.size() % 2 == 0 && layers_.size() >= 4 &&
                    layers_.size() <= 2 * dtfk::wde::MAXL,
                who, ": unsupported shape (K up to 128; 1 to 3 hidden layers and the last one, as [W, b] pairs)");
    TORCH_CHECK(P_ >= 0 && P_ <= dtfk::dfmf::MAXP && P_ * K <= dtfk::wde::MAXW, who,
                ": unsupported shape (at most 64 fields, num_fields * K <= 512)");
    nl_ = (int)layers_.size() / 2;
    K_ = (int)K;
    int64_t k = P_ > 0 ? P_ * K : K;                                // the tower's input: the concatenation / S
    dims_[0] = (int)k;
    for (int l = 0; l < nl_; ++l) {
      const at::Tensor& W = layers_[2 * l];
      const at::Tensor& b = layers_[2 * l + 1];
      TORCH_CHECK(on_device(W, dev, at::kFloat) && W.dim() == 2 && W.size(0) == k && on_device(b, dev, at::kFloat) &&
                      b.numel() == W.size(1),
                  who, ": layers must be contiguous fp32 GPU [K, N] weights and [N] biases in a chain");
      k = W.size(1);
      TORCH_CHECK(k <= dtfk::wde::MAXW, who, ": unsupported shape (hidden width above 512)");
      dims_[l + 1] = (int)k;
      if (l < nl_ - 1)
        TORCH_CHECK(((reinterpret_cast<uintptr_t>(W.data_ptr()) | reinterpret_cast<uintptr_t>(b.data_ptr())) & 15) == 0,
                    who, ": unsupported shape (tower tensors must be 16-byte aligned)");
    }
    TORCH_CHECK((P_ > 0 ? dtfk_dfmf_supported((int)P_, K_, nl_, dims_) : dtfk_dfm_supported(K_, nl_, dims_)) == 1, who,
                ": unsupported shape (K a multiple of 4 in 4 .. 128; 1 to 3 hidden widths, multiples of 16 up to 512; "
                "last width 1)");
    std::vector<int> widths(dims_, dims_ + nl_);                    // act
    widths.insert(widths.end(), dims_ + 1, dims_ + nl_);            // dzl
    widths.insert(widths.end(), {dims_[0], 1, 1, 1, 1});            // demb, dz, lrow, brow, z
    if (P_ > 0) widths.insert(widths.end(), {K_, (int)P_});         // S, dz per bag
    scratch_.init(who, std::move(widths), K_, false);
    sums_ = at::zeros({1}, V.options());
  }

  static bool supported(int64_t K, const std::vector<int64_t>& hidden, int64_t num_fields) {
    if (K < 1 || K > dtfk::wde::MAXD || hidden.empty() || (int)hidden.size() > dtfk::wde::MAXL - 1) return false;
    if (num_fields < 0 || num_fields > dtfk::dfmf::MAXP) return false;
    int dims[dtfk::wde::MAXL + 1];
    dims[0] = (int)(num_fields > 0 ? num_fields * K : K);
    for (size_t l = 0; l < hidden.size(); ++l) {
      if (hidden[l] < 1 || hidden[l] > dtfk::wde::MAXW) return false;
      dims[l + 1] = (int)hidden[l];
    }
    dims[hidden.size() + 1] = 1;
    const int nl = (int)hidden.size() + 1;
    return (num_fields > 0 ? dtfk_dfmf_supported((int)num_fields, (int)K, nl, dims) : dtfk_dfm_supported((int)K, nl, dims)) == 1;
  }

  // ids > 0 also sizes update()'s scratch
  void reserve(int64_t B, int64_t ids) { scratch_.reserve(B, ids, V_.options()); }

  // dfm_rows<TM, true> (with fields: dfmf_rows<TM, true>) on the current stream for one CSR / bag batch of
  // device tensors; gscale: the loss's scale per row (1 / B for a batch mean).
  void rows(at::Tensor labels, at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals, double gscale) {
    const CsrBatch in = batch("DeepFMPlan.rows", labels, offsets, ids, vals);
    reserve(in.B, 0);
    dtfk::wdt::Args a{};
    a.f = forward_args(in);
    for (int l = 0; l < nl_; ++l) a.act[l] = part(l);
    for (int l = 1; l < nl_; ++l) a.dzl[l] = part(nl_ + l - 1);
    a.demb = part(2 * nl_ - 1);
    a.dz = part(2 * nl_);
    a.f.lrow = part(2 * nl_ + 1);
    a.f.brow = reinterpret_cast<int*>(part(2 * nl_ + 2));
    a.f.z_out = part(2 * nl_ + 3);
    a.gscale = (float)gscale;
    hip_check(launch_rows(a, 1, cur_stream()), "DeepFMPlan: rows kernel");
    B_ = in.B;
    ++runs_;
  }

  // mean(lrow) of the last batch (a view of one persistent value), and sum(dz) into db_last /
  // dbias (one fp32 value each): one small kernel, float64 sums in a fixed order.
  at::Tensor sums(at::Tensor db_last, at::Tensor dbias) {
    TORCH_CHECK(B_ > 0, "DeepFMPlan.sums: no batch yet");
    const int dev = V_.get_device();
    TORCH_CHECK(on_device(db_last, dev, at::kFloat) && db_last.numel() == 1 && on_device(dbias, dev, at::kFloat) &&
                    dbias.numel() == 1,
                "DeepFMPlan.sums: db_last / dbias must be one fp32 value each on the plan's GPU");
    hip_check(dtfk_wd_train_sums(part(2 * nl_ + 1), part(2 * nl_), (int)B_, sums_.data_ptr<float>(),
                                 db_last.data_ptr<float>(), dbias.data_ptr<float>(), cur_stream()),
              "DeepFMPlan: sums kernel");
    return sums_.select(0, 0);
  }

  // The tables' half of the step, after rows(): FMPlan.update's, with this plan's dz and demb = dz S + da_0;
  // with fields over the B P bags: dz per bag and demb [B, P K] read as [B P, K].
  void update(at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals, int kind, double lr,
              std::vector<at::Tensor> w_slots, std::vector<at::Tensor> V_slots, const py::kwargs& hyper) {
    TORCH_CHECK(B_ > 0, "DeepFMPlan.update: no batch yet (rows() first)");
    if (table_update_host("DeepFMPlan.update", dtfk_fm_update, w_, V_, P_ > 0 ? B_ * P_ : B_, offsets, ids, vals, kind,
                          lr, w_slots, V_slots, c10::nullopt, hyper, part(P_ > 0 ? 2 * nl_ + 5 : 2 * nl_),
                          part(2 * nl_ - 1), [&](int64_t N, hipStream_t) {
                            reserve(B_, N);
                            return UpdateScratch{scratch_.bag_of(), scratch_.update_part(), nullptr};
                          }))
      ++updates_;
  }

  // dfm_rows<TM, false> (with fields: dfmf_rows<TM, false>) and the record's reduce: the batch into `record` (reset starts it
  // over, else the batch is added).  Returns the probabilities [B] when asked for.
  // T: the record's thresholds, checked against its length (0: taken from it).
  c10::optional<at::Tensor> evaluate(at::Tensor labels, at::Tensor offsets, at::Tensor ids,
                                     c10::optional<at::Tensor> vals, at::Tensor record, bool reset, bool want_pred,
                                     int T) {
    const int dev = V_.get_device();
    const CsrBatch in = batch("DeepFMPlan.evaluate", labels, offsets, ids, vals);
    c10::optional<at::Tensor> pred;
    if (want_pred) pred = at::empty({in.B}, V_.options());
    const EvalOut o = eval_out("DeepFMPlan", dev, in.B, record, reset, pred, c10::nullopt);
    TORCH_CHECK(T == 0 || T == o.T, "DeepFMPlan.evaluate: T does not match the record's length");
    eval_.ensure(in.B, V_.options());
    dtfk::wdt::Args a{};
    a.f = forward_args(in);
    a.f.lrow = eval_.part(0);
    a.f.prow = eval_.part(1);
    a.f.brow = reinterpret_cast<int*>(eval_.part(2));
    a.f.p_out = o.pred;
    hipStream_t st = cur_stream();
    hip_check(launch_rows(a, 0, st), "DeepFMPlan: rows kernel");
    hip_check(dtfk_eval_reduce(a.f.lrow, a.f.prow, a.f.brow, a.f.labels, a.f.B, o.T, o.reset, o.rec, st),
              "DeepFMPlan: reduce kernel");
    ++eval_runs_;
    return pred;
  }

  at::Tensor act(int l) const { return checked(l, 0, "act"), view(l); }
  at::Tensor dzl(int l) const { return checked(l, 1, "dzl"), view(nl_ + l - 1); }
  at::Tensor demb() const { return view(2 * nl_ - 1); }
  at::Tensor dz() const { return view(2 * nl_); }
  at::Tensor lrow() const { return view(2 * nl_ + 1).reshape({B_}); }
  at::Tensor brow() const { return view(2 * nl_ + 2).reshape({B_}).view(at::kInt); }
  at::Tensor z() const { return view(2 * nl_ + 3).reshape({B_}); }
  at::Tensor scratch() const { return scratch_.rows(); }
  int64_t row_floats() const { return scratch_.row_floats(); }
  int64_t runs() const { return runs_; }
  int64_t updates() const { return updates_; }
  int64_t eval_runs() const { return eval_runs_; }
  // 16 / 32 force the row tile, 0 (the default) picks it by the batch size
  void set_tile(int tile) {
    TORCH_CHECK(tile == 0 || tile == 16 || tile == 32, "DeepFMPlan.set_tile: 0, 16 or 32");
    tile_ = tile;
  }
  int tile_for(int64_t B) const {
    return tile_ != 0 ? tile_ : dtfk_dfm_tile((int)std::min<int64_t>(B, 1 << 30), nl_, dims_);
  }
  int64_t lds_bytes(int tile) const {
    return P_ > 0 ? dtfk_dfmf_lds_bytes((int)P_, K_, nl_, dims_, tile) : dtfk_dfm_lds_bytes(K_, nl_, dims_, tile);
  }

 private:
  void checked(int l, int lo, const char* what) const {
    TORCH_CHECK(l >= lo && l < nl_, "DeepFMPlan.", what, ": layer out of range");
  }
  // part k of the row scratch, in the order of the list above; view: the last batch's rows of it, [B, width]
  float* part(int k) const { return scratch_.part(k); }
  at::Tensor view(int k) const { return scratch_.view(k, B_); }
  // A checked batch: CSR rows (eval_record_host.h's csr_batch) or, with fields, the bag form: the same tensors
  // with offsets [B P + 1], one bag per (row, field), B P < 2^31.
  CsrBatch batch(const char* who, const at::Tensor& labels, const at::Tensor& offsets, const at::Tensor& ids,
                 const c10::optional<at::Tensor>& vals) const {
    const int dev = V_.get_device();
    if (P_ == 0) return csr_batch(who, dev, labels, offsets, ids, vals);
    TORCH_CHECK(on_device(labels, dev, at::kFloat), who, ": labels must be contiguous fp32 on the plan's GPU");
    TORCH_CHECK(on_device(offsets, dev, at::kLong), who, ": offsets must be contiguous int64 on the plan's GPU");
    TORCH_CHECK(on_device(ids, dev, at::kLong), who, ": ids must be contiguous int64 on the plan's GPU");
    const int64_t B = labels.numel();
    TORCH_CHECK(B >= 1 && B * P_ < (1ll << 31), who, ": 1 <= B and B * num_fields < 2^31");
    TORCH_CHECK(offsets.numel() == B * P_ + 1, who, ": offsets must hold B * num_fields + 1 entries, one bag per (row, field)");
    TORCH_CHECK(!vals.has_value() || (on_device(*vals, dev, at::kFloat) && vals->numel() == ids.numel()), who,
                ": vals must be contiguous fp32 on the plan's GPU, one per id");
    return {labels.data_ptr<float>(), reinterpret_cast<const long long*>(offsets.data_ptr<int64_t>()),
            reinterpret_cast<const long long*>(ids.data_ptr<int64_t>()), opt_ptr<float>(vals), B};
  }
  // the form's rows kernel; training: S and dz per bag are the scratch's last two parts
  hipError_t launch_rows(const dtfk::wdt::Args& a, int train, hipStream_t st) const {
    if (P_ == 0) return dtfk_dfm_rows(&a, train, tile_, st);
    dtfk::dfmf::Args fa{};
    fa.t = a;
    fa.P = (int)P_;
    if (train) {
      fa.S = part(2 * nl_ + 4);
      fa.dzbag = part(2 * nl_ + 5);
    }
    return dtfk_dfmf_rows(&fa, train, tile_, st);
  }
  // the kernel's view of the tensors and a checked batch (outputs left null)
  dtfk::wde::Args forward_args(const CsrBatch& in) const {
    dtfk::wde::Args a{};
    a.Wt = w_.data_ptr<float>();
    a.E = V_.data_ptr<float>();
    a.F = (long long)F_;
    a.D = K_;
    a.mode = 0;                                 // sum: the factors are pooled without a scale
    a.ids = in.ids;
    a.offsets = in.offsets;
    a.vals = in.vals;
    a.labels = in.labels;
    for (int l = 0; l < nl_; ++l) {
      a.W[l] = layers_[2 * l].data_ptr<float>();
      a.b[l] = layers_[2 * l + 1].data_ptr<float>();
    }
    for (int l = 0; l <= nl_; ++l) a.dims[l] = dims_[l];
    a.nl = nl_;
    a.bias = bias_.data_ptr<float>();
    a.B = (int)in.B;
    return a;
  }

  at::Tensor w_, V_, bias_, sums_;
  std::vector<at::Tensor> layers_;
  StepScratch scratch_;
  EvalScratch eval_{3};
  int dims_[dtfk::wde::MAXL + 1] = {0, 0, 0, 0, 0};
  int nl_ = 0, tile_ = 0, K_ = 0;
  int64_t P_ = 0, F_ = 0, B_ = 0;
  int64_t runs_ = 0, updates_ = 0, eval_runs_ = 0;
};

void init_deepfm(py::module& m) {
  py::class_<DeepFMPlan>(m, "DeepFMPlan")
      .def(py::init<at::Tensor, at::Tensor, std::vector<at::Tensor>, at::Tensor, int64_t>(), py::arg("w"), py::arg("V"),
           py::arg("layers"), py::arg("bias"), py::arg("num_fields") = 0)
      .def_static("supported", &DeepFMPlan::supported, py::arg("K"), py::arg("hidden"), py::arg("num_fields") = 0)
      .def("reserve", &DeepFMPlan::reserve, py::arg("rows"), py::arg("ids") = 0)
      .def("rows", &DeepFMPlan::rows, py::arg("labels"), py::arg("offsets"), py::arg("ids"), py::arg("vals"),
           py::arg("gscale"))
      .def("sums", &DeepFMPlan::sums, py::arg("db_last"), py::arg("dbias"))
      .def("update", &DeepFMPlan::update, py::arg("offsets"), py::arg("ids"), py::arg("vals"), py::arg("kind"),
           py::arg("lr"), py::arg("w_slots"), py::arg("V_slots"))
      .def("evaluate", &DeepFMPlan::evaluate, py::arg("labels"), py::arg("offsets"), py::arg("ids"), py::arg("vals"),
           py::arg("record"), py::arg("reset"), py::arg("want_pred") = false, py::arg("T") = 0)
      .def("act", &DeepFMPlan::act, py::arg("layer"))
      .def("dzl", &DeepFMPlan::dzl, py::arg("layer"))
      .def("demb", &DeepFMPlan::demb)
      .def("dz", &DeepFMPlan::dz)
      .def("z", &DeepFMPlan::z)
      .def("lrow", &DeepFMPlan::lrow)
      .def("brow", &DeepFMPlan::brow)
      .def("scratch", &DeepFMPlan::scratch)
      .def("row_floats", &DeepFMPlan::row_floats)
      .def("runs", &DeepFMPlan::runs)
      .def("updates", &DeepFMPlan::updates)
      .def("eval_runs", &DeepFMPlan::eval_runs)
      .def("set_tile", &DeepFMPlan::set_tile, py::arg("tile"))
      .def("tile_for", &DeepFMPlan::tile_for, py::arg("rows"))
      .def("lds_bytes", &DeepFMPlan::lds_bytes, py::arg("tile"));
}

}  // namespace dtf
