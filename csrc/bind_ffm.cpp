// The one-GPU field-aware factorization machine as host calls (csrc/kernels/ffm.hip).
// FFMPlan holds the model's tensors themselves, not copies.  A batch is a CSR over
// (row, field) bags: labels [B], offsets [B P + 1], ids, vals.  A training step is
// rows() (ffm_rows<true>: z, loss, dz per row; dz and the gradient G per bag), sums()
// (wide_deep_train.hip's fixed-order reduce: mean loss and sum(dz)) and update() (the
// one-writer update of table_update_host.h as it stands, over the B P bags of width
// P K, in the plain form dtfk_wd_update: no scale, no skip); an evaluation is
// ffm_rows<false> plus eval_record.hip's reduce.  Every refusal raises before anything
// is launched; no host read-back and no memset node, so a step can be captured in a
// hipGraph.
//
// Scratch (step_scratch.h), grown only when a batch exceeds it and never inside a
// stream capture:
//   rows:   G [cap, P P K] | dz per bag [cap, P] | dz | lrow | brow (int) | z [cap]
//   update: bag_of [ids cap] (int) | part (table_update.h)
// An evaluation has per-row arrays of its own (EvalScratch: lrow | prow | brow).
#include "bind_common.h"
#include "eval_record_host.h"
#include "kernels/ffm.h"
#include "kernels/wide_deep_train.h"
#include "kernels/wide_deep_update.h"
#include "step_scratch.h"
#include "table_update_host.h"

#include <vector>

namespace dtf {

class FFMPlan {
 public:
  FFMPlan(at::Tensor w, at::Tensor V, at::Tensor bias, int64_t num_fields) : w_(w), V_(V), bias_(bias), P_(num_fields) {
    const char* who = "FFMPlan";
    TORCH_CHECK(V.is_cuda() && V.scalar_type() == at::kFloat && V.is_contiguous() && V.dim() == 2, who,
                ": V must be a contiguous fp32 [F, P * K] GPU table");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(V.data_ptr()) & 15) == 0, who, ": V must be 16-byte aligned");
    const int dev = V.get_device();
    F_ = V.size(0);
    TORCH_CHECK(P_ >= 1 && V.size(1) % P_ == 0, who, ": V's width must be num_fields * K");
    K_ = V.size(1) / P_;
    TORCH_CHECK(F_ >= 1 && supported(P_, K_), who,
                ": unsupported shape (K a multiple of 4, 2 <= num_fields <= 32, num_fields * K <= 128)");
    TORCH_CHECK(on_device(w, dev, at::kFloat) && w.numel() == F_, who, ": w must be a contiguous fp32 [F] GPU table on V's device");
    TORCH_CHECK(on_device(bias, dev, at::kFloat) && bias.numel() == 1, who, ": bias must be one fp32 GPU value");
    sums_ = at::zeros({2}, V.options());
    scratch_.init(who, {(int)(P_ * P_ * K_), (int)P_, 1, 1, 1, 1}, (int)(P_ * K_), false);
  }

  static bool supported(int64_t P, int64_t K) {
    return P >= 0 && P <= 1024 && K >= 0 && K <= 1024 && dtfk_ffm_supported((int)P, (int)K) == 1;
  }

  // ids > 0 also sizes update()'s scratch
  void reserve(int64_t B, int64_t ids) { scratch_.reserve(B, ids, V_.options()); }

  // ffm_rows<true> on the current stream for one bag batch of device tensors;
  // gscale: the loss's scale per row (1 / B for a batch mean).
  void rows(at::Tensor labels, at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals, double gscale) {
    dtfk::ffm::RowArgs a = batch_args("FFMPlan.rows", labels, offsets, ids, vals);
    reserve(a.B, 0);
    a.G = part(0);
    a.dzbag = part(1);
    a.dz = part(2);
    a.lrow = part(3);
    a.brow = reinterpret_cast<int*>(part(4));
    a.z_out = part(5);
    a.gscale = (float)gscale;
    hip_check(dtfk_ffm_rows(&a, 1, cur_stream()), "FFMPlan: rows kernel");
    B_ = a.B;
    ++runs_;
  }

  // (mean(lrow), sum(dz)) of the last batch: views of one persistent tensor, float64 sums in a fixed order
  std::pair<at::Tensor, at::Tensor> sums() {
    TORCH_CHECK(B_ > 0, "FFMPlan.sums: no batch yet");
    float* s = sums_.data_ptr<float>();
    hip_check(dtfk_wd_train_sums(part(3), part(2), (int)B_, s, s + 1, nullptr, cur_stream()), "FFMPlan: sums kernel");
    return {sums_.select(0, 0), sums_.narrow(0, 1, 1)};
  }

  // The tables' half of the step, after rows(): w, V and their slots take rule `kind`
  // (optim_rules.h OptimKind, row-local kinds) with the last batch's per-bag dz and G:
  // duplicates summed, every touched row written once.  offsets / ids / vals: the
  // batch rows() saw; *_slots: slot a, slot b as the kind has them; hyper:
  // Rule.native_kwargs.
  void update(at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals, int kind, double lr,
              std::vector<at::Tensor> w_slots, std::vector<at::Tensor> V_slots, const py::kwargs& hyper) {
    TORCH_CHECK(B_ > 0, "FFMPlan.update: no batch yet (rows() first)");
    if (table_update_host("FFMPlan.update", dtfk_wd_update, w_, V_, B_ * P_, offsets, ids, vals, kind, lr, w_slots,
                          V_slots, c10::nullopt, hyper, part(1), part(0), [&](int64_t N, hipStream_t) {
                            reserve(B_, N);
                            return UpdateScratch{scratch_.bag_of(), scratch_.update_part(), nullptr};
                          }))
      ++updates_;
  }

  // ffm_rows<false> and the record's reduce: the batch into `record` (reset starts it
  // over, else the batch is added).  Returns the probabilities [B] when asked for.
  // T: the record's thresholds, checked against its length (0: taken from it).
  c10::optional<at::Tensor> evaluate(at::Tensor labels, at::Tensor offsets, at::Tensor ids,
                                     c10::optional<at::Tensor> vals, at::Tensor record, bool reset, bool want_pred,
                                     int T) {
    dtfk::ffm::RowArgs a = batch_args("FFMPlan.evaluate", labels, offsets, ids, vals);
    c10::optional<at::Tensor> pred;
    if (want_pred) pred = at::empty({a.B}, V_.options());
    const EvalOut o = eval_out("FFMPlan", V_.get_device(), a.B, record, reset, pred, c10::nullopt);
    TORCH_CHECK(T == 0 || T == o.T, "FFMPlan.evaluate: T does not match the record's length");
    eval_.ensure(a.B, V_.options());
    a.lrow = eval_.part(0);
    a.prow = eval_.part(1);
    a.brow = reinterpret_cast<int*>(eval_.part(2));
    a.p_out = o.pred;
    hipStream_t st = cur_stream();
    hip_check(dtfk_ffm_rows(&a, 0, st), "FFMPlan: rows kernel");
    hip_check(dtfk_eval_reduce(a.lrow, a.prow, a.brow, a.labels, a.B, o.T, o.reset, o.rec, st), "FFMPlan: reduce kernel");
    ++eval_runs_;
    return pred;
  }

  at::Tensor demb() const { return view(0).reshape({B_ * P_, P_ * K_}); }
  at::Tensor dz_bag() const { return view(1).reshape({B_ * P_}); }
  at::Tensor dz() const { return view(2).reshape({B_}); }
  at::Tensor lrow() const { return view(3).reshape({B_}); }
  at::Tensor brow() const { return view(4).reshape({B_}).view(at::kInt); }
  at::Tensor z() const { return view(5).reshape({B_}); }
  int64_t runs() const { return runs_; }
  int64_t updates() const { return updates_; }
  int64_t eval_runs() const { return eval_runs_; }
  // (LDS bytes of a row's tile, waves per workgroup) of ffm_rows for this shape
  std::pair<int, int> tile() const {
    int waves = 0;
    const int bytes = dtfk_ffm_tile_bytes((int)P_, (int)K_, &waves);
    return {bytes, waves};
  }

 private:
  // part k of the row scratch: G, dz per bag, dz, lrow, brow, z
  float* part(int k) const { return scratch_.part(k); }
  at::Tensor view(int k) const { return scratch_.view(k, B_); }

  // The bag form of a batch: labels [B] / [B, 1] f32, offsets [B P + 1] i64, ids [nnz] i64, vals [nnz] f32 or None,
  // contiguous on the plan's GPU, 1 <= B and B P < 2^31.  (eval_record_host.h's csr_batch is the [B + 1] form.)
  dtfk::ffm::RowArgs batch_args(const char* who, const at::Tensor& labels, const at::Tensor& offsets,
                                const at::Tensor& ids, const c10::optional<at::Tensor>& vals) const {
    const int dev = V_.get_device();
    TORCH_CHECK(on_device(labels, dev, at::kFloat), who, ": labels must be contiguous fp32 on the plan's GPU");
    TORCH_CHECK(on_device(offsets, dev, at::kLong), who, ": offsets must be contiguous int64 on the plan's GPU");
    TORCH_CHECK(on_device(ids, dev, at::kLong), who, ": ids must be contiguous int64 on the plan's GPU");
    const int64_t B = labels.numel();
    TORCH_CHECK(B >= 1 && B * P_ < (1ll << 31), who, ": 1 <= B and B * num_fields < 2^31");
    TORCH_CHECK(offsets.numel() == B * P_ + 1, who, ": offsets must hold B * num_fields + 1 entries, one bag per (row, field)");
    TORCH_CHECK(!vals.has_value() || (on_device(*vals, dev, at::kFloat) && vals->numel() == ids.numel()), who,
                ": vals must be contiguous fp32 on the plan's GPU, one per id");
    dtfk::ffm::RowArgs a{};
    a.w = w_.data_ptr<float>();
    a.V = V_.data_ptr<float>();
    a.bias = bias_.data_ptr<float>();
    a.F = F_;
    a.P = (int)P_;
    a.K = (int)K_;
    a.B = (int)B;
    a.ids = reinterpret_cast<const long long*>(ids.data_ptr<int64_t>());
    a.offsets = reinterpret_cast<const long long*>(offsets.data_ptr<int64_t>());
    a.vals = opt_ptr<float>(vals);
    a.labels = labels.data_ptr<float>();
    return a;
  }

  at::Tensor w_, V_, bias_, sums_;
  StepScratch scratch_;
  EvalScratch eval_{3};
  int64_t F_ = 0, P_ = 0, K_ = 0, B_ = 0;
  int64_t runs_ = 0, updates_ = 0, eval_runs_ = 0;
};

void init_ffm(py::module& m) {
  py::class_<FFMPlan>(m, "FFMPlan")
      .def(py::init<at::Tensor, at::Tensor, at::Tensor, int64_t>(), py::arg("w"), py::arg("V"), py::arg("bias"),
           py::arg("num_fields"))
      .def_static("supported", &FFMPlan::supported, py::arg("P"), py::arg("K"))
      .def("reserve", &FFMPlan::reserve, py::arg("rows"), py::arg("ids") = 0)
      .def("rows", &FFMPlan::rows, py::arg("labels"), py::arg("offsets"), py::arg("ids"), py::arg("vals"),
           py::arg("gscale"))
      .def("sums", &FFMPlan::sums)
      .def("update", &FFMPlan::update, py::arg("offsets"), py::arg("ids"), py::arg("vals"), py::arg("kind"),
           py::arg("lr"), py::arg("w_slots"), py::arg("V_slots"))
      .def("evaluate", &FFMPlan::evaluate, py::arg("labels"), py::arg("offsets"), py::arg("ids"), py::arg("vals"),
           py::arg("record"), py::arg("reset"), py::arg("want_pred") = false, py::arg("T") = 0)
      .def("eval_runs", &FFMPlan::eval_runs)
      .def("runs", &FFMPlan::runs)
      .def("updates", &FFMPlan::updates)
      .def("tile", &FFMPlan::tile)
      .def("dz", &FFMPlan::dz)
      .def("dz_bag", &FFMPlan::dz_bag)
      .def("demb", &FFMPlan::demb)
      .def("z", &FFMPlan::z)
      .def("lrow", &FFMPlan::lrow)
      .def("brow", &FFMPlan::brow);
}

}  // namespace dtf
