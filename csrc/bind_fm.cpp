// The one-GPU factorization machine as host calls (csrc/kernels/fm.hip).  FMPlan
// holds the model's tensors themselves, not copies.  A training step is rows()
// (fm_rows<true>: z, loss, dz, demb per row), sums() (wide_deep_train.hip's
// fixed-order reduce: mean loss and sum(dz)) and update() (one stable sort, then
// fm_update_runs + fm_update_carry); an evaluation is fm_rows<false> plus
// eval_record.hip's reduce.  Every refusal raises before anything is launched; no
// host read-back and no memset node, so a step can be captured in a hipGraph.
//
// Scratch (step_scratch.h), one tensor of `capacity` rows per part, grown only when
// a batch exceeds it and never inside a stream capture (an outgrown tensor is kept
// alive for the graphs that hold it):
//   rows:   demb [cap, K] | dz | lrow | brow (int) | z [cap]
//   update: bag_of [ids cap] (int) | part (table_update.h)
// An evaluation has per-row arrays of its own (EvalScratch: lrow | prow | brow), so it never disturbs the
// training step's rows between rows() and update().
#include "bind_common.h"
#include "eval_record_host.h"
#include "kernels/fm.h"
#include "step_scratch.h"
#include "table_update_host.h"
#include "kernels/wide_deep_train.h"

#include <algorithm>
#include <vector>

namespace dtf {

class FMPlan {
 public:
  FMPlan(at::Tensor w, at::Tensor V, at::Tensor bias) : w_(w), V_(V), bias_(bias) {
    const char* who = "FMPlan";
    TORCH_CHECK(V.is_cuda() && V.scalar_type() == at::kFloat && V.is_contiguous() && V.dim() == 2, who,
                ": V must be a contiguous fp32 [F, K] GPU table");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(V.data_ptr()) & 15) == 0, who, ": V must be 16-byte aligned");
    const int dev = V.get_device();
    F_ = V.size(0);
    K_ = V.size(1);
    TORCH_CHECK(F_ >= 1 && supported(K_), who, ": unsupported shape (K a multiple of 4 in 4 .. 128)");
    TORCH_CHECK(on_device(w, dev, at::kFloat) && w.numel() == F_, who, ": w must be a contiguous fp32 [F] GPU table on V's device");
    TORCH_CHECK(on_device(bias, dev, at::kFloat) && bias.numel() == 1, who, ": bias must be one fp32 GPU value");
    sums_ = at::zeros({2}, V.options());
    scratch_.init(who, {(int)K_, 1, 1, 1, 1}, (int)K_, false);
  }

  static bool supported(int64_t K) { return K >= 0 && K <= (1 << 20) && dtfk_fm_supported((int)K) == 1; }

  // ids > 0 also sizes update()'s scratch
  void reserve(int64_t B, int64_t ids) { scratch_.reserve(B, ids, V_.options()); }

  // fm_rows<true> on the current stream for one CSR batch of device tensors;
  // gscale: the loss's scale per row (1 / B for a batch mean).
  void rows(at::Tensor labels, at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals, double gscale) {
    const CsrBatch in = csr_batch("FMPlan.rows", V_.get_device(), labels, offsets, ids, vals);
    reserve(in.B, 0);
    dtfk::fm::RowArgs a = row_args(in);
    a.dz = part(1);
    a.demb = part(0);
    a.z_out = part(4);
    a.gscale = (float)gscale;
    hip_check(dtfk_fm_rows(&a, 1, rpw_, cur_stream()), "FMPlan: rows kernel");
    B_ = in.B;
    ++runs_;
  }

  // (mean(lrow), sum(dz)) of the last batch: views of one persistent tensor, float64 sums in a fixed order
  std::pair<at::Tensor, at::Tensor> sums() {
    TORCH_CHECK(B_ > 0, "FMPlan.sums: no batch yet");
    float* s = sums_.data_ptr<float>();
    hip_check(dtfk_wd_train_sums(part(2), part(1), (int)B_, s, s + 1, nullptr, cur_stream()), "FMPlan: sums kernel");
    return {sums_.select(0, 0), sums_.narrow(0, 1, 1)};
  }

  // The tables' half of the step, after rows(): w, V and their slots take rule
  // `kind` (optim_rules.h OptimKind, row-local kinds) with the last batch's dz /
  // demb: duplicates summed, every touched row written once.  offsets / ids / vals:
  // the batch rows() saw; *_slots: slot a, slot b as the kind has them; hyper:
  // Rule.native_kwargs.
  void update(at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals, int kind, double lr,
              std::vector<at::Tensor> w_slots, std::vector<at::Tensor> V_slots, const py::kwargs& hyper) {
    TORCH_CHECK(B_ > 0, "FMPlan.update: no batch yet (rows() first)");
    if (table_update_host("FMPlan.update", dtfk_fm_update, w_, V_, B_, offsets, ids, vals, kind, lr, w_slots, V_slots,
                          c10::nullopt, hyper, part(1), part(0), [&](int64_t N, hipStream_t) {
                            reserve(B_, N);
                            return UpdateScratch{scratch_.bag_of(), scratch_.update_part(), nullptr};
                          }))
      ++updates_;
  }

  // fm_rows<false> and the record's reduce: the batch into `record` (reset starts it
  // over, else the batch is added).  Returns the probabilities [B] when asked for.
  // T: the record's thresholds, checked against its length (0: taken from it).
  c10::optional<at::Tensor> evaluate(at::Tensor labels, at::Tensor offsets, at::Tensor ids,
                                     c10::optional<at::Tensor> vals, at::Tensor record, bool reset, bool want_pred,
                                     int T) {
    const int dev = V_.get_device();
    const CsrBatch in = csr_batch("FMPlan.evaluate", dev, labels, offsets, ids, vals);
    c10::optional<at::Tensor> pred;
    if (want_pred) pred = at::empty({in.B}, V_.options());
    const EvalOut o = eval_out("FMPlan", dev, in.B, record, reset, pred, c10::nullopt);
    TORCH_CHECK(T == 0 || T == o.T, "FMPlan.evaluate: T does not match the record's length");
    eval_.ensure(in.B, V_.options());
    dtfk::fm::RowArgs a = row_args(in);
    a.lrow = eval_.part(0);
    a.prow = eval_.part(1);
    a.brow = reinterpret_cast<int*>(eval_.part(2));
    a.p_out = o.pred;
    hipStream_t st = cur_stream();
    hip_check(dtfk_fm_rows(&a, 0, rpw_, st), "FMPlan: rows kernel");
    hip_check(dtfk_eval_reduce(a.lrow, a.prow, a.brow, a.labels, a.B, o.T, o.reset, o.rec, st), "FMPlan: reduce kernel");
    ++eval_runs_;
    return pred;
  }

  at::Tensor demb() const { return view(0); }
  at::Tensor dz() const { return view(1).reshape({B_}); }
  at::Tensor lrow() const { return view(2).reshape({B_}); }
  at::Tensor brow() const { return view(3).reshape({B_}).view(at::kInt); }
  at::Tensor z() const { return view(4).reshape({B_}); }
  int64_t runs() const { return runs_; }
  int64_t updates() const { return updates_; }
  int64_t eval_runs() const { return eval_runs_; }
  // rows per wave of fm_rows: 1 .. 64, or 0 (the default): picked by the batch size
  void set_rpw(int rpw) {
    TORCH_CHECK(rpw >= 0 && rpw <= dtfk::fm::MAXRPW, "FMPlan.set_rpw: 0 .. 64");
    rpw_ = rpw;
  }
  int rpw_for(int64_t B) const { return rpw_ != 0 ? rpw_ : dtfk_fm_rpw((int)std::min<int64_t>(B, 1 << 30)); }

 private:
  // part k of the row scratch: demb, dz, lrow, brow, z
  float* part(int k) const { return scratch_.part(k); }
  at::Tensor view(int k) const { return scratch_.view(k, B_); }
  dtfk::fm::RowArgs row_args(const CsrBatch& in) const {
    dtfk::fm::RowArgs a{};
    a.w = w_.data_ptr<float>();
    a.V = V_.data_ptr<float>();
    a.bias = bias_.data_ptr<float>();
    a.F = F_;
    a.K = (int)K_;
    a.B = (int)in.B;
    a.ids = in.ids;
    a.offsets = in.offsets;
    a.vals = in.vals;
    a.labels = in.labels;
    if (scratch_.rows().defined()) {                       // the training step's rows; evaluate() puts its own in their place
      a.lrow = part(2);
      a.brow = reinterpret_cast<int*>(part(3));
    }
    return a;
  }

  at::Tensor w_, V_, bias_, sums_;
  StepScratch scratch_;
  EvalScratch eval_{3};
  int64_t F_ = 0, K_ = 0, B_ = 0;
  int64_t runs_ = 0, updates_ = 0, eval_runs_ = 0;
  int rpw_ = 0;
};

void init_fm(py::module& m) {
  py::class_<FMPlan>(m, "FMPlan")
      .def(py::init<at::Tensor, at::Tensor, at::Tensor>(), py::arg("w"), py::arg("V"), py::arg("bias"))
      .def_static("supported", &FMPlan::supported, py::arg("K"))
      .def("reserve", &FMPlan::reserve, py::arg("rows"), py::arg("ids") = 0)
      .def("rows", &FMPlan::rows, py::arg("labels"), py::arg("offsets"), py::arg("ids"), py::arg("vals"),
           py::arg("gscale"))
      .def("sums", &FMPlan::sums)
      .def("update", &FMPlan::update, py::arg("offsets"), py::arg("ids"), py::arg("vals"), py::arg("kind"),
           py::arg("lr"), py::arg("w_slots"), py::arg("V_slots"))
      .def("evaluate", &FMPlan::evaluate, py::arg("labels"), py::arg("offsets"), py::arg("ids"), py::arg("vals"),
           py::arg("record"), py::arg("reset"), py::arg("want_pred") = false, py::arg("T") = 0)
      .def("eval_runs", &FMPlan::eval_runs)
      .def("runs", &FMPlan::runs)
      .def("updates", &FMPlan::updates)
      .def("set_rpw", &FMPlan::set_rpw, py::arg("rpw"))
      .def("rpw_for", &FMPlan::rpw_for, py::arg("rows"))
      .def("dz", &FMPlan::dz)
      .def("demb", &FMPlan::demb)
      .def("z", &FMPlan::z)
      .def("lrow", &FMPlan::lrow)
      .def("brow", &FMPlan::brow);
}

}  // namespace dtf
