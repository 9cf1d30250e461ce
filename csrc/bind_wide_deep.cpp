// The one-GPU forward-only Wide&Deep evaluation as one host call
// (csrc/kernels/wide_deep_eval.hip wd_eval_rows + eval_record.hip's
// eval_record_reduce).  WideDeepEvalPlan holds the model's tensors themselves, not
// copies: training between evaluations is seen by the next one.  evaluate()
// checks everything first and then makes its two launches on the current
// stream: no host read-back, no memset node, so it can be captured in a
// hipGraph (the capture holds the tensors' and the scratch's addresses).
#include "bind_common.h"
#include "eval_record_host.h"
//
// The one-GPU fused training step's per-row half is WideDeepTrainPlan
// (csrc/kernels/wide_deep_train.hip wd_train_rows + wd_train_sums): the same
// tensors, plus the step's scratch (activations, their gradients, per-row loss).
#include "kernels/wide_deep_eval.h"
#include "kernels/wide_deep_train.h"
//
// WideDeepTrainPlan.update is the step's table half (csrc/kernels/wide_deep_update.hip
// wd_update_runs + wd_update_carry): one stable sort of the batch's ids, then every
// touched row of both tables written once by a row-local rule of optim_rules.h.
#include "kernels/wide_deep_update.h"
#include "step_scratch.h"
#include "table_update_host.h"

#include <stdexcept>
#include <string>
#include <vector>

namespace dtf {

// The model's tensors, checked once: what both plans hold.  `who` prefixes the messages.
class WideDeepTensors {
 public:
  WideDeepTensors(const char* who, at::Tensor wide, at::Tensor emb, std::vector<at::Tensor> layers, at::Tensor bias,
                  const std::string& combiner)
      : wide_(wide), emb_(emb), layers_(std::move(layers)), bias_(bias) {
    TORCH_CHECK(emb.is_cuda() && emb.scalar_type() == at::kFloat && emb.is_contiguous() && emb.dim() == 2,
                who, ": emb_table must be a contiguous fp32 [F, D] GPU table");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(emb.data_ptr()) & 15) == 0,
                who, ": unsupported shape (emb_table must be 16-byte aligned)");
    const int64_t F = emb.size(0), D = emb.size(1);
    const int dev = emb.get_device();
    TORCH_CHECK(wide.is_cuda() && wide.scalar_type() == at::kFloat && wide.is_contiguous() && wide.numel() == F &&
                    wide.get_device() == dev && (wide.dim() == 1 || (wide.dim() == 2 && wide.size(1) == 1)),
                who, ": wide_table must be a contiguous fp32 [F, 1] GPU table on emb_table's device");
    TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == at::kFloat && bias.numel() == 1 && bias.is_contiguous() &&
                    bias.get_device() == dev,
                who, ": bias must be one fp32 GPU value");
    TORCH_CHECK(combiner == "sum" || combiner == "mean" || combiner == "sqrtn",
                who, ": combiner must be sum, mean or sqrtn");
    mode_ = combiner == "sum" ? 0 : (combiner == "mean" ? 1 : 2);
    TORCH_CHECK(F >= 1 && layers_.size() % 2 == 0 && layers_.size() >= 4 && layers_.size() <= 2 * dtfk::wde::MAXL,
                who, ": unsupported shape (1 to 3 hidden layers and the last one, as [W, b] pairs)");
    nl_ = (int)layers_.size() / 2;
    dims_[0] = (int)D;
    int64_t k = D;
    for (int l = 0; l < nl_; ++l) {
      const at::Tensor& W = layers_[2 * l];
      const at::Tensor& b = layers_[2 * l + 1];
      TORCH_CHECK(W.is_cuda() && W.scalar_type() == at::kFloat && W.is_contiguous() && W.dim() == 2 &&
                      W.size(0) == k && W.get_device() == dev && b.is_cuda() && b.scalar_type() == at::kFloat &&
                      b.is_contiguous() && b.numel() == W.size(1) && b.get_device() == dev,
                  who, ": layers must be contiguous fp32 GPU [K, N] weights and [N] biases in a chain");
      k = W.size(1);
      TORCH_CHECK(k <= dtfk::wde::MAXW, who, ": unsupported shape (hidden width above 512)");
      dims_[l + 1] = (int)k;
      if (l < nl_ - 1)
        TORCH_CHECK(((reinterpret_cast<uintptr_t>(W.data_ptr()) | reinterpret_cast<uintptr_t>(b.data_ptr())) & 15) == 0,
                    who, ": unsupported shape (tower tensors must be 16-byte aligned)");
    }
    TORCH_CHECK(D <= dtfk::wde::MAXD && dtfk_wd_eval_supported((int)D, nl_, dims_) == 1,
                who, ": unsupported shape (D a multiple of 4 up to 128; 1 to 3 hidden widths, multiples "
                "of 16 up to 512; last width 1)");
  }

  static bool supported(int64_t D, const std::vector<int64_t>& hidden) {
    if (D < 1 || D > dtfk::wde::MAXD || hidden.empty() || (int)hidden.size() > dtfk::wde::MAXL - 1) return false;
    int dims[dtfk::wde::MAXL + 1];
    dims[0] = (int)D;
    for (size_t l = 0; l < hidden.size(); ++l) {
      if (hidden[l] < 1 || hidden[l] > dtfk::wde::MAXW) return false;
      dims[l + 1] = (int)hidden[l];
    }
    dims[hidden.size() + 1] = 1;
    return dtfk_wd_eval_supported((int)D, (int)hidden.size() + 1, dims) == 1;
  }

 protected:
  // the kernels' view of the tensors and a checked CSR batch (outputs left null)
  dtfk::wde::Args forward_args(const CsrBatch& in) const {
    dtfk::wde::Args a{};
    a.Wt = wide_.data_ptr<float>();
    a.E = emb_.data_ptr<float>();
    a.F = (long long)emb_.size(0);
    a.D = dims_[0];
    a.mode = mode_;
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

  at::Tensor wide_, emb_, bias_;
  std::vector<at::Tensor> layers_;
  int dims_[dtfk::wde::MAXL + 1] = {0, 0, 0, 0, 0};
  int nl_ = 0, mode_ = 0;
};

class WideDeepEvalPlan : public WideDeepTensors {
 public:
  WideDeepEvalPlan(at::Tensor wide, at::Tensor emb, std::vector<at::Tensor> layers, at::Tensor bias,
                   const std::string& combiner)
      : WideDeepTensors("WideDeepEvalPlan", wide, emb, std::move(layers), bias, combiner) {}

  // A CSR batch of device tensors (csr_batch) into `record` (eval_out: reset
  // starts it over, else the batch is added; pred / logits: [B] f32 or None).
  // Every refusal raises before anything is launched.
  void evaluate(at::Tensor labels, at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals,
                at::Tensor record, bool reset, c10::optional<at::Tensor> pred, c10::optional<at::Tensor> logits) {
    const int dev = emb_.get_device();
    const CsrBatch in = csr_batch("WideDeepEvalPlan.evaluate", dev, labels, offsets, ids, vals);
    const EvalOut o = eval_out("WideDeepEvalPlan", dev, in.B, record, reset, pred, logits);
    scratch_.ensure(in.B, emb_.options());
    dtfk::wde::Args a = forward_args(in);
    a.lrow = scratch_.part(0);
    a.prow = scratch_.part(1);
    a.brow = reinterpret_cast<int*>(scratch_.part(2));
    a.p_out = o.pred;
    a.z_out = o.logits;
    hipStream_t st = cur_stream();
    hip_check(dtfk_wd_eval_rows(&a, tile_, st), "WideDeepEvalPlan: rows kernel");
    hip_check(dtfk_eval_reduce(a.lrow, a.prow, a.brow, a.labels, a.B, o.T, o.reset, o.rec, st),
              "WideDeepEvalPlan: reduce kernel");
    ++eval_runs_;
  }

  int64_t eval_runs() const { return eval_runs_; }
  // 16 / 32 force the row tile, 0 (the default) picks it by the batch size
  void set_tile(int tile) {
    TORCH_CHECK(tile == 0 || tile == 16 || tile == 32, "WideDeepEvalPlan.set_tile: 0, 16 or 32");
    tile_ = tile;
  }
  int tile_for(int64_t B) const { return tile_ != 0 ? tile_ : dtfk_wd_eval_tile((int)B, nl_, dims_); }
  int64_t lds_bytes(int tile) const { return dtfk_wd_eval_lds_bytes(dims_[0], nl_, dims_, tile); }
  at::Tensor scratch() const { return scratch_.tensor(); }   // thirds: lrow | prow | bad ids per row (int)

 private:
  EvalScratch scratch_{3};
  int tile_ = 0;
  int64_t eval_runs_ = 0;
};

// The per-row half of the one-GPU training step.  The plan owns the step's
// scratch (step_scratch.h), one tensor of `capacity` rows per part:
//   rows:   act[0 .. nl-1] [cap, dims[l]] | dzl[1 .. nl-1] [cap, dims[l]] | demb [cap, D] | dz | lrow | brow (int) | z [cap]
//   update: scale [cap] | bag_of [ids cap] (int) | part (table_update.h)
// reserve() grows it (never inside a stream capture: a captured graph holds the
// addresses; an outgrown tensor is kept alive for the graphs that hold it).  The
// accessors return the last batch's rows of a part.
class WideDeepTrainPlan : public WideDeepTensors {
 public:
  WideDeepTrainPlan(at::Tensor wide, at::Tensor emb, std::vector<at::Tensor> layers, at::Tensor bias,
                    const std::string& combiner)
      : WideDeepTensors("WideDeepTrainPlan", wide, emb, std::move(layers), bias, combiner) {
    TORCH_CHECK(dtfk_wd_train_supported(dims_[0], nl_, dims_) == 1, "WideDeepTrainPlan: unsupported shape");
    std::vector<int> widths(dims_, dims_ + nl_);                    // act
    widths.insert(widths.end(), dims_ + 1, dims_ + nl_);            // dzl
    widths.insert(widths.end(), {dims_[0], 1, 1, 1, 1});            // demb, dz, lrow, brow, z
    scratch_.init("WideDeepTrainPlan", std::move(widths), dims_[0], true);
  }

  // ids > 0 also sizes update()'s scratch
  void reserve(int64_t B, int64_t ids) { scratch_.reserve(B, ids, emb_.options()); }

  // The rows kernel on the current stream: forward, head and the backward through
  // the tower for one CSR batch of device tensors; gscale: the loss's scale per
  // row (1 / B for a batch mean).  Every refusal raises before anything is launched.
  void rows(at::Tensor labels, at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals, double gscale) {
    const CsrBatch in = csr_batch("WideDeepTrainPlan.rows", emb_.get_device(), labels, offsets, ids, vals);
    reserve(in.B, 0);
    dtfk::wdt::Args a{};
    a.f = forward_args(in);
    for (int l = 0; l < nl_; ++l) a.act[l] = scratch_.part(l);
    for (int l = 1; l < nl_; ++l) a.dzl[l] = scratch_.part(nl_ + l - 1);
    a.demb = scratch_.part(2 * nl_ - 1);
    a.dz = scratch_.part(2 * nl_);
    a.f.lrow = scratch_.part(2 * nl_ + 1);
    a.f.brow = reinterpret_cast<int*>(scratch_.part(2 * nl_ + 2));
    a.f.z_out = scratch_.part(2 * nl_ + 3);
    a.gscale = (float)gscale;
    hip_check(dtfk_wd_train_rows(&a, tile_, cur_stream()), "WideDeepTrainPlan: rows kernel");
    B_ = in.B;
    ++runs_;
  }

  // mean(lrow) of the last batch as a new fp32 scalar, and sum(dz) into db_last /
  // dbias (one fp32 value each, e.g. views of a flat gradient): one small kernel,
  // float64 sums in a fixed order.
  at::Tensor sums(at::Tensor db_last, at::Tensor dbias) {
    TORCH_CHECK(B_ > 0, "WideDeepTrainPlan.sums: no batch yet");
    const int dev = emb_.get_device();
    TORCH_CHECK(on_device(db_last, dev, at::kFloat) && db_last.numel() == 1 && on_device(dbias, dev, at::kFloat) &&
                    dbias.numel() == 1,
                "WideDeepTrainPlan.sums: db_last / dbias must be one fp32 value each on the plan's GPU");
    at::Tensor loss = at::empty({}, emb_.options());
    hip_check(dtfk_wd_train_sums(scratch_.part(2 * nl_ + 1), scratch_.part(2 * nl_), (int)B_, loss.data_ptr<float>(),
                                 db_last.data_ptr<float>(), dbias.data_ptr<float>(), cur_stream()),
              "WideDeepTrainPlan: sums kernel");
    return loss;
  }

  // The tables' half of the step, after rows(): both tables and their slots take
  // rule `kind` (optim_rules.h OptimKind, row-local kinds) with the last batch's
  // demb / dz: duplicates summed, every touched row written once.  offsets / ids /
  // vals: the batch rows() saw; *_slots: slot a, slot b as the kind has them; skip:
  // device int32 word (nonzero changes nothing) or None; hyper: Rule.native_kwargs.
  // One stable sort, bag_index, the combiner's scale and two launches on the current
  // stream; every refusal raises before anything is launched.
  void update(at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals, int kind, double lr,
              std::vector<at::Tensor> wide_slots, std::vector<at::Tensor> emb_slots, c10::optional<at::Tensor> skip,
              const py::kwargs& hyper) {
    TORCH_CHECK(B_ > 0, "WideDeepTrainPlan.update: no batch yet (rows() first)");
    if (table_update_host("WideDeepTrainPlan.update", dtfk_wd_update, wide_, emb_, B_, offsets, ids, vals, kind, lr,
                          wide_slots, emb_slots, skip, hyper, scratch_.part(2 * nl_), scratch_.part(2 * nl_ - 1),
                          [&](int64_t N, hipStream_t st) {
                            reserve(B_, N);
                            if (mode_ != 0)
                              hip_check(dtfk_wd_update_scale(reinterpret_cast<const long long*>(offsets.data_ptr<int64_t>()),
                                                             opt_ptr<float>(vals), (int)B_, mode_, scratch_.scale(), st),
                                        "WideDeepTrainPlan.update: scale kernel");
                            return UpdateScratch{scratch_.bag_of(), scratch_.update_part(),
                                                 mode_ != 0 ? scratch_.scale() : nullptr};
                          }))
      ++updates_;
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
  void set_tile(int tile) {
    TORCH_CHECK(tile == 0 || tile == 16 || tile == 32, "WideDeepTrainPlan.set_tile: 0, 16 or 32");
    tile_ = tile;
  }
  int tile_for(int64_t B) const { return tile_ != 0 ? tile_ : dtfk_wd_train_tile((int)B, nl_, dims_); }
  int64_t lds_bytes(int tile) const { return dtfk_wd_train_lds_bytes(dims_[0], nl_, dims_, tile); }

 private:
  void checked(int l, int lo, const char* what) const {
    TORCH_CHECK(l >= lo && l < nl_, "WideDeepTrainPlan.", what, ": layer out of range");
  }
  // part k of the scratch in rows()'s order, the last batch's rows: [B, width]
  at::Tensor view(int k) const { return scratch_.view(k, B_); }

  StepScratch scratch_;
  int64_t B_ = 0, runs_ = 0, updates_ = 0;
  int tile_ = 0;
};

void init_wide_deep(py::module& m) {
  py::class_<WideDeepEvalPlan>(m, "WideDeepEvalPlan")
      .def(py::init<at::Tensor, at::Tensor, std::vector<at::Tensor>, at::Tensor, const std::string&>(),
           py::arg("wide_table"), py::arg("emb_table"), py::arg("layers"), py::arg("bias"), py::arg("combiner") = "sum")
      .def_static("supported", &WideDeepEvalPlan::supported, py::arg("emb_dim"), py::arg("hidden"))
      .def("evaluate", &WideDeepEvalPlan::evaluate, py::arg("labels"), py::arg("offsets"), py::arg("ids"),
           py::arg("vals"), py::arg("record"), py::arg("reset"), py::arg("pred") = py::none(),
           py::arg("logits") = py::none())
      .def("eval_runs", &WideDeepEvalPlan::eval_runs)
      .def("set_tile", &WideDeepEvalPlan::set_tile, py::arg("tile"))
      .def("tile_for", &WideDeepEvalPlan::tile_for, py::arg("rows"))
      .def("lds_bytes", &WideDeepEvalPlan::lds_bytes, py::arg("tile"))
      .def("scratch", &WideDeepEvalPlan::scratch);
  py::class_<WideDeepTrainPlan>(m, "WideDeepTrainPlan")
      .def(py::init<at::Tensor, at::Tensor, std::vector<at::Tensor>, at::Tensor, const std::string&>(),
           py::arg("wide_table"), py::arg("emb_table"), py::arg("layers"), py::arg("bias"), py::arg("combiner") = "sum")
      .def_static("supported", &WideDeepTrainPlan::supported, py::arg("emb_dim"), py::arg("hidden"))
      .def("reserve", &WideDeepTrainPlan::reserve, py::arg("rows"), py::arg("ids") = 0)
      .def("rows", &WideDeepTrainPlan::rows, py::arg("labels"), py::arg("offsets"), py::arg("ids"), py::arg("vals"),
           py::arg("gscale"))
      .def("sums", &WideDeepTrainPlan::sums, py::arg("db_last"), py::arg("dbias"))
      .def("update", &WideDeepTrainPlan::update, py::arg("offsets"), py::arg("ids"), py::arg("vals"), py::arg("kind"),
           py::arg("lr"), py::arg("wide_slots"), py::arg("emb_slots"), py::arg("skip") = py::none())
      .def("updates", &WideDeepTrainPlan::updates)
      .def("act", &WideDeepTrainPlan::act, py::arg("layer"))
      .def("dzl", &WideDeepTrainPlan::dzl, py::arg("layer"))
      .def("demb", &WideDeepTrainPlan::demb)
      .def("dz", &WideDeepTrainPlan::dz)
      .def("lrow", &WideDeepTrainPlan::lrow)
      .def("brow", &WideDeepTrainPlan::brow)
      .def("z", &WideDeepTrainPlan::z)
      .def("scratch", &WideDeepTrainPlan::scratch)
      .def("row_floats", &WideDeepTrainPlan::row_floats)
      .def("runs", &WideDeepTrainPlan::runs)
      .def("set_tile", &WideDeepTrainPlan::set_tile, py::arg("tile"))
      .def("tile_for", &WideDeepTrainPlan::tile_for, py::arg("rows"))
      .def("lds_bytes", &WideDeepTrainPlan::lds_bytes, py::arg("tile"));
}

}  // namespace dtf
