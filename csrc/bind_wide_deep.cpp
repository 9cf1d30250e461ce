// The one-GPU forward-only Wide&Deep evaluation as one host call
// (csrc/kernels/wide_deep_eval.hip wd_eval_rows + eval_record.hip's
// eval_record_reduce).  WideDeepEvalPlan holds the model's tensors themselves, not
// copies: training between evaluations is seen by the next one.  evaluate()
// checks everything first and then makes its two launches on the current
// stream: no host read-back, no memset node, so it can be captured in a
// hipGraph (the capture holds the tensors' and the scratch's addresses).
#include "bind_common.h"
#include "eval_record_host.h"
#include "kernels/wide_deep_eval.h"

#include <stdexcept>
#include <string>
#include <vector>

namespace dtf {

class WideDeepEvalPlan {
 public:
  WideDeepEvalPlan(at::Tensor wide, at::Tensor emb, std::vector<at::Tensor> layers, at::Tensor bias,
                   const std::string& combiner)
      : wide_(wide), emb_(emb), layers_(std::move(layers)), bias_(bias) {
    TORCH_CHECK(emb.is_cuda() && emb.scalar_type() == at::kFloat && emb.is_contiguous() && emb.dim() == 2,
                "WideDeepEvalPlan: emb_table must be a contiguous fp32 [F, D] GPU table");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(emb.data_ptr()) & 15) == 0,
                "WideDeepEvalPlan: unsupported shape (emb_table must be 16-byte aligned)");
    const int64_t F = emb.size(0), D = emb.size(1);
    const int dev = emb.get_device();
    TORCH_CHECK(wide.is_cuda() && wide.scalar_type() == at::kFloat && wide.is_contiguous() && wide.numel() == F &&
                    wide.get_device() == dev && (wide.dim() == 1 || (wide.dim() == 2 && wide.size(1) == 1)),
                "WideDeepEvalPlan: wide_table must be a contiguous fp32 [F, 1] GPU table on emb_table's device");
    TORCH_CHECK(bias.is_cuda() && bias.scalar_type() == at::kFloat && bias.numel() == 1 && bias.is_contiguous() &&
                    bias.get_device() == dev,
                "WideDeepEvalPlan: bias must be one fp32 GPU value");
    TORCH_CHECK(combiner == "sum" || combiner == "mean" || combiner == "sqrtn",
                "WideDeepEvalPlan: combiner must be sum, mean or sqrtn");
    mode_ = combiner == "sum" ? 0 : (combiner == "mean" ? 1 : 2);
    TORCH_CHECK(F >= 1 && layers_.size() % 2 == 0 && layers_.size() >= 4 && layers_.size() <= 2 * dtfk::wde::MAXL,
                "WideDeepEvalPlan: unsupported shape (1 to 3 hidden layers and the last one, as [W, b] pairs)");
    nl_ = (int)layers_.size() / 2;
    dims_[0] = (int)D;
    int64_t k = D;
    for (int l = 0; l < nl_; ++l) {
      const at::Tensor& W = layers_[2 * l];
      const at::Tensor& b = layers_[2 * l + 1];
      TORCH_CHECK(W.is_cuda() && W.scalar_type() == at::kFloat && W.is_contiguous() && W.dim() == 2 &&
                      W.size(0) == k && W.get_device() == dev && b.is_cuda() && b.scalar_type() == at::kFloat &&
                      b.is_contiguous() && b.numel() == W.size(1) && b.get_device() == dev,
                  "WideDeepEvalPlan: layers must be contiguous fp32 GPU [K, N] weights and [N] biases in a chain");
      k = W.size(1);
      TORCH_CHECK(k <= dtfk::wde::MAXW, "WideDeepEvalPlan: unsupported shape (hidden width above 512)");
      dims_[l + 1] = (int)k;
      if (l < nl_ - 1)
        TORCH_CHECK(((reinterpret_cast<uintptr_t>(W.data_ptr()) | reinterpret_cast<uintptr_t>(b.data_ptr())) & 15) == 0,
                    "WideDeepEvalPlan: unsupported shape (tower tensors must be 16-byte aligned)");
    }
    TORCH_CHECK(D <= dtfk::wde::MAXD && dtfk_wd_eval_supported((int)D, nl_, dims_) == 1,
                "WideDeepEvalPlan: unsupported shape (D a multiple of 4 up to 128; 1 to 3 hidden widths, multiples "
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

  // A CSR batch of device tensors (csr_batch) into `record` (eval_out: reset
  // starts it over, else the batch is added; pred / logits: [B] f32 or None).
  // Every refusal raises before anything is launched.
  void evaluate(at::Tensor labels, at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals,
                at::Tensor record, bool reset, c10::optional<at::Tensor> pred, c10::optional<at::Tensor> logits) {
    const int dev = emb_.get_device();
    const CsrBatch in = csr_batch("WideDeepEvalPlan.evaluate", dev, labels, offsets, ids, vals);
    const EvalOut o = eval_out("WideDeepEvalPlan", dev, in.B, record, reset, pred, logits);
    scratch_.ensure(in.B, emb_.options());
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
  at::Tensor wide_, emb_, bias_;
  std::vector<at::Tensor> layers_;
  EvalScratch scratch_{3};
  int dims_[dtfk::wde::MAXL + 1] = {0, 0, 0, 0, 0};
  int nl_ = 0, mode_ = 0, tile_ = 0;
  int64_t eval_runs_ = 0;
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
}

}  // namespace dtf
