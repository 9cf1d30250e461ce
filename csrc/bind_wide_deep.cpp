// The one-GPU forward-only Wide&Deep evaluation as one host call
// (csrc/kernels/wide_deep_eval.hip wd_eval_rows + sparse_lr.hip's
// slr_eval_reduce).  WideDeepEvalPlan holds the model's tensors themselves, not
// copies: training between evaluations is seen by the next one.  evaluate()
// checks everything first and then makes its two launches on the current
// stream: no host read-back, no memset node, so it can be captured in a
// hipGraph (the capture holds the tensors' and the scratch's addresses).
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

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

  // Device tensors: labels [B] / [B, 1] f32, offsets [B + 1] i64, ids [nnz] i64,
  // vals [nnz] f32 or None.  record: 3 + 2 (T + 1) int64, T >= 2 (the sparse-LR
  // record); reset starts it over, else the batch is added.  pred / logits: [B]
  // f32 or None.  Every refusal raises before anything is launched.
  void evaluate(at::Tensor labels, at::Tensor offsets, at::Tensor ids, c10::optional<at::Tensor> vals,
                at::Tensor record, bool reset, c10::optional<at::Tensor> pred, c10::optional<at::Tensor> logits) {
    const int dev = emb_.get_device();
    TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kFloat && labels.is_contiguous() &&
                    labels.get_device() == dev, "WideDeepEvalPlan.evaluate: labels must be contiguous fp32 on the GPU");
    TORCH_CHECK(offsets.is_cuda() && offsets.scalar_type() == at::kLong && offsets.is_contiguous() &&
                    offsets.get_device() == dev, "WideDeepEvalPlan.evaluate: offsets must be contiguous int64 on the GPU");
    TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kLong && ids.is_contiguous() && ids.get_device() == dev,
                "WideDeepEvalPlan.evaluate: ids must be contiguous int64 on the GPU");
    const int64_t B = labels.numel();
    TORCH_CHECK(B >= 1 && B <= (1 << 30), "WideDeepEvalPlan.evaluate: 1 <= B <= 2^30 rows");
    TORCH_CHECK(offsets.numel() == B + 1, "WideDeepEvalPlan.evaluate: offsets must hold B + 1 entries");
    const float* vp = nullptr;
    if (vals.has_value()) {
      TORCH_CHECK(vals->is_cuda() && vals->scalar_type() == at::kFloat && vals->is_contiguous() &&
                      vals->numel() == ids.numel() && vals->get_device() == dev,
                  "WideDeepEvalPlan.evaluate: vals must be contiguous fp32 on the GPU, one per id");
      vp = vals->data_ptr<float>();
    }
    TORCH_CHECK(record.is_cuda() && record.scalar_type() == at::kLong && record.is_contiguous() &&
                    record.get_device() == dev && record.numel() >= 9 && (record.numel() - 3) % 2 == 0,
                "WideDeepEvalPlan: record must be a contiguous int64 GPU tensor of 3 + 2 (T + 1) entries, T >= 2");
    float* outs[2] = {nullptr, nullptr};
    for (int k = 0; k < 2; ++k) {
      const c10::optional<at::Tensor>& t = k == 0 ? pred : logits;
      if (!t.has_value()) continue;
      TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == B &&
                      t->get_device() == dev,
                  "WideDeepEvalPlan: pred / logits must be contiguous fp32 GPU tensors of B entries");
      outs[k] = t->data_ptr<float>();
    }
    const int T = (int)((record.numel() - 3) / 2 - 1);
    ensure_(B);
    float* sc = scratch_.data_ptr<float>();
    const int64_t cap = scratch_.numel() / 3;   // lrow | prow | bad ids per row (int)
    dtfk::wde::Args a{};
    a.Wt = wide_.data_ptr<float>();
    a.E = emb_.data_ptr<float>();
    a.F = (long long)emb_.size(0);
    a.D = dims_[0];
    a.mode = mode_;
    a.ids = reinterpret_cast<const long long*>(ids.data_ptr<int64_t>());
    a.offsets = reinterpret_cast<const long long*>(offsets.data_ptr<int64_t>());
    a.vals = vp;
    a.labels = labels.data_ptr<float>();
    for (int l = 0; l < nl_; ++l) {
      a.W[l] = layers_[2 * l].data_ptr<float>();
      a.b[l] = layers_[2 * l + 1].data_ptr<float>();
    }
    for (int l = 0; l <= nl_; ++l) a.dims[l] = dims_[l];
    a.nl = nl_;
    a.bias = bias_.data_ptr<float>();
    a.B = (int)B;
    a.lrow = sc;
    a.prow = sc + cap;
    a.brow = reinterpret_cast<int*>(sc + 2 * cap);
    a.p_out = outs[0];
    a.z_out = outs[1];
    hipStream_t st = c10::hip::getCurrentHIPStream().stream();
    hck_(dtfk_wd_eval_rows(&a, tile_, st), "WideDeepEvalPlan: rows kernel");
    hck_(dtfk_eval_reduce(a.lrow, a.prow, a.brow, a.labels, (int)B, T, reset ? 1 : 0,
                          reinterpret_cast<long long*>(record.data_ptr<int64_t>()), st),
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
  at::Tensor scratch() const { return scratch_; }

 private:
  static void hck_(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
  }
  // A larger batch gets a larger scratch; the outgrown one is kept alive: a
  // captured hipGraph of an evaluation holds its pointers.  12 bytes per row.
  void ensure_(int64_t B) {
    if (scratch_.defined() && scratch_.numel() >= 3 * B) return;
    if (scratch_.defined()) old_.push_back(scratch_);
    scratch_ = at::empty({3 * std::max<int64_t>(B, 1024)}, emb_.options());
  }

  at::Tensor wide_, emb_, bias_, scratch_;
  std::vector<at::Tensor> layers_, old_;
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
