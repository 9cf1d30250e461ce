// What every binding of a forward-only evaluation does before its launches
// (bind_sparse.cpp SparseLRPlan, bind_wide_deep.cpp WideDeepEvalPlan,
// bind_eval_record.cpp): the check of the record (kernels/eval_record.h) and
// the optional [B] outputs, the check of a CSR batch of device tensors, and the
// per-row scratch between the rows kernel and the reduce.  `who` prefixes the
// messages; every refusal raises before anything is launched.
#pragma once
#include <torch/extension.h>

#include "kernels/eval_record.h"

#include <algorithm>
#include <vector>

namespace dtf {

inline bool on_device(const at::Tensor& t, int dev, at::ScalarType dtype) {
  return t.is_cuda() && t.get_device() == dev && t.scalar_type() == dtype && t.is_contiguous();
}

struct EvalOut {
  long long* rec;
  float *pred, *logits;   // [B] or null
  int T, reset;
};

// record: contiguous int64 on device `dev`, evrec::length(T) entries, T >= 2;
// pred / logits: contiguous fp32 [B] on `dev`, or None
inline EvalOut eval_out(const char* who, int dev, int64_t B, const at::Tensor& record, bool reset,
                        const c10::optional<at::Tensor>& pred, const c10::optional<at::Tensor>& logits) {
  const int T = dtfk::evrec::thresholds_of(record.numel());
  TORCH_CHECK(on_device(record, dev, at::kLong) && T >= 2, who,
              ": record must be a contiguous int64 GPU tensor of an evaluation record's length, T >= 2");
  EvalOut o{reinterpret_cast<long long*>(record.data_ptr<int64_t>()), nullptr, nullptr, T, reset ? 1 : 0};
  for (int k = 0; k < 2; ++k) {
    const c10::optional<at::Tensor>& t = k == 0 ? pred : logits;
    if (!t.has_value()) continue;
    TORCH_CHECK(on_device(*t, dev, at::kFloat) && t->numel() == B, who,
                ": pred / logits must be contiguous fp32 GPU tensors of B entries");
    (k == 0 ? o.pred : o.logits) = t->data_ptr<float>();
  }
  return o;
}

struct CsrBatch {
  const float* labels;
  const long long* offsets;
  const long long* ids;
  const float* vals;   // null: every value is 1
  int64_t B;
};

// labels [B] / [B, 1] f32, offsets [B + 1] i64, ids [nnz] i64, vals [nnz] f32 or
// None: contiguous, on device `dev`, 1 <= B <= 2^30
inline CsrBatch csr_batch(const char* who, int dev, const at::Tensor& labels, const at::Tensor& offsets,
                          const at::Tensor& ids, const c10::optional<at::Tensor>& vals) {
  TORCH_CHECK(on_device(labels, dev, at::kFloat), who, ": labels must be contiguous fp32 on the plan's GPU");
  TORCH_CHECK(on_device(offsets, dev, at::kLong), who, ": offsets must be contiguous int64 on the plan's GPU");
  TORCH_CHECK(on_device(ids, dev, at::kLong), who, ": ids must be contiguous int64 on the plan's GPU");
  const int64_t B = labels.numel();
  TORCH_CHECK(B >= 1 && B <= (1 << 30), who, ": 1 <= B <= 2^30 rows");
  TORCH_CHECK(offsets.numel() == B + 1, who, ": offsets must hold B + 1 entries");
  const float* vp = nullptr;
  if (vals.has_value()) {
    TORCH_CHECK(on_device(*vals, dev, at::kFloat) && vals->numel() == ids.numel(), who,
                ": vals must be contiguous fp32 on the plan's GPU, one per id");
    vp = vals->data_ptr<float>();
  }
  return {labels.data_ptr<float>(), reinterpret_cast<const long long*>(offsets.data_ptr<int64_t>()),
          reinterpret_cast<const long long*>(ids.data_ptr<int64_t>()), vp, B};
}

// `parts` arrays of 4 bytes per row between the rows kernel and the reduce, in
// one tensor: part k starts at k * capacity.  A larger batch gets a larger
// tensor; the outgrown one is kept, not freed: a captured hipGraph of an
// evaluation holds its pointers (both kernels of a capture use the same
// scratch, so a replay stays right).
class EvalScratch {
 public:
  explicit EvalScratch(int parts) : parts_(parts) {}
  void ensure(int64_t B, const at::TensorOptions& f32) {
    if (cur_.defined() && cur_.numel() >= parts_ * B) return;
    if (cur_.defined()) old_.push_back(cur_);
    cur_ = at::empty({parts_ * std::max<int64_t>(B, 1024)}, f32);
  }
  float* part(int k) const { return cur_.data_ptr<float>() + k * (cur_.numel() / parts_); }
  const at::Tensor& tensor() const { return cur_; }

 private:
  int parts_;
  at::Tensor cur_;
  std::vector<at::Tensor> old_;
};

}  // namespace dtf
