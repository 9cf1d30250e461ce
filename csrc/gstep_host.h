// The one place a global_step tensor becomes the (pointer, kind) pair the
// kernels take (gstep_kind.h): a device scalar of float32 / int64 / int32 /
// float64, or no tensor -> {nullptr, GSTEP_NONE}.
#pragma once
#include <torch/extension.h>

#include "gstep_kind.h"

namespace dtf {

struct GstepRef {
  void* ptr = nullptr;
  int kind = dtfk::GSTEP_NONE;
};

inline GstepRef gstep_ref(const c10::optional<at::Tensor>& g, const char* who) {
  GstepRef r;
  if (!g.has_value()) return r;
  TORCH_CHECK(g->is_cuda() && g->numel() == 1, who, ": device scalar global_step");
  switch (g->scalar_type()) {
    case at::kFloat: r.kind = dtfk::GSTEP_F32; break;
    case at::kLong: r.kind = dtfk::GSTEP_I64; break;
    case at::kInt: r.kind = dtfk::GSTEP_I32; break;
    case at::kDouble: r.kind = dtfk::GSTEP_F64; break;
    default: TORCH_CHECK(false, who, ": unsupported global_step dtype");
  }
  r.ptr = g->data_ptr();
  return r;
}

}  // namespace dtf
