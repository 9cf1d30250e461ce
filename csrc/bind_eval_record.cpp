// eval_record_reduce: the evaluation record's reduce kernel
// (csrc/kernels/eval_record.hip) on per-row arrays the caller supplies, without
// a model's rows kernel in front of it.
#include "bind_common.h"
#include "eval_record_host.h"

namespace dtf {

// lrow, prow, labels: [B] f32; brow: [B] i32; record: int64 (kernels/eval_record.h);
// all contiguous on one GPU, 1 <= B <= 2^30.  Raises before the launch.
static void eval_record_reduce(at::Tensor lrow, at::Tensor prow, at::Tensor brow, at::Tensor labels, at::Tensor record,
                               bool reset) {
  const char* who = "eval_record_reduce";
  TORCH_CHECK(lrow.is_cuda(), who, ": lrow must be on a GPU");
  const int dev = lrow.get_device();
  TORCH_CHECK(on_device(lrow, dev, at::kFloat) && on_device(prow, dev, at::kFloat) &&
                  on_device(labels, dev, at::kFloat) && on_device(brow, dev, at::kInt),
              who, ": lrow, prow, labels (fp32) and brow (int32) must be contiguous on one GPU");
  const int64_t B = lrow.numel();
  TORCH_CHECK(B >= 1 && B <= (1 << 30) && prow.numel() == B && brow.numel() == B && labels.numel() == B, who,
              ": the four row arrays must hold the same 1 <= B <= 2^30 entries");
  const EvalOut o = eval_out(who, dev, B, record, reset, c10::nullopt, c10::nullopt);
  hip_check(dtfk_eval_reduce(lrow.data_ptr<float>(), prow.data_ptr<float>(), brow.data_ptr<int>(),
                             labels.data_ptr<float>(), (int)B, o.T, o.reset, o.rec, cur_stream()),
            who);
}

void init_eval_record(py::module& m) {
  m.def("eval_record_reduce", &eval_record_reduce, py::arg("lrow"), py::arg("prow"), py::arg("brow"),
        py::arg("labels"), py::arg("record"), py::arg("reset"));
}

}  // namespace dtf
