// The table half of a training step that ends in kernels/table_update.h's one-writer
// update, as FMPlan.update (bind_fm.cpp), DeepFMPlan.update (bind_deepfm.cpp),
// FFMPlan.update (bind_ffm.cpp) and WideDeepTrainPlan.update (bind_wide_deep.cpp) run it: the checks, one stable sort
// of the batch's ids, bag_index, then the file's launcher (dtfk_fm_update /
// dtfk_wd_update) with the plan's dz / demb.  `who` prefixes the messages; every
// refusal raises before anything is launched.
#pragma once
#include "bind_common.h"
#include "eval_record_host.h"
#include "kernels/ops_api.h"
#include "kernels/table_update.h"

#include <vector>

namespace dtf {

// what a plan's scratch gives one update of N ids
struct UpdateScratch {
  int* bag_of;          // [>= N]
  float* part;          // [>= dtfk::tu::part_floats(N, width)], 16-byte aligned
  const float* scale;   // [B] the combiner's scale per bag, or null
};

// lin [rows], row [rows, width] and their slots take rule `kind` with the last rows() batch's dz [B] /
// demb [B, width].  skip: device int32 word (nonzero changes nothing) or None.
// prepare(N, stream): called once after the checks, before any launch of this function: the plan grows its
// update scratch there and launches what fills `scale`.
// Returns false when the batch has no ids (nothing was launched).
template <class Prepare>
inline bool table_update_host(const char* who, hipError_t (*launch)(const dtfk::tu::Args*, hipStream_t),
                              const at::Tensor& lin, const at::Tensor& row, int64_t B, const at::Tensor& offsets,
                              const at::Tensor& ids, const c10::optional<at::Tensor>& vals, int kind, double lr,
                              const std::vector<at::Tensor>& lin_slots, const std::vector<at::Tensor>& row_slots,
                              const c10::optional<at::Tensor>& skip, const py::kwargs& hyper, const float* dz,
                              const float* demb, Prepare&& prepare) {
  const int dev = row.get_device();
  const int64_t rows = row.size(0);
  TORCH_CHECK(B > 0, who, ": no batch yet (rows() first)");
  TORCH_CHECK(on_device(offsets, dev, at::kLong) && offsets.numel() == B + 1, who,
              ": offsets must be contiguous int64 on the plan's GPU, B + 1 entries of the last rows() batch");
  TORCH_CHECK(on_device(ids, dev, at::kLong), who, ": ids must be contiguous int64 on the plan's GPU");
  const int64_t N = ids.numel();
  TORCH_CHECK(!vals.has_value() || (on_device(*vals, dev, at::kFloat) && vals->numel() == N), who,
              ": vals must be contiguous fp32 on the plan's GPU, one per id");
  TORCH_CHECK(!skip.has_value() || (on_device(*skip, dev, at::kInt) && skip->numel() >= 1), who,
              ": skip must be a device int32 word");
  TORCH_CHECK(lin_slots.size() <= 2 && row_slots.size() == lin_slots.size(), who,
              ": up to two slots per table, the same number for both");
  for (size_t i = 0; i < lin_slots.size(); ++i) {
    TORCH_CHECK(on_device(lin_slots[i], dev, at::kFloat) && lin_slots[i].numel() == rows, who,
                ": a slot of the linear table must be contiguous fp32 of the table's shape");
    TORCH_CHECK(on_device(row_slots[i], dev, at::kFloat) && row_slots[i].sizes() == row.sizes() &&
                    (reinterpret_cast<uintptr_t>(row_slots[i].data_ptr()) & 15) == 0,
                who, ": a slot of the row table must be contiguous fp32 of the table's shape, 16-byte aligned");
  }
  dtfk::tu::Args a{};
  a.kind = kind;
  a.h = optim_hyper(lr, hyper);
  a.width = (int)row.size(1);
  a.rows = rows;
  a.N = N;
  a.lin = lin.data_ptr<float>();
  a.row = row.data_ptr<float>();
  if (lin_slots.size() >= 1) a.lin_a = lin_slots[0].data_ptr<float>(), a.row_a = row_slots[0].data_ptr<float>();
  if (lin_slots.size() >= 2) a.lin_b = lin_slots[1].data_ptr<float>(), a.row_b = row_slots[1].data_ptr<float>();
  // the launcher's refusals, before the sort is launched
  TORCH_CHECK(dtfk::tu::values_ok(a), who,
              ": invalid argument (a row-local kind with its slots, FTRL hyper-parameters >= 0, a row width that is "
              "a multiple of 4 in 4 .. 128, fewer than 2^31 table rows and ids)");
  if (N == 0) return false;
  hipStream_t st = cur_stream();
  const UpdateScratch sc = prepare(N, st);
  // ids outside the table become -1 / rows: the two ends of the sorted order
  auto sorted = at::sort(at::clamp(ids, -1, rows).to(at::kInt), /*stable=*/true, 0, false);
  const at::Tensor sids = std::get<0>(sorted).contiguous(), perm = std::get<1>(sorted).contiguous();
  hip_check(dtfk_bag_index(offsets.data_ptr<int64_t>(), (int)B, sc.bag_of, N, st), who);
  a.sids = sids.data_ptr<int>();
  a.perm = reinterpret_cast<const long long*>(perm.data_ptr<int64_t>());
  a.bag_of = sc.bag_of;
  a.vals = opt_ptr<float>(vals);
  a.scale = sc.scale;
  a.dz = dz;
  a.demb = demb;
  a.part = sc.part;
  a.skip = opt_ptr<int>(skip);
  hip_check(launch(&a, st), who);
  return true;
}

}  // namespace dtf
