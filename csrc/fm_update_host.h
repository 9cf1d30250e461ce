// The table half of a training step that ends in kernels/fm.hip's one-writer update,
// as bind_fm.cpp FMPlan.update and bind_deepfm.cpp DeepFMPlan.update run it: the
// checks, one stable sort of the batch's ids, bag_index, then dtfk_fm_update with
// the plan's dz / demb.  `who` prefixes the messages; every refusal raises before
// anything is launched.
#pragma once
#include "bind_common.h"
#include "eval_record_host.h"
#include "kernels/fm.h"
#include "kernels/ops_api.h"

#include <utility>
#include <vector>

namespace dtf {

// w [F], V [F, K] and their slots take rule `kind` with the last rows() batch's dz [B] / demb [B, K].
// scratch(N): called once after the checks (the plan grows its update scratch there) and returns
// (bag_of [>= N] ints, part [>= dtfk_fm_update_part_floats(N, K)] floats, 16-byte aligned).
// Returns false when the batch has no ids (nothing was launched).
template <class Scratch>
inline bool fm_update_host(const char* who, const at::Tensor& w, const at::Tensor& V, int64_t B,
                           const at::Tensor& offsets, const at::Tensor& ids, const c10::optional<at::Tensor>& vals,
                           int kind, double lr, const std::vector<at::Tensor>& w_slots,
                           const std::vector<at::Tensor>& V_slots, const py::kwargs& hyper, const float* dz,
                           const float* demb, Scratch&& scratch) {
  const int dev = V.get_device();
  const int64_t F = V.size(0), K = V.size(1);
  TORCH_CHECK(B > 0, who, ": no batch yet (rows() first)");
  TORCH_CHECK(on_device(offsets, dev, at::kLong) && offsets.numel() == B + 1, who,
              ": offsets must be contiguous int64 on the plan's GPU, B + 1 entries of the last rows() batch");
  TORCH_CHECK(on_device(ids, dev, at::kLong), who, ": ids must be contiguous int64 on the plan's GPU");
  const int64_t N = ids.numel();
  TORCH_CHECK(!vals.has_value() || (on_device(*vals, dev, at::kFloat) && vals->numel() == N), who,
              ": vals must be contiguous fp32 on the plan's GPU, one per id");
  TORCH_CHECK(w_slots.size() <= 2 && V_slots.size() == w_slots.size(), who,
              ": up to two slots per table, the same number for both");
  for (size_t i = 0; i < w_slots.size(); ++i) {
    TORCH_CHECK(on_device(w_slots[i], dev, at::kFloat) && w_slots[i].numel() == F, who,
                ": a slot of w must be contiguous fp32 of the table's shape");
    TORCH_CHECK(on_device(V_slots[i], dev, at::kFloat) && V_slots[i].sizes() == V.sizes() &&
                    (reinterpret_cast<uintptr_t>(V_slots[i].data_ptr()) & 15) == 0,
                who, ": a slot of V must be contiguous fp32 of the table's shape, 16-byte aligned");
  }
  dtfk::fm::UpdArgs a{};
  a.kind = kind;
  a.h = optim_hyper(lr, hyper);
  a.K = (int)K;
  a.F = F;
  a.N = N;
  a.w = w.data_ptr<float>();
  a.V = V.data_ptr<float>();
  if (w_slots.size() >= 1) a.w_a = w_slots[0].data_ptr<float>(), a.V_a = V_slots[0].data_ptr<float>();
  if (w_slots.size() >= 2) a.w_b = w_slots[1].data_ptr<float>(), a.V_b = V_slots[1].data_ptr<float>();
  // the launcher's refusals, before the sort is launched
  TORCH_CHECK(dtfk::row_local(kind) && !(dtfk::uses_slot_a(kind) && a.w_a == nullptr) &&
                  !(dtfk::uses_slot_b(kind) && a.w_b == nullptr) &&
                  !(kind == dtfk::OPT_FTRL && !dtfk::ftrl_hyper_ok(a.h)) && F < (int64_t(1) << 31) &&
                  N < (int64_t(1) << 31),
              who, ": invalid argument (a row-local kind with its slots, FTRL hyper-parameters >= 0, fewer than "
              "2^31 table rows and ids)");
  if (N == 0) return false;
  const std::pair<int*, float*> sc = scratch(N);
  hipStream_t st = cur_stream();
  // ids outside the table become -1 / F: the two ends of the sorted order
  auto sorted = at::sort(at::clamp(ids, -1, F).to(at::kInt), /*stable=*/true, 0, false);
  const at::Tensor sids = std::get<0>(sorted).contiguous(), perm = std::get<1>(sorted).contiguous();
  hip_check(dtfk_bag_index(offsets.data_ptr<int64_t>(), (int)B, sc.first, N, st), who);
  a.sids = sids.data_ptr<int>();
  a.perm = reinterpret_cast<const long long*>(perm.data_ptr<int64_t>());
  a.bag_of = sc.first;
  a.vals = opt_ptr<float>(vals);
  a.dz = dz;
  a.demb = demb;
  a.part = sc.second;
  hip_check(dtfk_fm_update(&a, st), who);
  return true;
}

}  // namespace dtf
