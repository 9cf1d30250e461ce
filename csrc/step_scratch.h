// The scratch of a one-GPU training step's plan (bind_fm.cpp FMPlan, bind_deepfm.cpp
// DeepFMPlan, bind_ffm.cpp FFMPlan, bind_wide_deep.cpp WideDeepTrainPlan): two tensors that grow only
// when a batch exceeds them and never inside a stream capture (a captured graph
// holds the addresses; an outgrown tensor is kept alive for the graphs that hold it).
//   rows:   one part of [capacity, width] floats per entry of `widths`, after each other
//   update: scale [bag capacity] (only with bag_scale) | bag_of [ids capacity] (int) | part (kernels/table_update.h)
// Capacities are multiples of 1024, so every part starts 16-byte aligned.
#pragma once
#include "bind_common.h"
#include "kernels/table_update.h"

#include <algorithm>
#include <utility>
#include <vector>

namespace dtf {

class StepScratch {
 public:
  // who: the plan's name in messages; update_width: the tables' row width
  void init(const char* who, std::vector<int> widths, int update_width, bool bag_scale) {
    who_ = who;
    widths_ = std::move(widths);
    off_.assign(1, 0);
    for (int w : widths_) off_.push_back(off_.back() + w);
    update_width_ = update_width;
    bag_scale_ = bag_scale;
  }

  // rows for a batch of B; ids > 0 also sizes the update tensor
  void reserve(int64_t B, int64_t ids, const at::TensorOptions& f32) {
    const bool rows_ok = rows_.defined() && cap_ >= B;
    const bool ids_ok = ids <= 0 || (upd_.defined() && ucap_ >= ids && (!bag_scale_ || ubag_ >= B));
    if (rows_ok && ids_ok) return;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    hip_check(hipStreamIsCapturing(cur_stream(), &cs), who_);
    TORCH_CHECK(cs == hipStreamCaptureStatusNone, who_,
                ": the scratch cannot grow inside a stream capture; reserve(rows, ids) before it");
    if (!rows_ok) {
      if (rows_.defined()) old_.push_back(rows_);
      cap_ = round_up(B);
      rows_ = at::empty({cap_ * row_floats()}, f32);
    }
    if (!ids_ok) {
      if (upd_.defined()) old_.push_back(upd_);
      ucap_ = round_up(ids);
      ubag_ = bag_scale_ ? round_up(B) : 0;
      upd_ = at::empty({ubag_ + ucap_ + dtfk::tu::part_floats(ucap_, update_width_)}, f32);
    }
  }

  int64_t row_floats() const { return off_.back(); }
  const at::Tensor& rows() const { return rows_; }
  // part k of the rows tensor; view: its first B rows, [B, width]
  float* part(int k) const { return rows_.data_ptr<float>() + cap_ * off_[k]; }
  at::Tensor view(int k, int64_t B) const {
    TORCH_CHECK(rows_.defined() && B > 0, who_, ": no batch yet");
    return rows_.narrow(0, cap_ * off_[k], B * widths_[k]).view({B, widths_[k]});
  }
  // the parts of the update tensor (scale: only with bag_scale)
  float* scale() const { return upd_.data_ptr<float>(); }
  int* bag_of() const { return reinterpret_cast<int*>(upd_.data_ptr<float>() + ubag_); }
  float* update_part() const { return upd_.data_ptr<float>() + ubag_ + ucap_; }

 private:
  static int64_t round_up(int64_t n) { return (std::max<int64_t>(n, 1024) + 1023) / 1024 * 1024; }

  const char* who_ = "";
  std::vector<int> widths_;
  std::vector<int64_t> off_{0};
  at::Tensor rows_, upd_;
  std::vector<at::Tensor> old_;
  int64_t cap_ = 0, ucap_ = 0, ubag_ = 0;
  int update_width_ = 0;
  bool bag_scale_ = false;
};

}  // namespace dtf
