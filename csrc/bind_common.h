// What every binding file needs around a launcher call, defined once: the current stream,
// the HIP error thrower, the tensor requirement checks and the optional-tensor pointers.
// One name per meaning; a helper that only one file uses stays in that file.
#pragma once
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

namespace dtf {

// the stream PyTorch is issuing on: every launcher runs there
inline hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

// a failed HIP call or launch is an error: "<what>: <HIP's message>"
inline void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

// condition or throw: size and range refusals, raised before any launch
inline void require(bool ok, const char* what) {
  if (!ok) throw std::runtime_error(what);
}
inline void require(bool ok, const std::string& what) {
  if (!ok) throw std::runtime_error(what);
}

inline void need_gpu(const at::Tensor& t, const char* name) {
  if (!t.is_cuda()) throw std::runtime_error(std::string(name) + " must be a GPU tensor");
}

// a contiguous GPU tensor of dtype `dt`
inline void need(const at::Tensor& t, at::ScalarType dt, const char* name) {
  need_gpu(t, name);
  if (!t.is_contiguous()) throw std::runtime_error(std::string(name) + " must be contiguous");
  if (t.scalar_type() != dt) throw std::runtime_error(std::string(name) + " must be " + c10::toString(dt));
}
// ... of at least `numel` elements (numel < 0: any size)
inline void need(const at::Tensor& t, at::ScalarType dt, int64_t numel, const char* name) {
  need(t, dt, name);
  if (numel >= 0 && t.numel() < numel)
    throw std::runtime_error(std::string(name) + " too small: " + std::to_string(t.numel()) + " < " +
                             std::to_string(numel));
}

// the data pointer of an optional tensor, null when it is absent (opt_ptr<float>(bias); untyped: opt_ptr(res))
template <typename T>
inline T* opt_ptr(const c10::optional<at::Tensor>& t) {
  return t.has_value() ? t->data_ptr<T>() : nullptr;
}
inline void* opt_ptr(const c10::optional<at::Tensor>& t) { return t.has_value() ? t->data_ptr() : nullptr; }

}  // namespace dtf
