// The GPU libsvm parser's host side: libsvm_gpu_parse_into (the launcher on tensors the
// caller owns: capturable, nothing allocated) and LibsvmGpuParser (pinned staging, device
// text, workspace, one read-back per chunk, host fallback for an irregular chunk).
#include "bind_common.h"

#include <c10/hip/HIPFunctions.h>
#include <c10/hip/HIPGuard.h>

#include <cstring>

#include "kernels/libsvm_parse_api.h"
#include "runtime/libsvm_host.h"

namespace dtf {
namespace {

LsvPlan plan_or_throw(const char* who, int64_t n, int64_t batch_size, int64_t carry_rows) {
  require(n >= 0 && n < (1ll << 31), std::string(who) + ": a chunk holds 0 <= n < 2^31 bytes");
  require(batch_size >= 1, std::string(who) + ": batch_size must be at least 1");
  require(carry_rows >= 0 && carry_rows < batch_size, std::string(who) + ": 0 <= carry_rows < batch_size");
  LsvPlan p;
  require(dtfk_lsv_plan(n, batch_size, carry_rows, &p) != 0, std::string(who) + ": no plan");
  return p;
}

void check_rate(const char* who, double rate) {
  require(rate > 0.0 && rate <= 1.0, std::string(who) + ": sampling_rate must be in (0, 1]");
}

py::dict plan_dict(int64_t n, int64_t batch_size, int64_t carry_rows) {
  const LsvPlan p = plan_or_throw("libsvm_gpu_plan", n, batch_size, carry_rows);
  py::dict d;
  d["workspace_bytes"] = p.ws_bytes;
  d["rows"] = p.rows_cap;
  d["nnz"] = p.nnz_cap;
  d["batches"] = p.batch_cap;
  d["meta"] = p.meta_len;
  return d;
}

// Launches the parse of text[0, n) into the caller's tensors, all on text's GPU and each
// at least as large as libsvm_gpu_plan(n, ...) says: workspace (uint8), labels (f32),
// ids (i64), vals (f32), offsets (i64, batches * (batch_size + 1)), meta (i64).  Raises
// before any launch; synchronises nothing.
void parse_into(at::Tensor text, int64_t n, int64_t first_ordinal, uint64_t seed, double rate, int64_t batch_size,
                int64_t carry_rows, int64_t carry_nnz, at::Tensor workspace, at::Tensor labels, at::Tensor ids,
                at::Tensor vals, at::Tensor offsets, at::Tensor meta) {
  const char* who = "libsvm_gpu_parse_into";
  const LsvPlan p = plan_or_throw(who, n, batch_size, carry_rows);
  check_rate(who, rate);
  require(first_ordinal >= 0 && carry_nnz >= 0, std::string(who) + ": first_ordinal and carry_nnz must not be negative");
  need(text, at::kByte, std::max<int64_t>(n, 1), "text");
  need(workspace, at::kByte, p.ws_bytes, "workspace");
  need(labels, at::kFloat, p.rows_cap, "labels");
  need(ids, at::kLong, p.nnz_cap, "ids");
  need(vals, at::kFloat, p.nnz_cap, "vals");
  need(offsets, at::kLong, p.batch_cap * (batch_size + 1), "offsets");
  need(meta, at::kLong, p.meta_len, "meta");
  const auto dev = text.device();
  for (const at::Tensor* t : {&workspace, &labels, &ids, &vals, &offsets, &meta})
    require(t->device() == dev, std::string(who) + ": every tensor must be on the text's GPU");
  require(dev.index() == c10::hip::current_device(), std::string(who) + ": the tensors are not on the current GPU");
  hip_check(dtfk_lsv_parse(text.data_ptr<uint8_t>(), n, first_ordinal, seed, rate, batch_size, carry_rows, carry_nnz,
                           workspace.data_ptr(), workspace.numel(), labels.data_ptr<float>(), labels.numel(),
                           reinterpret_cast<long long*>(ids.data_ptr<int64_t>()), vals.data_ptr<float>(),
                           std::min(ids.numel(), vals.numel()),
                           reinterpret_cast<long long*>(offsets.data_ptr<int64_t>()),
                           offsets.numel() / (batch_size + 1), reinterpret_cast<long long*>(meta.data_ptr<int64_t>()),
                           meta.numel(), cur_stream()),
            who);
}

class LibsvmGpuParser {
 public:
  LibsvmGpuParser(int device, int64_t chunk_bytes, int64_t batch_size, double rate, uint64_t seed)
      : device_(device), cap_(chunk_bytes), bs_(batch_size), rate_(rate), seed_(seed) {
    const char* who = "LibsvmGpuParser";
    require(chunk_bytes >= 1 && chunk_bytes < (1ll << 31), std::string(who) + ": 1 <= chunk_bytes < 2^31");
    check_rate(who, rate);
    int ndev = 0;
    hip_check(hipGetDeviceCount(&ndev), who);
    require(device >= 0 && device < ndev, std::string(who) + ": no such GPU");
    // the largest plan over the carried rows a chunk can meet (carry_rows < batch_size)
    const LsvPlan p = plan_or_throw(who, chunk_bytes, batch_size, batch_size - 1);
    c10::hip::HIPGuard guard(device_);
    const auto bytes = at::TensorOptions().dtype(at::kByte).device(at::kCUDA, device_);
    text_ = at::empty({cap_ + 64}, bytes);
    ws_ = at::empty({p.ws_bytes}, bytes);
    for (int s = 0; s < 2; ++s)
      hip_check(hipHostMalloc(&stage_[s], (size_t)cap_ + 64, hipHostMallocDefault), "LibsvmGpuParser: pinned staging");
    hip_check(hipHostMalloc(reinterpret_cast<void**>(&hmeta_), 8 * kHostMeta, hipHostMallocDefault),
              "LibsvmGpuParser: pinned record");
  }
  ~LibsvmGpuParser() {
    for (int s = 0; s < 2; ++s)
      if (stage_[s]) (void)hipHostFree(stage_[s]);
    if (hmeta_) (void)hipHostFree(hmeta_);
  }
  LibsvmGpuParser(const LibsvmGpuParser&) = delete;
  LibsvmGpuParser& operator=(const LibsvmGpuParser&) = delete;

  // pinned staging buffer `slot` as a CPU uint8 tensor [chunk_bytes] (a reader fills it in place)
  at::Tensor staging(int slot) {
    require(slot == 0 || slot == 1, "LibsvmGpuParser.staging: slot is 0 or 1");
    return at::from_blob(stage_[slot], {cap_}, at::TensorOptions().dtype(at::kByte));
  }

  // data: bytes (copied into the next pinned slot) or a slot number whose first `nbytes`
  // bytes a reader filled.  Returns (labels [R], offsets [batches, batch_size + 1], ids,
  // vals, bases (host int64 [batches + 1]), rows, nnz, lines, irregular, bad_lines).
  py::tuple parse(py::object data, int64_t first_ordinal, int64_t nbytes, int64_t carry_rows, int64_t carry_nnz) {
    const char* who = "LibsvmGpuParser.parse";
    int slot;
    int64_t n;
    std::string copy;
    const bool is_bytes = py::isinstance<py::bytes>(data);
    if (is_bytes) {
      copy = data.cast<std::string>();
      n = (int64_t)copy.size();
      slot = next_ ^= 1;
    } else {
      slot = data.cast<int>();
      n = nbytes;
      require(slot == 0 || slot == 1, std::string(who) + ": slot is 0 or 1");
    }
    require(n >= 0 && n < (1ll << 31), std::string(who) + ": a chunk holds 0 <= n < 2^31 bytes");
    require(n <= cap_, std::string(who) + ": the chunk is larger than chunk_bytes");
    require(first_ordinal >= 0 && carry_nnz >= 0, std::string(who) + ": first_ordinal and carry_nnz must not be negative");
    const LsvPlan p = plan_or_throw(who, n, bs_, carry_rows);
    c10::hip::HIPGuard guard(device_);
    char* h = static_cast<char*>(stage_[slot]);
    if (is_bytes) std::memcpy(h, copy.data(), (size_t)n);
    h[n] = '\0';                                  // the host fallback's terminator
    const auto f32 = at::TensorOptions().dtype(at::kFloat).device(at::kCUDA, device_);
    const auto i64 = f32.dtype(at::kLong);
    at::Tensor labels = at::empty({p.rows_cap}, f32), ids = at::empty({p.nnz_cap}, i64);
    at::Tensor vals = at::empty({p.nnz_cap}, f32), offsets = at::empty({p.batch_cap, bs_ + 1}, i64);
    at::Tensor meta = at::empty({p.meta_len}, i64);
    const int64_t back = std::min<int64_t>(p.meta_len, kHostMeta);
    hipStream_t st = cur_stream();
    {
      py::gil_scoped_release nogil;
      if (n) hip_check(hipMemcpyAsync(text_.data_ptr(), h, (size_t)n, hipMemcpyHostToDevice, st), "text copy");
      hip_check(dtfk_lsv_parse(text_.data_ptr<uint8_t>(), n, first_ordinal, seed_, rate_, bs_, carry_rows, carry_nnz,
                               ws_.data_ptr(), ws_.numel(), labels.data_ptr<float>(), labels.numel(),
                               reinterpret_cast<long long*>(ids.data_ptr<int64_t>()), vals.data_ptr<float>(),
                               ids.numel(), reinterpret_cast<long long*>(offsets.data_ptr<int64_t>()), p.batch_cap,
                               reinterpret_cast<long long*>(meta.data_ptr<int64_t>()), meta.numel(), st),
                who);
      hip_check(hipMemcpyAsync(hmeta_, meta.data_ptr(), 8 * (size_t)back, hipMemcpyDeviceToHost, st), "record copy");
      hip_check(hipStreamSynchronize(st), who);   // the one read-back of the chunk
    }
    const int64_t lines = hmeta_[LSV_LINES];
    if (hmeta_[LSV_IRREGULAR]) return fallback(h, n, first_ordinal, carry_rows, carry_nnz);
    ++gpu_chunks_;
    const int64_t rows = hmeta_[LSV_ROWS], nnz = hmeta_[LSV_NNZ], nb = hmeta_[LSV_BATCHES];
    at::Tensor bases;
    if (LSV_META_HEAD + nb + 1 <= back) {
      bases = at::empty({nb + 1}, at::TensorOptions().dtype(at::kLong));
      std::memcpy(bases.data_ptr(), hmeta_ + LSV_META_HEAD, 8 * (size_t)(nb + 1));
    } else {
      bases = meta.narrow(0, LSV_META_HEAD, nb + 1).cpu();
    }
    return py::make_tuple(labels.narrow(0, 0, rows), offsets.narrow(0, 0, nb), ids.narrow(0, 0, nnz),
                          vals.narrow(0, 0, nnz), bases, rows, nnz, lines, false, (int64_t)0);
  }

  int64_t gpu_chunks() const { return gpu_chunks_; }
  int64_t fallback_chunks() const { return fallback_chunks_; }
  int64_t bad_lines() const { return bad_lines_; }
  int64_t chunk_bytes() const { return cap_; }
  int64_t batch_size() const { return bs_; }

 private:
  // the chunk again, on the host with libc (the existing parser; the hashed sample at rate < 1),
  // laid out as the kernels lay it out, then uploaded
  py::tuple fallback(const char* h, int64_t n, int64_t first_ordinal, int64_t carry_rows, int64_t carry_nnz) {
    ++fallback_chunks_;
    libsvm::CSR c;
    int64_t bad = 0, lines = 0;
    const int64_t bs = bs_;
    at::Tensor hl, ho, hi, hv, bases;
    int64_t rows = 0, nnz = 0;
    {
      py::gil_scoped_release nogil;
      lines = libsvm::parse_buffer_hashed(h, (size_t)n, rate_, seed_, first_ordinal, c, &bad);
      rows = c.rows();
      nnz = (int64_t)c.ids.size();
    }
    bad_lines_ += bad;
    const int64_t nb = rows > 0 ? (rows + carry_rows + bs - 1) / bs : 0;
    hl = at::empty({rows}, at::TensorOptions().dtype(at::kFloat));
    hi = at::empty({nnz}, at::TensorOptions().dtype(at::kLong));
    hv = at::empty({nnz}, at::TensorOptions().dtype(at::kFloat));
    ho = at::zeros({nb, bs + 1}, at::TensorOptions().dtype(at::kLong));
    bases = at::empty({nb + 1}, at::TensorOptions().dtype(at::kLong));
    if (rows) std::memcpy(hl.data_ptr(), c.labels.data(), 4 * (size_t)rows);
    if (nnz) {
      std::memcpy(hi.data_ptr(), c.ids.data(), 8 * (size_t)nnz);
      std::memcpy(hv.data_ptr(), c.vals.data(), 4 * (size_t)nnz);
    }
    int64_t* o = ho.data_ptr<int64_t>();
    int64_t* b = bases.data_ptr<int64_t>();
    for (int64_t k = 0; k < nb; ++k) {
      const int64_t br = std::max<int64_t>(k * bs - carry_rows, 0);
      const int64_t base = c.row_ptr[std::min(br, rows)];
      b[k] = base;
      for (int64_t j = 0; j <= bs; ++j) {
        const int64_t q = k * bs + j - carry_rows;
        o[k * (bs + 1) + j] = q < 0 ? 0 : c.row_ptr[std::min(q, rows)] - base + (k == 0 ? carry_nnz : 0);
      }
    }
    b[nb] = nnz;
    const auto dev = at::Device(at::kCUDA, device_);
    return py::make_tuple(hl.to(dev), ho.to(dev), hi.to(dev), hv.to(dev), bases, rows, nnz, lines, true, bad);
  }

  static constexpr int64_t kHostMeta = 4096;
  int device_;
  int64_t cap_, bs_;
  double rate_;
  uint64_t seed_;
  at::Tensor text_, ws_;
  void* stage_[2] = {nullptr, nullptr};
  int64_t* hmeta_ = nullptr;
  int next_ = 0;
  int64_t gpu_chunks_ = 0, fallback_chunks_ = 0, bad_lines_ = 0;
};

}  // namespace

void init_libsvm_gpu(py::module& m) {
  m.attr("LIBSVM_GPU_TILE") = dtfk_lsv_tile_bytes();
  m.def("libsvm_gpu_plan", &plan_dict, py::arg("n"), py::arg("batch_size"), py::arg("carry_rows") = 0);
  m.def("libsvm_gpu_parse_into", &parse_into, py::arg("text"), py::arg("n"), py::arg("first_ordinal"), py::arg("seed"),
        py::arg("sampling_rate"), py::arg("batch_size"), py::arg("carry_rows"), py::arg("carry_nnz"),
        py::arg("workspace"), py::arg("labels"), py::arg("ids"), py::arg("vals"), py::arg("offsets"), py::arg("meta"));
  py::class_<LibsvmGpuParser>(m, "LibsvmGpuParser")
      .def(py::init<int, int64_t, int64_t, double, uint64_t>(), py::arg("device"), py::arg("chunk_bytes"),
           py::arg("batch_size"), py::arg("sampling_rate") = 1.0, py::arg("seed") = 0)
      .def("staging", &LibsvmGpuParser::staging, py::arg("slot"))
      .def("parse", &LibsvmGpuParser::parse, py::arg("data"), py::arg("first_ordinal") = 0, py::arg("nbytes") = 0,
           py::arg("carry_rows") = 0, py::arg("carry_nnz") = 0)
      .def_property_readonly("gpu_chunks", &LibsvmGpuParser::gpu_chunks)
      .def_property_readonly("fallback_chunks", &LibsvmGpuParser::fallback_chunks)
      .def_property_readonly("bad_lines", &LibsvmGpuParser::bad_lines)
      .def_property_readonly("chunk_bytes", &LibsvmGpuParser::chunk_bytes)
      .def_property_readonly("batch_size", &LibsvmGpuParser::batch_size);
}

}  // namespace dtf
