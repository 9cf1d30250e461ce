// Native RCCL communicator (data plane for sync data parallelism over xGMI).
//
// Replaces the reference's implicit gRPC Send/Recv between /job:worker and
// /job:ps (example.py:64-67 replica_device_setter) with RCCL
// collectives issued directly on the caller's HIP stream, so they can be
// captured into a hipGraph together with the compute kernels of a step.
// Bootstrap (unique-id exchange) is done by the Python control plane over
// the TCP store; this file only owns the communicator.
#include "bind_common.h"

#include <rccl/rccl.h>

#include <chrono>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace dtf {

#define RCCL_CHECK(cmd)                                                              \
  do {                                                                               \
    ncclResult_t r_ = (cmd);                                                         \
    if (r_ != ncclSuccess)                                                           \
      throw std::runtime_error(std::string("RCCL error ") + ncclGetErrorString(r_) + \
                               " at " #cmd);                                         \
  } while (0)

// calls on a non-blocking communicator may return ncclInProgress: wait for the
// communicator to settle (bounded by the init timeout)
#define RCCL_CALL(cmd)                                                               \
  do {                                                                               \
    ncclResult_t r_ = (cmd);                                                         \
    if (r_ == ncclInProgress && nonblocking_) r_ = poll_(timeout_s_);                \
    if (r_ != ncclSuccess)                                                           \
      throw std::runtime_error(std::string("RCCL error ") + ncclGetErrorString(r_) + \
                               " at " #cmd);                                         \
  } while (0)

static ncclDataType_t to_nccl(at::ScalarType t) {
  switch (t) {
    case at::kFloat: return ncclFloat32;
    case at::kBFloat16: return ncclBfloat16;
    case at::kHalf: return ncclFloat16;
    case at::kDouble: return ncclFloat64;
    case at::kInt: return ncclInt32;
    case at::kLong: return ncclInt64;
    case at::kByte: return ncclUint8;
    case at::kChar: return ncclInt8;
    default: throw std::runtime_error("unsupported dtype for RCCL");
  }
}

static ncclRedOp_t to_op(const std::string& op) {
  if (op == "sum") return ncclSum;
  if (op == "max") return ncclMax;
  if (op == "min") return ncclMin;
  if (op == "prod") return ncclProd;
  if (op == "avg") return ncclAvg;
  throw std::runtime_error("unknown reduce op " + op);
}

py::bytes rccl_unique_id() {
  ncclUniqueId id;
  RCCL_CHECK(ncclGetUniqueId(&id));
  return py::bytes(reinterpret_cast<const char*>(&id), sizeof(id));
}

int rccl_version() {
  int v = 0;
  ncclGetVersion(&v);
  return v;
}

class RcclComm {
 public:
  // timeout_s > 0: non-blocking init (ncclCommInitRankConfig, blocking = 0)
  // polled until it completes, aborted after timeout_s -- a peer that never
  // arrives or a fabric that never comes up ends in an exception, not a hang.
  // The communicator then stays non-blocking: every call is followed by wait_()
  // (a call may return ncclInProgress while RCCL finishes its host-side work).
  RcclComm(py::bytes uid, int nranks, int rank, double timeout_s = 0.0) : nranks_(nranks), rank_(rank) {
    std::string s = uid;
    if (s.size() != sizeof(ncclUniqueId)) throw std::runtime_error("bad unique id size");
    ncclUniqueId id;
    memcpy(&id, s.data(), sizeof(id));
    if (timeout_s <= 0.0) {
      RCCL_CHECK(ncclCommInitRank(&comm_, nranks, id, rank));
      return;
    }
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    nonblocking_ = true;
    timeout_s_ = timeout_s;
    ncclResult_t r;
    {
      py::gil_scoped_release nogil;
      r = ncclCommInitRankConfig(&comm_, nranks, id, rank, &cfg);
      if (r == ncclInProgress || (r == ncclSuccess && comm_ != nullptr)) r = poll_(timeout_s);
    }
    if (r != ncclSuccess) {
      if (comm_) ncclCommAbort(comm_);
      comm_ = nullptr;
      throw std::runtime_error(std::string("RCCL init failed: ") +
                               (r == ncclInProgress ? "timed out" : ncclGetErrorString(r)));
    }
  }
  ~RcclComm() {
    if (comm_) ncclCommDestroy(comm_);
  }
  int rank() const { return rank_; }
  int size() const { return nranks_; }

  void all_reduce(at::Tensor t, const std::string& op) {
    check(t);
    RCCL_CALL(ncclAllReduce(t.data_ptr(), t.data_ptr(), t.numel(), to_nccl(t.scalar_type()),
                             to_op(op), comm_, cur_stream()));
  }
  void all_reduce_out(at::Tensor src, at::Tensor dst, const std::string& op) {
    check(src); check(dst);
    RCCL_CALL(ncclAllReduce(src.data_ptr(), dst.data_ptr(), src.numel(),
                             to_nccl(src.scalar_type()), to_op(op), comm_, cur_stream()));
  }
  void broadcast(at::Tensor t, int root) {
    check(t);
    RCCL_CALL(ncclBroadcast(t.data_ptr(), t.data_ptr(), t.numel(), to_nccl(t.scalar_type()), root,
                             comm_, cur_stream()));
  }
  // dst holds nranks * src.numel() elements
  void all_gather(at::Tensor src, at::Tensor dst) {
    check(src); check(dst);
    if (dst.numel() != src.numel() * nranks_) throw std::runtime_error("all_gather size mismatch");
    RCCL_CALL(ncclAllGather(src.data_ptr(), dst.data_ptr(), src.numel(),
                             to_nccl(src.scalar_type()), comm_, cur_stream()));
  }
  // src holds nranks * dst.numel() elements
  void reduce_scatter(at::Tensor src, at::Tensor dst, const std::string& op) {
    check(src); check(dst);
    if (src.numel() != dst.numel() * nranks_) throw std::runtime_error("reduce_scatter size mismatch");
    RCCL_CALL(ncclReduceScatter(src.data_ptr(), dst.data_ptr(), dst.numel(),
                                 to_nccl(src.scalar_type()), to_op(op), comm_, cur_stream()));
  }
  // Variable-split all-to-all over grouped point-to-point (each xGMI peer link
  // carries exactly its pair's bytes). Counts are in elements, per rank.
  void all_to_all(at::Tensor src, std::vector<int64_t> send_counts, at::Tensor dst,
                  std::vector<int64_t> recv_counts) {
    check(src); check(dst);
    if ((int)send_counts.size() != nranks_ || (int)recv_counts.size() != nranks_)
      throw std::runtime_error("all_to_all counts must have nranks entries");
    const auto dt = to_nccl(src.scalar_type());
    const size_t es = src.element_size();
    char* s = reinterpret_cast<char*>(src.data_ptr());
    char* d = reinterpret_cast<char*>(dst.data_ptr());
    int64_t so = 0, ro = 0;
    hipStream_t st = cur_stream();
    RCCL_CALL(ncclGroupStart());
    for (int p = 0; p < nranks_; ++p) {
      if (send_counts[p] > 0) RCCL_CALL(ncclSend(s + so * es, send_counts[p], dt, p, comm_, st));
      if (recv_counts[p] > 0) RCCL_CALL(ncclRecv(d + ro * es, recv_counts[p], dt, p, comm_, st));
      so += send_counts[p];
      ro += recv_counts[p];
    }
    RCCL_CALL(ncclGroupEnd());
  }
  void send(at::Tensor t, int peer) {
    check(t);
    RCCL_CALL(ncclSend(t.data_ptr(), t.numel(), to_nccl(t.scalar_type()), peer, comm_, cur_stream()));
  }
  void recv(at::Tensor t, int peer) {
    check(t);
    RCCL_CALL(ncclRecv(t.data_ptr(), t.numel(), to_nccl(t.scalar_type()), peer, comm_, cur_stream()));
  }
  bool nonblocking() const { return nonblocking_; }
  void abort() {
    if (comm_) {
      ncclCommAbort(comm_);
      comm_ = nullptr;
    }
  }
  std::string async_error() {
    if (!comm_) return "aborted";
    ncclResult_t r = ncclSuccess;
    ncclCommGetAsyncError(comm_, &r);
    return r == ncclSuccess ? "" : ncclGetErrorString(r);
  }

 private:
  void check(const at::Tensor& t) const {
    if (!comm_) throw std::runtime_error("communicator aborted");
    if (!t.is_cuda()) throw std::runtime_error("RCCL tensors must live on the GPU");
    if (!t.is_contiguous()) throw std::runtime_error("RCCL tensors must be contiguous");
  }
  // wait until the communicator's pending host-side work settled: ncclSuccess,
  // an error, or ncclInProgress after timeout_s
  ncclResult_t poll_(double timeout_s) const {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
      ncclResult_t r = ncclSuccess;
      const ncclResult_t q = ncclCommGetAsyncError(comm_, &r);
      if (q != ncclSuccess) return q;
      if (r != ncclInProgress) return r;
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
        return ncclInProgress;
      std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
  }
  ncclComm_t comm_ = nullptr;
  int nranks_, rank_;
  bool nonblocking_ = false;
  double timeout_s_ = 0.0;
};

void init_comm(py::module& m) {
  m.def("rccl_unique_id", &rccl_unique_id);
  m.def("rccl_version", &rccl_version);
  py::class_<RcclComm>(m, "RcclComm")
      .def(py::init<py::bytes, int, int, double>(), py::arg("uid"), py::arg("nranks"), py::arg("rank"),
           py::arg("timeout_s") = 0.0)
      .def("nonblocking", &RcclComm::nonblocking)
      .def("rank", &RcclComm::rank)
      .def("size", &RcclComm::size)
      .def("all_reduce", &RcclComm::all_reduce)
      .def("all_reduce_out", &RcclComm::all_reduce_out)
      .def("broadcast", &RcclComm::broadcast)
      .def("all_gather", &RcclComm::all_gather)
      .def("reduce_scatter", &RcclComm::reduce_scatter)
      .def("all_to_all", &RcclComm::all_to_all)
      .def("send", &RcclComm::send)
      .def("recv", &RcclComm::recv)
      .def("abort", &RcclComm::abort)
      .def("async_error", &RcclComm::async_error);
}

}  // namespace dtf
