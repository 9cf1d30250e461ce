// The host libsvm parser's result type and the one entry point other native
// files use (csrc/bind_libsvm_gpu.cpp: the fallback of the GPU parser).  Plain C++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace dtf {
namespace libsvm {

struct CSR {
  std::vector<float> labels;
  std::vector<int64_t> row_ptr{0};
  std::vector<int64_t> ids;
  std::vector<float> vals;
  int64_t rows() const { return (int64_t)labels.size(); }
  void append(const CSR& o) {
    const int64_t base = (int64_t)ids.size();
    labels.insert(labels.end(), o.labels.begin(), o.labels.end());
    for (size_t i = 1; i < o.row_ptr.size(); ++i) row_ptr.push_back(base + o.row_ptr[i]);
    ids.insert(ids.end(), o.ids.begin(), o.ids.end());
    vals.insert(vals.end(), o.vals.begin(), o.vals.end());
  }
};

// Parses data[0, n) with strtof / strtoll, appending to `out`; data[n] must be readable
// and hold a byte no number continues into (NUL).  Line `first_ordinal + k`, k counting
// the '\n'-separated pieces, is kept iff lsv::keep(seed, ordinal, rate) (libsvm_rule.h);
// at rate 1 that is every line, as parse_buffer does.  Returns the number of pieces.
int64_t parse_buffer_hashed(const char* data, size_t n, double rate, uint64_t seed, int64_t first_ordinal, CSR& out,
                            int64_t* bad_lines);

}  // namespace libsvm
}  // namespace dtf
