// The host entry points of the GPU libsvm parser (libsvm_parse.hip), declared once:
// csrc/bind_libsvm_gpu.cpp calls through these declarations and libsvm_parse.hip includes
// them.  Host-only: no device code here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// What a chunk of n text bytes needs, from n, the batch size and the carried rows alone:
// a kept line is at least 3 bytes with its newline and an entry at least 4.
struct LsvPlan {
  long long ws_bytes;      // workspace
  long long rows_cap;      // labels [rows_cap] f32
  long long nnz_cap;       // ids [nnz_cap] i64, vals [nnz_cap] f32
  long long batch_cap;     // offsets [batch_cap, batch_size + 1] i64
  long long meta_len;      // meta [LSV_META_HEAD + batch_cap + 1] i64: the record, then the batch bases
};

// the record at the head of `meta` (int64 words)
enum { LSV_ROWS = 0, LSV_NNZ = 1, LSV_IRREGULAR = 2, LSV_LINES = 3, LSV_VALID_LINES = 4, LSV_COLONS = 5,
       LSV_BATCHES = 6, LSV_META_HEAD = 8 };

extern "C" {

int dtfk_lsv_tile_bytes(void);
// false (and no plan) when n, batch_size or carry_rows is out of range
int dtfk_lsv_plan(long long n, long long batch_size, long long carry_rows, LsvPlan* plan);
// Parses text[0, n) into device CSR cut into batches of batch_size rows; the first batch
// is short by carry_rows (rows a caller carries over from the chunk before) and its offsets
// start at carry_nnz.  Every buffer is at least as large as dtfk_lsv_plan says for n;
// hipErrorInvalidValue, with nothing launched, otherwise.  No allocation, no
// synchronisation, no memset node: capturable.
hipError_t dtfk_lsv_parse(const unsigned char* text, long long n, long long first_ordinal, unsigned long long seed,
                          double rate, long long batch_size, long long carry_rows, long long carry_nnz, void* ws,
                          long long ws_bytes, float* labels, long long rows_cap, long long* ids, float* vals,
                          long long nnz_cap, long long* offsets, long long batch_cap, long long* meta,
                          long long meta_len, hipStream_t stream);

}  // extern "C"
