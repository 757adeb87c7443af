// Text columns from the spans of a batch of delimited text: the unquoted bytes of every value,
// packed, produced where the batch lies: the kernels of text_column.hip for a device batch, the
// loops of text_column_host.h for a host batch (DRAM dirs, CPU-only use).  Both follow the rule in
// text_column_host.h and give the same bytes.
#pragma once
#include <cstdint>

#include "text_column_host.h"

namespace amdx {

// Value r is data[start[r], start[r] + length[r]) (int64 starts, int32 lengths); status (0: none)
// is the span column's status array.  device < 0: all pointers are host memory and the call returns
// when its output is written; otherwise they are memory of that device, the kernel is queued on
// `stream` and nothing is waited for.  n == 0 launches nothing.  A quote outside -1..255, more than
// 2^31 values or a null array with n > 0 throw StoreError(kErrInvalidArgument) before anything is
// launched or written.
//
// measure: out_len[r] (int32) = the output length of value r, 0 for a value that is not live.
void text_measure_raw(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status, uint64_t n,
                      int device, int64_t quote, uint64_t out_len, uint64_t stream);
// emit: offsets (int64, n + 1) is the exclusive scan of out_len; value r goes to out[offsets[r] ...]
// and nothing is written outside [offsets[r], offsets[r + 1]) cut to [0, out_bytes).
void text_emit_raw(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status, uint64_t n,
                   int device, int64_t quote, uint64_t offsets, uint64_t out, uint64_t out_bytes, uint64_t stream);

// Kernel launches so far in this process (tests: a rejected or empty call launches nothing).
uint64_t text_column_launches();

}  // namespace amdx
