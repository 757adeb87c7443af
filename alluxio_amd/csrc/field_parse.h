// Typed columns from a batch of delimited text rows, parsed where the batch lies: the kernel of
// field_parse.hip for a device batch, the loop of field_parse_host.h for a host batch (DRAM dirs,
// CPU-only use).  Both follow the rule in field_parse_host.h and give the same bytes.
#pragma once
#include <cstdint>
#include <vector>

#include "field_parse_host.h"

namespace amdx {

// Row r is data[off[r], off[r] + len[r]) (len: int32, or int64 with len_is_64); a row outside
// [0, data_bytes) is not read and gets status kFpBad in every column.  device < 0: all pointers
// are host memory and the call returns when the columns are written; otherwise they are memory of
// that device, the kernel is queued on `stream` and nothing is waited for.  nrows == 0 launches
// nothing.  Scalars outside their ranges (see launch_field_parse) throw
// StoreError(kErrInvalidArgument) before anything is launched or written.
void field_parse_raw(uint64_t data, uint64_t data_bytes, uint64_t off, uint64_t len, bool len_is_64, uint64_t nrows,
                     int device, uint32_t sep, int64_t quote, uint32_t terminator,
                     const std::vector<FieldParseCol>& cols, uint64_t stream);

// Kernel launches so far in this process (tests: a rejected call launches nothing).
uint64_t field_parse_launches();

}  // namespace amdx
