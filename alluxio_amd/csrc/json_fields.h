// Typed columns from a batch of JSON Lines rows, produced where the batch lies: the kernels of
// json_fields.hip for a device batch, the loops of json_fields_host.h and json_text_host.h for a
// host batch (DRAM dirs, CPU-only use).  Both follow the rules in those headers and give the same
// bytes.
#pragma once
#include <cstdint>
#include <vector>

#include "json_fields_host.h"
#include "json_text_host.h"

namespace amdx {

// Locate: row r is data[off[r], off[r] + len[r]) (len: int32, or int64 with len_is_64); a row
// outside [0, data_bytes) is not read and gets status 2 in every column.  names: the requested
// names end to end (names_bytes of them), each column pointing into it.  device < 0: all pointers
// are host memory and the call returns when the columns are written; otherwise they are memory of
// that device, the kernel is queued on `stream` and nothing is waited for.  nrows == 0 launches
// nothing.  A terminator above 255, a column count outside 1..32, an unknown type, a name length
// outside 1..255 or a name outside the buffer throw StoreError(kErrInvalidArgument) before
// anything is launched or written.
void json_fields_raw(uint64_t data, uint64_t data_bytes, uint64_t off, uint64_t len, bool len_is_64, uint64_t nrows,
                     int device, uint64_t names, uint64_t names_bytes, uint32_t terminator,
                     const std::vector<JsonFieldsCol>& cols, uint64_t stream);

// Unescape: value r is data[start[r], start[r] + length[r]) (int64 starts, int32 lengths), the
// content of a JSON string; status (0: none) is the string column's status array.  measure writes
// out_len[r] (int32) and out_status[r] (uint8); emit takes offsets (int64, n + 1: the exclusive
// scan of out_len) and writes value r at out[offsets[r] ...], nothing outside
// [offsets[r], offsets[r + 1]) cut to [0, out_bytes) and nothing for a bad value.  device and
// stream as above; n == 0 launches nothing; more than 2^31 values or a null array with n > 0 throw.
void json_text_measure_raw(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status,
                           uint64_t n, int device, uint64_t out_len, uint64_t out_status, uint64_t stream);
void json_text_emit_raw(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status, uint64_t n,
                        int device, uint64_t offsets, uint64_t out, uint64_t out_bytes, uint64_t stream);

// Kernel launches so far in this process (tests: a rejected or empty call launches nothing).
uint64_t json_fields_launches();
uint64_t json_text_launches();

}  // namespace amdx
