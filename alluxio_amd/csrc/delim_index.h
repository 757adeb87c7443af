// Record index of a delimited text file (JSONL, CSV, one document per line) built where the bytes
// are: the cut positions, the byte after each delimiter, of a cached file.  With a device arena
// the count, scan and emit kernels of delim_index.hip do the work and the host reads one total
// and one result; with a host arena (DRAM dirs, CPU-only builds) the same call is a memchr loop
// per page (delim_index_host.h).  Two entry points, like RaggedGatherSession's constructors.
#pragma once
#include <cstdint>
#include <vector>

#include "block_store.h"

namespace amdx {

// Device time of the three launches of one call, in milliseconds (tools/delim_index_bench.py).
struct DelimIndexTimes {
  float count_ms = 0, scan_ms = 0, emit_ms = 0;
};

// Store form: the blocks (ids, lengths) of ONE file, read-locked for the duration of the call.
// Cuts are relative to the file start.  Throws StoreError(kErrInvalidArgument) for blocks in a
// file tier or spread over several dirs, as RaggedGatherSession does: the caller falls back.
//
// quote (both forms): -1 = none, every delimiter is a cut.  Otherwise one byte != delim that
// toggles the state "inside quotes"; a delimiter is a cut only outside, which is the record
// structure of a well-formed RFC 4180 file (a doubled quote toggles twice).  The file starts
// outside quotes; the raw form takes the state at vstart as in_quote.  A range that ends inside
// quotes is no error.  Any other quote, or in_quote without one, is kErrInvalidArgument before
// anything is launched.
std::vector<uint64_t> delim_index_store(BlockStore* store, int64_t session, const std::vector<int64_t>& ids,
                                        const std::vector<uint64_t>& lens, uint32_t delim, int64_t quote = -1);

// Raw form: `pages` maps virtual page -> arena page of an arena that is addressable from this
// process; device < 0: host memory.  Cuts are add + (offset from vstart) + 1.  Block locks, if
// any, are the caller's.
std::vector<uint64_t> delim_index_raw(uint64_t arena_base, const std::vector<int64_t>& pages, uint64_t page_size,
                                      int device, uint64_t vstart, uint64_t bytes, uint32_t delim, uint64_t add = 0,
                                      DelimIndexTimes* times = nullptr, int64_t quote = -1, bool in_quote = false);

// Kernel launches so far in this process (tests: a rejected call launches nothing).
uint64_t delim_index_launches();

}  // namespace amdx
