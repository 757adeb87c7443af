// Parquet column statistics computed where the columns lie: the kernels of parquet_stats.hip for
// device memory, the loops of parquet_stats_host.h for host memory.  Both follow the rules in that
// header and give the same result rows.  Every argument that is a pointer is an address as an
// integer, and the segment table holds the addresses of the columns' arrays; device < 0: host
// memory, done on return; otherwise memory of that device, the kernels are queued on `stream` and
// nothing is waited for.  A null array where one is needed, a range outside the table or a count
// above 2^31 throw StoreError(kErrInvalidArgument) before anything is launched or written.
#pragma once
#include <cstdint>

#include "parquet_stats_host.h"

namespace amdx {

// All passes over the table (nsegs rows of kPeCols int64, ordered so that the dictionary-index
// segments are [mark_first, mark_last) and the text segments, dictionaries included, are
// [text_first, nsegs)): mark, first and the rounds.  results has nsegs rows of kPsCols int64 that
// the caller initialised (kPsMin: INT64_MAX, kPsMax: INT64_MIN, the kPsRoundMin columns: all bits set,
// all others 0); alive has flat_n bytes (0 is allowed when there is no text segment).  largest: the
// most rows of a segment.  On a device: one launch for mark if its range is not empty, one for
// first, and kPsRounds - 1 for the rounds if there is a text segment, whatever nsegs is.
void parquet_stats_raw(uint64_t segs, uint64_t nsegs, uint64_t mark_first, uint64_t mark_last, uint64_t text_first,
                       uint64_t largest, uint64_t alive, uint64_t flat_n, uint64_t results, int device, uint64_t stream);

// Kernel launches so far in this process (tests: a host call launches none, and the launches of a row
// group do not depend on how many columns it has).
uint64_t parquet_stats_launches();

}  // namespace amdx
