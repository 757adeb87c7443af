// Parquet pages encoded where the columns lie: the kernels of parquet_encode.hip for device memory,
// the loops of parquet_encode_host.h for host memory.  Both follow the rules in that header and give
// the same bytes.  Every argument that is a pointer is an address as an integer, and the page table
// holds the addresses of the columns' arrays; device < 0: host memory, done on return; otherwise
// memory of that device, the kernel is queued on `stream` and nothing is waited for.  An empty range
// launches nothing.  A null array where one is needed, a range outside the table or a count above
// 2^31 throw StoreError(kErrInvalidArgument) before anything is launched or written.
#pragma once
#include <cstdint>

#include "lz4_block_host.h"
#include "parquet_encode_host.h"

namespace amdx {

// measure: pages [first, last) of the table (npages rows of kPeCols int64); flags (uint8) and
// text_bytes (int32, or 0 without a text column) have flat_n slots; measure has npages rows of
// kPmCols int64 that the caller zeroed (kPmMaxCode: -1).  largest: the most rows of a page.
void parquet_encode_measure_raw(uint64_t pages, uint64_t npages, uint64_t first, uint64_t last, uint64_t largest,
                                uint64_t flags, uint64_t text_bytes, uint64_t flat_n, uint64_t measure, int device,
                                uint64_t stream);

// The emit passes: kPePassRows (level bits, fixed-width values, booleans and indices to scratch),
// kPePassText, kPePassPack (largest: the most value bytes of a page).  rank and text_at are the
// exclusive scans (flat_n + 1 int64) of flags and text_bytes.
void parquet_encode_emit_raw(int pass, uint64_t pages, uint64_t npages, uint64_t first, uint64_t last, uint64_t largest,
                             uint64_t flags, uint64_t rank, uint64_t text_at, uint64_t scratch, uint64_t flat_n,
                             uint64_t out, uint64_t out_bytes, int device, uint64_t stream);

// copy: nsegs rows of (source in blob, place in out, length).
void parquet_encode_copy_raw(uint64_t blob, uint64_t blob_bytes, uint64_t segs, uint64_t nsegs, uint64_t out,
                             uint64_t out_bytes, int device, uint64_t stream);

// LZ4_RAW: one LZ4 block per page body (lz4_block_host.h has the tables).  src holds the bodies;
// pages (npages rows of kLbPageCols) and segs (nsegs rows of kLbSegCols) are the caller's tables;
// scratch starts with lb_scratch_head(nsegs) bytes of records, 4-byte aligned, and the segment rows
// name places behind them; result has npages rows of kLbResCols; no segment has more than `segment`
// bytes and segment + warm <= 65535.  mode 0: parse and link (two
// launches), after which result holds the blocks' sizes; mode 1: merge (one launch), every block
// written at out + dst[page] (dst: npages int64).  With host memory every row is checked before
// anything is written and what does not fit throws; on a device the kernels skip such rows and
// flag their pages in result (kLbStatus).
void parquet_encode_lz4_raw(int mode, uint64_t src, uint64_t src_bytes, uint64_t pages, uint64_t npages, uint64_t segs,
                            uint64_t nsegs, uint64_t scratch, uint64_t scratch_bytes, uint64_t result, uint64_t dst,
                            uint64_t out, uint64_t out_bytes, uint32_t warm, uint32_t segment, int device, uint64_t stream);

// Kernel launches so far in this process (tests: a host call launches none, and the launches of a row
// group do not depend on how many columns it has).
uint64_t parquet_encode_launches();

}  // namespace amdx
