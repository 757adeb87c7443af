// Parquet pages decoded where the bytes lie: the kernels of parquet_decode.hip for device memory, the
// loops of parquet_host.h for host memory (DRAM dirs, CPU-only use).  Both follow the rules in that
// header and give the same bytes.  Every argument that is a pointer is an address as an integer;
// device < 0: host memory, done on return; otherwise memory of that device, the kernels are queued
// on `stream` and nothing is waited for.  A count of 0 launches nothing.  A null array where one is
// needed, a count above 2^31 or a value width that is not 1, 4 or 8 throw
// StoreError(kErrInvalidArgument) before anything is launched or written.
#pragma once
#include <cstdint>

#include "parquet_host.h"

namespace amdx {

// Page walk.  table == 0: count (counts and errors are written); otherwise fill, with page_base the
// exclusive scan of the counts (nchunks + 1) and table_rows rows of kPqCols int64.
void parquet_walk_raw(uint64_t data, uint64_t data_bytes, uint64_t chunk_off, uint64_t chunk_len, uint64_t nchunks,
                      int device, uint64_t counts, uint64_t errors, uint64_t page_base, uint64_t table,
                      uint64_t table_rows, uint64_t stream);

// LZ4_RAW pages: the chunk list is built from the page table where it lies (chunks: npages entries
// of 24 bytes, expect: int32 npages) and the LZ4 block decoder writes into out; sizes (int32
// npages) is what it produced per page, to be compared with expect.
void parquet_lz4_raw(uint64_t data, uint64_t data_bytes, uint64_t table, uint64_t npages, uint64_t dst_off,
                     uint64_t out, uint64_t out_bytes, uint64_t chunks, uint64_t expect, uint64_t sizes, int device,
                     uint64_t stream);
// The same for the pages of any codec that has a decoder: `codec` is the format's number, 1 (SNAPPY:
// the Snappy raw decoder) or 7 (LZ4_RAW); another one is an invalid argument.  parquet_lz4_raw is
// codec 7.  Two launches per call on a device, none on the host.
void parquet_decompress_raw(int codec, uint64_t data, uint64_t data_bytes, uint64_t table, uint64_t npages,
                            uint64_t dst_off, uint64_t out, uint64_t out_bytes, uint64_t chunks, uint64_t expect,
                            uint64_t sizes, int device, uint64_t stream);

// Hybrid streams.  mode 0: each stream decoded serially (the host loop; kernel variant 0).  The
// cooperative form is three calls: mode 1 counts the runs (run_counts, errors), mode 2 fills the run
// table (run_base: the exclusive scan, nstreams + 1; runs: runs_rows rows of 4 int64), mode 3 gives
// every output slot its value through the table.
void parquet_hybrid_raw(uint64_t data, uint64_t data_bytes, uint64_t streams, uint64_t nstreams, uint64_t out,
                        uint64_t out_n, uint64_t errors, int mode, uint64_t run_counts, uint64_t run_base,
                        uint64_t runs, uint64_t runs_rows, int device, uint64_t stream);

// Place: rows of `width` bytes into values, one status byte each.
void parquet_place_raw(uint64_t data, uint64_t data_bytes, uint64_t pages, uint64_t npages, uint64_t excl, uint64_t idx,
                       uint64_t idx_n, uint64_t dict, uint64_t dict_size, uint64_t stream_err, uint64_t nstreams,
                       uint32_t width, bool is_bool, uint64_t values, uint64_t status, uint64_t rows, int device,
                       uint64_t stream);

// PLAIN BYTE_ARRAY pages: start (int64), length (int32) and status (uint8) per value slot.
void parquet_bytes_raw(uint64_t data, uint64_t data_bytes, uint64_t pages, uint64_t npages, uint64_t excl, uint64_t rows,
                       uint64_t stream_err, uint64_t nstreams, uint64_t start, uint64_t length, uint64_t status,
                       uint64_t nvalues, int device, uint64_t stream);

// Kernel launches so far in this process (tests: a rejected or empty call launches nothing, a host
// call none).
uint64_t parquet_decode_launches();

}  // namespace amdx
