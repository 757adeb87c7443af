#include "parquet_decode.h"

#include <atomic>
#include <string>

#include "block_store.h"
#include "cpu_codecs.h"
#include "kernels.h"
#include "paged_view.h"

namespace amdx {

namespace {

std::atomic<uint64_t> g_pq_launches{0};
constexpr uint64_t kMax = 1ull << 31;
constexpr int kPqCodecSnappy = 1, kPqCodecLz4Raw = 7;   // CompressionCodec of the format

void bad(const std::string& what) { throw StoreError(kErrInvalidArgument, "parquet decode: " + what); }

template <typename T>
T* ptr(uint64_t p) { return reinterpret_cast<T*>(p); }

}  // namespace

uint64_t parquet_decode_launches() { return g_pq_launches.load(); }

void parquet_walk_raw(uint64_t data, uint64_t data_bytes, uint64_t chunk_off, uint64_t chunk_len, uint64_t nchunks,
                      int device, uint64_t counts, uint64_t errors, uint64_t page_base, uint64_t table,
                      uint64_t table_rows, uint64_t stream) {
  if (nchunks > kMax || table_rows > kMax) bad("too many chunks or pages for one call");
  PqWalkArgs a{};
  a.data = ptr<const uint8_t>(data);
  a.data_bytes = data_bytes;
  a.chunk_off = ptr<const int64_t>(chunk_off);
  a.chunk_len = ptr<const int64_t>(chunk_len);
  a.nchunks = nchunks;
  a.counts = ptr<int32_t>(counts);
  a.errors = ptr<int32_t>(errors);
  a.page_base = ptr<const int64_t>(page_base);
  a.table = ptr<int64_t>(table);
  a.table_rows = table_rows;
  if (nchunks == 0) return;
  if (!a.data && data_bytes) bad("no data");
  if (!a.chunk_off || !a.chunk_len) bad("no chunk table");
  if (a.table ? !a.page_base : (!a.counts || !a.errors)) bad("no counts, errors or page bases");
  if (device < 0) {
    parquet_walk_host(a);
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch_parquet_walk(a, reinterpret_cast<hipStream_t>(stream)));
  ++g_pq_launches;
}

void parquet_lz4_raw(uint64_t data, uint64_t data_bytes, uint64_t table, uint64_t npages, uint64_t dst_off,
                     uint64_t out, uint64_t out_bytes, uint64_t chunks, uint64_t expect, uint64_t sizes, int device,
                     uint64_t stream) {
  parquet_decompress_raw(kPqCodecLz4Raw, data, data_bytes, table, npages, dst_off, out, out_bytes, chunks, expect, sizes,
                         device, stream);
}

void parquet_decompress_raw(int codec, uint64_t data, uint64_t data_bytes, uint64_t table, uint64_t npages,
                            uint64_t dst_off, uint64_t out, uint64_t out_bytes, uint64_t chunks, uint64_t expect,
                            uint64_t sizes, int device, uint64_t stream) {
  if (codec != kPqCodecSnappy && codec != kPqCodecLz4Raw) bad("no decoder for codec " + std::to_string(codec));
  const bool snappy = codec == kPqCodecSnappy;
  if (npages > kMax) bad("too many pages for one call");
  PqLz4Args a{};
  a.data = ptr<const uint8_t>(data);
  a.data_bytes = data_bytes;
  a.table = ptr<const int64_t>(table);
  a.npages = npages;
  a.dst_off = ptr<const int64_t>(dst_off);
  a.out = ptr<uint8_t>(out);
  a.out_bytes = out_bytes;
  a.chunks = ptr<PqLz4Chunk>(chunks);
  a.expect = ptr<int32_t>(expect);
  if (npages == 0) return;
  if (!a.data && data_bytes) bad("no data");
  if (!a.out && out_bytes) bad("no output buffer");
  if (!a.table || !a.dst_off || !a.chunks || !a.expect || !sizes) bad("no page table, offsets, chunks or sizes");
  if (device < 0) {
    parquet_lz4_plan_host(a);
    int32_t* sz = ptr<int32_t>(sizes);
    for (uint64_t p = 0; p < npages; ++p) {
      const PqLz4Chunk& c = a.chunks[p];
      if (c.src_bytes == 0) sz[p] = 0;
      else if (snappy)
        sz[p] = (int32_t)snappy_decompress_block(ptr<const uint8_t>(c.src), c.src_bytes, ptr<uint8_t>(c.dst), c.dst_capacity);
      else
        sz[p] = (int32_t)lz4_decompress_block(ptr<const uint8_t>(c.src), c.src_bytes, ptr<uint8_t>(c.dst), c.dst_capacity);
    }
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  AMDX_HIP(launch_parquet_lz4_plan(a, st));
  AMDX_HIP((snappy ? launch_snappy_decompress : launch_lz4_decompress)(reinterpret_cast<const Lz4Chunk*>(a.chunks),
                                                                      (int)npages, ptr<int32_t>(sizes), st));
  g_pq_launches += 2;
}

void parquet_hybrid_raw(uint64_t data, uint64_t data_bytes, uint64_t streams, uint64_t nstreams, uint64_t out,
                        uint64_t out_n, uint64_t errors, int mode, uint64_t run_counts, uint64_t run_base,
                        uint64_t runs, uint64_t runs_rows, int device, uint64_t stream) {
  if (nstreams > kMax || out_n > kMax || runs_rows > kMax) bad("too many streams, values or runs for one call");
  if (mode < 0 || mode > 3) bad("the mode is 0 to 3");
  PqStreamArgs a{};
  a.data = ptr<const uint8_t>(data);
  a.data_bytes = data_bytes;
  a.streams = ptr<const int64_t>(streams);
  a.nstreams = nstreams;
  a.out = ptr<int32_t>(out);
  a.out_n = out_n;
  a.errors = ptr<int32_t>(errors);
  a.run_counts = ptr<int32_t>(run_counts);
  a.run_base = ptr<const int64_t>(run_base);
  a.runs = mode == 1 ? nullptr : ptr<int64_t>(runs);
  a.runs_rows = runs_rows;
  if (nstreams == 0) return;
  if (!a.data && data_bytes) bad("no data");
  if (!a.streams) bad("no streams");
  if (!a.out && out_n) bad("no output");
  if ((mode == 0 || mode == 1) && !a.errors) bad("no error codes");
  if (mode == 1 && !a.run_counts) bad("no run counts");
  if (mode >= 2 && (!a.run_base || (!a.runs && runs_rows))) bad("no run table");
  if (mode == 2 && !a.runs) return;
  if (mode == 3 && out_n == 0) return;
  if (device < 0) {
    if (mode == 0) {
      parquet_hybrid_host(a);
    } else if (mode == 3) {
      for (uint64_t t = 0; t < out_n; ++t) pq_stream_value(a, t);
    } else {
      for (uint64_t s = 0; s < nstreams; ++s) pq_stream_runs(a, s);
    }
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch_parquet_hybrid(a, mode, reinterpret_cast<hipStream_t>(stream)));
  ++g_pq_launches;
}

void parquet_place_raw(uint64_t data, uint64_t data_bytes, uint64_t pages, uint64_t npages, uint64_t excl, uint64_t idx,
                       uint64_t idx_n, uint64_t dict, uint64_t dict_size, uint64_t stream_err, uint64_t nstreams,
                       uint32_t width, bool is_bool, uint64_t values, uint64_t status, uint64_t rows, int device,
                       uint64_t stream) {
  if (rows > kMax || npages > kMax || idx_n > kMax || dict_size > kMax) bad("too many rows or pages for one call");
  if (width != 1 && width != 4 && width != 8) bad("a value is 1, 4 or 8 bytes");
  if (is_bool && width != 1) bad("a boolean is one byte");
  PqPlaceArgs a{};
  a.data = ptr<const uint8_t>(data);
  a.data_bytes = data_bytes;
  a.pages = ptr<const int64_t>(pages);
  a.npages = npages;
  a.excl = ptr<const int64_t>(excl);
  a.idx = ptr<const int32_t>(idx);
  a.idx_n = idx_n;
  a.dict = ptr<const uint8_t>(dict);
  a.dict_size = dict_size;
  a.stream_err = ptr<const int32_t>(stream_err);
  a.nstreams = nstreams;
  a.width = width;
  a.is_bool = is_bool ? 1u : 0u;
  a.values = ptr<uint8_t>(values);
  a.status = ptr<uint8_t>(status);
  a.rows = rows;
  if (rows == 0) return;
  if (!a.values || !a.status) bad("no outputs");
  if (!a.data && data_bytes) bad("no data");
  if (!a.pages && npages) bad("no pages");
  if (!a.idx && idx_n) bad("no indices");
  if (!a.dict && dict_size) bad("no dictionary");
  if (device < 0) {
    parquet_place_host(a);
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch_parquet_place(a, reinterpret_cast<hipStream_t>(stream)));
  ++g_pq_launches;
}

void parquet_bytes_raw(uint64_t data, uint64_t data_bytes, uint64_t pages, uint64_t npages, uint64_t excl, uint64_t rows,
                       uint64_t stream_err, uint64_t nstreams, uint64_t start, uint64_t length, uint64_t status,
                       uint64_t nvalues, int device, uint64_t stream) {
  if (rows > kMax || npages > kMax || nvalues > kMax) bad("too many values or pages for one call");
  PqBytesArgs a{};
  a.data = ptr<const uint8_t>(data);
  a.data_bytes = data_bytes;
  a.pages = ptr<const int64_t>(pages);
  a.npages = npages;
  a.excl = ptr<const int64_t>(excl);
  a.rows = rows;
  a.stream_err = ptr<const int32_t>(stream_err);
  a.nstreams = nstreams;
  a.start = ptr<int64_t>(start);
  a.length = ptr<int32_t>(length);
  a.status = ptr<uint8_t>(status);
  a.nvalues = nvalues;
  if (npages == 0 || nvalues == 0) return;
  if (!a.pages || !a.start || !a.length || !a.status) bad("no pages or outputs");
  if (!a.data && data_bytes) bad("no data");
  if (device < 0) {
    parquet_bytes_host(a);
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch_parquet_bytes(a, reinterpret_cast<hipStream_t>(stream)));
  ++g_pq_launches;
}

}  // namespace amdx
