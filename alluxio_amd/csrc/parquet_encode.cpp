#include "parquet_encode.h"

#include <atomic>
#include <string>

#include "block_store.h"
#include "kernels.h"
#include "paged_view.h"

namespace amdx {

namespace {

std::atomic<uint64_t> g_pe_launches{0};
constexpr uint64_t kMax = 1ull << 31;

void bad(const std::string& what) { throw StoreError(kErrInvalidArgument, "parquet encode: " + what); }

template <typename T>
T* ptr(uint64_t p) { return reinterpret_cast<T*>(p); }

void check_range(const PeArgs& a, uint64_t largest) {
  if (a.npages > kMax || a.flat_n > kMax || largest > kMax) bad("too many pages or rows for one call");
  if (a.first > a.last || a.last > a.npages) bad("the page range lies outside the table");
  if (a.first < a.last && !a.pages) bad("no page table");
}

void launch(const PeArgs& a, int pass, uint64_t largest, int device, uint64_t stream) {
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch_parquet_encode(a, pass, largest, reinterpret_cast<hipStream_t>(stream)));
  ++g_pe_launches;
}

}  // namespace

uint64_t parquet_encode_launches() { return g_pe_launches.load(); }

void parquet_encode_measure_raw(uint64_t pages, uint64_t npages, uint64_t first, uint64_t last, uint64_t largest,
                                uint64_t flags, uint64_t text_bytes, uint64_t flat_n, uint64_t measure, int device,
                                uint64_t stream) {
  PeArgs a{};
  a.pages = ptr<const int64_t>(pages);
  a.npages = npages;
  a.first = first;
  a.last = last;
  a.flags = ptr<uint8_t>(flags);
  a.text_bytes = ptr<int32_t>(text_bytes);
  a.flat_n = flat_n;
  a.measure = ptr<int64_t>(measure);
  check_range(a, largest);
  if (first == last || largest == 0) return;
  if (!a.flags || !a.measure) bad("no flags or measure table");
  if (device < 0) {
    parquet_encode_measure_host(a);
    return;
  }
  launch(a, kPePassMeasure, largest, device, stream);
}

void parquet_encode_emit_raw(int pass, uint64_t pages, uint64_t npages, uint64_t first, uint64_t last, uint64_t largest,
                             uint64_t flags, uint64_t rank, uint64_t text_at, uint64_t scratch, uint64_t flat_n,
                             uint64_t out, uint64_t out_bytes, int device, uint64_t stream) {
  if (pass != kPePassRows && pass != kPePassText && pass != kPePassPack) bad("the pass is rows, text or pack");
  PeArgs a{};
  a.pages = ptr<const int64_t>(pages);
  a.npages = npages;
  a.first = first;
  a.last = last;
  a.flags = ptr<uint8_t>(flags);
  a.rank = ptr<const int64_t>(rank);
  a.text_at = ptr<const int64_t>(text_at);
  a.scratch = ptr<int32_t>(scratch);
  a.flat_n = flat_n;
  a.out = ptr<uint8_t>(out);
  a.out_bytes = out_bytes;
  check_range(a, largest);
  if (first == last || largest == 0) return;
  if (!a.out || !a.flags || !a.rank) bad("no output, flags or ranks");
  if (pass == kPePassPack && !a.scratch) bad("no scratch values");
  if (device < 0) {
    if (pass == kPePassRows) parquet_encode_rows_host(a);
    else if (pass == kPePassText) parquet_encode_text_host(a);
    else parquet_encode_pack_host(a);
    return;
  }
  launch(a, pass, largest, device, stream);
}

void parquet_encode_copy_raw(uint64_t blob, uint64_t blob_bytes, uint64_t segs, uint64_t nsegs, uint64_t out,
                             uint64_t out_bytes, int device, uint64_t stream) {
  if (nsegs > kMax) bad("too many segments for one call");
  PeArgs a{};
  a.blob = ptr<const uint8_t>(blob);
  a.blob_bytes = blob_bytes;
  a.segs = ptr<const int64_t>(segs);
  a.nsegs = nsegs;
  a.out = ptr<uint8_t>(out);
  a.out_bytes = out_bytes;
  if (nsegs == 0) return;
  if (!a.blob || !a.segs || !a.out) bad("no blob, segments or output");
  if (device < 0) {
    parquet_encode_copy_host(a);
    return;
  }
  launch(a, kPePassCopy, 0, device, stream);
}

void parquet_encode_lz4_raw(int mode, uint64_t src, uint64_t src_bytes, uint64_t pages, uint64_t npages, uint64_t segs,
                            uint64_t nsegs, uint64_t scratch, uint64_t scratch_bytes, uint64_t result, uint64_t dst,
                            uint64_t out, uint64_t out_bytes, uint32_t warm, uint32_t segment, int device, uint64_t stream) {
  if (mode != 0 && mode != 1) bad("the mode is 0 (parse and link) or 1 (merge)");
  if (npages > kMax || nsegs > kMax) bad("too many pages or segments for one call");
  if (npages == 0 && nsegs == 0) return;
  if (npages == 0 || nsegs < npages) bad("every page has at least one segment");
  LbArgs a{};
  a.src = ptr<const uint8_t>(src);
  a.src_bytes = src_bytes;
  a.pages = ptr<const int64_t>(pages);
  a.npages = npages;
  a.segs = ptr<const int64_t>(segs);
  a.nsegs = nsegs;
  a.scratch = ptr<uint8_t>(scratch);
  a.scratch_bytes = scratch_bytes;
  a.result = ptr<int64_t>(result);
  a.dst = ptr<const int64_t>(dst);
  a.out = ptr<uint8_t>(out);
  a.out_bytes = out_bytes;
  a.warm = warm;
  a.segment = segment;
  if (!a.src || !a.pages || !a.segs || !a.scratch || !a.result) bad("no source, page table, segment table, scratch or result");
  if (scratch & 3) bad("the scratch buffer is not aligned to 4 bytes");
  if (scratch_bytes < lb_scratch_head(nsegs)) bad("the scratch buffer is shorter than its records");
  if (segment < 1 || (uint64_t)segment + warm > 65535) bad("segment + warm-up is at most 65535 bytes");
  if (mode == 1 && (!a.dst || !a.out)) bad("no output or block offsets");
  if (device < 0) {
    // host memory: the tables can be read here, so everything that does not fit is refused up front
    for (uint64_t s = 0; s < nsegs; ++s)
      if (!lb_seg_ok(a, a.segs + s * kLbSegCols)) bad("segment " + std::to_string(s) + " lies outside its page, the source or the scratch buffer");
    if (mode == 0) {
      lz4_block_parse_host(a);
      lz4_block_link_host(a);
    } else {
      for (uint64_t p = 0; p < npages; ++p) {
        const int64_t size = a.result[p * kLbResCols + kLbSize], at = a.dst[p];
        if (a.result[p * kLbResCols + kLbStatus] != 0 || size < 1) bad("page " + std::to_string(p) + " has no linked block");
        if (at < 0 || (uint64_t)at > out_bytes || (uint64_t)size > out_bytes - (uint64_t)at)
          bad("the block of page " + std::to_string(p) + " lies outside the output");
      }
      lz4_block_merge_host(a);
    }
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (mode == 0) {
    AMDX_HIP(launch_lz4_page_parse(a, st));
    ++g_pe_launches;
    AMDX_HIP(launch_lz4_page_link(a, st));
    ++g_pe_launches;
  } else {
    AMDX_HIP(launch_lz4_page_merge(a, st));
    ++g_pe_launches;
  }
}

}  // namespace amdx
