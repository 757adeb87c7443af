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

}  // namespace amdx
