#include "text_column.h"

#include <atomic>
#include <string>

#include "block_store.h"
#include "kernels.h"
#include "paged_view.h"

namespace amdx {

namespace {

std::atomic<uint64_t> g_launches{0};

void bad(const std::string& what) { throw StoreError(kErrInvalidArgument, "text column: " + what); }

TextColumnArgs common(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status, uint64_t n,
                      int64_t quote) {
  if (quote < -1 || quote > 255) bad("the quote is one byte");
  if (n > (1ull << 31)) bad("too many values for one call");
  TextColumnArgs a{};
  a.data = reinterpret_cast<const uint8_t*>(data);
  a.data_bytes = data_bytes;
  a.start = reinterpret_cast<const int64_t*>(start);
  a.length = reinterpret_cast<const int32_t*>(length);
  a.status = reinterpret_cast<const uint8_t*>(status);
  a.n = n;
  a.quote = (int32_t)quote;
  if (n) {
    if (!a.data && data_bytes) bad("no data");
    if (!a.start || !a.length) bad("no spans");
  }
  return a;
}

}  // namespace

uint64_t text_column_launches() { return g_launches.load(); }

void text_measure_raw(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status, uint64_t n,
                      int device, int64_t quote, uint64_t out_len, uint64_t stream) {
  TextColumnArgs a = common(data, data_bytes, start, length, status, n, quote);
  a.out_len = reinterpret_cast<int32_t*>(out_len);
  if (n == 0) return;
  if (!a.out_len) bad("no output lengths");
  if (device < 0) {
    text_measure_host(a);
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch_text_measure(a, reinterpret_cast<hipStream_t>(stream)));
  ++g_launches;
}

void text_emit_raw(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status, uint64_t n,
                   int device, int64_t quote, uint64_t offsets, uint64_t out, uint64_t out_bytes, uint64_t stream) {
  TextColumnArgs a = common(data, data_bytes, start, length, status, n, quote);
  a.offsets = reinterpret_cast<const int64_t*>(offsets);
  a.out = reinterpret_cast<uint8_t*>(out);
  a.out_bytes = out_bytes;
  if (n == 0) return;
  if (!a.offsets) bad("no offsets");
  if (!a.out && out_bytes) bad("no output buffer");
  if (device < 0) {
    text_emit_host(a);
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch_text_emit(a, reinterpret_cast<hipStream_t>(stream)));
  ++g_launches;
}

}  // namespace amdx
