#include "json_fields.h"

#include <atomic>
#include <string>

#include "block_store.h"
#include "kernels.h"
#include "paged_view.h"

namespace amdx {

namespace {

std::atomic<uint64_t> g_fields_launches{0};
std::atomic<uint64_t> g_text_launches{0};

void bad(const std::string& what) { throw StoreError(kErrInvalidArgument, "json fields: " + what); }

JsonTextArgs text_common(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status,
                         uint64_t n) {
  if (n > (1ull << 31)) bad("too many values for one call");
  JsonTextArgs a{};
  a.t.data = reinterpret_cast<const uint8_t*>(data);
  a.t.data_bytes = data_bytes;
  a.t.start = reinterpret_cast<const int64_t*>(start);
  a.t.length = reinterpret_cast<const int32_t*>(length);
  a.t.status = reinterpret_cast<const uint8_t*>(status);
  a.t.n = n;
  a.t.quote = -1;
  if (n) {
    if (!a.t.data && data_bytes) bad("no data");
    if (!a.t.start || !a.t.length) bad("no spans");
  }
  return a;
}

}  // namespace

uint64_t json_fields_launches() { return g_fields_launches.load(); }
uint64_t json_text_launches() { return g_text_launches.load(); }

void json_fields_raw(uint64_t data, uint64_t data_bytes, uint64_t off, uint64_t len, bool len_is_64, uint64_t nrows,
                     int device, uint64_t names, uint64_t names_bytes, uint32_t terminator,
                     const std::vector<JsonFieldsCol>& cols, uint64_t stream) {
  if (terminator > 255) bad("the terminator is one byte");
  if (cols.empty() || cols.size() > kJsonFieldsMaxCols) bad("1 to 32 columns per call");
  if (nrows > (1ull << 31)) bad("too many rows for one call");
  if (names_bytes > kJsonFieldsMaxCols * kJsonFieldsMaxName) bad("the names are longer than 32 names can be");
  JsonFieldsArgs a{};
  a.data = reinterpret_cast<const uint8_t*>(data);
  a.data_bytes = data_bytes;
  a.off = reinterpret_cast<const int64_t*>(off);
  a.len = reinterpret_cast<const void*>(len);
  a.nrows = nrows;
  a.names = reinterpret_cast<const uint8_t*>(names);
  a.names_bytes = (uint32_t)names_bytes;
  a.len_is_64 = len_is_64 ? 1u : 0u;
  a.terminator = terminator;
  a.ncols = (uint32_t)cols.size();
  for (size_t j = 0; j < cols.size(); ++j) {
    const JsonFieldsCol& c = cols[j];
    if (c.type > kJfString) bad("unknown column type");
    if (c.name_len < 1 || c.name_len > kJsonFieldsMaxName) bad("a name is 1 to 255 bytes");
    if (c.name_off > a.names_bytes || c.name_len > a.names_bytes - c.name_off) bad("a name outside the name buffer");
    if (nrows && (!c.values || !c.status || ((c.type == kFpSpan || c.type == kJfString) && !c.length)))
      bad("column without outputs");
    a.cols[j] = c;
  }
  if (!json_fields_scalars_ok(a)) bad("bad scalars");
  if (nrows == 0) return;
  if (!a.data && data_bytes) bad("no data");
  if (!a.off || !a.len) bad("no row table");
  if (!a.names) bad("no names");
  if (device < 0) {
    json_fields_host(a);
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch_json_fields(a, reinterpret_cast<hipStream_t>(stream)));
  ++g_fields_launches;
}

void json_text_measure_raw(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status,
                           uint64_t n, int device, uint64_t out_len, uint64_t out_status, uint64_t stream) {
  JsonTextArgs a = text_common(data, data_bytes, start, length, status, n);
  a.t.out_len = reinterpret_cast<int32_t*>(out_len);
  a.out_status = reinterpret_cast<uint8_t*>(out_status);
  if (n == 0) return;
  if (!a.t.out_len || !a.out_status) bad("no output lengths or status");
  if (device < 0) {
    json_text_measure_host(a);
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch_json_text_measure(a, reinterpret_cast<hipStream_t>(stream)));
  ++g_text_launches;
}

void json_text_emit_raw(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status, uint64_t n,
                        int device, uint64_t offsets, uint64_t out, uint64_t out_bytes, uint64_t stream) {
  JsonTextArgs a = text_common(data, data_bytes, start, length, status, n);
  a.t.offsets = reinterpret_cast<const int64_t*>(offsets);
  a.t.out = reinterpret_cast<uint8_t*>(out);
  a.t.out_bytes = out_bytes;
  if (n == 0) return;
  if (!a.t.offsets) bad("no offsets");
  if (!a.t.out && out_bytes) bad("no output buffer");
  if (device < 0) {
    json_text_emit_host(a);
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch_json_text_emit(a, reinterpret_cast<hipStream_t>(stream)));
  ++g_text_launches;
}

}  // namespace amdx
