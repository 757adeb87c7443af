#include "field_parse.h"

#include <atomic>
#include <string>

#include "block_store.h"
#include "kernels.h"
#include "paged_view.h"

namespace amdx {

namespace {

std::atomic<uint64_t> g_launches{0};

void bad(const std::string& what) { throw StoreError(kErrInvalidArgument, "field parse: " + what); }

}  // namespace

uint64_t field_parse_launches() { return g_launches.load(); }

void field_parse_raw(uint64_t data, uint64_t data_bytes, uint64_t off, uint64_t len, bool len_is_64, uint64_t nrows,
                     int device, uint32_t sep, int64_t quote, uint32_t terminator,
                     const std::vector<FieldParseCol>& cols, uint64_t stream) {
  if (sep > 255 || terminator > 255) bad("the separator and the terminator are one byte each");
  if (quote < -1 || quote > 255) bad("the quote is one byte");
  if (sep == terminator || quote == (int64_t)sep || quote == (int64_t)terminator)
    bad("separator, quote and terminator must differ");
  if (cols.empty() || cols.size() > kFieldParseMaxCols) bad("1 to 32 columns per call");
  if (nrows > (1ull << 31)) bad("too many rows for one call");
  FieldParseArgs a{};
  a.data = reinterpret_cast<const uint8_t*>(data);
  a.data_bytes = data_bytes;
  a.off = reinterpret_cast<const int64_t*>(off);
  a.len = reinterpret_cast<const void*>(len);
  a.nrows = nrows;
  a.len_is_64 = len_is_64 ? 1u : 0u;
  a.sep = sep;
  a.quote = (int32_t)quote;
  a.terminator = terminator;
  a.ncols = (uint32_t)cols.size();
  for (size_t j = 0; j < cols.size(); ++j) {
    const FieldParseCol& c = cols[j];
    if (c.field > kFieldParseMaxField) bad("field number above 65535");
    if (c.type > kFpFloat32) bad("unknown column type");
    if (nrows && (!c.values || !c.status || (c.type == kFpSpan && !c.length))) bad("column without outputs");
    if (c.field > a.max_field) a.max_field = c.field;
    a.cols[j] = c;
  }
  if (!field_parse_scalars_ok(a)) bad("bad scalars");
  if (nrows == 0) return;
  if (!a.data && data_bytes) bad("no data");
  if (!a.off || !a.len) bad("no row table");
  if (device < 0) {
    field_parse_host(a);
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch_field_parse(a, reinterpret_cast<hipStream_t>(stream)));
  ++g_launches;
}

}  // namespace amdx
