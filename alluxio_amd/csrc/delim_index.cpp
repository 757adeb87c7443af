#include "delim_index.h"

#include <atomic>
#include <string>

#include "delim_index_host.h"
#include "kernels.h"
#include "paged_view.h"

namespace amdx {

namespace {

std::atomic<uint64_t> g_launches{0};

void bad(const std::string& what) { throw StoreError(kErrInvalidArgument, "delimiter index: " + what); }

void check_quote(uint32_t delim, int64_t quote, bool in_quote) {
  if (delim > 255) bad("the delimiter is one byte");
  if (quote < -1 || quote > 255) bad("the quote is one byte");
  if (quote == (int64_t)delim) bad("the quote equals the delimiter");
  if (in_quote && quote < 0) bad("in_quote without a quote");
}

// The events of one call: released on every path out of it.
struct Events {
  hipEvent_t e[4] = {};
  Events() = default;
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  void create() {
    for (auto& x : e) AMDX_HIP(hipEventCreate(&x));
  }
  ~Events() {
    for (auto& x : e)
      if (x) (void)hipEventDestroy(x);
  }
};

// The range has been validated against the view.  A device arena is memory of the current device.
std::vector<uint64_t> run(const PagedView& view, uint64_t vstart, uint64_t bytes, uint32_t delim, uint64_t add,
                          DelimIndexTimes* times, int64_t quote, bool in_quote) {
  std::vector<uint64_t> out;
  if (bytes == 0) return out;
  const bool quoted = quote >= 0;
  const std::vector<int64_t>& vtab = view.vtab;
  const uint32_t page_shift = view.page_shift;
  if (!view.arena_device) {
    if (quoted)
      delim_index_host_quoted(view.base(), vtab.data(), page_shift, vstart, bytes, (uint8_t)delim, (uint8_t)quote,
                              in_quote, add, &out);
    else
      delim_index_host(view.base(), vtab.data(), page_shift, vstart, bytes, (uint8_t)delim, add, &out);
    return out;
  }
  if (view.arena & 15) bad("arena base must be 16-byte aligned");
  DelimIndexArgs a{};
  a.tile_shift = delim_index_tile_shift();
  const uint64_t nt = delim_index_tiles(vstart, bytes, a.tile_shift);
  if (nt > (1ull << 30)) bad("range too large for one call");
  DevBuf d_vtab, d_count, d_base, d_out, d_odd, d_parity;
  Events ev;
  // only the pages the range touches travel
  const uint64_t p0 = vstart >> page_shift, p1 = (vstart + bytes - 1) >> page_shift;
  d_vtab.alloc((p1 - p0 + 1) * sizeof(int64_t));
  d_count.alloc(nt * sizeof(uint32_t));
  d_base.alloc((nt + 1) * sizeof(uint64_t));
  AMDX_HIP(hipMemcpy(d_vtab.p, vtab.data() + p0, (p1 - p0 + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  a.arena = view.base();
  a.vtab = static_cast<const int64_t*>(d_vtab.p);
  a.tile_count = static_cast<uint32_t*>(d_count.p);
  a.tile_base = static_cast<uint64_t*>(d_base.p);
  a.vstart = vstart - (p0 << page_shift);           // the uploaded table starts at the range's first page
  a.bytes = bytes;
  a.add = add;
  a.ntiles = (uint32_t)nt;
  a.page_shift = page_shift;
  a.delim = delim;
  if (quoted) {
    d_odd.alloc(nt * sizeof(uint32_t));
    d_parity.alloc((nt + 1) * sizeof(uint32_t));
    a.tile_count_odd = static_cast<uint32_t*>(d_odd.p);
    a.tile_parity = static_cast<uint32_t*>(d_parity.p);
    a.quote = (uint32_t)quote;
    a.in_quote = in_quote ? 1u : 0u;
  }
  hipStream_t st = nullptr;
  if (times) {
    ev.create();
    AMDX_HIP(hipEventRecord(ev.e[0], st));
  }
  AMDX_HIP(quoted ? launch_delim_count_quoted(a, st) : launch_delim_count(a, st));
  ++g_launches;
  if (times) AMDX_HIP(hipEventRecord(ev.e[1], st));
  AMDX_HIP(quoted ? launch_delim_scan_quoted(a, st) : launch_delim_scan(a, st));
  ++g_launches;
  if (times) AMDX_HIP(hipEventRecord(ev.e[2], st));
  uint64_t total = 0;
  AMDX_HIP(hipMemcpy(&total, a.tile_base + nt, sizeof(total), hipMemcpyDeviceToHost));   // the one synchronising read
  if (total > bytes) throw StoreError(kErrInvalidState, "delimiter index: more delimiters than bytes");
  if (total) {
    d_out.alloc(total * sizeof(uint64_t));
    a.out = static_cast<uint64_t*>(d_out.p);
    a.out_cap = total;
    AMDX_HIP(quoted ? launch_delim_emit_quoted(a, total, st) : launch_delim_emit(a, total, st));
    ++g_launches;
  }
  if (times) {
    AMDX_HIP(hipEventRecord(ev.e[3], st));
    AMDX_HIP(hipEventSynchronize(ev.e[3]));
    AMDX_HIP(hipEventElapsedTime(&times->count_ms, ev.e[0], ev.e[1]));
    AMDX_HIP(hipEventElapsedTime(&times->scan_ms, ev.e[1], ev.e[2]));
    AMDX_HIP(hipEventElapsedTime(&times->emit_ms, ev.e[2], ev.e[3]));
  }
  if (total) {
    out.resize(total);
    AMDX_HIP(hipMemcpy(out.data(), d_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  return out;
}

}  // namespace

uint64_t delim_index_launches() { return g_launches.load(); }

std::vector<uint64_t> delim_index_raw(uint64_t arena_base, const std::vector<int64_t>& pages, uint64_t page_size,
                                      int device, uint64_t vstart, uint64_t bytes, uint32_t delim, uint64_t add,
                                      DelimIndexTimes* times, int64_t quote, bool in_quote) {
  const PagedView view = PagedView::raw(arena_base, pages, page_size, device, "delimiter index");
  check_quote(delim, quote, in_quote);
  if (vstart > view.bytes() || bytes > view.bytes() - vstart) bad("range outside the page table");
  if (device >= 0) AMDX_HIP(hipSetDevice(device));
  return run(view, vstart, bytes, delim, add, times, quote, in_quote);
}

std::vector<uint64_t> delim_index_store(BlockStore* store, int64_t session, const std::vector<int64_t>& ids,
                                        const std::vector<uint64_t>& lens, uint32_t delim, int64_t quote) {
  check_quote(delim, quote, false);
  BlockPins pins(store);           // released on every path out of the call
  PagedView view;
  const uint64_t file_len = view.append_file(store, pins, session, ids, lens, "delimiter index").second;
  if (file_len == 0) return {};
  if (view.arena_device) {
    if (!store->has_device()) throw StoreError(kErrInvalidState, "delimiter index: device dir without a device");
    store->use_device();
  }
  return run(view, 0, file_len, delim, 0, nullptr, quote, false);
}

}  // namespace amdx
