#include "delim_index.h"

#include <atomic>
#include <string>

#include "delim_index_host.h"
#include "kernels.h"

namespace amdx {

#define DI_HIP(expr)                                                                           \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      throw StoreError(kErrHip, std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr); \
  } while (0)

namespace {

std::atomic<uint64_t> g_launches{0};

void bad(const std::string& what) { throw StoreError(kErrInvalidArgument, "delimiter index: " + what); }

void check_quote(uint32_t delim, int64_t quote, bool in_quote) {
  if (delim > 255) bad("the delimiter is one byte");
  if (quote < -1 || quote > 255) bad("the quote is one byte");
  if (quote == (int64_t)delim) bad("the quote equals the delimiter");
  if (in_quote && quote < 0) bad("in_quote without a quote");
}

// Device allocations and events of one call: released on every path out of it.
struct DevMem {
  void* p = nullptr;
  DevMem() = default;
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  void alloc(size_t n) { DI_HIP(hipMalloc(&p, n ? n : 1)); }
  ~DevMem() {
    if (p) (void)hipFree(p);
  }
};
struct Events {
  hipEvent_t e[4] = {};
  Events() = default;
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  void create() {
    for (auto& x : e) DI_HIP(hipEventCreate(&x));
  }
  ~Events() {
    for (auto& x : e)
      if (x) (void)hipEventDestroy(x);
  }
};

uint32_t shift_of(uint64_t page_size) {
  if (page_size < 16 || (page_size & (page_size - 1))) bad("page size must be a power of two");
  uint32_t s = 0;
  while ((1ull << s) < page_size) ++s;
  return s;
}

// The range has been validated against vtab.  on_device: the arena is device memory of the
// current device.
std::vector<uint64_t> run(uint64_t arena, const std::vector<int64_t>& vtab, uint32_t page_shift, bool on_device,
                          uint64_t vstart, uint64_t bytes, uint32_t delim, uint64_t add, DelimIndexTimes* times,
                          int64_t quote, bool in_quote) {
  std::vector<uint64_t> out;
  if (bytes == 0) return out;
  const bool quoted = quote >= 0;
  if (!on_device) {
    if (quoted)
      delim_index_host_quoted(reinterpret_cast<const uint8_t*>(arena), vtab.data(), page_shift, vstart, bytes,
                              (uint8_t)delim, (uint8_t)quote, in_quote, add, &out);
    else
      delim_index_host(reinterpret_cast<const uint8_t*>(arena), vtab.data(), page_shift, vstart, bytes, (uint8_t)delim,
                     add, &out);
    return out;
  }
  if (arena & 15) bad("arena base must be 16-byte aligned");
  DelimIndexArgs a{};
  a.tile_shift = delim_index_tile_shift();
  const uint64_t nt = delim_index_tiles(vstart, bytes, a.tile_shift);
  if (nt > (1ull << 30)) bad("range too large for one call");
  DevMem d_vtab, d_count, d_base, d_out, d_odd, d_parity;
  Events ev;
  // only the pages the range touches travel
  const uint64_t p0 = vstart >> page_shift, p1 = (vstart + bytes - 1) >> page_shift;
  d_vtab.alloc((p1 - p0 + 1) * sizeof(int64_t));
  d_count.alloc(nt * sizeof(uint32_t));
  d_base.alloc((nt + 1) * sizeof(uint64_t));
  DI_HIP(hipMemcpy(d_vtab.p, vtab.data() + p0, (p1 - p0 + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  a.arena = reinterpret_cast<const uint8_t*>(arena);
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
    DI_HIP(hipEventRecord(ev.e[0], st));
  }
  DI_HIP(quoted ? launch_delim_count_quoted(a, st) : launch_delim_count(a, st));
  ++g_launches;
  if (times) DI_HIP(hipEventRecord(ev.e[1], st));
  DI_HIP(quoted ? launch_delim_scan_quoted(a, st) : launch_delim_scan(a, st));
  ++g_launches;
  if (times) DI_HIP(hipEventRecord(ev.e[2], st));
  uint64_t total = 0;
  DI_HIP(hipMemcpy(&total, a.tile_base + nt, sizeof(total), hipMemcpyDeviceToHost));   // the one synchronising read
  if (total > bytes) throw StoreError(kErrInvalidState, "delimiter index: more delimiters than bytes");
  if (total) {
    d_out.alloc(total * sizeof(uint64_t));
    a.out = static_cast<uint64_t*>(d_out.p);
    a.out_cap = total;
    DI_HIP(quoted ? launch_delim_emit_quoted(a, total, st) : launch_delim_emit(a, total, st));
    ++g_launches;
  }
  if (times) {
    DI_HIP(hipEventRecord(ev.e[3], st));
    DI_HIP(hipEventSynchronize(ev.e[3]));
    DI_HIP(hipEventElapsedTime(&times->count_ms, ev.e[0], ev.e[1]));
    DI_HIP(hipEventElapsedTime(&times->scan_ms, ev.e[1], ev.e[2]));
    DI_HIP(hipEventElapsedTime(&times->emit_ms, ev.e[2], ev.e[3]));
  }
  if (total) {
    out.resize(total);
    DI_HIP(hipMemcpy(out.data(), d_out.p, total * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  return out;
}

struct Locks {
  BlockStore* store;
  std::vector<int64_t> ids;
  explicit Locks(BlockStore* s) : store(s) {}
  Locks(const Locks&) = delete;
  Locks& operator=(const Locks&) = delete;
  ~Locks() {
    for (int64_t l : ids) {
      try {
        store->unlock(l);
      } catch (...) {
      }
    }
  }
};

}  // namespace

uint64_t delim_index_launches() { return g_launches.load(); }

std::vector<uint64_t> delim_index_raw(uint64_t arena_base, const std::vector<int64_t>& pages, uint64_t page_size,
                                      int device, uint64_t vstart, uint64_t bytes, uint32_t delim, uint64_t add,
                                      DelimIndexTimes* times, int64_t quote, bool in_quote) {
  const uint32_t page_shift = shift_of(page_size);
  check_quote(delim, quote, in_quote);
  const uint64_t vbytes = (uint64_t)pages.size() << page_shift;
  if (vstart > vbytes || bytes > vbytes - vstart) bad("range outside the page table");
  for (int64_t p : pages)
    if (p < 0) bad("negative arena page");
  if (device >= 0) DI_HIP(hipSetDevice(device));
  return run(arena_base, pages, page_shift, device >= 0, vstart, bytes, delim, add, times, quote, in_quote);
}

std::vector<uint64_t> delim_index_store(BlockStore* store, int64_t session, const std::vector<int64_t>& ids,
                                        const std::vector<uint64_t>& lens, uint32_t delim, int64_t quote) {
  if (ids.size() != lens.size()) bad("bad block list");
  check_quote(delim, quote, false);
  Locks locks(store);
  std::vector<int64_t> vtab;
  int dir0 = -1;
  uint64_t page_size = 0, arena = 0, file_len = 0;
  uint32_t page_shift = 0;
  bool arena_device = false;
  for (size_t b = 0; b < ids.size(); ++b) {
    locks.ids.push_back(store->lock_block(session, ids[b], false, -1));
    int dir = -1;
    uint64_t ps = 0, base = 0;
    std::vector<int64_t> pages = store->block_pages(ids[b], &dir, &ps, &base);
    const DirSpec spec = store->dir_spec(dir);
    if (spec.kind == DirKind::kFile) bad("block in a file tier");
    if (dir0 < 0) {
      dir0 = dir;
      page_size = ps;
      arena = base;
      arena_device = spec.kind == DirKind::kDevice;
      page_shift = shift_of(ps);
    } else if (dir != dir0) {
      bad("blocks span several dirs");
    }
    const uint64_t np = (lens[b] + ps - 1) / ps;
    if (b + 1 < ids.size() && lens[b] % ps != 0) bad("block size must be a multiple of the page size");
    if (pages.size() < np) throw StoreError(kErrInvalidState, "delimiter index: block shorter than its length");
    for (uint64_t i = 0; i < np; ++i)
      if (pages[i] < 0) throw StoreError(kErrInvalidState, "delimiter index: block without a page");
    vtab.insert(vtab.end(), pages.begin(), pages.begin() + np);
    file_len += lens[b];
  }
  if (file_len == 0) return {};
  if (arena_device) {
    if (!store->has_device()) throw StoreError(kErrInvalidState, "delimiter index: device dir without a device");
    store->use_device();
  }
  return run(arena, vtab, page_shift, arena_device, 0, file_len, delim, 0, nullptr, quote, false);
}

}  // namespace amdx
