// What ring read, ragged gather and the delimiter index share on the host: the read-locked blocks
// of cached files seen as one virtual page table over one arena, the device buffers such tables
// are uploaded into, and the HIP error check.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "block_store.h"
#include "paged_view_host.h"

namespace amdx {

#define AMDX_HIP(expr)                                                                         \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess)                                                                      \
      throw StoreError(kErrHip, std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr); \
  } while (0)

// One device allocation, freed on every path out of its scope.  Move-only.
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
  DevBuf& operator=(DevBuf&&) = delete;
  ~DevBuf() { reset(); }
  void alloc(size_t n) {           // at least one byte, so an empty table still has an address
    reset();
    AMDX_HIP(hipMalloc(&p, n ? n : 1));
  }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// Read locks on blocks of one store.  release() and the destructor unlock every one; an unlock that
// throws does not keep the others locked.  Move-only.
class BlockPins {
 public:
  explicit BlockPins(BlockStore* store) : store_(store) {}
  BlockPins(BlockPins&& o) noexcept : store_(o.store_), locks_(std::move(o.locks_)) {}
  BlockPins& operator=(BlockPins&&) = delete;
  ~BlockPins() { release(); }
  void lock(int64_t session, int64_t block_id) { locks_.push_back(store_->lock_block(session, block_id, false, -1)); }
  void release() noexcept;

 private:
  BlockStore* store_;
  std::vector<int64_t> locks_;
};

// The virtual page table: virtual page v is arena page vtab[v] of the arena of one memory dir.
struct PagedView {
  uint64_t arena = 0, page_size = 0;
  uint32_t page_shift = 0;
  int dir = -1;
  bool arena_device = false;       // the arena is device memory (not host-readable)
  std::vector<int64_t> vtab;

  // Raw form: the caller names the arena (device < 0: host memory) and its pages.  `who` prefixes
  // every message, here and below.
  static PagedView raw(uint64_t arena, const std::vector<int64_t>& pages, uint64_t page_size, int device,
                       const std::string& who);
  // Read-locks the blocks (ids, lens) of one file into `pins` and appends their pages, starting on
  // a fresh virtual page.  Returns {first virtual page, file length}.  kErrInvalidArgument: lists
  // of different sizes, a block in a file tier, blocks in more than one dir, a block but the last
  // that does not end on a page, a page size that is no power of two >= 16.  kErrInvalidState: a
  // block with fewer pages than its length needs, or with a negative page among them.
  std::pair<uint64_t, uint64_t> append_file(BlockStore* store, BlockPins& pins, int64_t session,
                                            const std::vector<int64_t>& ids, const std::vector<uint64_t>& lens,
                                            const std::string& who);
  const uint8_t* base() const { return reinterpret_cast<const uint8_t*>(arena); }
  uint64_t bytes() const { return (uint64_t)vtab.size() << page_shift; }
};

}  // namespace amdx
