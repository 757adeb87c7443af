// Host side of a virtual byte range behind a page table: page v of the range is arena page
// vtab[v].  No HIP include, so a stand-alone program can compile it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>

#include "store_error.h"

namespace amdx {

// log2 of a page size.  The one place that demands a power of two >= 16: the kernels read 16-byte
// vectors that must not straddle a page.  `who` prefixes the message.
inline uint32_t page_shift_of(uint64_t page_size, const std::string& who) {
  if (page_size < 16 || (page_size & (page_size - 1)))
    throw StoreError(kErrInvalidArgument, who + ": page size must be a power of two");
  uint32_t s = 0;
  while ((1ull << s) < page_size) ++s;
  return s;
}

// Calls fn(p, n, done) for every piece of [va, va + len) that lies inside one page, ascending:
// p = the piece's first byte, n = its length, done = bytes of the range before it.  The caller has
// checked that the range lies inside vtab.
template <class Fn>
inline void for_each_page_run(const uint8_t* arena, const int64_t* vtab, uint32_t page_shift, uint64_t va,
                              uint64_t len, Fn&& fn) {
  const uint64_t psize = 1ull << page_shift, pmask = psize - 1;
  uint64_t done = 0;
  while (done < len) {
    const uint64_t a = va + done, po = a & pmask;
    const uint64_t n = std::min(len - done, psize - po);
    fn(arena + ((uint64_t)vtab[a >> page_shift] << page_shift) + po, n, done);
    done += n;
  }
}

}  // namespace amdx
