// Host form of the delimiter index (see DelimIndexArgs in kernels.h): a memchr loop per page of a
// virtual byte range behind a page table, and its quoted form, which carries the state "inside
// quotes" along.  No HIP include, so a stand-alone program can compile it.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "paged_view_host.h"

namespace amdx {

// Appends add + (offset in the range) + 1 for every byte of [vstart, vstart + bytes) that equals
// `delim`, ascending.  The caller has checked that the range lies inside vtab.
inline void delim_index_host(const uint8_t* arena, const int64_t* vtab, uint32_t page_shift, uint64_t vstart,
                             uint64_t bytes, uint8_t delim, uint64_t add, std::vector<uint64_t>* out) {
  for_each_page_run(arena, vtab, page_shift, vstart, bytes, [&](const uint8_t* p, uint64_t n, uint64_t done) {
    const uint8_t* e = p + n;
    for (const uint8_t* q = p; q < e; ++q) {
      q = static_cast<const uint8_t*>(std::memchr(q, delim, (size_t)(e - q)));
      if (!q) break;
      out->push_back(add + done + (uint64_t)(q - p) + 1);
    }
  });
}

// The quoted form: a byte equal to `quote` (!= delim) toggles the state "inside quotes", which is
// `in_quote` at vstart, and only a delimiter outside quotes is a cut.  Same contract otherwise.
// Returns the state after the last byte.
inline bool delim_index_host_quoted(const uint8_t* arena, const int64_t* vtab, uint32_t page_shift, uint64_t vstart,
                                    uint64_t bytes, uint8_t delim, uint8_t quote, bool in_quote, uint64_t add,
                                    std::vector<uint64_t>* out) {
  bool inside = in_quote;
  for_each_page_run(arena, vtab, page_shift, vstart, bytes, [&](const uint8_t* p, uint64_t n, uint64_t done) {
    const uint8_t* e = p + n;
    const uint8_t* q = p;
    while (q < e) {
      if (inside) {                                 // nothing counts up to the closing quote
        q = static_cast<const uint8_t*>(std::memchr(q, quote, (size_t)(e - q)));
        if (!q) break;
        inside = false;
        ++q;
        continue;
      }
      const uint8_t b = *q++;
      if (b == quote) inside = true;
      else if (b == delim) out->push_back(add + done + (uint64_t)(q - p));
    }
  });
  return inside;
}

}  // namespace amdx
