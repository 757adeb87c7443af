#include "paged_view.h"

namespace amdx {

void BlockPins::release() noexcept {
  for (int64_t l : locks_) {
    try {
      store_->unlock(l);
    } catch (...) {
    }
  }
  locks_.clear();
}

PagedView PagedView::raw(uint64_t arena, const std::vector<int64_t>& pages, uint64_t page_size, int device,
                         const std::string& who) {
  PagedView v;
  v.arena = arena;
  v.page_size = page_size;
  v.page_shift = page_shift_of(page_size, who);
  v.arena_device = device >= 0;
  for (int64_t p : pages)
    if (p < 0) throw StoreError(kErrInvalidArgument, who + ": negative arena page");
  v.vtab = pages;
  return v;
}

std::pair<uint64_t, uint64_t> PagedView::append_file(BlockStore* store, BlockPins& pins, int64_t session,
                                                     const std::vector<int64_t>& ids,
                                                     const std::vector<uint64_t>& lens, const std::string& who) {
  auto bad = [&](const char* what) { throw StoreError(kErrInvalidArgument, who + ": " + what); };
  if (ids.size() != lens.size()) bad("bad block list");
  const uint64_t vpage0 = vtab.size();
  uint64_t file_len = 0;
  for (size_t b = 0; b < ids.size(); ++b) {
    pins.lock(session, ids[b]);
    int d = -1;
    uint64_t ps = 0, base = 0;
    const std::vector<int64_t> pages = store->block_pages(ids[b], &d, &ps, &base);
    const DirSpec spec = store->dir_spec(d);
    if (spec.kind == DirKind::kFile) bad("block in a file tier");
    if (dir < 0) {
      dir = d;
      page_size = ps;
      arena = base;
      arena_device = spec.kind == DirKind::kDevice;
      page_shift = page_shift_of(ps, who);
    } else if (d != dir) {
      bad("blocks span several dirs");
    }
    const uint64_t np = (lens[b] + ps - 1) / ps;
    if (b + 1 < ids.size() && lens[b] % ps != 0) bad("block size must be a multiple of the page size");
    if (pages.size() < np) throw StoreError(kErrInvalidState, who + ": block shorter than its length");
    for (uint64_t i = 0; i < np; ++i)
      if (pages[i] < 0) throw StoreError(kErrInvalidState, who + ": block without a page");
    vtab.insert(vtab.end(), pages.begin(), pages.begin() + np);
    file_len += lens[b];
  }
  return {vpage0, file_len};
}

}  // namespace amdx
