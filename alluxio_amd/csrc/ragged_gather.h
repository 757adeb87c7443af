// Device-planned gather of variable-length records (see RaggedGatherArgs in kernels.h).
//
// A dataset of ragged records (tokenised documents, encoded images) laid end to end in cached
// files.  The session read-locks every block for its lifetime and uploads three tables once: the
// virtual page table of the files (each file starts on a fresh virtual page) and the start and
// length of every record.  A batch is then two launches: the record numbers go into a pinned
// buffer of the session, which the plan kernel reads (or, set_index_copy, a hipMemcpyAsync moves
// first); the host does one pass over the numbers to check them and size the grid, and nothing per
// page.  With a host arena (DRAM dirs, CPU-only builds) the same call is a plain loop
// of memcpy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "paged_view.h"

namespace amdx {

struct RaggedLayout {
  bool padded = false;
  uint32_t align = 16;       // packed: row starts are multiples of align (power of two, 1..256)
  uint64_t row_stride = 0;   // padded
  uint32_t max_len = 0;      // padded
  uint32_t pad_value = 0;    // padded
};

class RaggedGatherSession {
 public:
  using FileBlocks = std::pair<std::vector<int64_t>, std::vector<uint64_t>>;   // (block ids, block lengths)
  // offsets[f]: n+1 monotone record offsets inside file f.
  RaggedGatherSession(BlockStore* store, int64_t session, const std::vector<FileBlocks>& files,
                      const std::vector<std::vector<uint64_t>>& offsets);
  // Raw-arena form: `pages` maps virtual page -> arena page of an arena that is addressable from
  // this process; rec_start are virtual byte addresses.  device < 0: host memory.  Block locks, if
  // any, are the caller's.
  RaggedGatherSession(uint64_t arena_base, const std::vector<int64_t>& pages, uint64_t page_size, int device,
                      const std::vector<uint64_t>& rec_start, const std::vector<uint32_t>& rec_len);
  ~RaggedGatherSession();
  // Gather records idx[0..batch) into dst (dst_kind: MemKind of dst, out_off and out_len).
  // Validates first and throws StoreError without touching dst.  Returns the bytes of dst the
  // batch occupies (out_off[batch]); *data_bytes = sum of out_len.  Device destinations: the work
  // is queued on `stream` (calls of one session must use one stream at a time).
  uint64_t gather(const int64_t* idx, uint64_t batch, uint64_t dst, uint64_t capacity, uint64_t out_off,
                  uint64_t out_len, const RaggedLayout& lay, int dst_kind, uint64_t stream, uint64_t* data_bytes);
  void close();
  uint64_t records() const { return rec_len_.size(); }
  bool arena_on_device() const { return view_.arena_device; }
  uint64_t gathers() const { return gathers_; }
  // A/B: true = the record numbers go to a device buffer with hipMemcpyAsync before the plan;
  // false (default) = the plan kernel reads them from the pinned buffer.
  static void set_index_copy(bool on);

 private:
  void finish_init();
  void set_device() const;
  BlockStore* store_;
  int64_t session_ = 0;
  BlockPins pins_;              // read locks on every block for the session's lifetime
  int device_ = -1;
  bool on_device_ = false;      // kernels available (a device is in use)
  PagedView view_;              // the files, each starting on a fresh virtual page
  std::vector<uint64_t> rec_start_;
  std::vector<uint32_t> rec_len_;
  DevBuf d_vtab_, d_recs_, d_idx_, d_rows_, d_chunk_pre_;
  // Pinned index buffers: a ring, so the host may queue this many gathers ahead of the device.
  // Each is sized (and grown) to the batches it carried.
  static constexpr int kSlots = 64;
  int64_t* h_idx_[kSlots] = {};
  uint64_t h_cap_[kSlots] = {};
  hipEvent_t ev_[kSlots] = {};
  bool ev_used_[kSlots] = {};
  int slot_ = 0;
  uint64_t last_stream_ = 0;
  uint64_t gathers_ = 0;
  bool closed_ = false;
};

}  // namespace amdx
