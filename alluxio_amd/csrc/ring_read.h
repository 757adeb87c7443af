// Device-cursor multi-stream sequential reader (see SeqReadArgs in kernels.h).
//
// The StressWorkerBench loop (stress/shell/.../StressWorkerBench.java:251-276: T threads each
// call read(buf) over one file and reopen at EOF) with `depth` calls per stream issued per
// launch into a per-stream ring of `depth` buffers.  The session read-locks every block of the
// file for its lifetime, uploads the file's page table once, and then each step is ONE kernel
// launch whose arguments are scalars — host work is O(1) per step, independent of the number of
// streams or calls, which is what makes small (4 KiB) reads run at HBM speed.
#pragma once
#include <cstdint>
#include <vector>

#include "kernels.h"
#include "paged_view.h"

namespace amdx {

class RingReadSession {
 public:
  RingReadSession(BlockStore* store, int64_t session, const std::vector<int64_t>& block_ids,
                  const std::vector<uint64_t>& block_lens, uint64_t dst_base, uint64_t stream_stride,
                  uint64_t buf_bytes, uint32_t depth, uint32_t streams, int dst_kind,
                  const std::vector<uint64_t>& start_offsets);
  // Remote (peer) form: the file's pages live in an arena that is already addressable from this
  // process (a peer worker's HBM mapped through HIP IPC, read over xGMI by the kernel running on
  // `device`), described by `file_pages` (arena page index per file page).  Block locks are held
  // by the caller (OpenDeviceBlock) for the session's lifetime.  device < 0: host arena (tests).
  RingReadSession(uint64_t arena_base, const std::vector<int64_t>& file_pages, uint64_t page_size,
                  uint64_t file_len, int device, uint64_t dst_base, uint64_t stream_stride, uint64_t buf_bytes,
                  uint32_t depth, uint32_t streams, int dst_kind, const std::vector<uint64_t>& start_offsets);
  ~RingReadSession();
  // One launch: every stream issues `depth` read calls.  Returns bytes read; *eofs = EOF calls
  // (reopens) in this step.
  uint64_t step(uint64_t stream, uint64_t* eofs);
  void close();
  uint64_t total_bytes() const { return total_; }
  uint64_t reopens() const { return reopens_; }
  uint64_t calls() const { return calls_per_stream_; }
  // File offset of stream s's next read.
  uint64_t position(uint32_t s) const;
  // (file offset, length) of stream s's k-th call in the most recent step (length 0 = EOF).
  std::pair<uint64_t, uint64_t> last_call(uint32_t s, uint32_t k) const;
  uint64_t file_len() const { return file_len_; }

 private:
  // bytes and EOF calls of `depth` consecutive calls of one stream whose first call index is
  // c0 < cycle; no division (full_passes_ and rem_calls_ are fixed at construction)
  uint64_t step_bytes(uint64_t c0, uint64_t* eofs) const;
  void check_shape();
  void finish_init(const std::vector<uint64_t>& start_offsets);
  void set_device() const;
  BlockStore* store_;                       // null for the remote form
  int64_t session_;
  std::vector<int64_t> blocks_;
  BlockPins pins_;                          // read locks on blocks_ for the session's lifetime
  uint64_t file_len_ = 0, buf_, stride_, dst_;
  uint32_t depth_, streams_, cycle_;
  int kind_;
  bool on_device_ = false;
  int device_ = -1;
  PagedView view_;                          // the file's pages
  std::vector<uint64_t> c_init_;
  uint64_t footprint_ = 0;   // distinct file bytes one step touches (see finish_init)
  bool lockstep_ = false;    // every stream starts at the same call: one accounting serves all
  uint32_t full_passes_ = 0, rem_calls_ = 0;   // depth / cycle, depth % cycle
  uint64_t base_mod_ = 0;    // calls_per_stream_ % cycle, carried from step to step
  uint32_t file_pages_ = 0, inline_pages_ = 0;   // pages of the file; entries a launch carries (0: none)
  SeqReadPlan plan_;         // kernel and grid of this session's launches (see plan_seq_read)
  DevBuf d_ftab_, d_cinit_;
  uint64_t calls_per_stream_ = 0, total_ = 0, reopens_ = 0;
  bool closed_ = false;
};

}  // namespace amdx
