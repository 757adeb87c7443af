#include "ring_read.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "kernels.h"

namespace amdx {

RingReadSession::RingReadSession(BlockStore* store, int64_t session, const std::vector<int64_t>& block_ids,
                                 const std::vector<uint64_t>& block_lens, uint64_t dst_base,
                                 uint64_t stream_stride, uint64_t buf_bytes, uint32_t depth, uint32_t streams,
                                 int dst_kind, const std::vector<uint64_t>& start_offsets)
    : store_(store), session_(session), blocks_(block_ids), pins_(store), buf_(buf_bytes), stride_(stream_stride),
      dst_(dst_base), depth_(depth), streams_(streams), kind_(dst_kind) {
  if (block_ids.size() != block_lens.size() || block_ids.empty())
    throw StoreError(kErrInvalidArgument, "ring read: bad block list");
  for (uint64_t l : block_lens) file_len_ += l;
  check_shape();
  view_.append_file(store_, pins_, session_, blocks_, block_lens, "ring read");
  on_device_ = store_->has_device();   // a store with a device reads a DRAM dir through the kernel too
  finish_init(start_offsets);
}

RingReadSession::RingReadSession(uint64_t arena_base, const std::vector<int64_t>& file_pages, uint64_t page_size,
                                 uint64_t file_len, int device, uint64_t dst_base, uint64_t stream_stride,
                                 uint64_t buf_bytes, uint32_t depth, uint32_t streams, int dst_kind,
                                 const std::vector<uint64_t>& start_offsets)
    : store_(nullptr), session_(0), pins_(nullptr), file_len_(file_len), buf_(buf_bytes), stride_(stream_stride),
      dst_(dst_base), depth_(depth), streams_(streams), kind_(dst_kind), on_device_(device >= 0), device_(device) {
  check_shape();
  view_ = PagedView::raw(arena_base, file_pages, page_size, device, "ring read");
  if (view_.vtab.size() < (file_len_ + page_size - 1) / page_size)
    throw StoreError(kErrInvalidArgument, "ring read: page table shorter than the file");
  finish_init(start_offsets);
}

void RingReadSession::check_shape() {
  if (buf_ == 0 || depth_ == 0 || streams_ == 0 || streams_ > kSeqReadMaxStreams)
    throw StoreError(kErrInvalidArgument, "ring read: bad buffer/depth/stream count");
  if (stride_ < (uint64_t)depth_ * buf_) throw StoreError(kErrInvalidArgument, "ring read: stride too small");
  if (file_len_ == 0) throw StoreError(kErrInvalidArgument, "ring read: empty file");
  const uint64_t calls = (file_len_ + buf_ - 1) / buf_;
  if (calls + 1 >= (1ull << 32)) throw StoreError(kErrInvalidArgument, "ring read: too many calls per pass");
  cycle_ = (uint32_t)(calls + 1);
  full_passes_ = depth_ / cycle_;
  rem_calls_ = depth_ % cycle_;
}

void RingReadSession::set_device() const {
  if (store_) store_->use_device();
  else if (device_ >= 0) AMDX_HIP(hipSetDevice(device_));
}

void RingReadSession::finish_init(const std::vector<uint64_t>& start_offsets) {
  c_init_.assign(streams_, 0);
  for (uint32_t s = 0; s < streams_ && s < start_offsets.size(); ++s) {
    if (start_offsets[s] % buf_) throw StoreError(kErrInvalidArgument, "ring read: start offsets must be buffer aligned");
    c_init_[s] = std::min<uint64_t>(start_offsets[s] / buf_, cycle_ - 1);
  }
  // streams that start at distinct calls read distinct bytes each step (lockstep streams re-read
  // the same depth*buf window): the kernel's cache policy keys on this footprint
  std::vector<uint64_t> starts(c_init_);
  std::sort(starts.begin(), starts.end());
  const uint64_t distinct = (uint64_t)(std::unique(starts.begin(), starts.end()) - starts.begin());
  footprint_ = std::min<uint64_t>(file_len_, distinct * depth_ * buf_);
  lockstep_ = distinct == 1;
  // page entries a launch carries in its arguments: only where page numbers and entries fit 32 bits
  const uint64_t pages = (file_len_ + (1ull << view_.page_shift) - 1) >> view_.page_shift;
  bool fit = pages < (1ull << 32) && pages <= view_.vtab.size();
  for (uint64_t p = 0; fit && p < pages; ++p) fit = view_.vtab[p] >= 0 && view_.vtab[p] < (int64_t)(1ull << 32);
  if (fit) {
    file_pages_ = (uint32_t)pages;
    inline_pages_ = kSeqInlinePages;
  }
  if (on_device_) {
    if (buf_ & 15 || stride_ & 15 || dst_ & 15)
      throw StoreError(kErrInvalidArgument, "ring read: buffer size, stride and ring base must be 16-byte aligned");
    set_device();
    d_ftab_.alloc(view_.vtab.size() * sizeof(int64_t));
    d_cinit_.alloc(c_init_.size() * sizeof(uint64_t));
    AMDX_HIP(hipMemcpy(d_ftab_.p, view_.vtab.data(), view_.vtab.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    AMDX_HIP(hipMemcpy(d_cinit_.p, c_init_.data(), c_init_.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  }
}

RingReadSession::~RingReadSession() {
  try {
    close();
  } catch (...) {
  }
}

void RingReadSession::close() {
  if (closed_) return;
  closed_ = true;
  d_ftab_.reset();
  d_cinit_.reset();
  pins_.release();
}

uint64_t RingReadSession::step_bytes(uint64_t c0, uint64_t* eofs) const {
  // depth = full_passes_ * cycle + rem_calls_: every full pass reads the file once and ends in one
  // EOF call; the other rem_calls_ calls are [c0, c1) with c1 < 2 * cycle
  auto before = [this](uint64_t x) {                     // bytes of calls [0, x), x < 2 * cycle
    return x < cycle_ ? std::min<uint64_t>(x * buf_, file_len_)
                      : file_len_ + std::min<uint64_t>((x - cycle_) * buf_, file_len_);
  };
  const uint64_t c1 = c0 + rem_calls_;
  *eofs = (uint64_t)full_passes_ + (c1 >= cycle_ ? 1 : 0);
  return (uint64_t)full_passes_ * file_len_ + before(c1) - before(c0);
}

uint64_t RingReadSession::step(uint64_t stream, uint64_t* eofs) {
  if (closed_) throw StoreError(kErrInvalidState, "ring read session closed");
  const uint64_t base = calls_per_stream_;
  if (on_device_) {
    set_device();
    SeqReadArgs a;
    a.arena = view_.base();
    a.ftab = d_ftab_.as<int64_t>();
    a.c_init = d_cinit_.as<uint64_t>();
    a.dst = reinterpret_cast<uint8_t*>(dst_);
    a.stream_stride = stride_;
    a.file_len = file_len_;
    a.buf = buf_;
    a.launch_base = base;
    a.base_mod = base_mod_;
    a.cycle = cycle_;
    a.streams = streams_;
    a.depth = depth_;
    a.page_shift = view_.page_shift;
    a.footprint = footprint_;
    // what the kernel would otherwise look up before its first load: the shared cursor, and the
    // page entries from the launch's earliest call on (stream 0's where the cursors differ); after
    // the file's last page comes page 0, as call 0 follows the EOF call
    a.cursor_set = lockstep_;
    a.c_uniform = c_init_[0];
    uint64_t first = c_init_[0] + base_mod_;
    if (first >= cycle_) first -= cycle_;
    uint64_t page = first == cycle_ - 1 ? 0 : (first * buf_) >> view_.page_shift;
    a.page_first = (uint32_t)page;
    a.file_pages = file_pages_;
    a.page_n = inline_pages_;
    for (uint32_t i = 0; i < inline_pages_; ++i) {
      a.page_tab[i] = (uint32_t)view_.vtab[page];
      if (++page == file_pages_) page = 0;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // kernel, persistent grid and shifts are the session's until the variant is set anew
    if (plan_.epoch != seq_read_epoch()) AMDX_HIP(plan_seq_read(a, &plan_));
    AMDX_HIP(launch_seq_plan(plan_, a, st));
    if (kind_ == (int)MemKind::kHost) AMDX_HIP(hipStreamSynchronize(st));
  } else {
    // CPU-only build/test path: same schedule with memcpy from the host arena
    for (uint32_t s = 0; s < streams_; ++s)
      for (uint32_t k = 0; k < depth_; ++k) {
        auto [off, len] = std::pair<uint64_t, uint64_t>(0, 0);
        const uint64_t c = (c_init_[s] + base_mod_ + k) % cycle_;
        if (c == cycle_ - 1) continue;
        off = c * buf_;
        len = std::min(buf_, file_len_ - off);
        uint8_t* d = reinterpret_cast<uint8_t*>(dst_ + s * stride_ + (uint64_t)k * buf_);
        for_each_page_run(view_.base(), view_.vtab.data(), view_.page_shift, off, len,
                          [d](const uint8_t* p, uint64_t n, uint64_t done) { std::memcpy(d + done, p, n); });
      }
  }
  // accounting without a division: c_init_[s] and base_mod_ are both below cycle
  auto first_call = [this](uint32_t s) {
    const uint64_t c = c_init_[s] + base_mod_;
    return c >= cycle_ ? c - cycle_ : c;
  };
  uint64_t bytes = 0, eof = 0;
  if (lockstep_) {
    bytes = step_bytes(first_call(0), &eof) * streams_;
    eof *= streams_;
  } else {
    for (uint32_t s = 0; s < streams_; ++s) {
      uint64_t e = 0;
      bytes += step_bytes(first_call(s), &e);
      eof += e;
    }
  }
  calls_per_stream_ += depth_;
  base_mod_ += rem_calls_;                                // (base + depth) % cycle
  if (base_mod_ >= cycle_) base_mod_ -= cycle_;
  total_ += bytes;
  reopens_ += eof;
  if (store_) store_->access_blocks(blocks_);
  if (eofs) *eofs = eof;
  return bytes;
}

uint64_t RingReadSession::position(uint32_t s) const {
  const uint64_t c = (c_init_.at(s) + calls_per_stream_) % cycle_;
  return std::min<uint64_t>(c * buf_, file_len_);
}

std::pair<uint64_t, uint64_t> RingReadSession::last_call(uint32_t s, uint32_t k) const {
  if (calls_per_stream_ < depth_) return {0, 0};
  const uint64_t c = (c_init_.at(s) + calls_per_stream_ - depth_ + k) % cycle_;
  if (c == cycle_ - 1) return {file_len_, 0};
  const uint64_t off = c * buf_;
  return {off, std::min(buf_, file_len_ - off)};
}

}  // namespace amdx
