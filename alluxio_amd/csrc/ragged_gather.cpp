#include "ragged_gather.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "kernels.h"

namespace amdx {

static bool g_index_copy = false;
void RaggedGatherSession::set_index_copy(bool on) { g_index_copy = on; }

static void bad(const std::string& what) { throw StoreError(kErrInvalidArgument, "ragged gather: " + what); }

RaggedGatherSession::RaggedGatherSession(BlockStore* store, int64_t session, const std::vector<FileBlocks>& files,
                                         const std::vector<std::vector<uint64_t>>& offsets)
    : store_(store), session_(session), pins_(store) {
  if (files.empty() || files.size() != offsets.size()) bad("one offset array per file is required");
  for (size_t f = 0; f < files.size(); ++f) {
    const auto [vpage0, file_len] =
        view_.append_file(store_, pins_, session_, files[f].first, files[f].second, "ragged gather");
    const std::vector<uint64_t>& off = offsets[f];
    if (off.empty()) bad("an offset array needs at least one entry");
    if (off.back() > file_len) bad("record offsets run past the end of the file");
    if (off.size() > 1 && view_.dir < 0) bad("records in a file without blocks");
    const uint64_t vbase = vpage0 << view_.page_shift;
    for (size_t i = 0; i + 1 < off.size(); ++i) {
      if (off[i + 1] < off[i]) bad("record offsets must not decrease");
      if (off[i + 1] - off[i] > 0xFFFFFFFFull - 256) bad("record longer than 4 GiB");
      rec_start_.push_back(vbase + off[i]);
      rec_len_.push_back((uint32_t)(off[i + 1] - off[i]));
    }
  }
  on_device_ = view_.arena_device;
  if (on_device_ && !store_->has_device()) throw StoreError(kErrInvalidState, "ragged gather: device dir without a device");
  finish_init();
}

RaggedGatherSession::RaggedGatherSession(uint64_t arena_base, const std::vector<int64_t>& pages, uint64_t page_size,
                                         int device, const std::vector<uint64_t>& rec_start,
                                         const std::vector<uint32_t>& rec_len)
    : store_(nullptr), pins_(nullptr), device_(device), on_device_(device >= 0), rec_start_(rec_start),
      rec_len_(rec_len) {
  view_ = PagedView::raw(arena_base, pages, page_size, device, "ragged gather");
  if (rec_start_.size() != rec_len_.size()) bad("record starts and lengths differ in number");
  const uint64_t vbytes = view_.bytes();
  for (size_t i = 0; i < rec_len_.size(); ++i) {
    if (rec_len_[i] > 0xFFFFFFFFull - 256) bad("record longer than 4 GiB");
    if (rec_start_[i] > vbytes || rec_len_[i] > vbytes - rec_start_[i]) bad("record outside the page table");
  }
  finish_init();
}

void RaggedGatherSession::set_device() const {
  if (store_) store_->use_device();
  else if (device_ >= 0) AMDX_HIP(hipSetDevice(device_));
}

void RaggedGatherSession::finish_init() {
  if (!on_device_) return;
  if (view_.arena & 15) bad("arena base must be 16-byte aligned");
  set_device();
  const std::vector<int64_t>& vtab = view_.vtab;
  d_vtab_.alloc(vtab.size() * sizeof(int64_t));
  d_recs_.alloc(rec_len_.size() * sizeof(RaggedRec));
  d_idx_.alloc((size_t)kRaggedGatherMaxBatch * sizeof(int64_t));
  d_rows_.alloc((size_t)kRaggedGatherMaxBatch * sizeof(RaggedRow));
  d_chunk_pre_.alloc(((size_t)kRaggedGatherMaxBatch + 1) * sizeof(uint32_t));
  if (!vtab.empty()) AMDX_HIP(hipMemcpy(d_vtab_.p, vtab.data(), vtab.size() * sizeof(int64_t), hipMemcpyHostToDevice));
  if (!rec_len_.empty()) {
    std::vector<RaggedRec> recs(rec_len_.size());
    for (size_t i = 0; i < recs.size(); ++i) recs[i] = RaggedRec{rec_start_[i], rec_len_[i], 0};
    AMDX_HIP(hipMemcpy(d_recs_.p, recs.data(), recs.size() * sizeof(RaggedRec), hipMemcpyHostToDevice));
  }
  try {
    for (int s = 0; s < kSlots; ++s) AMDX_HIP(hipEventCreateWithFlags(&ev_[s], hipEventDisableTiming));
  } catch (...) {
    close();   // the events are no members with destructors
    throw;
  }
}

RaggedGatherSession::~RaggedGatherSession() {
  try {
    close();
  } catch (...) {
  }
}

void RaggedGatherSession::close() {
  if (closed_) return;
  closed_ = true;
  if (on_device_ && d_vtab_.p) {
    try {
      set_device();
    } catch (...) {
    }
    if (gathers_) (void)hipStreamSynchronize(reinterpret_cast<hipStream_t>(last_stream_));
  }
  for (DevBuf* b : {&d_vtab_, &d_recs_, &d_idx_, &d_rows_, &d_chunk_pre_}) b->reset();
  for (int s = 0; s < kSlots; ++s) {
    if (h_idx_[s]) (void)hipHostFree(h_idx_[s]);
    if (ev_[s]) (void)hipEventDestroy(ev_[s]);
    h_idx_[s] = nullptr;
    h_cap_[s] = 0;
    ev_[s] = nullptr;
  }
  pins_.release();
}

uint64_t RaggedGatherSession::gather(const int64_t* idx, uint64_t batch, uint64_t dst, uint64_t capacity,
                                     uint64_t out_off, uint64_t out_len, const RaggedLayout& lay, int dst_kind,
                                     uint64_t stream, uint64_t* data_bytes) {
  if (closed_) throw StoreError(kErrInvalidState, "ragged gather session closed");
  if (batch > kRaggedGatherMaxBatch) bad("batch larger than " + std::to_string(kRaggedGatherMaxBatch));
  if (lay.padded) {
    if (lay.row_stride < lay.max_len) bad("row stride smaller than max_len");
    if (lay.pad_value > 255) bad("pad value must be one byte");
  } else if (lay.align == 0 || lay.align > 256 || (lay.align & (lay.align - 1))) {
    bad("align must be a power of two from 1 to 256");
  }
  const bool to_device = dst_kind == (int)MemKind::kDevice;
  if (to_device && !on_device_) bad("device destination but the arena is host memory");
  if (!to_device && view_.arena_device) bad("host destination but the arena is device memory");
  // One pass over the record numbers: range check, total size, work items of the copy launch.
  const uint64_t n = rec_len_.size();
  const uint32_t chunk_shift = ragged_gather_chunk_shift();
  const uint64_t vpc_mask = (1ull << chunk_shift) - 1;
  uint64_t total = 0, data = 0, chunks = 0;
  for (uint64_t r = 0; r < batch; ++r) {
    const int64_t id = idx[r];
    if (id < 0 || (uint64_t)id >= n) bad("record index " + std::to_string(id) + " outside [0, " + std::to_string(n) + ")");
    uint64_t len = rec_len_[(size_t)id], adv, span;
    if (lay.padded) {
      len = std::min<uint64_t>(len, lay.max_len);
      adv = lay.row_stride;
      span = lay.max_len;
    } else {
      adv = span = (len + lay.align - 1) & ~(uint64_t)(lay.align - 1);
    }
    const uint64_t D = dst + total;
    const uint64_t nvec = span ? ((D + span + 15) >> 4) - (D >> 4) : 0;
    chunks += (nvec + vpc_mask) >> chunk_shift;
    data += len;
    total += adv;
  }
  const uint64_t need = lay.padded ? (batch ? (batch - 1) * lay.row_stride + lay.max_len : 0) : total;
  if (need > capacity)
    bad("destination holds " + std::to_string(capacity) + " bytes, the batch needs " + std::to_string(need));
  if (chunks >= (1ull << 31)) bad("batch too large for one launch");
  if (data_bytes) *data_bytes = data;
  ++gathers_;

  if (!to_device) {
    uint64_t* off = reinterpret_cast<uint64_t*>(out_off);
    uint32_t* ol = reinterpret_cast<uint32_t*>(out_len);
    uint64_t o = 0;
    for (uint64_t r = 0; r < batch; ++r) {
      const size_t id = (size_t)idx[r];
      uint64_t len = rec_len_[id], adv, span;
      if (lay.padded) {
        len = std::min<uint64_t>(len, lay.max_len);
        adv = lay.row_stride;
        span = lay.max_len;
      } else {
        adv = span = (len + lay.align - 1) & ~(uint64_t)(lay.align - 1);
      }
      uint8_t* d = reinterpret_cast<uint8_t*>(dst + o);
      for_each_page_run(view_.base(), view_.vtab.data(), view_.page_shift, rec_start_[id], len,
                        [d](const uint8_t* p, uint64_t n, uint64_t done) { std::memcpy(d + done, p, n); });
      if (span > len) std::memset(d + len, lay.padded ? (int)lay.pad_value : 0, span - len);
      off[r] = o;
      ol[r] = (uint32_t)len;
      o += adv;
    }
    off[batch] = o;
    return o;
  }

  set_device();
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (gathers_ > 1 && last_stream_ != stream)   // the workspace is ordered by one stream at a time
    AMDX_HIP(hipStreamSynchronize(reinterpret_cast<hipStream_t>(last_stream_)));
  last_stream_ = stream;
  if (batch == 0) {
    AMDX_HIP(hipMemsetAsync(reinterpret_cast<void*>(out_off), 0, sizeof(uint64_t), st));
    return 0;
  }
  const int s = slot_;
  slot_ = (slot_ + 1) % kSlots;
  if (ev_used_[s]) AMDX_HIP(hipEventSynchronize(ev_[s]));   // the upload that last used this buffer
  if (h_cap_[s] < batch) {
    if (h_idx_[s]) AMDX_HIP(hipHostFree(h_idx_[s]));
    h_idx_[s] = nullptr;
    h_cap_[s] = 0;
    uint64_t cap = 1024;
    while (cap < batch) cap <<= 1;
    AMDX_HIP(hipHostMalloc((void**)&h_idx_[s], cap * sizeof(int64_t), hipHostMallocMapped));
    h_cap_[s] = cap;
  }
  std::memcpy(h_idx_[s], idx, batch * sizeof(int64_t));
  RaggedGatherArgs a;
  if (g_index_copy) {
    AMDX_HIP(hipMemcpyAsync(d_idx_.p, h_idx_[s], batch * sizeof(int64_t), hipMemcpyHostToDevice, st));
    a.idx = d_idx_.as<int64_t>();
  } else {
    // the plan kernel is the upload: it reads the pinned buffer (one pass, 8 bytes per row)
    void* dp = nullptr;
    AMDX_HIP(hipHostGetDevicePointer(&dp, h_idx_[s], 0));
    a.idx = static_cast<const int64_t*>(dp);
  }
  a.arena = view_.base();
  a.vtab = d_vtab_.as<int64_t>();
  a.recs = d_recs_.as<RaggedRec>();
  a.dst = reinterpret_cast<uint8_t*>(dst);
  a.out_off = reinterpret_cast<uint64_t*>(out_off);
  a.out_len = reinterpret_cast<uint32_t*>(out_len);
  a.rows = d_rows_.as<RaggedRow>();
  a.chunk_pre = d_chunk_pre_.as<uint32_t>();
  a.n_rec = n;
  a.row_stride = lay.row_stride;
  a.batch = (uint32_t)batch;
  a.page_shift = view_.page_shift;
  a.align = lay.padded ? 1 : lay.align;
  a.max_len = lay.max_len;
  a.padded = lay.padded ? 1 : 0;
  a.pad_value = lay.pad_value;
  a.total_chunks = (uint32_t)chunks;
  a.chunk_shift = chunk_shift;
  AMDX_HIP(launch_ragged_gather(a, st));
  AMDX_HIP(hipEventRecord(ev_[s], st));   // the pinned buffer is free once the plan has run
  ev_used_[s] = true;
  return lay.padded ? batch * lay.row_stride : total;
}

}  // namespace amdx
