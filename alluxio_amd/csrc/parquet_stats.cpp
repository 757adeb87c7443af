#include "parquet_stats.h"

#include <atomic>
#include <string>

#include "block_store.h"
#include "kernels.h"
#include "paged_view.h"

namespace amdx {

namespace {

std::atomic<uint64_t> g_ps_launches{0};
constexpr uint64_t kMax = 1ull << 31;

void bad(const std::string& what) { throw StoreError(kErrInvalidArgument, "parquet stats: " + what); }

void pass(PsArgs a, int which, uint64_t first, uint64_t last, uint32_t round, uint64_t largest, int device,
          uint64_t stream) {
  a.first = first;
  a.last = last;
  a.round = round;
  if (first == last) return;
  if (device < 0) {
    parquet_stats_host(a, which);
    return;
  }
  AMDX_HIP(launch_parquet_stats(a, which, largest, reinterpret_cast<hipStream_t>(stream)));
  ++g_ps_launches;
}

}  // namespace

uint64_t parquet_stats_launches() { return g_ps_launches.load(); }

void parquet_stats_raw(uint64_t segs, uint64_t nsegs, uint64_t mark_first, uint64_t mark_last, uint64_t text_first,
                       uint64_t largest, uint64_t alive, uint64_t flat_n, uint64_t results, int device, uint64_t stream) {
  PsArgs a{};
  a.segs = reinterpret_cast<const int64_t*>(segs);
  a.nsegs = nsegs;
  a.alive = reinterpret_cast<uint8_t*>(alive);
  a.flat_n = flat_n;
  a.results = reinterpret_cast<int64_t*>(results);
  if (nsegs > kMax || flat_n > kMax || largest > kMax) bad("too many segments or rows for one call");
  if (mark_first > mark_last || mark_last > nsegs || text_first > nsegs) bad("a segment range lies outside the table");
  if (nsegs == 0 || largest == 0) return;
  if (!a.segs || !a.results) bad("no segment table or result rows");
  if (text_first < nsegs && !a.alive) bad("text segments and no alive bytes");
  if (device >= 0) AMDX_HIP(hipSetDevice(device));
  pass(a, kPsPassMark, mark_first, mark_last, 0, largest, device, stream);
  pass(a, kPsPassFirst, 0, nsegs, 0, largest, device, stream);
  for (uint32_t r = 1; r < kPsRounds; ++r) pass(a, kPsPassRound, text_first, nsegs, r, largest, device, stream);
}

}  // namespace amdx
