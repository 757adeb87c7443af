#include "text_dict.h"

#include <atomic>
#include <string>

#include "block_store.h"
#include "kernels.h"
#include "paged_view.h"

namespace amdx {

namespace {

std::atomic<uint64_t> g_launches{0};
std::atomic<int> g_hash_bits{64};

void bad(const std::string& what) { throw StoreError(kErrInvalidArgument, "text dictionary: " + what); }

TextDictArgs common(uint64_t table, uint64_t capacity, uint64_t n, uint64_t D) {
  TextDictArgs a{};
  a.table = reinterpret_cast<uint64_t*>(table);
  a.capacity = capacity;
  a.in.n = n;
  a.D = D;
  a.hash_bits = g_hash_bits.load();
  if (!td_pow2(capacity) || capacity > kTdMaxCapacity) bad("the capacity is a power of two, at most 2^31");
  if (n > kTdMaxRows) bad("too many values for one call");
  if (!text_dict_scalars_ok(a)) bad("too many entries");
  return a;
}

template <class Host, class Launch>
void run(const TextDictArgs& a, int device, uint64_t stream, Host host, Launch launch) {
  if (device < 0) {
    host(a);
    return;
  }
  AMDX_HIP(hipSetDevice(device));
  AMDX_HIP(launch(a, reinterpret_cast<hipStream_t>(stream)));
  ++g_launches;
}

}  // namespace

uint64_t text_dict_launches() { return g_launches.load(); }

void set_text_dict_hash_bits(int bits) {
  if (bits < 0 || bits > 64) bad("hash bits are 0..64");
  g_hash_bits.store(bits);
}

int text_dict_hash_bits() { return g_hash_bits.load(); }

void text_dict_probe_raw(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status, uint64_t n,
                         int device, uint64_t ent_data, uint64_t ent_bytes, uint64_t ent_off, uint64_t D, uint64_t table,
                         uint64_t capacity, bool insert, uint64_t slot_of, uint64_t hash, uint64_t stream) {
  TextDictArgs a = common(table, capacity, n, D);
  a.in.data = reinterpret_cast<const uint8_t*>(data);
  a.in.data_bytes = data_bytes;
  a.in.start = reinterpret_cast<const int64_t*>(start);
  a.in.length = reinterpret_cast<const int32_t*>(length);
  a.in.status = reinterpret_cast<const uint8_t*>(status);
  a.in.quote = -1;
  a.ent_data = reinterpret_cast<const uint8_t*>(ent_data);
  a.ent_bytes = ent_bytes;
  a.ent_off = reinterpret_cast<int64_t*>(ent_off);
  a.ent_cap = D;
  a.insert = insert ? 1 : 0;
  a.slot_of = reinterpret_cast<int32_t*>(slot_of);
  a.hash = reinterpret_cast<uint64_t*>(hash);
  if (!text_dict_probe_fits(a)) bad("the table is too small: capacity >= 2 * (entries + new values)");
  if (n == 0) return;
  if (!a.in.data && data_bytes) bad("no data");
  if (!a.in.start || !a.in.length) bad("no spans");
  if (!a.table) bad("no table");
  if (!a.slot_of || !a.hash) bad("no output arrays");
  if (D && (!a.ent_off || (!a.ent_data && ent_bytes))) bad("no entries");
  run(a, device, stream, text_dict_probe_host, launch_text_dict_probe);
}

void text_dict_first_raw(uint64_t table, uint64_t capacity, uint64_t slot_of, uint64_t length, uint64_t n, int device,
                         uint64_t first, uint64_t first_len, uint64_t stream) {
  TextDictArgs a = common(table, capacity, n, 0);
  a.slot_of = reinterpret_cast<int32_t*>(slot_of);
  a.in.length = reinterpret_cast<const int32_t*>(length);
  a.first = reinterpret_cast<int32_t*>(first);
  a.first_len = reinterpret_cast<int32_t*>(first_len);
  if (n == 0) return;
  if (!a.table || !a.slot_of || !a.in.length) bad("no input arrays");
  if (!a.first || !a.first_len) bad("no output arrays");
  run(a, device, stream, text_dict_first_host, launch_text_dict_first);
}

void text_dict_codes_raw(uint64_t table, uint64_t capacity, uint64_t slot_of, uint64_t rank, uint64_t n, uint64_t D,
                         int device, uint64_t codes, uint64_t stream) {
  TextDictArgs a = common(table, capacity, n, D);
  a.slot_of = reinterpret_cast<int32_t*>(slot_of);
  a.rank = reinterpret_cast<const int64_t*>(rank);
  a.codes = reinterpret_cast<int32_t*>(codes);
  if (n == 0) return;
  if (!a.table || !a.slot_of) bad("no input arrays");
  if (!a.codes) bad("no output array");
  run(a, device, stream, text_dict_codes_host, launch_text_dict_codes);
}

void text_dict_commit_raw(uint64_t table, uint64_t capacity, uint64_t slot_of, uint64_t hash, uint64_t first,
                          uint64_t rank, uint64_t byte_off, uint64_t n, uint64_t D, uint64_t ent_hash, uint64_t ent_off,
                          uint64_t ent_cap, uint64_t old_bytes, int device, uint64_t stream) {
  TextDictArgs a = common(table, capacity, n, D);
  a.slot_of = reinterpret_cast<int32_t*>(slot_of);
  a.hash = reinterpret_cast<uint64_t*>(hash);
  a.first = reinterpret_cast<int32_t*>(first);
  a.rank = reinterpret_cast<const int64_t*>(rank);
  a.byte_off = reinterpret_cast<const int64_t*>(byte_off);
  a.ent_hash = reinterpret_cast<uint64_t*>(ent_hash);
  a.ent_off = reinterpret_cast<int64_t*>(ent_off);
  a.ent_cap = ent_cap;
  a.old_bytes = old_bytes;
  if (ent_cap >= (1ull << 31) || old_bytes > (uint64_t)INT64_MAX) bad("too many entries");
  if (n == 0) return;
  if (!a.table || !a.slot_of || !a.hash || !a.first || !a.rank || !a.byte_off) bad("no input arrays");
  if (!a.ent_hash || !a.ent_off) bad("no entry arrays");
  run(a, device, stream, text_dict_commit_host, launch_text_dict_commit);
}

void text_dict_rehash_raw(uint64_t ent_hash, uint64_t D, uint64_t table, uint64_t capacity, int device, uint64_t stream) {
  TextDictArgs a = common(table, capacity, 0, D);
  a.ent_hash = reinterpret_cast<uint64_t*>(ent_hash);
  if (capacity < 2 * D) bad("the table is too small: capacity >= 2 * entries");
  if (D == 0) return;
  if (!a.table || !a.ent_hash) bad("no arrays");
  run(a, device, stream, text_dict_rehash_host, launch_text_dict_rehash);
}

}  // namespace amdx
