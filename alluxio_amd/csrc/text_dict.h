// Dictionary encoding of text values (first-occurrence codes that persist across calls), done
// where the values lie: the kernels of text_dict.hip for device memory, the loops of
// text_dict_host.h for host memory.  Both follow the rule in text_dict_host.h and give the same
// codes and the same dictionary bytes.  All state (table, entry hashes, entry bytes and offsets)
// lives in arrays the caller owns and sizes; nothing is kept here between calls.
#pragma once
#include <cstdint>

#include "text_dict_host.h"

namespace amdx {

// Common to all: device < 0: every pointer is host memory and the call returns when its output is
// written; otherwise they are memory of that device, one kernel is queued on `stream` and nothing
// is waited for.  n == 0 (rehash: D == 0) launches and writes nothing.  A capacity that is not a
// power of two or above 2^31, more than 2^30 rows, D + n >= 2^31 or a null array that the pass
// needs throw StoreError(kErrInvalidArgument) before anything is launched or written.  The values
// are unquoted bytes (what a text column holds), so no pass takes a quote.
//
// probe: value r is data[start[r], start[r] + length[r]) (int64 starts, int32 lengths, status uint8
// or 0: none).  The dictionary holds D entries: entry e is ent_data[ent_off[e], ent_off[e + 1])
// (ent_off int64).  insert != 0 (encode) claims slots for new values and needs capacity >=
// 2 * (D + n); insert == 0 (lookup) writes nothing to the table and needs capacity >= 2 * D; a
// smaller table is refused.  Writes slot_of[r] (int32, -1: none) and hash[r] (uint64).
void text_dict_probe_raw(uint64_t data, uint64_t data_bytes, uint64_t start, uint64_t length, uint64_t status, uint64_t n,
                         int device, uint64_t ent_data, uint64_t ent_bytes, uint64_t ent_off, uint64_t D, uint64_t table,
                         uint64_t capacity, bool insert, uint64_t slot_of, uint64_t hash, uint64_t stream);
// first: first[r] (int32) = 1 where slot_of[r] still holds pending row r; first_len[r] (int32) =
// length[r] there, else 0.
void text_dict_first_raw(uint64_t table, uint64_t capacity, uint64_t slot_of, uint64_t length, uint64_t n, int device,
                         uint64_t first, uint64_t first_len, uint64_t stream);
// codes: rank (int64, n) is the inclusive scan of first (0: a lookup, no slot is pending).
void text_dict_codes_raw(uint64_t table, uint64_t capacity, uint64_t slot_of, uint64_t rank, uint64_t n, uint64_t D,
                         int device, uint64_t codes, uint64_t stream);
// commit: byte_off (int64, n + 1) is the exclusive scan of first_len; ent_hash has ent_cap entries
// and ent_off ent_cap + 1; old_bytes is ent_off[D].  A code at or past ent_cap is not written.
void text_dict_commit_raw(uint64_t table, uint64_t capacity, uint64_t slot_of, uint64_t hash, uint64_t first,
                          uint64_t rank, uint64_t byte_off, uint64_t n, uint64_t D, uint64_t ent_hash, uint64_t ent_off,
                          uint64_t ent_cap, uint64_t old_bytes, int device, uint64_t stream);
// rehash: the D entries with hashes ent_hash into a table of empty slots, capacity >= 2 * D.
void text_dict_rehash_raw(uint64_t ent_hash, uint64_t D, uint64_t table, uint64_t capacity, int device, uint64_t stream);

// A test hook: every hash is cut to its low `bits` bits (0..64, 64 by default) before use, so a
// small value sends all values down one chain.  Set it before a dictionary's first entry.
void set_text_dict_hash_bits(int bits);
int text_dict_hash_bits();

// Kernel launches so far in this process (tests: a rejected or empty call launches nothing).
uint64_t text_dict_launches();

}  // namespace amdx
