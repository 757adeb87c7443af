// Text dictionaries for gfx950 (wave64): the passes of text_dict_host.h.  first, codes, commit and
// rehash are one lane per row (per entry) running the header's functions as they stand.  probe has
// two variants.
//
// Variant 0, one lane per value: td_probe_one as it stands, a serial hash, walk and compare.
//
// Variant 1, cooperative: a group of 16 lanes owns a value (four values per wave).  The hash is
// summed over steps of 256 bytes, lane l of the group taking the two words of the 16 bytes at
// step * 256 + 16 * l (lg_load16 of lane_group.h, as the group shuffles), and added up with a
// 16-lane butterfly; the sum of terms is the same in any
// order, so it equals the serial hash.  The walk: the group's lane 0 loads the slot (and claims an
// empty one), the slot is broadcast, a candidate with an equal tag and length is compared by the
// whole group in the same 256-byte steps with a ballot for "any lane differs", and lane 0 applies
// the atomic min on a pending slot.  The four groups of a wave finish their chains at different
// times, so every loop runs while a ballot says some group still needs it and a group that is done
// only goes through the motions; no lane waits for another lane's or workgroup's progress, and
// every walk ends after at most `capacity` slots.
//
// No path loads a byte outside a value or an entry: a vector that reaches past the end is assembled
// from byte loads.  All atomics are HIP's global atomics issued by vector lanes.
#include "kernels.h"
#include "lane_group.h"

namespace amdx {

namespace {

__global__ __launch_bounds__(kLgThreads) void text_dict_probe_lane_kernel(TextDictArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kLgThreads + threadIdx.x;
  if (r < a.in.n) td_probe_one(a, r);
}

__global__ __launch_bounds__(kLgThreads) void text_dict_first_kernel(TextDictArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kLgThreads + threadIdx.x;
  if (r < a.in.n) td_first_one(a, r);
}

__global__ __launch_bounds__(kLgThreads) void text_dict_codes_kernel(TextDictArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kLgThreads + threadIdx.x;
  if (r < a.in.n) td_codes_one(a, r);
}

__global__ __launch_bounds__(kLgThreads) void text_dict_commit_kernel(TextDictArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kLgThreads + threadIdx.x;
  if (r < a.in.n) td_commit_one(a, r);
}

__global__ __launch_bounds__(kLgThreads) void text_dict_rehash_kernel(TextDictArgs a) {
  const uint64_t e = (uint64_t)blockIdx.x * kLgThreads + threadIdx.x;
  if (e < a.D) td_rehash_one(a, e);
}

__global__ __launch_bounds__(kLgThreads) void text_dict_probe_coop_kernel(TextDictArgs a) {
  const uint32_t lane = threadIdx.x & 63, gl = lane & (kLgGroup - 1), g = lane / kLgGroup;
  const uint64_t r = (uint64_t)blockIdx.x * kLgPerBlock + threadIdx.x / kLgGroup;
  uint64_t off = 0, n = 0;
  const bool row = r < a.in.n;
  const bool live = row && tc_live(a.in, r, &off, &n);
  if (!live) n = 0;                                 // such a value is not read
  const uint8_t* p = a.in.data + off;

  uint64_t sum = 0;
  for (uint64_t base = 0; __ballot(base < n) != 0ull; base += kLgStep) {
    const uint64_t pos = base + (uint64_t)gl * 16;
    if (pos < n) {
      const uint64_t rem = n - pos;
      const u32x4 v = lg_load16(p + pos, rem);      // zero padded past the end
      sum += td_term(pos / 8, lg_lo64(v));
      if (rem > 8) sum += td_term(pos / 8 + 1, lg_hi64(v));
    }
  }
#pragma unroll
  for (int d = kLgGroup / 2; d; d >>= 1) sum += lg_shfl64_xor_group(sum, d);
  const uint64_t h = live ? td_finish(sum, n, a.hash_bits) : 0;

  const uint64_t mask = a.capacity - 1, tag = h & kTdTagMask;
  const uint64_t mine = tag | kTdPending | r;
  uint64_t i = h & mask, step = 0;
  int32_t found = -1;
  bool probing = live;                              // uniform in the group
  while (__ballot(probing) != 0ull) {
    uint64_t v = 0;
    if (probing && gl == 0) {
      v = td_load(&a.table[i]);
      if (v == kTdEmpty && a.insert) {
        v = td_cas(&a.table[i], kTdEmpty, mine);
        if (v == kTdEmpty) v = mine;                // claimed; a lost race leaves what stands there now
      }
    }
    v = lg_shfl64_group(v, 0);
    bool cand = false;
    const uint8_t* q = p;
    uint64_t qn = 0;
    if (probing) {
      if (v == kTdEmpty) {                          // a lookup: the value is not in the dictionary
        probing = false;
      } else if (v == mine) {
        found = (int32_t)i;
        probing = false;
      } else if ((v & kTdTagMask) == tag) {
        cand = td_candidate(a, v, &q, &qn) && qn == n;
      }
    }
    bool cmp = cand, differs = false;
    for (uint64_t base = 0; __ballot(cmp && base < n) != 0ull; base += kLgStep) {
      const uint64_t pos = base + (uint64_t)gl * 16;
      bool d = false;
      if (cmp && pos < n) {
        const uint64_t rem = n - pos;
        const u32x4 pv = lg_load16(p + pos, rem), qv = lg_load16(q + pos, rem);
        d = lg_lo64(pv) != lg_lo64(qv) || lg_hi64(pv) != lg_hi64(qv);
      }
      if (lg_group16(__ballot(d), g)) {
        differs = true;
        cmp = false;
      }
    }
    if (probing) {
      if (cand && !differs) {
        if (gl == 0 && ((uint32_t)v & kTdPending) && a.insert) td_min(&a.table[i], mine);
        found = (int32_t)i;
        probing = false;
      } else {
        i = (i + 1) & mask;
        if (++step >= a.capacity) probing = false;
      }
    }
  }
  if (row && gl == 0) {
    a.slot_of[r] = found;
    a.hash[r] = h;
  }
}

// Measured by tools/text_dict_bench.py (profiles/text_dict.md): on 65,536 values of 12 bytes the two
// tie in encode and variant 0 is faster in lookup and when every value is new; variant 1 is ahead
// only slightly, and only on values of about 200 bytes.
int g_td_variant = 0;

unsigned td_grid(uint64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

bool td_values_ok(const TextDictArgs& a) {
  return a.in.start && a.in.length && (a.in.data || !a.in.data_bytes);
}

}  // namespace

void set_text_dict_variant(int variant) { g_td_variant = variant ? 1 : 0; }

int text_dict_variant() { return g_td_variant; }

hipError_t launch_text_dict_probe(const TextDictArgs& a, hipStream_t stream) {
  if (!text_dict_scalars_ok(a) || !text_dict_probe_fits(a)) return hipErrorInvalidValue;
  if (a.in.n == 0) return hipSuccess;
  if (!td_values_ok(a) || !a.table || !a.slot_of || !a.hash) return hipErrorInvalidValue;
  if (a.D && (!a.ent_off || (!a.ent_data && a.ent_bytes))) return hipErrorInvalidValue;
  if (g_td_variant == 1) {
    hipLaunchKernelGGL(text_dict_probe_coop_kernel, dim3(td_grid(a.in.n, kLgPerBlock)), dim3(kLgThreads), 0,
                       stream, a);
  } else {
    hipLaunchKernelGGL(text_dict_probe_lane_kernel, dim3(td_grid(a.in.n, kLgThreads)), dim3(kLgThreads), 0, stream, a);
  }
  return hipGetLastError();
}

hipError_t launch_text_dict_first(const TextDictArgs& a, hipStream_t stream) {
  if (!text_dict_scalars_ok(a)) return hipErrorInvalidValue;
  if (a.in.n == 0) return hipSuccess;
  if (!a.table || !a.slot_of || !a.in.length || !a.first || !a.first_len) return hipErrorInvalidValue;
  hipLaunchKernelGGL(text_dict_first_kernel, dim3(td_grid(a.in.n, kLgThreads)), dim3(kLgThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_text_dict_codes(const TextDictArgs& a, hipStream_t stream) {
  if (!text_dict_scalars_ok(a)) return hipErrorInvalidValue;
  if (a.in.n == 0) return hipSuccess;
  if (!a.table || !a.slot_of || !a.codes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(text_dict_codes_kernel, dim3(td_grid(a.in.n, kLgThreads)), dim3(kLgThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_text_dict_commit(const TextDictArgs& a, hipStream_t stream) {
  if (!text_dict_scalars_ok(a)) return hipErrorInvalidValue;
  if (a.in.n == 0) return hipSuccess;
  if (!a.table || !a.slot_of || !a.hash || !a.first || !a.rank || !a.byte_off || !a.ent_hash || !a.ent_off)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(text_dict_commit_kernel, dim3(td_grid(a.in.n, kLgThreads)), dim3(kLgThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_text_dict_rehash(const TextDictArgs& a, hipStream_t stream) {
  if (!text_dict_scalars_ok(a) || a.capacity < 2 * a.D) return hipErrorInvalidValue;
  if (a.D == 0) return hipSuccess;
  if (!a.table || !a.ent_hash) return hipErrorInvalidValue;
  hipLaunchKernelGGL(text_dict_rehash_kernel, dim3(td_grid(a.D, kLgThreads)), dim3(kLgThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace amdx
