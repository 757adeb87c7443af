// JSON Lines columns for gfx950 (wave64): the locate pass of json_fields_host.h and the two
// unescape passes of json_text_host.h, each in two variants.  The rules, the typing of a located
// value and the liveness and window checks are those of the headers, compiled for the device.
//
// Variant 0, one lane per row or per value: jf_row / jt_measure_one / jt_emit_one as they stand.
//
// Variant 1, cooperative: a group of 16 lanes owns a row or a value (four per wave) and walks it
// in steps of 256 bytes, lane l of the group loading the 16 bytes at step * 256 + 16 * l.  The
// loads, masks, scans, the hand-off of state and the placing of kept bytes are the lg_ functions of
// lane_group.h.
//
// Both passes first find the code bytes of escapes.  A vector's backslash mask goes through
// jf_escaped16; what it needs from the bytes before it is whether the byte before the vector
// starts an escape.  A vector that is not all backslashes knows what it hands on without knowing
// what it got, and one of 16 backslashes hands on what it got, so a lane's incoming state is that
// of the nearest lower lane whose vector is not all backslashes, or the group's carried state:
// two ballots, no chain through the lanes and no backward walk (lg_carry).
//
// Locate: the real quotes are the quotes that are no code bytes; their parity below a lane (one
// ballot) and a prefix xor inside the vector give "inside a string"; a 16-lane signed prefix sum of
// opens minus closes outside strings gives the depth before each vector.  The events of a row are
// its depth-1 commas, colons and closes outside strings.  There are a few per member, and the
// group takes them in order, one ballot and one shuffle each: at a member's first colon the lanes
// that own a column (column c: lane c % 16) compare the key with their name, and at the member's
// end those that matched keep the value's bounds.  After the walk the owner lanes type their
// values.  Parity, depth, escape state and the member under way are carried from step to step.
//
// Unescape: a step whose escapes are all two-byte ones is done in parallel: the starts are
// dropped, the codes translated, and the kept bytes placed by a 16-lane prefix sum (lg_scan16,
// lg_place); whether the step's last byte starts an escape is carried to the next step.  A
// code of no known escape, or a start as the value's last byte, makes the value bad there and
// then.  A step with a \u escape is walked by lane 0 of the group with jt_span (one dependent byte
// load per byte: \n is in almost every step of real text, \u is not), which takes an escape that
// starts in the step whole; the bytes it took from the next step are skipped there.  A step
// without a backslash anywhere in the wave takes a short cut.  Emit walks a value twice: once to
// learn whether it is bad, once to write.
//
// No path loads a byte outside the row or value it was given: a vector that reaches past the end
// is assembled from byte loads.  Rows and values are independent, so there are no atomics and no
// waits between workgroups, and two runs write the same bytes.
#include "kernels.h"
#include "lane_group.h"

namespace amdx {

namespace {

__global__ __launch_bounds__(kLgThreads) void json_fields_lane_kernel(JsonFieldsArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kLgThreads + threadIdx.x;
  if (r < a.nrows) jf_row(a, r);
}

__global__ __launch_bounds__(kLgThreads) void json_text_measure_lane_kernel(JsonTextArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kLgThreads + threadIdx.x;
  if (r < a.t.n) jt_measure_one(a, r);
}

__global__ __launch_bounds__(kLgThreads) void json_text_emit_lane_kernel(JsonTextArgs a) {
  const uint64_t r = (uint64_t)blockIdx.x * kLgThreads + threadIdx.x;
  if (r < a.t.n) jt_emit_one(a, r);
}

__device__ __forceinline__ uint32_t jf_byte(uint8_t c) { return (uint32_t)c * 0x01010101u; }

// The code bytes of this lane's vector.  bm: its backslash mask (a vector cut at either end is
// never all backslashes); *carry: the group's state before the step, replaced by the state after
// it (uniform in the group).  Every lane of the wave calls it.
__device__ __forceinline__ uint32_t jf_lane_escaped(uint32_t bm, uint32_t gl, uint32_t g, uint32_t* carry) {
  uint32_t mine, unused;
  jf_escaped16(bm, 0, &mine);                       // exact unless all backslashes
  return jf_escaped16(bm, lg_carry(bm == 0xFFFFu, mine != 0, gl, g, carry), &unused);
}

__global__ __launch_bounds__(kLgThreads) void json_fields_coop_kernel(JsonFieldsArgs a) {
  const uint32_t lane = threadIdx.x & 63, gl = lane & (kLgGroup - 1), g = lane / kLgGroup;
  const uint32_t gs = g * kLgGroup;                 // the wave lane of the group's lane 0
  const uint64_t r = (uint64_t)blockIdx.x * kLgPerBlock + threadIdx.x / kLgGroup;
  const bool live = r < a.nrows;
  uint64_t off = 0, n = 0;
  const bool ok = live && jf_row_bytes(a, r, &off, &n);
  if (!ok) n = 0;                                   // such a row is not read
  const uint8_t* row = a.data + off;

  // the two columns this lane owns: gl and gl + 16; positions are relative to the row
  const bool own0 = gl < a.ncols, own1 = gl + kLgGroup < a.ncols;
  uint64_t vs0 = kJfNoPos, ve0 = 0, vs1 = kJfNoPos, ve1 = 0;
  bool m0 = false, m1 = false;                      // the member under way has this lane's name as its key

  // uniform in the group: the state before the step
  uint32_t st = kJfBefore, par = 0, depth = 0, ecar = 0;
  uint64_t mstart = 0, colon = kJfNoPos, closed_at = 0;

  for (uint64_t base = 0; __ballot(base < n && st != kJfBadRow) != 0ull; base += kLgStep) {
    const bool walking = base < n && st != kJfBadRow;
    const uint64_t pos = base + (uint64_t)gl * 16;
    uint32_t bm = 0, qm = 0, om = 0, cm = 0, km = 0, lm = 0, nw = 0;
    if (walking && pos < n) {
      const uint64_t rem = n - pos;
      const u32x4 v = lg_load16(row + pos, rem);
      const uint32_t valid = rem >= 16 ? 0xFFFFu : ((1u << (uint32_t)rem) - 1u);
      const u32x4 w = {v.x | 0x20202020u, v.y | 0x20202020u, v.z | 0x20202020u, v.w | 0x20202020u};
      bm = lg_mask16(v, jf_byte('\\')) & valid;
      qm = lg_mask16(v, jf_byte('"')) & valid;
      om = lg_mask16(w, jf_byte('{')) & valid;      // { and [ differ in bit 5 only, as do } and ]
      cm = lg_mask16(w, jf_byte('}')) & valid;
      km = lg_mask16(v, jf_byte(',')) & valid;
      lm = lg_mask16(v, jf_byte(':')) & valid;
      nw = valid & ~(lg_mask16(v, jf_byte(0x20)) | lg_mask16(v, jf_byte(0x09)) | lg_mask16(v, jf_byte(0x0A)) |
                     lg_mask16(v, jf_byte(0x0D)));
    }
    // strings
    const uint32_t rq = qm & ~jf_lane_escaped(bm, gl, g, &ecar);
    const uint32_t gq = lg_group16(__ballot(__popc(rq) & 1), g);
    const uint32_t before = (par ^ (uint32_t)__popc(gq & ((1u << gl) - 1u))) & 1u;
    par = (par ^ (uint32_t)__popc(gq)) & 1u;
    const uint32_t outside = ~(lg_inside16(rq) ^ (before ? 0xFFFFu : 0u));
    om &= outside;
    cm &= outside;
    // depth before this lane's vector (wraps as the host's does)
    const uint32_t delta = (uint32_t)__popc(om) - (uint32_t)__popc(cm);
    uint32_t dsum;
    const uint32_t dl = depth + (lg_scan16(delta, gl, &dsum) - delta);
    depth += dsum;
    // events: commas, colons and closes outside strings with depth 1 before them
    const uint32_t cand = ((km | lm) & outside) | cm;
    uint32_t ev = 0;
    if ((om | cm) == 0) {
      ev = dl == 1 ? cand : 0;
    } else {
      for (uint32_t m = cand; m; m &= m - 1) {
        const uint32_t j = (uint32_t)__builtin_ctz(m), lowm = (1u << j) - 1u;
        if (dl + (uint32_t)__popc(om & lowm) - (uint32_t)__popc(cm & lowm) == 1) ev |= 1u << j;
      }
    }
    // nothing but whitespace so far: the first other byte opens the object or the row is bad
    {
      const uint32_t gn = lg_group16(__ballot(nw != 0), g);
      const uint64_t first =
          lg_shfl64_wave(nw ? pos + (uint32_t)__builtin_ctz(nw) : 0, (int)(gs + (gn ? __builtin_ctz(gn) : 0)));
      if (st == kJfBefore && gn) {
        if (row[first] == '{') {
          st = kJfOpen;
          mstart = first + 1;
        } else {
          st = kJfBadRow;
        }
      }
    }
    // the events of the step, in order
    uint32_t pend = st == kJfOpen ? ev : 0;
    for (;;) {
      const uint64_t bal = __ballot(pend != 0 && st == kJfOpen);
      if (bal == 0ull) break;
      const uint32_t ge = lg_group16(bal, g);
      const uint32_t src = ge ? (uint32_t)__builtin_ctz(ge) : 0;
      const uint32_t bit = pend ? (uint32_t)__builtin_ctz(pend) : 0;
      const uint32_t kind = ((lm >> bit) & 1u) ? 0u : ((km >> bit) & 1u) ? 1u : 2u;   // colon, comma, close
      const uint32_t got = __shfl(bit | (kind << 4), (int)(gs + src));
      if (!ge) continue;                            // uniform in the group
      const uint64_t p = base + (uint64_t)src * 16 + (got & 15u);
      if (gl == src) pend &= pend - 1;
      if ((got >> 4) == 0) {
        if (colon == kJfNoPos) {
          colon = p;
          m0 = own0 && jf_key_match(row, mstart, p, a.names + a.cols[gl].name_off, a.cols[gl].name_len);
          m1 = own1 && jf_key_match(row, mstart, p, a.names + a.cols[gl + kLgGroup].name_off,
                                    a.cols[gl + kLgGroup].name_len);
        }
        continue;
      }
      if (colon != kJfNoPos) {                      // the member ends here
        if (m0) {
          vs0 = colon + 1;
          ve0 = p;
        }
        if (m1) {
          vs1 = colon + 1;
          ve1 = p;
        }
      }
      colon = kJfNoPos;
      m0 = m1 = false;
      mstart = p + 1;
      if ((got >> 4) == 2) {
        st = row[p] == '}' ? kJfClosed : kJfBadRow;
        closed_at = p;
      }
    }
    // after the closing brace: whitespace only
    uint32_t tail = 0;
    if (st == kJfClosed && nw) {
      if (pos > closed_at) tail = nw;
      else if (pos + 15 > closed_at) tail = nw & ~((2u << (uint32_t)(closed_at - pos)) - 1u);
    }
    const uint32_t gt = lg_group16(__ballot(tail != 0), g);
    if (st == kJfClosed && gt) st = kJfBadRow;
  }

  if (!live) return;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t col = gl + j * kLgGroup;
    if (col >= a.ncols) break;
    const uint64_t vs = j ? vs1 : vs0, ve = j ? ve1 : ve0;
    if (!ok) jf_emit_none(a.cols[col], r, kFpBad);
    else if (st == kJfBefore) jf_emit_none(a.cols[col], r, kFpNone);
    else if (st != kJfClosed) jf_emit_none(a.cols[col], r, kFpBad);
    else if (vs == kJfNoPos) jf_emit_none(a.cols[col], r, kFpNone);
    else jf_emit(a.cols[col], r, row, off, vs, ve);
  }
}

// The walk of one value of n bytes at p by its group.  Returns false for a bad value; *total: the
// output length.  With EMIT, output byte j in [jlo, jhi) goes to out[lo + j].  Every lane of the
// wave calls it; a group without a value to walk passes n = 0.
template <bool EMIT>
__device__ __forceinline__ bool jt_coop_walk(const uint8_t* p, uint64_t n, uint32_t gl, uint32_t g, uint8_t* out,
                                             int64_t lo, uint64_t jlo, uint64_t jhi, uint64_t* total) {
  const uint32_t gs = g * kLgGroup;                 // the wave lane of the group's lane 0
  // uniform in the group
  uint64_t done = 0;                                // output bytes before the step
  uint64_t begin = 0;                               // the first byte that is not consumed yet
  uint32_t ecar = 0;                                // the byte before the step starts an escape
  bool bad = false;
  for (uint64_t base = 0; __ballot(base < n && !bad) != 0ull; base += kLgStep) {
    const bool walking = base < n && !bad;
    const uint64_t pos = base + (uint64_t)gl * 16;
    uint64_t vlo = 0, vhi = 0;
    uint32_t valid = 0, bm = 0;
    if (walking && pos < n && pos + 16 > begin) {
      const uint64_t rem = n - pos;
      const u32x4 v = lg_load16(p + pos, rem);
      valid = rem >= 16 ? 0xFFFFu : ((1u << (uint32_t)rem) - 1u);
      if (begin > pos) valid &= ~((1u << (uint32_t)(begin - pos)) - 1u);
      bm = lg_mask16(v, jf_byte('\\')) & valid;
      vlo = lg_lo64(v);
      vhi = lg_hi64(v);
    }
    uint32_t keep = valid, c;
    uint64_t j0;                                    // the output index of this lane's first kept byte
    bool stored = false;                            // the step's bytes are written already, or never
    if (__ballot(walking && (bm != 0 || ecar != 0 || begin > base)) == 0ull) {   // wave-uniform: plain bytes only
      c = (uint32_t)__popc(valid);
      j0 = done + (uint64_t)gl * 16;
      done += walking ? (n - base < kLgStep ? n - base : kLgStep) : 0;
      begin = base + kLgStep;
    } else {
      const uint32_t cin = ecar;                    // the byte before the step starts an escape
      const uint32_t codes = jf_lane_escaped(bm, gl, g, &ecar);
      const uint32_t starts = bm & ~codes;
      // a start as the value's last byte and a code of no known escape make the value bad; a \u
      // escape sends the step to lane 0
      bool lane_bad = false, lane_u = false;
      if (starts) {
        const uint32_t hi = 31u - (uint32_t)__builtin_clz(valid);   // starts != 0: valid != 0
        lane_bad = ((starts >> hi) & 1u) && pos + hi + 1 >= n;
      }
      for (uint32_t m = codes & valid; m; m &= m - 1) {
        const uint32_t j = (uint32_t)__builtin_ctz(m), sh = 8 * (j & 7);
        const uint8_t code = (uint8_t)((j < 8 ? vlo : vhi) >> sh);
        const int t = jt_simple(code);
        if (t < 0) {
          if (code == 'u') lane_u = true;
          else lane_bad = true;
        } else if (j < 8) {
          vlo = (vlo & ~(0xFFull << sh)) | ((uint64_t)t << sh);
        } else {
          vhi = (vhi & ~(0xFFull << sh)) | ((uint64_t)t << sh);
        }
      }
      const bool group_bad = lg_group16(__ballot(lane_bad), g) != 0;
      const bool group_serial = !group_bad && lg_group16(__ballot(lane_u), g) != 0;
      keep = valid & ~starts;
      c = (uint32_t)__popc(keep);
      uint32_t kept;                                // by the group in this step
      j0 = done + (lg_scan16(c, gl, &kept) - c);
      uint64_t ndone = done + kept;
      uint64_t nbegin = base + kLgStep;
      uint32_t sbad = 0;
      if (group_serial && gl == 0) {
        // from the first byte not consumed, or from the backslash before the step whose code
        // opens it (that backslash gave no output); an escape that starts in the step is taken
        // whole, so no escape state is left over
        uint64_t i = begin > base ? begin : base - cin, k = done;
        const uint64_t stop = n - base < kLgStep ? n : base + kLgStep;
        sbad = jt_span(p, n, &i, stop, &k, EMIT ? out : nullptr, lo, jlo, jhi) ? 0u : 1u;
        ndone = k;
        nbegin = i;
      }
      done = lg_shfl64_wave(ndone, (int)gs);
      begin = lg_shfl64_wave(nbegin, (int)gs);
      bad = bad || group_bad || __shfl(sbad, (int)gs) != 0;
      if (group_serial) ecar = 0;
      stored = group_serial || group_bad;
    }
    // valid is not always a run of low bits here: only a vector kept whole needs no compaction
    if (EMIT && !stored) lg_place(out, lo, jlo, jhi, j0, vlo, vhi, keep, c, keep != 0xFFFFu);
  }
  *total = done;
  return !bad;
}

__global__ __launch_bounds__(kLgThreads) void json_text_measure_coop_kernel(JsonTextArgs a) {
  const uint32_t lane = threadIdx.x & 63, gl = lane & (kLgGroup - 1), g = lane / kLgGroup;
  const uint64_t r = (uint64_t)blockIdx.x * kLgPerBlock + threadIdx.x / kLgGroup;
  uint64_t off = 0, n = 0, total = 0;
  const bool ok = r < a.t.n && tc_live(a.t, r, &off, &n);
  if (!ok) n = 0;                                   // such a value is not read
  const bool good = jt_coop_walk<false>(a.t.data + off, n, gl, g, nullptr, 0, 0, 0, &total);
  if (r < a.t.n && gl == 0) {
    a.t.out_len[r] = ok && good ? (int32_t)total : 0;
    a.out_status[r] = !ok ? jt_dead_status(a.t, r) : good ? (uint8_t)0 : (uint8_t)2;
  }
}

__global__ __launch_bounds__(kLgThreads) void json_text_emit_coop_kernel(JsonTextArgs a) {
  const uint32_t lane = threadIdx.x & 63, gl = lane & (kLgGroup - 1), g = lane / kLgGroup;
  const uint64_t r = (uint64_t)blockIdx.x * kLgPerBlock + threadIdx.x / kLgGroup;
  uint64_t off = 0, n = 0, jlo = 0, jhi = 0, total = 0;
  int64_t lo = 0;
  const bool ok = r < a.t.n && tc_live(a.t, r, &off, &n) && tc_window(a.t, r, &lo, &jlo, &jhi);
  if (!ok) n = 0;                                   // such a value is neither read nor written
  const uint8_t* p = a.t.data + off;
  const bool good = jt_coop_walk<false>(p, n, gl, g, nullptr, 0, 0, 0, &total);
  jt_coop_walk<true>(p, good ? n : 0, gl, g, a.t.out, lo, jlo, jhi, &total);
}

// By analogy with field parse; tools/json_fields_bench.py measures both, profiles/json_fields.md.
int g_jf_variant = 1;
int g_jt_variant = 1;

bool jt_args_ok(const JsonTextArgs& a) { return a.t.n <= (1ull << 31); }

unsigned jf_grid(uint64_t n, int variant) {
  const uint64_t per = variant == 1 ? kLgPerBlock : kLgThreads;
  return (unsigned)((n + per - 1) / per);
}

}  // namespace

void set_json_fields_variant(int variant) { g_jf_variant = variant ? 1 : 0; }
int json_fields_variant() { return g_jf_variant; }
void set_json_text_variant(int variant) { g_jt_variant = variant ? 1 : 0; }
int json_text_variant() { return g_jt_variant; }

hipError_t launch_json_fields(const JsonFieldsArgs& a, hipStream_t stream) {
  if (!json_fields_scalars_ok(a) || a.nrows > (1ull << 31)) return hipErrorInvalidValue;
  if (a.nrows == 0) return hipSuccess;
  if (!a.off || !a.len || !a.names || (!a.data && a.data_bytes)) return hipErrorInvalidValue;
  const dim3 grid(jf_grid(a.nrows, g_jf_variant));
  if (g_jf_variant == 1) hipLaunchKernelGGL(json_fields_coop_kernel, grid, dim3(kLgThreads), 0, stream, a);
  else hipLaunchKernelGGL(json_fields_lane_kernel, grid, dim3(kLgThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_json_text_measure(const JsonTextArgs& a, hipStream_t stream) {
  if (!jt_args_ok(a)) return hipErrorInvalidValue;
  if (a.t.n == 0) return hipSuccess;
  if (!a.t.start || !a.t.length || !a.t.out_len || !a.out_status || (!a.t.data && a.t.data_bytes))
    return hipErrorInvalidValue;
  const dim3 grid(jf_grid(a.t.n, g_jt_variant));
  if (g_jt_variant == 1) hipLaunchKernelGGL(json_text_measure_coop_kernel, grid, dim3(kLgThreads), 0, stream, a);
  else hipLaunchKernelGGL(json_text_measure_lane_kernel, grid, dim3(kLgThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_json_text_emit(const JsonTextArgs& a, hipStream_t stream) {
  if (!jt_args_ok(a)) return hipErrorInvalidValue;
  if (a.t.n == 0) return hipSuccess;
  if (!a.t.start || !a.t.length || !a.t.offsets || (!a.t.data && a.t.data_bytes) || (!a.t.out && a.t.out_bytes))
    return hipErrorInvalidValue;
  const dim3 grid(jf_grid(a.t.n, g_jt_variant));
  if (g_jt_variant == 1) hipLaunchKernelGGL(json_text_emit_coop_kernel, grid, dim3(kLgThreads), 0, stream, a);
  else hipLaunchKernelGGL(json_text_emit_lane_kernel, grid, dim3(kLgThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace amdx
