// Snappy raw decoders for gfx950 (launch_snappy_decompress): one wave per page, grid-stride over the
// pages, the chunk table of the LZ4 decoders.  The header rules are those of snappy_host.h.
//
// Variant 0 takes one element per step and is the correctness anchor.  Variant 1 does for Snappy
// what lz4_decompress_window_kernel<.., kVec, kPre> (kernels.hip) does for LZ4: every step covers a
// 64-byte window of the compressed stream.  Shared with that kernel, through lz_wave.h, are the
// wave barrier, the shuffles and the scans; the stage refill, the ring flush and the four stages
// (candidate parse, chain by pointer doubling, codes, gather) are written again here for a format
// whose elements are a literal or a copy, never both, and whose copies are at most 64 bytes.
//
// Both kernels: the compressed stream is staged in LDS in aligned 16-byte granules, none of which
// holds no stream byte; every position is checked against src_bytes and dst_capacity before it is
// used; every loop iteration consumes an input byte, produces an output byte or leaves with a
// negative code, so a malformed page ends and writes nothing outside its dst range.
//
// LDS per block (one wave): variant 0 2 KiB; variant 1 1056 B stage + 4 KiB ring + 1 KiB codes +
// 256 B marks + 256 B window bytes = 6688 B, so the 160 KiB of a CU hold 24 such blocks.
#include "kernels.h"
#include "lz_wave.h"
#include "snappy_host.h"

#include <algorithm>

namespace amdx {

namespace {

typedef uint32_t sn_v4u __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) sn_v4u sn_gu4;

__device__ __forceinline__ uint32_t sn_uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// S bytes of the stream from the 16-byte granule of input byte pos (< slen) into the stage:
// stage[0] is input byte sbase (-15..0 for the first stage), stage[0, vend) are valid.
template <uint32_t S>
__device__ __forceinline__ void sn_refill(uint8_t* stage, const gu8* src, uint32_t slen, uint32_t pos, uint32_t lane,
                                          int32_t& sbase, uint32_t& vend, bool& at_end) {
  const uint64_t a = (reinterpret_cast<uint64_t>(src) + pos) & ~15ull;
  const uint64_t send = reinterpret_cast<uint64_t>(src) + slen;
  lz_wave_sync();
  for (uint32_t g = lane; g < S / 16; g += kLzThreads) {
    const uint64_t ga = a + 16ull * g;
    if (ga < send) *reinterpret_cast<sn_v4u*>(stage + 16 * g) = *reinterpret_cast<const sn_gu4*>(ga);
  }
  sbase = (int32_t)(int64_t)(a - reinterpret_cast<uint64_t>(src));
  const uint32_t left = (uint32_t)((int32_t)slen - sbase);
  vend = left < S ? left : S;
  at_end = (int32_t)vend + sbase == (int32_t)slen;
  lz_wave_sync();
}

// The preamble, read from memory by every lane alike: where the elements start, or a negative code.
// An empty chunk with no capacity is a page the plan had nothing to decode for: 0 bytes, no error.
__device__ __forceinline__ int32_t sn_begin(const gu8* src, uint32_t slen, uint32_t cap) {
  if (slen == 0) return cap ? (int32_t)kSnPreamble : 0;
  uint32_t want = 0;
  const int32_t pre = snappy_preamble_at([src](uint32_t i) -> uint32_t { return (uint32_t)src[i]; }, slen, &want);
  if (pre < 0) return pre;
  return want == cap ? pre : (int32_t)kSnLength;
}

// ---- variant 0: one element per step -------------------------------------------------------------
__global__ __launch_bounds__(kLzThreads) void snappy_decode_element_kernel(const Lz4Chunk* __restrict__ ch, int n,
                                                                          int32_t* __restrict__ out_sizes) {
  constexpr uint32_t S = kSnStage0;
  __shared__ __attribute__((aligned(16))) uint8_t stage[S];
  const uint32_t lane = threadIdx.x;
  for (int w = blockIdx.x; w < n; w += gridDim.x) {
    const gu8* src = reinterpret_cast<const gu8*>(ch[w].src);
    gu8* const dst = reinterpret_cast<gu8*>(ch[w].dst);
    const uint32_t slen = ch[w].src_bytes, cap = ch[w].dst_capacity;
    uint32_t ip = 0, op = 0, fenced = 0, vend = 0;
    int32_t sbase = 0, status = 0;
    bool at_end = false;
    const int32_t pre = sn_begin(src, slen, cap);
    if (pre < 0) status = pre;
    else ip = (uint32_t)pre;
    while (!status && ip < slen) {
      if (vend == 0 || (!at_end && (uint32_t)((int32_t)ip - sbase) + kSnMaxHeader > vend))
        sn_refill<S>(stage, src, slen, ip, lane, sbase, vend, at_end);
      const uint32_t r0 = (uint32_t)((int32_t)ip - sbase);                // < vend: ip < slen
      const SnappyHeader h = snappy_header_at([&](uint32_t i) -> uint32_t { return (uint32_t)stage[r0 + i]; }, vend - r0);
      const uint32_t kind = sn_uniform(h.kind), len = sn_uniform(h.len), off = sn_uniform(h.off), hdr = sn_uniform(h.hdr);
      if (!hdr) {                                       // only at the end of the stream: the stage held 5 bytes otherwise
        status = kSnInput;
        break;
      }
      ip += hdr;
      if (kind == 0) {
        if (len > slen - ip) status = kSnInput;
        else if (len > cap - op) status = kSnOutput;
        if (status) break;
#pragma unroll 4
        for (uint32_t i = lane; i < len; i += kLzThreads) dst[op + i] = src[ip + i];
        ip += len;
      } else {
        if (off == 0 || off > op) status = kSnOffset;
        else if (len > cap - op) status = kSnOutput;
        if (status) break;
        // the bytes copied from end at op - off + min(len, off): stored by this wave, so they are
        // read only once every store up to them has completed
        if (op - off + (len < off ? len : off) > fenced) {
          __threadfence_block();
          fenced = op;
        }
        if (lane < len) dst[op + lane] = dst[op - off + lane % off];
      }
      op += len;
    }
    if (!status && op != cap) status = kSnShort;
    if (lane == 0) out_sizes[w] = status ? status : (int32_t)op;
    lz_wave_sync();
  }
}

// ---- variant 1: window parse ----------------------------------------------------------------------
//   1. candidate parse: lane l decodes a header as if an element began at ip + l;
//   2. chain: the true elements from ip by pointer doubling over the candidates, output offsets by a
//      wave prefix sum, cut where the window's output would pass kSnWindow bytes;
//   3. codes: one per output byte: a literal byte in the stage, older output (absolute position) or
//      a reference to an earlier byte of this window, resolved by pointer jumping;
//   4. gather: bytes from the stage, the LDS ring of the last kSnRing output bytes, or HBM (output
//      older than the ring, flushed and fenced by then); the ring goes to HBM in aligned 16-byte
//      vectors every kSnFlush bytes.
// A literal that does not fit the stage or the window is copied from HBM by all lanes.
__global__ __launch_bounds__(kLzThreads) void snappy_decode_window_kernel(const Lz4Chunk* __restrict__ ch, int n,
                                                                         int32_t* __restrict__ out_sizes) {
  constexpr uint32_t R = kSnRing, S = kSnStage, TMAX = kSnWindow, NB = TMAX / kLzThreads, rmask = R - 1;
  static_assert((R & (R - 1)) == 0 && S % 16 == 0 && S >= 4 * kLzThreads && TMAX % kLzThreads == 0 &&
                    TMAX >= kSnMaxCopy && R >= 2 * (kSnFlush + TMAX + 16),
                "window kernel shape");
  constexpr uint32_t kInc = 1u << 24, kErrShift = 26, kNxt = 0xFFFFFFu;
  // codes: 0x: older output at that position (< 2^31); 10: reference to window byte; 11: stage index
  constexpr uint32_t kRef = 0x80000000u, kLit = 0xC0000000u, kVal = 0x3FFFFFFFu;
  __shared__ __attribute__((aligned(16))) uint8_t stage[S + 32];
  __shared__ __attribute__((aligned(16))) uint8_t ring[R];
  __shared__ uint32_t code[TMAX];
  __shared__ uint8_t marks[TMAX];
  __shared__ uint8_t winb[TMAX];                        // the window's output bytes (reference targets)
  const uint32_t lane = threadIdx.x;
  auto is_ref = [](uint32_t c) -> bool { return (c >> 30) == 2u; };
  for (uint32_t i = lane; i < TMAX; i += kLzThreads) marks[i] = 0;
  for (int w = blockIdx.x; w < n; w += gridDim.x) {
    const gu8* src = reinterpret_cast<const gu8*>(ch[w].src);
    gu8* const dst = reinterpret_cast<gu8*>(ch[w].dst);
    const uint32_t slen = ch[w].src_bytes, cap = ch[w].dst_capacity;
    const uint64_t daddr = reinterpret_cast<uint64_t>(dst);
    const uint32_t aoff = (uint32_t)daddr & 15u;
    // ring slot of output position pos, aligned to the destination address so that 16-byte
    // address granules are 16-byte ring granules
    auto ridx = [&](uint32_t pos) -> uint32_t { return (pos + aoff) & rmask; };
    uint32_t ip = 0, op = 0, flushed = 0, fenced = 0, vend = 0;
    int32_t sbase = 0, status = 0;
    bool at_end = false;

    // output bytes [lo, hi) from the ring to HBM: whole 16-byte granules as vectors, the partial
    // granules at the ends bytewise
    auto flush = [&](uint32_t lo, uint32_t hi) {
      if (hi <= lo) return;
      const uint64_t b0 = daddr + lo, b1 = daddr + hi;
      const uint64_t a0 = b0 & ~15ull;
      const uint32_t ng = (uint32_t)((b1 - a0 + 15) >> 4);
      for (uint32_t g = lane; g < ng; g += kLzThreads) {
        const uint64_t ga = a0 + 16ull * g;
        if (ga >= b0 && ga + 16 <= b1) {
          *reinterpret_cast<sn_gu4*>(ga) = *reinterpret_cast<const sn_v4u*>(ring + ridx((uint32_t)(ga - daddr)));
        } else {
          for (uint32_t j = 0; j < 16; ++j) {
            const uint64_t ba = ga + j;
            if (ba >= b0 && ba < b1) *reinterpret_cast<gu8*>(ba) = ring[ridx((uint32_t)(ba - daddr))];
          }
        }
      }
    };
    // the literal at ip (its header is in the stage) with all 64 lanes straight from HBM to HBM and
    // the ring
    auto long_literal = [&](uint32_t r0) {
      flush(flushed, op);
      const SnappyHeader h = snappy_header_at([&](uint32_t i) -> uint32_t { return (uint32_t)stage[r0 + i]; }, vend - r0);
      const uint32_t kind = sn_uniform(h.kind), len = sn_uniform(h.len), hdr = sn_uniform(h.hdr);
      if (!hdr || kind != 0) {                          // a copy always fits a window, a cut header is an error before
        status = kSnInternal;
        return;
      }
      const uint32_t p = ip + hdr;
      if (len > slen - p) status = kSnInput;
      else if (len > cap - op) status = kSnOutput;
      if (status) return;
      const uint32_t keep = len > R ? len - R : 0;      // the ring takes the last R bytes
#pragma unroll 8
      for (uint32_t i = lane; i < len; i += kLzThreads) {
        const uint8_t v = src[p + i];
        dst[op + i] = v;
        if (i >= keep) ring[ridx(op + i)] = v;
      }
      lz_wave_sync();
      op += len;
      ip = p + len;
      flushed = op;
    };

    const int32_t pre = sn_begin(src, slen, cap);
    if (pre < 0) status = pre;
    else ip = (uint32_t)pre;
    while (!status && ip < slen) {
      const uint32_t r0 = (uint32_t)((int32_t)ip - sbase);
      if (vend == 0 || (!at_end && r0 + 2 * kLzThreads > vend)) {
        sn_refill<S>(stage, src, slen, ip, lane, sbase, vend, at_end);
        continue;
      }
      // 1. candidate headers: an element at stage index r = r0 + lane
      const uint32_t r = r0 + lane;
      uint32_t A = kInc, tot = 0, q = 0, off = 0, kind = 0;
      if (r < vend) {
        const uint32_t a8 = r & ~7u;
        const uint64_t lo = *reinterpret_cast<const uint64_t*>(stage + a8);
        const uint64_t hi = *reinterpret_cast<const uint64_t*>(stage + a8 + 8);
        const uint32_t sh = (r & 7u) * 8u;
        const uint64_t wv = sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
        const SnappyHeader h = snappy_header_at([wv](uint32_t i) -> uint32_t { return (uint32_t)(wv >> (8u * i)) & 255u; },
                                                vend - r);
        if (!h.hdr) {
          A = at_end ? (uint32_t)(-kSnInput) << kErrShift : kInc;
        } else {
          kind = h.kind;
          off = h.off;
          q = r + h.hdr;                                // <= vend
          if (kind == 0 && h.len > vend - q) {          // the literal's bytes are not all in the stage
            A = at_end ? (uint32_t)(-kSnInput) << kErrShift : kInc;
          } else {
            tot = h.len;
            A = q + (kind == 0 ? h.len : 0u) - r0;      // where the next element starts, from r0
          }
        }
      }
      // 2. the chain from lane 0
      const uint32_t ecode = A >> kErrShift;
      const bool regular = !(A & kInc) && !ecode;
      const bool ends = regular && ip + (A & kNxt) >= slen;   // the stream ends after this element
      uint32_t J = regular && !ends && (A & kNxt) < kLzThreads ? (A & kNxt) : kLzThreads;
      uint64_t Rm = 1ull << lane;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const uint32_t from = J < kLzThreads ? J : lane;
        const uint32_t rlo = lz_shfl((uint32_t)Rm, from), rhi = lz_shfl((uint32_t)(Rm >> 32), from);
        const uint32_t jj = lz_shfl(J, from);
        if (J < kLzThreads) {
          Rm |= ((uint64_t)rhi << 32) | rlo;
          J = jj;
        }
      }
      const uint64_t C = ((uint64_t)sn_uniform((uint32_t)(Rm >> 32)) << 32) | sn_uniform((uint32_t)Rm);
      const uint64_t badc = C & __ballot((A & kInc) || ecode);
      const uint32_t fb = badc ? (uint32_t)__builtin_ctzll(badc) : 64u;
      const uint64_t prefix = fb < 64 ? C & ((1ull << fb) - 1) : C;
      const uint32_t v = (prefix >> lane) & 1ull ? tot : 0u;
      const uint32_t incl = lz_scan_add(v, lane);
      const uint64_t over = prefix & __ballot(incl > TMAX);
      const uint32_t fo = over ? (uint32_t)__builtin_ctzll(over) : 64u;
      const uint64_t mask = fo < 64 ? prefix & ((1ull << fo) - 1) : prefix;
      const uint32_t cnt = (uint32_t)__builtin_popcountll(mask);
      const uint32_t opo = incl - v;
      uint32_t cur = 0;
      bool need_input = false;
      if (fo < fb) {
        cur = fo;                                       // the next window starts at the element that did not fit
      } else if (fb < 64) {
        const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)A, (int)fb);
        cur = fb;
        if (a & kInc) {
          need_input = true;
        } else {
          status = -(int32_t)(a >> kErrShift);
          break;
        }
      } else {
        cur = (uint32_t)__builtin_amdgcn_readlane((int)A, (int)(63u - (uint32_t)__builtin_clzll(mask))) & kNxt;
      }
      if (cnt == 0) {
        if (need_input && !(r0 < 16 && vend == S)) {
          sn_refill<S>(stage, src, slen, ip, lane, sbase, vend, at_end);   // restart the stage at the element
          continue;
        }
        long_literal(r0);                               // longer than a stage, or than a window
        continue;
      }
      const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl, (int)(63u - (uint32_t)__builtin_clzll(mask)));
      // 3. per-element checks, then one code per output byte
      const bool tok = (mask >> lane) & 1ull;
      const uint32_t at = op + opo;
      int32_t bad = 0;
      if (tok) {
        if (kind != 0 && (off == 0 || off > at)) bad = kSnOffset;
        else if (at > cap || tot > cap - at) bad = kSnOutput;
      }
      const uint64_t badm = __ballot(bad != 0);
      if (badm) {
        status = __builtin_amdgcn_readlane(bad, (int)__builtin_ctzll(badm));
        break;
      }
      // start marks, then per block of 64 output bytes: owner = max-scan of the marks
      if (tok) marks[opo] = (uint8_t)(lane + 1);
      lz_wave_sync();
      uint32_t carry = 0;
      for (uint32_t b0 = 0; b0 < T; b0 += kLzThreads) {
        const uint32_t x = b0 + lane;
        const bool in = x < T;
        uint32_t m = 0;
        if (in) {
          m = marks[x];
          marks[x] = 0;
        }
        uint32_t own = lz_scan_max(m, lane);
        own = own ? own : carry;
        carry = (uint32_t)__builtin_amdgcn_readlane((int)own, 63);
        const uint32_t j = own ? own - 1 : 0;
        const uint32_t o_opo = lz_shfl(opo, j), o_kind = lz_shfl(kind, j), o_q = lz_shfl(q, j), o_off = lz_shfl(off, j);
        if (in) {
          const int32_t y = (int32_t)x - (int32_t)o_off;      // off <= op + opo < 2^31: checked above
          code[x] = o_kind == 0 ? (kLit | (o_q + (x - o_opo)))
                                : (y >= 0 ? (kRef | (uint32_t)y) : (uint32_t)((int32_t)op + y));
        }
      }
      lz_wave_sync();
      // 4. the bytes of every non-reference position are fetched first (stage / ring / HBM: the far
      // loads are in flight while the references resolve), references resolve to window positions
      // by pointer jumping block by block (earlier blocks are final), then read the window's bytes
      uint32_t cb[NB], outb[NB];
      bool farb[NB];
      bool anyfar = false;
#pragma unroll
      for (uint32_t bi = 0; bi < NB; ++bi) {
        const uint32_t x = bi * kLzThreads + lane;
        cb[bi] = x < T ? code[x] : kLit;
        farb[bi] = x < T && !(cb[bi] >> 31) && op - cb[bi] > R;   // older than the ring: below `flushed`
        anyfar = anyfar || (farb[bi] && cb[bi] >= fenced);
      }
      if (__ballot(anyfar)) {
        __threadfence_block();
        fenced = flushed;
      }
#pragma unroll
      for (uint32_t bi = 0; bi < NB; ++bi) {
        const uint32_t x = bi * kLzThreads + lane, c = cb[bi];
        outb[bi] = 0;
        if (x < T && !is_ref(c))
          outb[bi] = farb[bi] ? (uint32_t)dst[c] : (!(c >> 31) ? (uint32_t)ring[ridx(c)] : (uint32_t)stage[c & kVal]);
      }
#pragma unroll
      for (uint32_t bi = 0; bi < NB; ++bi) {
        if (bi * kLzThreads < T) {
          const uint32_t x = bi * kLzThreads + lane;
          const bool in = x < T;
          uint32_t c = cb[bi];
          bool done = !in || !is_ref(c);
          while (__ballot(!done)) {                     // a reference points below its position: chains end
            if (!done) {
              const uint32_t t = code[c & kVal];
              if (is_ref(t)) c = t;
              else done = true;
            }
            lz_wave_sync();
            if (in && is_ref(c)) code[x] = c;
            lz_wave_sync();
          }
          cb[bi] = c;
        }
      }
#pragma unroll
      for (uint32_t bi = 0; bi < NB; ++bi) {
        const uint32_t x = bi * kLzThreads + lane;
        if (x < T && !is_ref(cb[bi])) winb[x] = (uint8_t)outb[bi];
      }
      lz_wave_sync();
#pragma unroll
      for (uint32_t bi = 0; bi < NB; ++bi) {
        const uint32_t x = bi * kLzThreads + lane;
        if (x < T && is_ref(cb[bi])) outb[bi] = winb[cb[bi] & kVal];
      }
      lz_wave_sync();
#pragma unroll
      for (uint32_t bi = 0; bi < NB; ++bi) {
        const uint32_t x = bi * kLzThreads + lane;
        if (x < T) ring[ridx(op + x)] = (uint8_t)outb[bi];
      }
      lz_wave_sync();
      op += T;
      ip += cur;
      if (op - flushed >= kSnFlush) {
        const uint32_t hi = (uint32_t)(((daddr + op) & ~15ull) - daddr);
        flush(flushed, hi);
        flushed = hi;
      }
    }
    if (!status) {
      flush(flushed, op);
      if (op != cap) status = kSnShort;
    }
    if (lane == 0) out_sizes[w] = status ? status : (int32_t)op;
    lz_wave_sync();
  }
}

// -1: kSnDefaultVariant, the window parse: 0.88 ms against 1.35 ms per row group of the README's shape, and
// level with the LZ4 window kernel on the same data (profiles/snappy_decode.md).
int g_snappy_decode_variant = -1;

}  // namespace

void set_snappy_decode_variant(int v) { g_snappy_decode_variant = v; }

hipError_t launch_snappy_decompress(const Lz4Chunk* chunks, int n, int32_t* out_sizes, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (!chunks || !out_sizes) return hipErrorInvalidValue;
  const int variant = g_snappy_decode_variant < 0 ? kSnDefaultVariant : g_snappy_decode_variant;
  const unsigned grid = (unsigned)std::min(n, 65536);
  if (variant == 0) {
    hipLaunchKernelGGL(snappy_decode_element_kernel, dim3(grid), dim3(kLzThreads), 0, stream, chunks, n, out_sizes);
  } else if (variant == 1) {
    hipLaunchKernelGGL(snappy_decode_window_kernel, dim3(grid), dim3(kLzThreads), 0, stream, chunks, n, out_sizes);
  } else {
    return hipErrorInvalidValue;                        // a missing kernel is an error
  }
  return hipGetLastError();
}

}  // namespace amdx
