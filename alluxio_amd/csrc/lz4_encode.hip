// LZ4 block encoders for gfx950: 64 KiB chunks (launch_lz4_compress) and Parquet page bodies of any
// size (launch_lz4_page_*).  One wave parses a chunk or a segment of one; the hash, the length
// bytes and the format constants are those of lz4_block_host.h.  The decoders are in kernels.hip.
#include "kernels.h"

#include <algorithm>

namespace amdx {

constexpr uint32_t kLzTableBytes = sizeof(uint16_t) << kLbHashLog;   // 4096 16-bit positions, 8 KiB

// The token and literal-length bytes of a sequence at dst[o] (thread 0) and its `lit` literals from
// src[from] (all T threads); returns where the literals end.
template <int T>
__device__ __forceinline__ uint32_t lz_put_literals(uint8_t* dst, uint32_t o, const uint8_t* src, uint32_t from,
                                                    uint32_t lit, uint32_t mcode, uint32_t tid) {
  if (tid == 0) {
    dst[o] = lb_token(lit, mcode);
    lb_put_len(dst, o + 1, lit);
  }
  const uint32_t q = o + 1 + lb_len_bytes(lit);
  for (uint32_t i = tid; i < lit; i += T) dst[q + i] = src[from + i];
  return q + lit;
}

// Compression: chunk staged into LDS, 4096-entry u16 hash table in LDS.  Lanes evaluate 64
// candidate positions at once (hash, probe, match length) against the table state at batch
// start; a wave ballot then drives the greedy parse.  Output is standard LZ4 block format.
__global__ __launch_bounds__(kLzThreads) void lz4_compress_kernel(const Lz4Chunk* __restrict__ ch,
                                                                 int n, int32_t* __restrict__ out_sizes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* src = smem;                                            // 64 KiB
  uint16_t* table = reinterpret_cast<uint16_t*>(smem + kLzWindow);  // 8 KiB
  const int lane = threadIdx.x;
  for (int w = blockIdx.x; w < n; w += gridDim.x) {
    const uint8_t* __restrict__ gsrc = reinterpret_cast<const uint8_t*>(ch[w].src);
    uint8_t* __restrict__ dst = reinterpret_cast<uint8_t*>(ch[w].dst);
    const uint32_t len = ch[w].src_bytes < kLzWindow ? ch[w].src_bytes : kLzWindow;
    const uint32_t cap = ch[w].dst_capacity;
    for (uint32_t i = lane; i < len; i += kLzThreads) src[i] = gsrc[i];
    for (uint32_t i = lane; i < (1u << kLbHashLog); i += kLzThreads) table[i] = 0xFFFF;
    __syncthreads();
    uint32_t op = 0, anchor = 0, ip = 0;
    int32_t status = 0;
    const uint32_t match_limit = len > kLbMfLimit ? len - kLbMfLimit : 0;   // last match start
    const uint32_t end_match = len > kLbLastLiterals ? len - kLbLastLiterals : 0;
    while (ip < match_limit && status == 0) {
      // each lane probes position ip + lane
      const uint32_t pos = ip + lane;
      uint32_t cand = 0xFFFFFFFFu, mlen = 0;
      uint32_t h = 0;
      if (pos < match_limit) {
        const uint32_t v = lb_read32(src + pos);
        h = lb_hash(v);
        const uint32_t c = table[h];
        if (c != 0xFFFF && c < pos && pos - c <= 65535 && lb_read32(src + c) == v) {
          cand = c;
          mlen = kLbMinMatch;
          while (pos + mlen < end_match && src[c + mlen] == src[pos + mlen]) ++mlen;
        }
      }
      __syncthreads();
      if (pos < match_limit) table[h] = (uint16_t)pos;  // last writer wins: any entry is valid
      __syncthreads();
      const unsigned long long hits = __ballot(cand != 0xFFFFFFFFu);
      if (hits == 0) { ip += kLzThreads; continue; }
      const int first = __ffsll((long long)hits) - 1;
      const uint32_t mpos = ip + first;
      const uint32_t moff = mpos - __shfl(cand, first);
      const uint32_t ml = __shfl(mlen, first);
      // emit sequence: literals [anchor, mpos) + match (moff, ml)
      const uint32_t lit = mpos - anchor, mcode = ml - kLbMinMatch;
      const uint32_t need = 1 + lb_len_bytes(lit) + lit + 2 + lb_len_bytes(mcode);
      if (op + need > cap) { status = -1; break; }
      const uint32_t q = lz_put_literals<kLzThreads>(dst, op, src, anchor, lit, mcode, lane);
      if (lane == 0) {
        dst[q] = (uint8_t)(moff & 255);
        dst[q + 1] = (uint8_t)(moff >> 8);
        lb_put_len(dst, q + 2, mcode);
      }
      op += need;
      ip = mpos + ml;
      anchor = ip;
    }
    // the closing literal-only sequence
    const uint32_t lit = len - anchor;
    if (status == 0 && op + 1 + lb_len_bytes(lit) + lit > cap) status = -1;
    if (status == 0) op = lz_put_literals<kLzThreads>(dst, op, src, anchor, lit, 0, lane);
    if (lane == 0) out_sizes[w] = status ? -1 : (int32_t)op;
    __syncthreads();
  }
}

// Batch parse.  The kernel above emits ONE sequence per 64-position probe batch and throws the
// other 63 lanes' matches away, so text (≈8-byte sequences) costs one full probe round (two
// barriers, a ballot, a serial token write) per ~8 input bytes.  Here every probe batch is parsed
// completely: a uniform greedy walk over the ballot of hits selects every non-overlapping match in
// position order, each selected lane sizes its own sequence, a wave prefix sum places all of them,
// and the owning lanes write their tokens / length bytes / offsets in parallel while literal runs
// are copied by the whole wave.  Match extension compares 4 bytes at a time.
//
// Parses body positions [begin, match_limit) with one wave: a match starts before match_limit and
// ends by end_match.  Body byte p is src[p - base], and the table holds 16-bit positions counted
// from `base` (0xFFFF: empty), so every position hashed is below base + 65535.  Sequences go to
// dst[0, cap).  SPLIT leaves the first sequence's token and literals out (the merge writes them,
// joined across the segment boundary) and reports where its match starts and its length code.
struct LzParsed {
  uint32_t op;           // bytes written
  uint32_t anchor;       // the end of the last match (begin: none)
  uint32_t first_mpos;   // SPLIT: position of the first match (kLbNone: no match)
  uint32_t first_mcode;  // SPLIT: its match length - 4
  bool overflow;         // the sequences do not fit cap; the parse stopped
};

template <bool SPLIT>
__device__ __forceinline__ LzParsed lz_batch_parse(const uint8_t* src, uint32_t base, uint16_t* table, uint8_t* dst,
                                                   uint32_t cap, uint32_t begin, uint32_t match_limit,
                                                   uint32_t end_match, int lane) {
  LzParsed r{0, begin, kLbNone, 0, false};
  uint32_t ip = begin;
  bool have_first = false;
  while (ip < match_limit) {
    const uint32_t pos = ip + lane;
    uint32_t cand = 0xFFFFFFFFu, mlen = 0, h = 0;
    if (pos < match_limit) {
      const uint32_t v = lb_read32(src + (pos - base));
      h = lb_hash(v);
      const uint32_t c = table[h];
      if (c != 0xFFFF && base + c < pos && lb_read32(src + c) == v) {
        cand = base + c;
        mlen = kLbMinMatch;
        while (pos + mlen + 4 <= end_match &&
               lb_read32(src + (cand - base) + mlen) == lb_read32(src + (pos - base) + mlen))
          mlen += 4;
        while (pos + mlen < end_match && src[cand - base + mlen] == src[pos - base + mlen]) ++mlen;
      }
    }
    __syncthreads();
    if (pos < match_limit) table[h] = (uint16_t)(pos - base);  // last writer wins: any entry is verified
    __syncthreads();
    unsigned long long m = __ballot(cand != 0xFFFFFFFFu);
    if (m == 0) { ip += kLzThreads; continue; }
    // uniform greedy walk: take the first hit at/after the end of the last taken match
    unsigned long long sel = 0;
    uint32_t my_lit = 0, last_end = ip, prev_end = r.anchor;
    while (m) {
      const int g = __ffsll((long long)m) - 1;
      const uint32_t gml = __shfl(mlen, g);
      if (lane == g) my_lit = prev_end;
      sel |= 1ull << g;
      prev_end = last_end = ip + g + gml;
      const uint32_t skip = last_end - ip;       // hits before last_end overlap the match (skip > g)
      m = skip >= 64 ? 0ull : (m & (~0ull << skip));
    }
    bool is_first = false;                       // SPLIT: token + literals written by the merge
    if (SPLIT && !have_first) {
      const int g0 = __ffsll((long long)sel) - 1;
      is_first = lane == g0;
      r.first_mpos = ip + g0;
      r.first_mcode = __shfl(mlen, g0) - kLbMinMatch;
      have_first = true;
    }
    const bool mine = (sel >> lane) & 1ull;
    const uint32_t lit = mine && !is_first ? pos - my_lit : 0;
    const uint32_t need = !mine ? 0
                        : is_first ? 2 + lb_len_bytes(mlen - kLbMinMatch)
                                   : 1 + lb_len_bytes(lit) + lit + 2 + lb_len_bytes(mlen - kLbMinMatch);
    uint32_t incl = need;                        // wave inclusive prefix sum of sequence sizes
#pragma unroll
    for (int d = 1; d < kLzThreads; d <<= 1) {
      const uint32_t t = __shfl_up(incl, d);
      if (lane >= d) incl += t;
    }
    const uint32_t total = __shfl(incl, kLzThreads - 1);
    if (r.op + total > cap) { r.overflow = true; break; }
    const uint32_t o = r.op + incl - need;
    if (mine) {
      const uint32_t mcode = mlen - kLbMinMatch;
      const uint32_t moff = pos - cand;
      uint32_t q = o;
      if (!is_first) {
        dst[q] = lb_token(lit, mcode);
        q = lb_put_len(dst, q + 1, lit) + lit;
      }
      dst[q] = (uint8_t)(moff & 255);
      dst[q + 1] = (uint8_t)(moff >> 8);
      lb_put_len(dst, q + 2, mcode);
    }
    // literal runs, one selected sequence at a time, copied by the whole wave
    unsigned long long rest = sel;
    while (rest) {
      const int g = __ffsll((long long)rest) - 1;
      rest &= rest - 1;
      const uint32_t gl = __shfl(lit, g);
      if (gl == 0) continue;
      const uint32_t gs = __shfl(my_lit, g);
      const uint32_t go = __shfl(o, g) + 1 + lb_len_bytes(gl);
      for (uint32_t i = lane; i < gl; i += kLzThreads) dst[go + i] = src[gs - base + i];
    }
    r.op += total;
    r.anchor = prev_end;
    ip = last_end > ip + kLzThreads ? last_end : ip + kLzThreads;
  }
  return r;
}

// Whole chunks, one wave each.  STAGE: chunk staged in LDS (72 KiB per wave) vs read from global/L2
// with only the 8 KiB hash table in LDS (8x the waves per CU).
template <bool STAGE>
__global__ __launch_bounds__(kLzThreads) void lz4_compress_batch_kernel(const Lz4Chunk* __restrict__ ch,
                                                                       int n, int32_t* __restrict__ out_sizes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint16_t* table = reinterpret_cast<uint16_t*>(smem);                     // 8 KiB
  uint8_t* stage = smem + kLzTableBytes;                                   // 64 KiB (STAGE)
  const int lane = threadIdx.x;
  for (int w = blockIdx.x; w < n; w += gridDim.x) {
    const uint8_t* __restrict__ gsrc = reinterpret_cast<const uint8_t*>(ch[w].src);
    uint8_t* __restrict__ dst = reinterpret_cast<uint8_t*>(ch[w].dst);
    const uint32_t len = ch[w].src_bytes < kLzWindow ? ch[w].src_bytes : kLzWindow;
    const uint32_t cap = ch[w].dst_capacity;
    const uint8_t* src = gsrc;
    if constexpr (STAGE) {
      for (uint32_t i = lane; i < len; i += kLzThreads) stage[i] = gsrc[i];
      src = stage;
    }
    for (uint32_t i = lane; i < (1u << kLbHashLog); i += kLzThreads) table[i] = 0xFFFF;
    __syncthreads();
    const uint32_t match_limit = len > kLbMfLimit ? len - kLbMfLimit : 0;
    const uint32_t end_match = len > kLbLastLiterals ? len - kLbLastLiterals : 0;
    const LzParsed r = lz_batch_parse<false>(src, 0, table, dst, cap, 0, match_limit, end_match, lane);
    // the closing literal-only sequence
    const uint32_t lit = len - r.anchor;
    const bool fits = !r.overflow && r.op + 1 + lb_len_bytes(lit) + lit <= cap;
    uint32_t op = 0;
    if (fits) op = lz_put_literals<kLzThreads>(dst, r.op, src, r.anchor, lit, 0, lane);
    if (lane == 0) out_sizes[w] = fits ? (int32_t)op : -1;
    __syncthreads();
  }
}

// Segmented encoder for batches too small to fill the chip (one wave per 64 KiB chunk leaves
// 1k chunks at one wave per SIMD, latency-bound).  Each chunk is cut into up to S segments of
// >= 4 KiB parsed by S independent waves: a wave first re-hashes the `warm` bytes before its
// segment into its own table (so matches into the preceding data are still found), then runs the
// batch parse over its segment with matches confined to it.  The first sequence's literal run of a
// segment depends on where the previous segments' parses ended, so a wave writes its sequences to
// scratch WITHOUT that first header + literals; the merge kernel places the segments back to back
// and writes each first header with the literal run joined across the boundary.  Output is the
// same standard LZ4 block; ratio differs from the one-wave parse only at segment boundaries.
struct LzSeg {
  uint32_t first_mpos;   // position of the segment's first match (0xFFFFFFFF: no match)
  uint32_t first_mcode;  // its match length - 4
  uint32_t bytes;        // scratch bytes (0xFFFFFFFF: overflow)
  uint32_t tail;         // anchor after the segment's last match
};
constexpr uint32_t kLzSegMin = 4096;

__device__ __forceinline__ uint32_t lz_seg_count(uint32_t len, int S) {
  const uint32_t k = len / kLzSegMin;
  return k == 0 ? 1u : (k < (uint32_t)S ? k : (uint32_t)S);
}

__device__ __forceinline__ void lz_seg_bounds(uint32_t len, uint32_t nseg, uint32_t s, uint32_t* b, uint32_t* e) {
  const uint32_t seg = ((len + nseg - 1) / nseg + 63) & ~63u;
  *b = s * seg < len ? s * seg : len;
  *e = (s + 1) * seg < len && s + 1 < nseg ? (s + 1) * seg : len;
}

__global__ __launch_bounds__(kLzThreads) void lz4_seg_parse_kernel(const Lz4Chunk* __restrict__ ch, int n, int S,
                                                                  uint8_t* __restrict__ scratch, uint32_t seg_cap,
                                                                  LzSeg* __restrict__ segs, uint32_t warm) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint16_t* table = reinterpret_cast<uint16_t*>(smem);                     // 8 KiB
  const int lane = threadIdx.x;
  for (int t = blockIdx.x; t < n * S; t += gridDim.x) {
    const int w = t / S, s = t - (t / S) * S;
    const uint8_t* __restrict__ src = reinterpret_cast<const uint8_t*>(ch[w].src);
    const uint32_t len = ch[w].src_bytes < kLzWindow ? ch[w].src_bytes : kLzWindow;
    const uint32_t nseg = lz_seg_count(len, S);
    if ((uint32_t)s >= nseg) {
      if (lane == 0) segs[t] = LzSeg{0xFFFFFFFFu, 0, 0, 0};
      continue;
    }
    uint32_t sb, se;
    lz_seg_bounds(len, nseg, (uint32_t)s, &sb, &se);
    const bool last = (uint32_t)s + 1 == nseg;
    uint8_t* __restrict__ dst = scratch + (size_t)t * seg_cap;
    for (uint32_t i = lane; i < (1u << kLbHashLog); i += kLzThreads) table[i] = 0xFFFF;
    __syncthreads();
    for (uint32_t p = (sb > warm ? sb - warm : 0) + lane; p < sb; p += kLzThreads)
      table[lb_hash(lb_read32(src + p))] = (uint16_t)p;
    __syncthreads();
    // a match starts before match_limit and ends by end_match; inner segments keep their
    // matches inside the segment (the block-end rules only bind the last one)
    const uint32_t match_limit = last ? (len > kLbMfLimit ? len - kLbMfLimit : 0) : se - 3;
    const uint32_t end_match = last ? (len > kLbLastLiterals ? len - kLbLastLiterals : 0) : se;
    const LzParsed r = lz_batch_parse<true>(src, 0, table, dst, seg_cap, sb, match_limit, end_match, lane);
    if (lane == 0) segs[t] = LzSeg{r.first_mpos, r.first_mcode, r.overflow ? 0xFFFFFFFFu : r.op, r.anchor};
    __syncthreads();
  }
}

constexpr int kLzMergeThreads = 256;
constexpr int kLzMaxSeg = 16;

__global__ __launch_bounds__(kLzMergeThreads) void lz4_seg_merge_kernel(const Lz4Chunk* __restrict__ ch, int n, int S,
                                                                       const uint8_t* __restrict__ scratch,
                                                                       uint32_t seg_cap, const LzSeg* __restrict__ segs,
                                                                       int32_t* __restrict__ out_sizes) {
  __shared__ uint32_t s_off[kLzMaxSeg], s_p[kLzMaxSeg], s_fin[3];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  for (int w = blockIdx.x; w < n; w += gridDim.x) {
    const uint8_t* __restrict__ src = reinterpret_cast<const uint8_t*>(ch[w].src);
    uint8_t* __restrict__ dst = reinterpret_cast<uint8_t*>(ch[w].dst);
    const uint32_t len = ch[w].src_bytes < kLzWindow ? ch[w].src_bytes : kLzWindow;
    const LzSeg* sg = segs + (size_t)w * S;
    if (tid == 0) {
      uint32_t P = 0, out = 0;
      int bad = 0;
      for (int s = 0; s < S; ++s) {
        const LzSeg g = sg[s];
        if (g.bytes == 0xFFFFFFFFu) bad = 1;
        if (g.first_mpos == 0xFFFFFFFFu) { s_off[s] = 0xFFFFFFFFu; continue; }
        const uint32_t lit = g.first_mpos - P;
        s_off[s] = out;
        s_p[s] = P;
        out += 1 + lb_len_bytes(lit) + lit + g.bytes;
        P = g.tail;
      }
      const uint32_t lit = len - P;
      s_fin[0] = P;
      s_fin[1] = out;
      out += 1 + lb_len_bytes(lit) + lit;
      s_fin[2] = out;
      s_bad = bad || out > ch[w].dst_capacity;
    }
    __syncthreads();
    if (s_bad) {
      if (tid == 0) out_sizes[w] = -1;
      __syncthreads();
      continue;
    }
    for (int s = 0; s < S; ++s) {
      if (s_off[s] == 0xFFFFFFFFu) continue;
      const LzSeg g = sg[s];
      const uint32_t P = s_p[s];
      const uint32_t q = lz_put_literals<kLzMergeThreads>(dst, s_off[s], src, P, g.first_mpos - P, g.first_mcode, tid);
      const uint8_t* sc = scratch + ((size_t)w * S + s) * seg_cap;
      for (uint32_t i = tid; i < g.bytes; i += kLzMergeThreads) dst[q + i] = sc[i];
    }
    lz_put_literals<kLzMergeThreads>(dst, s_fin[1], src, s_fin[0], len - s_fin[0], 0, tid);
    if (tid == 0) out_sizes[w] = (int32_t)s_fin[2];
    __syncthreads();
  }
}

static hipError_t launch_lz4_compress_segmented(const Lz4Chunk* chunks, int n, int32_t* out_sizes, int S,
                                                hipStream_t stream) {
  S = S < 1 ? 1 : (S > kLzMaxSeg ? kLzMaxSeg : S);
  // seg_cap: LZ4's bound for the largest segment (64 KiB / S rounded up to 64, or 4 KiB minimum)
  const uint32_t seg = std::max<uint32_t>(kLzSegMin * 2, ((kLzWindow + S - 1) / S + 63) & ~63u);
  const uint32_t seg_cap = (seg + seg / 255 + 16 + 15) & ~15u;
  const size_t nseg = (size_t)n * S;
  void* mem = nullptr;
  hipError_t e = hipMallocAsync(&mem, nseg * seg_cap + nseg * sizeof(LzSeg), stream);
  if (e != hipSuccess) return e;
  uint8_t* scratch = static_cast<uint8_t*>(mem);
  LzSeg* segs = reinterpret_cast<LzSeg*>(scratch + nseg * seg_cap);
  hipLaunchKernelGGL(lz4_seg_parse_kernel, dim3((unsigned)std::min<size_t>(nseg, 65536)), dim3(kLzThreads),
                     kLzTableBytes, stream, chunks, n, S, scratch, seg_cap, segs, 4096u);
  e = hipGetLastError();
  if (e == hipSuccess) {
    hipLaunchKernelGGL(lz4_seg_merge_kernel, dim3((unsigned)std::min(n, 65536)), dim3(kLzMergeThreads), 0, stream,
                       chunks, n, S, scratch, seg_cap, segs, out_sizes);
    e = hipGetLastError();
  }
  const hipError_t f = hipFreeAsync(mem, stream);
  return e != hipSuccess ? e : f;
}

// 0: one sequence per probe batch (lz4_compress_kernel); 1: batch parse, chunk in LDS;
// 2: batch parse reading the chunk from global/L2 (8 KiB LDS per wave); 3: segmented parse
// (4 waves per chunk) + merge; 4 (default): segmented below 2048 chunks (S = 4096 waves / n,
// 2..8), batch parse above -- the batch parse fills the chip by itself there
static int g_lz4_encode_variant = 4;
void set_lz4_encode_variant(int v) { g_lz4_encode_variant = v; }

hipError_t launch_lz4_compress(const Lz4Chunk* chunks, int n, int32_t* out_sizes,
                               hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (g_lz4_encode_variant == 0) {
    const unsigned grid = (unsigned)std::min(n, 4096);
    hipLaunchKernelGGL(lz4_compress_kernel, dim3(grid), dim3(kLzThreads), kLzWindow + kLzTableBytes, stream,
                       chunks, n, out_sizes);
  } else if (g_lz4_encode_variant == 1) {
    const unsigned grid = (unsigned)std::min(n, 4096);
    hipLaunchKernelGGL((lz4_compress_batch_kernel<true>), dim3(grid), dim3(kLzThreads), kLzTableBytes + kLzWindow,
                       stream, chunks, n, out_sizes);
  } else if (g_lz4_encode_variant == 3) {
    return launch_lz4_compress_segmented(chunks, n, out_sizes, 4, stream);
  } else if (g_lz4_encode_variant == 4 && n < 2048) {
    return launch_lz4_compress_segmented(chunks, n, out_sizes, std::max(2, std::min(8, 4096 / n)), stream);
  } else {
    const unsigned grid = (unsigned)std::min(n, 65536);
    hipLaunchKernelGGL((lz4_compress_batch_kernel<false>), dim3(grid), dim3(kLzThreads), kLzTableBytes, stream,
                       chunks, n, out_sizes);
  }
  return hipGetLastError();
}

// One LZ4 block per page body of any size below 2^31 (Parquet LZ4_RAW pages): the segmented scheme
// above without its limits.  The rules, the link and the merge plan are those of lz4_block_host.h.
// Segments of a fixed size come from a host-built table, so one wave parses one segment of any page
// with the 8 KiB table holding positions relative to `begin - warm`; the link is a pass of its own
// (one lane per page), and the merge runs one workgroup per segment instead of one per chunk.
// Positions are 32-bit offsets in the page against that table base, the block's end rules bind
// every segment near the end, and the segment and its warm-up bytes are staged in LDS (a page has
// few segments, so a wave's chain of dependent loads, not occupancy, sets the time).
__global__ __launch_bounds__(kLzThreads) void lz4_page_parse_kernel(const LbArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint16_t* table = reinterpret_cast<uint16_t*>(smem);                     // 8 KiB
  uint8_t* stage = smem + kLzTableBytes;                                   // segment + warm bytes
  const int lane = threadIdx.x;
  uint32_t* recs = lb_recs(a);
  for (uint64_t t = blockIdx.x; t < a.nsegs; t += gridDim.x) {
    const int64_t* sg = a.segs + t * kLbSegCols;
    uint32_t* rec = recs + t * kLbRecCols;
    if (!lb_seg_ok(a, sg)) {                            // uniform: the whole wave skips the row
      if (lane == 0) {
        rec[kLbRecFirst] = kLbNone;
        rec[kLbRecCode] = rec[kLbRecTail] = 0;
        rec[kLbRecBytes] = kLbNone;
      }
      continue;
    }
    const uint8_t* __restrict__ gsrc = a.src + sg[kLbSegSrc];
    const uint32_t len = (uint32_t)a.pages[(uint64_t)sg[kLbSegPage] * kLbPageCols + kLbPageLen];
    const uint32_t sb = (uint32_t)sg[kLbSegBegin], se = (uint32_t)sg[kLbSegEnd];
    const uint32_t base = sb > a.warm ? sb - a.warm : 0;
    uint8_t* __restrict__ dst = a.scratch + sg[kLbSegScratch];
    const uint32_t seg_cap = (uint32_t)lb_bound(se - sb);
    // body bytes [base, se) into LDS: every read below lies in them (a probe reads 4 bytes before
    // se, a match ends by se, literals start at or after sb); src[p - base] is body byte p
    for (uint32_t i = lane; i < se - base; i += kLzThreads) stage[i] = gsrc[base + i];
    const uint8_t* src = stage;
    for (uint32_t i = lane; i < (1u << kLbHashLog); i += kLzThreads) table[i] = 0xFFFF;
    __syncthreads();
    for (uint32_t p = base + lane; p < sb; p += kLzThreads)
      if (p + 4 <= se) table[lb_hash(lb_read32(src + (p - base)))] = (uint16_t)(p - base);
    __syncthreads();
    uint32_t match_limit, end_match;
    lb_limits(len, se, &match_limit, &end_match);
    const LzParsed r = lz_batch_parse<true>(src, base, table, dst, seg_cap, sb, match_limit, end_match, lane);
    if (lane == 0) {
      rec[kLbRecFirst] = r.first_mpos;
      rec[kLbRecCode] = r.first_mcode;
      rec[kLbRecBytes] = r.overflow ? kLbNone : r.op;
      rec[kLbRecTail] = r.anchor;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kLzThreads) void lz4_page_link_kernel(const LbArgs a) {
  const uint64_t p = (uint64_t)blockIdx.x * kLzThreads + threadIdx.x;
  if (p < a.npages) lb_link_page(a, p);
}

__global__ __launch_bounds__(kLzMergeThreads) void lz4_page_merge_kernel(const LbArgs a) {
  const uint32_t tid = threadIdx.x;
  for (uint64_t t = blockIdx.x; t < a.nsegs; t += gridDim.x) {
    LbMerge m;
    lb_merge_plan(a, t, &m);                            // the same plan in every thread
    if (m.head) {
      if (tid == 0) lb_put_head(m);
      uint8_t* q = m.dst + m.o + 1 + lb_len_bytes(m.lit);
      for (uint32_t i = tid; i < m.lit; i += kLzMergeThreads) q[i] = m.src[m.P + i];
      for (uint32_t i = tid; i < m.bytes; i += kLzMergeThreads) q[m.lit + i] = m.seq[i];
    }
    if (m.fin) {
      if (tid == 0) lb_put_fin(m);
      uint8_t* q = m.dst + m.fin_o + 1 + lb_len_bytes(m.fin_lit);
      for (uint32_t i = tid; i < m.fin_lit; i += kLzMergeThreads) q[i] = m.src[m.fin_p + i];
    }
  }
}

static bool lz4_page_args_ok(const LbArgs& a, bool merge) {
  constexpr uint64_t kMax = 1ull << 31;
  if (a.npages == 0 || a.nsegs == 0 || a.npages > kMax || a.nsegs > kMax) return false;
  if (!a.src || !a.pages || !a.segs || !a.scratch || !a.result) return false;
  if (a.scratch_bytes < lb_scratch_head(a.nsegs) || (reinterpret_cast<uintptr_t>(a.scratch) & 3)) return false;
  if (a.segment < 1 || (uint64_t)a.segment + a.warm > 65535) return false;
  return !merge || (a.dst && a.out);
}

hipError_t launch_lz4_page_parse(const LbArgs& a, hipStream_t stream) {
  if (!lz4_page_args_ok(a, false)) return hipErrorInvalidValue;
  const size_t lds = kLzTableBytes + (((size_t)a.segment + a.warm + 15) & ~(size_t)15);
  hipLaunchKernelGGL(lz4_page_parse_kernel, dim3((unsigned)std::min<uint64_t>(a.nsegs, 65536)), dim3(kLzThreads), lds,
                     stream, a);
  return hipGetLastError();
}

hipError_t launch_lz4_page_link(const LbArgs& a, hipStream_t stream) {
  if (!lz4_page_args_ok(a, false)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lz4_page_link_kernel, dim3((unsigned)((a.npages + kLzThreads - 1) / kLzThreads)),
                     dim3(kLzThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_lz4_page_merge(const LbArgs& a, hipStream_t stream) {
  if (!lz4_page_args_ok(a, true)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lz4_page_merge_kernel, dim3((unsigned)std::min<uint64_t>(a.nsegs, 65536)),
                     dim3(kLzMergeThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace amdx
