// Parquet pages into typed columns: the rules, as plain C++.  Five passes, each over tables of
// int64 rows that the caller lays out:
//
//   walk    one column chunk per lane: the Thrift-compact PageHeaders that sit between the pages
//           become page-table rows (kPqCols int64 each).  Two calls, count then fill.
//   lz4     one page per lane: the page becomes a chunk for the LZ4 block decoder and the bytes
//           that are stored raw (the levels of a V2 page, a page that is not compressed) are copied.
//   hybrid  one RLE / bit-packed hybrid stream (kPqStreamCols int64 each) becomes int32 values:
//           definition levels, dictionary indices, RLE booleans.
//   place   one row per lane: a row of a data page (kPqPageCols int64 each) takes value number
//           `rank` of its page, from PLAIN bytes at any byte phase, from the chunk's dictionary
//           through a decoded index, or from a decoded boolean.
//   bytes   one PLAIN BYTE_ARRAY page per lane: the chain of 4-byte length prefixes becomes
//           start / length / status per value.
//
// Nothing is trusted: every length, offset, count and index is checked against the window it
// belongs to before a byte is read, and against the output's size before one is written.  What
// does not fit gives an error code (walk, hybrid) or status 2 (place, bytes), never an access
// outside.  Status: 0 a value, 1 null, 2 corrupt.
//
// Written once and compiled twice, as json_fields_host.h is: the host loops (DRAM tiers, CPU-only
// use, the stand-alone check program) and, through PQ_HD, the device code of parquet_decode.hip.
// No HIP include.
#pragma once
#include <cstdint>

#if defined(__HIP__)
#define PQ_HD __attribute__((host)) __attribute__((device))
#else
#define PQ_HD
#endif

namespace amdx {

// ---- tables ---------------------------------------------------------------------------------------
// Page-table row (walk output).
enum {
  kPqType = 0,          // 0 DATA_PAGE, 2 DICTIONARY_PAGE, 3 DATA_PAGE_V2
  kPqPayload = 1,       // offset of the page's bytes in the buffer
  kPqCompressed = 2,    // compressed_page_size
  kPqUncompressed = 3,  // uncompressed_page_size
  kPqNumValues = 4,
  kPqEncoding = 5,      // value encoding
  kPqDefLen = 6,        // V2: definition_levels_byte_length
  kPqRepLen = 7,        // V2: repetition_levels_byte_length
  kPqNumNulls = 8,      // V2 (-1 otherwise)
  kPqIsCompressed = 9,  // V2 (1 otherwise)
  kPqChunk = 10,        // the chunk the page belongs to
  kPqDefEncoding = 11,  // V1: definition_level_encoding
  kPqCols = 12
};
// Stream row (hybrid input).
enum {
  kPsOff = 0,           // a window of the buffer
  kPsLen = 1,
  kPsKind = 2,          // 0: the window is the stream; 1: 4-byte length, then the stream; 2: one byte
                        // that holds the bit width, then the stream to the window's end
  kPsSkip = 3,          // 1: a 4-byte length and that many bytes come first and are skipped
  kPsWidth = 4,         // bit width (kinds 0 and 1)
  kPsCount = 5,         // values to produce
  kPsOut = 6,           // the first of them is out[kPsOut]; rows ascend in kPsOut
  kPsSpare = 7,
  kPqStreamCols = 8
};
// Data-page row (place and bytes input).
enum {
  kPpRowBase = 0,       // the page's first row in the column's output; rows ascend in kPpRowBase
  kPpNumValues = 1,     // rows of the page
  kPpSource = 2,        // 0 PLAIN, 1 dictionary index, 2 decoded boolean, 3 corrupt page
  kPpOff = 3,           // PLAIN: a window of the buffer
  kPpLen = 4,
  kPpSkip = 5,          // PLAIN: as kPsSkip
  kPpIdxBase = 6,       // sources 1 and 2: value k of the page is idx[kPpIdxBase + k]
  kPpDefStream = 7,     // the page's streams, for their error codes (-1: none)
  kPpValStream = 8,
  kPpSpare = 9,
  kPqPageCols = 10
};
enum {
  kPqOk = 0,
  kPqErrHeader = 1,     // a header that runs past its chunk or is no Thrift struct
  kPqErrPageType = 2,   // a page type that is none of data, dictionary, index, data V2
  kPqErrSize = 3,       // a negative or missing size or count
  kPqErrPayload = 4,    // a payload that runs past its chunk
  kPqErrChunk = 5,      // a chunk outside the buffer
  kPqErrStream = 6,     // a stream outside the buffer, a length prefix past its window, a width above 32
  kPqErrRun = 7         // a run that reads past its stream's end, or a stream that ends early
};
constexpr int kPqSkipDepth = 8;

// ---- Thrift compact -------------------------------------------------------------------------------
struct PqCur {
  const uint8_t* p;
  const uint8_t* end;
  bool ok;
};

PQ_HD inline uint64_t pq_varint(PqCur& c) {
  uint64_t v = 0;
  for (int s = 0; s < 64; s += 7) {
    if (c.p >= c.end) break;
    const uint8_t b = *c.p++;
    v |= (uint64_t)(b & 0x7F) << s;
    if (!(b & 0x80)) return v;
  }
  c.ok = false;
  return 0;
}
PQ_HD inline int64_t pq_zigzag(uint64_t v) { return (int64_t)(v >> 1) ^ -(int64_t)(v & 1); }
PQ_HD inline void pq_advance(PqCur& c, uint64_t n) {
  if (n > (uint64_t)(c.end - c.p)) {
    c.ok = false;
    c.p = c.end;
  } else {
    c.p += n;
  }
}

// One field header of a struct: false at the stop byte or at the end of the bytes.
PQ_HD inline bool pq_field(PqCur& c, int32_t* id, uint32_t* type) {
  if (c.p >= c.end) {
    c.ok = false;
    return false;
  }
  const uint8_t b = *c.p++;
  if (b == 0) return false;
  *type = b & 15u;
  if (b >> 4) *id += b >> 4;
  else *id = (int32_t)pq_zigzag(pq_varint(c));
  return c.ok;
}

// Skips one value of a Thrift type, containers and nested structs included, without recursion: a
// small stack of open containers (rem: elements left, or kStruct).  Deeper nesting than
// kPqSkipDepth, an unknown type or a length past the end clear c.ok.
PQ_HD inline void pq_skip(PqCur& c, uint32_t type) {
  constexpr uint32_t kStruct = 0xFFFFFFFFu;
  uint32_t rem[kPqSkipDepth];
  uint8_t tk[kPqSkipDepth], tv[kPqSkipDepth];
  int d = 0;
  uint32_t t = type;
  for (;;) {
    uint32_t push_rem = 0, push_k = 0, push_v = 0;
    bool push = false;
    switch (t) {
      case 1: case 2: break;                          // a bool lives in its field header
      case 3: pq_advance(c, 1); break;
      case 4: case 5: case 6: pq_varint(c); break;
      case 7: pq_advance(c, 8); break;
      case 8: {
        const uint64_t n = pq_varint(c);
        pq_advance(c, n);
        break;
      }
      case 9: case 10: {
        if (c.p >= c.end) { c.ok = false; break; }
        const uint8_t h = *c.p++;
        uint64_t n = h >> 4;
        if (n == 15) n = pq_varint(c);
        if (n > (uint64_t)(c.end - c.p)) { c.ok = false; break; }     // an element is a byte at least
        uint32_t et = h & 15u;
        if (et == 1 || et == 2) et = 3;               // a bool in a list is one byte
        push = n > 0;
        push_rem = (uint32_t)n;
        push_k = push_v = et;
        break;
      }
      case 11: {
        const uint64_t n = pq_varint(c);
        if (n > (uint64_t)(c.end - c.p)) { c.ok = false; break; }
        if (n == 0) break;
        if (c.p >= c.end) { c.ok = false; break; }
        const uint8_t kv = *c.p++;
        push = true;
        push_rem = (uint32_t)(2 * n);
        push_k = kv >> 4;
        push_v = kv & 15u;
        if (push_k == 1 || push_k == 2) push_k = 3;
        if (push_v == 1 || push_v == 2) push_v = 3;
        break;
      }
      case 12: push = true; push_rem = kStruct; break;
      default: c.ok = false; break;
    }
    if (!c.ok) return;
    if (push) {
      if (d == kPqSkipDepth) { c.ok = false; return; }
      rem[d] = push_rem;
      tk[d] = (uint8_t)push_k;
      tv[d] = (uint8_t)push_v;
      ++d;
    }
    for (;;) {                                        // the next value to skip, if any
      if (d == 0) return;
      if (rem[d - 1] == kStruct) {
        int32_t id = 0;
        uint32_t ft = 0;
        if (!pq_field(c, &id, &ft)) {
          if (!c.ok) return;
          --d;
          continue;
        }
        t = ft;
        break;
      }
      if (rem[d - 1] == 0) {
        --d;
        continue;
      }
      t = (rem[d - 1] & 1u) ? tv[d - 1] : tk[d - 1]; // a map counts 2n down: even is a key
      --rem[d - 1];
      break;
    }
  }
}

// The fields of DataPageHeader (kind 0), DictionaryPageHeader (1) or DataPageHeaderV2 (2) that the
// page table keeps; statistics and everything unknown are skipped by type.
PQ_HD inline void pq_sub_header(PqCur& c, int kind, int64_t* v) {
  int32_t id = 0;
  uint32_t t = 0;
  while (pq_field(c, &id, &t)) {
    const bool isint = t == 4 || t == 5 || t == 6;
    int col = -1;
    if (kind == 0) col = id == 1 ? kPqNumValues : id == 2 ? kPqEncoding : id == 3 ? kPqDefEncoding : -1;
    else if (kind == 1) col = id == 1 ? kPqNumValues : id == 2 ? kPqEncoding : -1;
    else col = id == 1 ? kPqNumValues : id == 2 ? kPqNumNulls : id == 4 ? kPqEncoding : id == 5 ? kPqDefLen
               : id == 6 ? kPqRepLen : -1;
    if (col >= 0 && isint) v[col] = pq_zigzag(pq_varint(c));
    else if (kind == 2 && id == 7 && (t == 1 || t == 2)) v[kPqIsCompressed] = t == 1 ? 1 : 0;
    else pq_skip(c, t);
    if (!c.ok) return;
  }
}

// One PageHeader in p[0, avail): the row's columns except kPqPayload and kPqChunk, and the header's
// size.  Returns an error code.
PQ_HD inline int pq_page_header(const uint8_t* p, uint64_t avail, int64_t* v, uint64_t* header_bytes) {
  PqCur c{p, p + avail, true};
  for (int i = 0; i < kPqCols; ++i) v[i] = 0;
  v[kPqType] = v[kPqCompressed] = v[kPqUncompressed] = v[kPqNumNulls] = v[kPqEncoding] = -1;
  v[kPqIsCompressed] = 1;
  v[kPqDefEncoding] = 3;                              // RLE
  int32_t id = 0;
  uint32_t t = 0;
  while (pq_field(c, &id, &t)) {
    const bool isint = t == 4 || t == 5 || t == 6;
    if (isint && id >= 1 && id <= 3) {
      v[id == 1 ? kPqType : id == 2 ? kPqUncompressed : kPqCompressed] = pq_zigzag(pq_varint(c));
    } else if (t == 12 && (id == 5 || id == 7 || id == 8)) {
      pq_sub_header(c, id == 5 ? 0 : id == 7 ? 1 : 2, v);
    } else {
      pq_skip(c, t);
    }
    if (!c.ok) return kPqErrHeader;
  }
  if (!c.ok) return kPqErrHeader;
  *header_bytes = (uint64_t)(c.p - p);
  if (v[kPqType] < 0 || v[kPqCompressed] < 0 || v[kPqUncompressed] < 0 || v[kPqNumValues] < 0 || v[kPqDefLen] < 0 ||
      v[kPqRepLen] < 0 || v[kPqCompressed] > 0x7FFFFFFFll || v[kPqUncompressed] > 0x7FFFFFFFll ||
      v[kPqNumValues] > 0x7FFFFFFFll)
    return kPqErrSize;
  if (v[kPqType] == 3 && v[kPqDefLen] + v[kPqRepLen] > v[kPqCompressed]) return kPqErrSize;
  return kPqOk;
}

// ---- walk -------------------------------------------------------------------------------------------
struct PqWalkArgs {
  const uint8_t* data;
  uint64_t data_bytes;
  const int64_t* chunk_off;  // [nchunks] a chunk is data[chunk_off, chunk_off + chunk_len)
  const int64_t* chunk_len;
  uint64_t nchunks;
  int32_t* counts;           // [nchunks] pages found (index pages are not counted)
  int32_t* errors;           // [nchunks]
  const int64_t* page_base;  // fill: [nchunks + 1] the exclusive scan of the counts
  int64_t* table;            // fill: [table_rows][kPqCols]; null: count only
  uint64_t table_rows;
};

PQ_HD inline void pq_walk_chunk(const PqWalkArgs& a, uint64_t c) {
  const int64_t off = a.chunk_off[c], len = a.chunk_len[c];
  int32_t count = 0, err = kPqOk;
  if (off < 0 || len < 0 || (uint64_t)off > a.data_bytes || (uint64_t)len > a.data_bytes - (uint64_t)off) {
    err = kPqErrChunk;
  } else {
    int64_t lo = 0, hi = 0;
    if (a.table) {
      lo = a.page_base[c];
      hi = a.page_base[c + 1];
      if (lo < 0) lo = hi = 0;
      if (hi > (int64_t)a.table_rows) hi = (int64_t)a.table_rows;
    }
    const uint8_t* base = a.data + off;
    uint64_t pos = 0;
    while (pos < (uint64_t)len) {
      int64_t v[kPqCols];
      uint64_t hb = 0;
      err = pq_page_header(base + pos, (uint64_t)len - pos, v, &hb);
      if (err) break;
      const uint64_t payload = pos + hb;
      if ((uint64_t)v[kPqCompressed] > (uint64_t)len - payload) {
        err = kPqErrPayload;
        break;
      }
      pos = payload + (uint64_t)v[kPqCompressed];
      if (v[kPqType] == 1) continue;                  // INDEX_PAGE
      if (v[kPqType] != 0 && v[kPqType] != 2 && v[kPqType] != 3) {
        err = kPqErrPageType;
        break;
      }
      if (a.table && lo + count < hi) {
        v[kPqPayload] = off + (int64_t)payload;
        v[kPqChunk] = (int64_t)c;
        int64_t* row = a.table + (uint64_t)(lo + count) * kPqCols;
        for (int i = 0; i < kPqCols; ++i) row[i] = v[i];
      }
      ++count;
    }
  }
  if (a.counts) a.counts[c] = count;
  if (a.errors) a.errors[c] = err;
}

// ---- windows and streams ----------------------------------------------------------------------------
PQ_HD inline uint32_t pq_le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// The window data[off, off + len), after the skipped block when skip is set.  False: not inside the
// buffer, or the block's length prefix runs past the window.
PQ_HD inline bool pq_window(const uint8_t* data, uint64_t data_bytes, int64_t off, int64_t len, int64_t skip,
                            const uint8_t** p, uint64_t* n) {
  if (off < 0 || len < 0 || (uint64_t)off > data_bytes || (uint64_t)len > data_bytes - (uint64_t)off) return false;
  const uint8_t* q = data + off;
  uint64_t m = (uint64_t)len;
  if (skip) {
    if (m < 4) return false;
    const uint64_t l = pq_le32(q);
    if (l > m - 4) return false;
    q += 4 + l;
    m -= 4 + l;
  }
  *p = q;
  *n = m;
  return true;
}

struct PqStreamArgs {
  const uint8_t* data;
  uint64_t data_bytes;
  const int64_t* streams;    // [nstreams][kPqStreamCols]
  uint64_t nstreams;
  int32_t* out;              // [out_n]
  uint64_t out_n;
  int32_t* errors;           // [nstreams]
  // the cooperative form's run table: counted, then filled
  int32_t* run_counts;       // [nstreams]
  const int64_t* run_base;   // [nstreams + 1] the exclusive scan of run_counts
  int64_t* runs;             // [runs_rows][4]: first value, count | kind << 32, byte position, value
  uint64_t runs_rows;
};

struct PqStream {
  const uint8_t* p;          // the hybrid runs
  uint64_t len;
  uint32_t width;
  uint64_t n;                // values to produce, cut to the output
  uint64_t out;
  int err;
};

PQ_HD inline PqStream pq_open(const PqStreamArgs& a, uint64_t s) {
  const int64_t* r = a.streams + s * kPqStreamCols;
  PqStream st{nullptr, 0, 0, 0, 0, kPqOk};
  const int64_t ob = r[kPsOut], cnt = r[kPsCount];
  if (ob >= 0 && (uint64_t)ob < a.out_n && cnt > 0) {
    st.out = (uint64_t)ob;
    st.n = (uint64_t)cnt < a.out_n - st.out ? (uint64_t)cnt : a.out_n - st.out;
  }
  int64_t w = r[kPsWidth];
  if (!pq_window(a.data, a.data_bytes, r[kPsOff], r[kPsLen], r[kPsSkip], &st.p, &st.len)) {
    st.err = kPqErrStream;
    return st;
  }
  if (r[kPsKind] == 1) {
    if (st.len < 4 || pq_le32(st.p) > st.len - 4) {
      st.err = kPqErrStream;
      return st;
    }
    st.len = pq_le32(st.p);
    st.p += 4;
  } else if (r[kPsKind] == 2) {
    if (st.len < 1) {
      if (st.n) st.err = kPqErrStream;                // a page without values may be empty
      return st;
    }
    w = st.p[0];
    st.p += 1;
    st.len -= 1;
  } else if (r[kPsKind] != 0) {
    st.err = kPqErrStream;
    return st;
  }
  if (w < 0 || w > 32) {
    st.err = kPqErrStream;
    return st;
  }
  st.width = (uint32_t)w;
  return st;
}

struct PqRun {
  uint64_t count;            // values of the run (a bit-packed run: groups * 8)
  uint32_t kind;             // 0 repeated, 1 bit-packed
  uint64_t pos;              // bit-packed: where its bytes start in the stream
  uint32_t value;            // repeated: the value
};

// The run whose header is at *pos; *pos moves past the run.  An error when its bytes are not all
// inside the stream.
PQ_HD inline int pq_next_run(const PqStream& st, uint64_t* pos, PqRun* r) {
  if (*pos >= st.len) return kPqErrRun;
  PqCur c{st.p + *pos, st.p + st.len, true};
  const uint64_t h = pq_varint(c);
  if (!c.ok) return kPqErrRun;
  uint64_t at = (uint64_t)(c.p - st.p);
  if (h & 1) {
    const uint64_t groups = h >> 1;
    uint64_t bytes = 0;
    if (st.width) {
      if (groups > st.len - at) return kPqErrRun;     // also keeps groups * width from overflowing
      bytes = groups * st.width;
      if (bytes > st.len - at) return kPqErrRun;
    }
    r->count = groups > (1ull << 60) ? ~0ull : groups * 8;
    r->kind = 1;
    r->pos = at;
    r->value = 0;
    at += bytes;
  } else {
    const uint32_t nb = (st.width + 7) / 8;
    if (nb > st.len - at) return kPqErrRun;
    uint32_t v = 0;
    for (uint32_t i = 0; i < nb; ++i) v |= (uint32_t)st.p[at + i] << (8 * i);
    r->count = h >> 1;
    r->kind = 0;
    r->pos = at;
    r->value = st.width == 32 ? v : v & ((1u << st.width) - 1u);
    at += nb;
  }
  *pos = at;
  return kPqOk;
}

// Value i of a bit-packed run at st.p + pos: its bits at whatever byte they start.  The run's bytes
// are inside the stream, so the bytes of value i are; eight bytes are loaded at once where the
// stream has them, else the bytes that hold the value one by one.
PQ_HD inline uint32_t pq_unpack(const PqStream& st, uint64_t pos, uint64_t i) {
  if (st.width == 0) return 0;
  const uint64_t bit = i * st.width;
  const uint64_t at = pos + (bit >> 3);
  const uint32_t sh = (uint32_t)(bit & 7);
  uint64_t w = 0;
  if (at + 8 <= st.len) {
    __builtin_memcpy(&w, st.p + at, 8);
  } else {
    const uint32_t nb = (sh + st.width + 7) / 8;
    for (uint32_t j = 0; j < nb; ++j) w |= (uint64_t)st.p[at + j] << (8 * j);
  }
  w >>= sh;
  return st.width == 32 ? (uint32_t)w : (uint32_t)w & ((1u << st.width) - 1u);
}

// One stream, serially: the host loop and one lane's work in kernel variant 0.  The values of the
// runs before a bad one are produced; the rest are 0.
PQ_HD inline void pq_stream_serial(const PqStreamArgs& a, uint64_t s) {
  const PqStream st = pq_open(a, s);
  int err = st.err;
  uint64_t done = 0, pos = 0;
  while (!err && done < st.n) {
    PqRun r;
    err = pq_next_run(st, &pos, &r);
    if (err) break;
    const uint64_t m = r.count < st.n - done ? r.count : st.n - done;
    int32_t* o = a.out + st.out + done;
    if (r.kind == 0) {
      for (uint64_t i = 0; i < m; ++i) o[i] = (int32_t)r.value;
    } else {
      for (uint64_t i = 0; i < m; ++i) o[i] = (int32_t)pq_unpack(st, r.pos, i);
    }
    done += m;
  }
  for (uint64_t i = done; i < st.n; ++i) a.out[st.out + i] = 0;
  if (a.errors) a.errors[s] = err;
}

// The run table of one stream: with a.runs null the runs that the stream's values need are counted
// (and the error code is set), otherwise they are written, inside [run_base[s], run_base[s + 1])
// cut to the table.
PQ_HD inline void pq_stream_runs(const PqStreamArgs& a, uint64_t s) {
  const PqStream st = pq_open(a, s);
  int err = st.err;
  uint64_t done = 0, pos = 0;
  int32_t k = 0;
  int64_t lo = 0, hi = 0;
  if (a.runs) {
    lo = a.run_base[s];
    hi = a.run_base[s + 1];
    if (lo < 0) lo = hi = 0;
    if (hi > (int64_t)a.runs_rows) hi = (int64_t)a.runs_rows;
  }
  while (!err && done < st.n) {
    PqRun r;
    err = pq_next_run(st, &pos, &r);
    if (err) break;
    const uint64_t m = r.count < st.n - done ? r.count : st.n - done;
    if (m == 0) continue;                             // an empty run holds no value
    if (a.runs && lo + k < hi) {
      int64_t* row = a.runs + (uint64_t)(lo + k) * 4;
      row[0] = (int64_t)done;
      row[1] = (int64_t)(m | ((uint64_t)r.kind << 32));
      row[2] = (int64_t)r.pos;
      row[3] = (int64_t)r.value;
    }
    ++k;
    done += m;
  }
  if (!a.runs) {
    if (a.run_counts) a.run_counts[s] = k;
    if (a.errors) a.errors[s] = err;
  }
}

// Output slot t through the run table: the stream that owns it (the last whose kPsOut is not above
// t), then the run (the last whose first value is not above t's place in the stream).  A slot that
// no stream's values reach is left as it is; one past the stream's good runs is 0.
PQ_HD inline void pq_stream_value(const PqStreamArgs& a, uint64_t t) {
  uint64_t lo = 0, hi = a.nstreams;                   // streams[lo].out <= t < streams[hi].out
  if (a.nstreams == 0 || a.streams[kPsOut] > (int64_t)t) return;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) / 2;
    if (a.streams[mid * kPqStreamCols + kPsOut] <= (int64_t)t) lo = mid;
    else hi = mid;
  }
  const PqStream st = pq_open(a, lo);
  if (st.n == 0 || t < st.out || t - st.out >= st.n) return;
  const uint64_t i = t - st.out;
  int64_t rlo = a.run_base[lo], rhi = a.run_base[lo + 1];
  if (rlo < 0) rlo = rhi = 0;
  if (rhi > (int64_t)a.runs_rows) rhi = (int64_t)a.runs_rows;
  int32_t v = 0;
  if (!st.err && rhi > rlo) {
    const int64_t* runs = a.runs;
    int64_t x = rlo, y = rhi;                         // runs[x].first <= i (the first run starts at 0)
    while (y - x > 1) {
      const int64_t mid = (x + y) / 2;
      if ((uint64_t)runs[mid * 4] <= i) x = mid;
      else y = mid;
    }
    const int64_t* row = runs + x * 4;
    const uint64_t first = (uint64_t)row[0], cnt = (uint64_t)row[1] & 0xFFFFFFFFull;
    if (i >= first && i - first < cnt) {
      // a row of the table was checked against the stream when it was written
      v = ((uint64_t)row[1] >> 32) ? (int32_t)pq_unpack(st, (uint64_t)row[2], i - first) : (int32_t)row[3];
    }
  }
  a.out[t] = v;
}

// ---- place ------------------------------------------------------------------------------------------
struct PqPlaceArgs {
  const uint8_t* data;
  uint64_t data_bytes;
  const int64_t* pages;      // [npages][kPqPageCols]
  uint64_t npages;
  const int64_t* excl;       // [rows + 1] the exclusive scan of validity; null: every row is valid
  const int32_t* idx;        // [idx_n] decoded indices or booleans
  uint64_t idx_n;
  const uint8_t* dict;       // [dict_size] entries of `width` bytes
  uint64_t dict_size;
  const int32_t* stream_err; // [nstreams] or null
  uint64_t nstreams;
  uint32_t width;            // bytes of a value: 1, 4 or 8
  uint32_t is_bool;          // PLAIN values are bits, least significant first; the output is one byte
  uint8_t* values;           // [rows] of `width` bytes
  uint8_t* status;           // [rows]
  uint64_t rows;
};

PQ_HD inline bool pq_stream_bad(const int32_t* errs, uint64_t n, int64_t s) {
  return errs && s >= 0 && (uint64_t)s < n && errs[s] != 0;
}

// The page of row r: the last whose kPpRowBase is not above r; -1 when no page holds the row.
PQ_HD inline int64_t pq_page_of(const int64_t* pages, uint64_t npages, uint64_t r) {
  if (npages == 0 || pages[kPpRowBase] > (int64_t)r) return -1;
  uint64_t lo = 0, hi = npages;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) / 2;
    if (pages[mid * kPqPageCols + kPpRowBase] <= (int64_t)r) lo = mid;
    else hi = mid;
  }
  const int64_t* pg = pages + lo * kPqPageCols;
  if (pg[kPpNumValues] < 0 || r - (uint64_t)pg[kPpRowBase] >= (uint64_t)pg[kPpNumValues]) return -1;
  return (int64_t)lo;
}

PQ_HD inline void pq_place_row(const PqPlaceArgs& a, uint64_t r) {
  uint8_t* out = a.values + r * a.width;
  for (uint32_t i = 0; i < a.width; ++i) out[i] = 0;
  uint8_t st = 2;
  const int64_t p = pq_page_of(a.pages, a.npages, r);
  if (p >= 0) {
    const int64_t* pg = a.pages + (uint64_t)p * kPqPageCols;
    const uint64_t rb = (uint64_t)pg[kPpRowBase];
    const bool bad = pg[kPpSource] == 3 || pq_stream_bad(a.stream_err, a.nstreams, pg[kPpDefStream]) ||
                     pq_stream_bad(a.stream_err, a.nstreams, pg[kPpValStream]);
    const bool valid = !a.excl || a.excl[r + 1] > a.excl[r];
    if (bad) {
      st = 2;
    } else if (!valid) {
      st = 1;
    } else {
      const int64_t rank64 = a.excl ? a.excl[r] - a.excl[rb] : (int64_t)(r - rb);
      const uint64_t rank = (uint64_t)rank64;
      if (rank64 < 0) {
        st = 2;
      } else if (pg[kPpSource] == 0) {
        const uint8_t* q;
        uint64_t n;
        if (pq_window(a.data, a.data_bytes, pg[kPpOff], pg[kPpLen], pg[kPpSkip], &q, &n)) {
          if (a.is_bool) {
            if (rank / 8 < n) {
              out[0] = (q[rank / 8] >> (rank & 7)) & 1u;
              st = 0;
            }
          } else if (rank < n / a.width) {
            const uint8_t* src = q + rank * a.width;  // any byte phase: byte loads
            for (uint32_t i = 0; i < a.width; ++i) out[i] = src[i];
            st = 0;
          }
        }
      } else if (pg[kPpSource] == 1 || pg[kPpSource] == 2) {
        const int64_t j = pg[kPpIdxBase] + rank64;
        if (pg[kPpIdxBase] >= 0 && (uint64_t)j < a.idx_n) {
          const uint32_t ix = (uint32_t)a.idx[j];
          if (pg[kPpSource] == 2) {
            out[0] = ix & 1u;
            st = 0;
          } else if (ix < a.dict_size) {
            const uint8_t* src = a.dict + (uint64_t)ix * a.width;
            for (uint32_t i = 0; i < a.width; ++i) out[i] = src[i];
            st = 0;
          }
        }
      }
    }
  }
  a.status[r] = st;
}

// ---- PLAIN BYTE_ARRAY -------------------------------------------------------------------------------
struct PqBytesArgs {
  const uint8_t* data;
  uint64_t data_bytes;
  const int64_t* pages;      // [npages][kPqPageCols], source 0 (others are left alone)
  uint64_t npages;
  const int64_t* excl;       // [rows + 1] or null; value slots are numbered by it (else by row)
  uint64_t rows;
  const int32_t* stream_err;
  uint64_t nstreams;
  int64_t* start;            // [nvalues] offset of the value's bytes in the buffer
  int32_t* length;
  uint8_t* status;
  uint64_t nvalues;
};

PQ_HD inline void pq_bytes_page(const PqBytesArgs& a, uint64_t p) {
  const int64_t* pg = a.pages + p * kPqPageCols;
  if (pg[kPpSource] != 0 && pg[kPpSource] != 3) return;
  const int64_t rb = pg[kPpRowBase], nv = pg[kPpNumValues];
  if (rb < 0 || nv < 0 || (uint64_t)rb > a.rows || (uint64_t)nv > a.rows - (uint64_t)rb) return;
  uint64_t base = (uint64_t)rb, n = (uint64_t)nv;
  if (a.excl) {
    const int64_t b = a.excl[rb], e = a.excl[rb + nv];
    if (b < 0 || e < b) return;
    base = (uint64_t)b;
    n = (uint64_t)(e - b);
  }
  if (base >= a.nvalues) return;
  if (n > a.nvalues - base) n = a.nvalues - base;
  const uint8_t* q = nullptr;
  uint64_t len = 0;
  bool bad = pg[kPpSource] == 3 || pq_stream_bad(a.stream_err, a.nstreams, pg[kPpDefStream]) ||
             !pq_window(a.data, a.data_bytes, pg[kPpOff], pg[kPpLen], pg[kPpSkip], &q, &len);
  uint64_t pos = 0;
  for (uint64_t k = 0; k < n; ++k) {
    int32_t l = 0;
    if (!bad) {
      if (len - pos < 4) {
        bad = true;
      } else {
        l = (int32_t)pq_le32(q + pos);
        if (l < 0 || (uint64_t)l > len - pos - 4) bad = true;
      }
    }
    if (bad) {                                        // this value and every later one of the page
      a.start[base + k] = 0;
      a.length[base + k] = 0;
      a.status[base + k] = 2;
      continue;
    }
    a.start[base + k] = (int64_t)(q - a.data) + (int64_t)pos + 4;
    a.length[base + k] = l;
    a.status[base + k] = 0;
    pos += 4 + (uint64_t)l;
  }
}

// ---- LZ4_RAW pages ----------------------------------------------------------------------------------
struct PqLz4Chunk {          // the layout of Lz4Chunk (kernels.h)
  uint64_t src;
  uint64_t dst;
  uint32_t src_bytes;
  uint32_t dst_capacity;
};

struct PqLz4Args {
  const uint8_t* data;
  uint64_t data_bytes;
  const int64_t* table;      // [npages][kPqCols]
  uint64_t npages;
  const int64_t* dst_off;    // [npages] where the page's uncompressed bytes go in out
  uint8_t* out;
  uint64_t out_bytes;
  PqLz4Chunk* chunks;        // [npages]
  int32_t* expect;           // [npages] the bytes the decoder has to produce for the page
};

// A V1 or dictionary page is compressed whole.  A V2 page has its levels stored raw (they are
// copied) and its values compressed when is_compressed is set (else they are copied too).  A page
// that does not fit the buffers gets an empty chunk and expect -1, which no decoder output equals.
PQ_HD inline void pq_lz4_page(const PqLz4Args& a, uint64_t p) {
  const int64_t* r = a.table + p * kPqCols;
  PqLz4Chunk ch{0, 0, 0, 0};
  int32_t expect = -1;
  const int64_t src = r[kPqPayload], comp = r[kPqCompressed], unc = r[kPqUncompressed], dst = a.dst_off[p];
  const bool v2 = r[kPqType] == 3;
  const int64_t raw = v2 ? r[kPqDefLen] + r[kPqRepLen] : 0;
  if (src >= 0 && comp >= 0 && unc >= 0 && dst >= 0 && raw >= 0 && raw <= comp && raw <= unc &&
      comp <= 0x7FFFFFFFll && unc <= 0x7FFFFFFFll && (uint64_t)src <= a.data_bytes &&
      (uint64_t)comp <= a.data_bytes - (uint64_t)src && (uint64_t)dst <= a.out_bytes &&
      (uint64_t)unc <= a.out_bytes - (uint64_t)dst) {
    const uint8_t* s = a.data + src;
    uint8_t* d = a.out + dst;
    const bool packed = !v2 || r[kPqIsCompressed] != 0;
    if (packed) {
      for (int64_t i = 0; i < raw; ++i) d[i] = s[i];
      ch.src = (uint64_t)(uintptr_t)(s + raw);
      ch.dst = (uint64_t)(uintptr_t)(d + raw);
      ch.src_bytes = (uint32_t)(comp - raw);
      ch.dst_capacity = (uint32_t)(unc - raw);
      expect = (int32_t)(unc - raw);
    } else if (comp == unc) {
      for (int64_t i = 0; i < comp; ++i) d[i] = s[i];
      expect = 0;
    }
  }
  a.chunks[p] = ch;
  a.expect[p] = expect;
}

// ---- the host loops ---------------------------------------------------------------------------------
inline void parquet_walk_host(const PqWalkArgs& a) {
  for (uint64_t c = 0; c < a.nchunks; ++c) pq_walk_chunk(a, c);
}
inline void parquet_hybrid_host(const PqStreamArgs& a) {
  for (uint64_t s = 0; s < a.nstreams; ++s) pq_stream_serial(a, s);
}
inline void parquet_place_host(const PqPlaceArgs& a) {
  for (uint64_t r = 0; r < a.rows; ++r) pq_place_row(a, r);
}
inline void parquet_bytes_host(const PqBytesArgs& a) {
  for (uint64_t p = 0; p < a.npages; ++p) pq_bytes_page(a, p);
}
inline void parquet_lz4_plan_host(const PqLz4Args& a) {
  for (uint64_t p = 0; p < a.npages; ++p) pq_lz4_page(a, p);
}

}  // namespace amdx
