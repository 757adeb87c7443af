// Host-side launch interface of the CDNA4 (gfx950) kernels used by the worker data plane.
//
// Reference hot loops these replace:
//   K1/K2  block read/write chunk copy   W/grpc/BlockReadHandler.java:124-130, BlockWriteHandler.java:124-149
//   K4-K6  LRU/LRFU ordering + free-space loop  W/block/annotator/LRFUAnnotator.java:81-95,
//          W/block/TieredBlockStore.java:740-815
//   K10    CRC32C (new; reference only has whole-file MD5 in ChecksumCommand.java:78-88)
//   K11    LZ4 block codec (new)
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "field_parse_host.h"
#include "json_fields_host.h"
#include "json_text_host.h"
#include "lz4_block_host.h"
#include "parquet_encode_host.h"
#include "parquet_host.h"
#include "parquet_stats_host.h"
#include "text_column_host.h"
#include "text_dict_host.h"

namespace amdx {

// One contiguous copy piece (never crosses a page boundary on the arena side).
struct CopySeg {
  uint64_t src;      // byte address (device or host-pinned mapped)
  uint64_t dst;      // byte address
  uint64_t bytes;
  uint64_t chunk0;   // exclusive prefix of chunk counts (filled by the planner)
};

// Tile (bytes) one workgroup moves per work item of the batched copy.
constexpr uint64_t kCopyChunk = 256 * 1024;

// Batched gather/scatter copy.  `segs` must be device-visible; `total_chunks` = sum of
// ceil(bytes / kCopyChunk).  Grid is capped and grid-strided.
hipError_t launch_batched_copy(const CopySeg* segs, int nseg, uint64_t total_chunks,
                               hipStream_t stream);
// Select the copy kernel variant (cache policy / unroll) and grid cap (0 keeps it); used for A/B
// tuning.  The getter returns both as they stand.
void set_copy_variant(int variant, unsigned grid_cap);
void copy_variant(int* variant, unsigned* grid_cap);

constexpr uint32_t kSeqInlinePages = 4;   // page-table entries a launch carries in its arguments
// Device-cursor sequential multi-stream read (StressWorkerBench shape, K1 without per-read
// descriptors).  S streams each issue `depth` consecutive read(buf) calls per launch over one
// cached file whose pages are listed in `ftab` (file page -> arena page).  Stream s's call
// index of launch L is g = c_init[s] + launch_base + k; with cycle = ceil(file_len/buf) + 1
// calls per pass (the last call of a pass hits EOF and reopens), call c = g % cycle reads
// [c*buf, min(file_len, (c+1)*buf)) into dst + s*stream_stride + k*buf (a ring of `depth`
// slots per stream).  Everything the kernel needs is computed from scalars: O(1) host work
// per launch regardless of S and depth.
struct SeqReadArgs {
  const uint8_t* arena;
  const int64_t* ftab;
  const uint64_t* c_init;
  uint8_t* dst;
  uint64_t stream_stride;
  uint64_t file_len;
  uint64_t buf;
  uint64_t launch_base;
  uint32_t cycle;
  uint32_t streams;
  uint32_t depth;
  uint32_t page_shift;
  uint64_t footprint = 0;   // distinct file bytes one launch touches (host estimate; 0 = file_len)
  // launch_base % cycle, for the fast kernel (which never divides); the general kernel reduces
  // launch_base itself.  Left unset (>= cycle), the launch takes the general kernel.
  uint64_t base_mod = ~0ull;
  // What the host already knows about the start of this launch, for the fast kernel alone, so that
  // a wave's first data load does not wait for two dependent table loads (all zero: nothing known).
  //   cursor_set: every c_init[s] equals c_uniform (< cycle); the kernel does not load c_init.
  //   page_n:     page_tab[i] = ftab[(page_first + i) % file_pages] for i < page_n (<= kSeqInlinePages; entries below 2^32),
  //               file_pages = ceil(file_len / page size): the pages from the launch's earliest
  //               call on, page 0 following the file's last page as call 0 follows the EOF call.
  uint64_t c_uniform = 0;
  uint32_t cursor_set = 0;
  uint32_t page_n = 0;
  uint32_t page_first = 0;
  uint32_t file_pages = 0;
  uint32_t page_tab[kSeqInlinePages] = {};
};
constexpr uint32_t kSeqReadMaxStreams = 8192;
// Two kernels (kernels.hip): the fast one when buf is a multiple of 1 KiB, the page size is at
// least 1 KiB, base_mod is set and the launch's and the file's 1 KiB chunks count below 2^32; the
// general one for every other shape.
hipError_t launch_seq_read(const SeqReadArgs& a, hipStream_t stream);
// The same in two halves, for a caller that repeats one shape: plan_seq_read validates, picks the
// kernel and (fast kernel) asks the current device for its persistent grid, once; launch_seq_plan
// launches what was picked with this step's scalars and asks the runtime nothing.  A plan holds
// while seq_read_epoch() stays what it was when the plan was made (set_seq_read_variant moves it)
// and the shape (buf, depth, streams, page_shift, file_len, cycle, footprint) and device are the
// plan's.
struct SeqReadPlan {
  const void* kernel = nullptr;   // fast instantiation; null: the general kernel, chosen per launch
  uint32_t epoch = 0;             // 0: no plan yet
  uint32_t grid = 0;
  uint32_t cpr_shift = 0, depth_shift = 0;
  int unroll = 0;
};
uint32_t seq_read_epoch();
hipError_t plan_seq_read(const SeqReadArgs& a, SeqReadPlan* plan);
hipError_t launch_seq_plan(const SeqReadPlan& plan, const SeqReadArgs& a, hipStream_t stream);
// A/B switch for the sequential-read kernels (bit0: nontemporal ring stores, bit1: unroll 16 — in
// the general kernel only where depth and buf / 16 are powers of two —, bit2: nontemporal loads;
// -1: the launcher chooses by the launch's footprint).  grid_cap 0 keeps the cap; the fast kernel's
// persistent grid (CUs x resident workgroups) is capped by it too.  The getter returns both as
// they stand, so a caller can put them back.
void set_seq_read_variant(int variant, unsigned grid_cap);
void seq_read_variant(int* variant, unsigned* grid_cap);
// What the most recent ring-read launch in this process launched (fast = 0: the general kernel;
// grid = 0: nothing yet), and what it took from its arguments instead of from memory.
struct SeqReadLaunch {
  int fast;
  int unroll;
  unsigned grid;
  int cursor_inline;      // 1: the kernel took the shared cursor from the arguments
  unsigned pages_inline;  // page-table entries the kernel could take from the arguments
};
SeqReadLaunch seq_read_last_launch();
// Store-only roof of the ring read: `bytes` (a multiple of 16) at dst (16-byte aligned) are filled
// with `word` by 16-B vector stores from a persistent grid (grid 0: CUs x resident workgroups),
// plain or nontemporal.  *grid_used (may be null) = workgroups launched.
hipError_t launch_store_fill(uint8_t* dst, uint64_t bytes, uint32_t word, bool nontemporal, unsigned grid,
                             unsigned* grid_used, hipStream_t stream);

// Ragged gather (ragged_gather.hip): `batch` variable-length records, picked by `idx` from a
// device-resident record index (RaggedRec: virtual byte address and length), are read through a
// virtual page table (vtab: virtual page -> arena page) into one destination buffer.
//   packed: row r starts at out_off[r] = previous end rounded up to `align` (a power of two,
//           1..256); the gap bytes are zero; out_off[batch] is the total.
//   padded: row r starts at r * row_stride and holds min(len, max_len) bytes followed by
//           pad_value up to max_len; out_len[r] is the truncated length.
// Two launches: a one-workgroup plan (lengths, prefix sums of the row offsets and of the work-item
// counts, in rounds of 4096 rows with a carry) and a copy whose waves grid-stride over work items
// of 2^chunk_shift 16-byte destination vectors.  The caller validates everything that decides
// addresses (indices, capacity, record index inside vtab); the launcher re-checks the scalars.
struct RaggedRow {
  uint64_t src;       // virtual byte address of the record
  uint64_t dst_off;   // byte offset of the row in dst
  uint64_t span;      // bytes of dst the row owns: data, then fill (gap or padding)
  uint32_t len;       // data bytes (truncated in the padded layout)
  uint32_t chunk0;    // exclusive prefix of the work-item counts
};
struct RaggedRec {      // one 16-byte load per row in the plan
  uint64_t start;     // virtual byte address
  uint32_t len;
  uint32_t pad;
};
struct RaggedGatherArgs {
  const uint8_t* arena;
  const int64_t* vtab;
  const RaggedRec* recs;     // [n_rec] record index (device)
  const int64_t* idx;        // [batch] record numbers (device memory, or pinned host memory the device can read)
  uint8_t* dst;
  uint64_t* out_off;         // [batch + 1]
  uint32_t* out_len;         // [batch]
  RaggedRow* rows;           // [batch] workspace
  uint32_t* chunk_pre;       // [batch + 1] workspace
  uint64_t n_rec;
  uint64_t row_stride;       // padded
  uint32_t batch;
  uint32_t page_shift;
  uint32_t align;            // packed
  uint32_t max_len;          // padded
  uint32_t padded;           // 0 = packed, 1 = padded
  uint32_t pad_value;
  uint32_t total_chunks;     // host count of the work items (same formula as the plan)
  uint32_t chunk_shift;      // log2(16-byte vectors per work item), from ragged_gather_chunk_shift()
};
constexpr uint32_t kRaggedGatherMaxBatch = 65536;
hipError_t launch_ragged_gather(const RaggedGatherArgs& a, hipStream_t stream);
// Inner loop of the copy: 0 = unaligned 16-byte loads feeding the aligned stores (a vector that
// straddles a page or a row edge takes the funnel), 1 = aligned loads + a byte funnel over two
// registers, the second register taken from the next lane.  chunk_shift (0 = keep) sets the
// work-item size: 2^chunk_shift vectors of 16 bytes per wave.
void set_ragged_gather_variant(int variant, unsigned chunk_shift);
uint32_t ragged_gather_chunk_shift();

// Delimiter index (delim_index.hip): the cut positions of a delimited text range.  The virtual
// byte range [vstart, vstart + bytes) is read through a virtual page table (vtab: virtual page ->
// arena page, as in the ragged gather); for every byte equal to `delim`, in ascending order,
//   out[k] = add + (offset of the byte in the range) + 1.
// Three launches in stream order: count (one wave per tile of 2^tile_shift bytes -> tile_count),
// scan (one workgroup, exclusive prefix -> tile_base, tile_base[ntiles] = total) and emit (each
// wave re-reads its tile and writes its cuts from tile_base[t] on; no atomics, so two runs give
// the same array).  Between scan and emit the caller reads the total and sizes `out`; emit never
// writes at or past out_cap and its launcher refuses total > out_cap.  The caller validates that
// the range lies inside vtab and that no page is negative; the launchers re-check the scalars.
struct DelimIndexArgs {
  const uint8_t* arena;     // 16-byte aligned
  const int64_t* vtab;      // device
  uint32_t* tile_count;     // [ntiles] workspace
  uint64_t* tile_base;      // [ntiles + 1] workspace
  uint64_t* out;            // [out_cap] (emit only)
  uint64_t out_cap;
  uint64_t vstart;
  uint64_t bytes;           // > 0
  uint64_t add;
  uint32_t ntiles;          // delim_index_tiles(vstart, bytes, tile_shift)
  uint32_t page_shift;
  uint32_t tile_shift;      // from delim_index_tile_shift()
  uint32_t delim;           // one byte
  // Quoted form only (launch_delim_*_quoted; the unquoted launches ignore these):
  uint32_t quote;           // one byte, != delim
  uint32_t in_quote;        // 0 or 1: the state at vstart
  uint32_t* tile_count_odd; // [ntiles] workspace
  uint32_t* tile_parity;    // [ntiles + 1] workspace
};
uint64_t delim_index_tiles(uint64_t vstart, uint64_t bytes, uint32_t tile_shift);
hipError_t launch_delim_count(const DelimIndexArgs& a, hipStream_t stream);
hipError_t launch_delim_scan(const DelimIndexArgs& a, hipStream_t stream);
hipError_t launch_delim_emit(const DelimIndexArgs& a, uint64_t total, hipStream_t stream);
// Quoted form: every byte equal to `quote` toggles the state "inside quotes" (in_quote at vstart)
// and a delimiter is a cut only outside, i.e. when the number of quote bytes before it in the
// range plus in_quote is even.  The same three launches, still without atomics or any wait of
// one workgroup on another; the tiles talk through the scan alone:
//   count: a tile does not know its incoming state, so it stores the parity of its quote bytes
//          (tile_parity[t]) and its delimiters at even (tile_count[t]) and at odd
//          (tile_count_odd[t]) quote parity relative to the tile's start.
//   scan:  carries the running parity and the running count across its rounds; per tile it turns
//          tile_parity[t] into the tile's incoming state, picks the even or the odd count by it
//          and prefix-sums the pick into tile_base.  tile_base[ntiles] = total as above,
//          tile_parity[ntiles] = the state after the last byte.
//   emit:  re-reads the tile from tile_parity[t] on and keeps the delimiters outside quotes.
// The launchers re-check quote <= 255, quote != delim and in_quote <= 1.
hipError_t launch_delim_count_quoted(const DelimIndexArgs& a, hipStream_t stream);
hipError_t launch_delim_scan_quoted(const DelimIndexArgs& a, hipStream_t stream);
hipError_t launch_delim_emit_quoted(const DelimIndexArgs& a, uint64_t total, hipStream_t stream);
// Count kernel of the quoted form: 0 (default) = every step works out the state of each byte,
// 1 = a step without a quote byte (one ballot) takes the SWAR popcount of the unquoted kernel
// into the counter chosen by the running parity.
void set_delim_quote_variant(int variant);
int delim_quote_variant();
// variant: 0 = plain loads, 1 (default) = nontemporal loads.  tile_shift (0 = keep; 10..24) sets the bytes
// one wave owns.
void set_delim_index_variant(int variant, unsigned tile_shift);
uint32_t delim_index_tile_shift();
int delim_index_variant();

// Field parse (field_parse.hip): typed columns from the rows of a batch of delimited text.
// FieldParseArgs and the rule are in field_parse_host.h.  One launch, no workspace, no atomics; it
// reads only bytes of rows that lie inside [data, data + data_bytes) and writes row r of every
// column's outputs.  The launcher re-checks the scalars (sep, quote, terminator one byte each and
// distinct, 1..32 columns, field numbers below 65536) and refuses with hipErrorInvalidValue.
hipError_t launch_field_parse(const FieldParseArgs& a, hipStream_t stream);
// 0 = one lane per row (a serial byte walk), 1 (default) = sixteen lanes per row over 256-byte steps.
void set_field_parse_variant(int variant);
int field_parse_variant();

// Text columns (text_column.hip): the bytes of span values with doubled quotes collapsed, packed.
// TextColumnArgs and the rule are in text_column_host.h.  measure writes out_len[r]; emit, given
// the exclusive scan of out_len in offsets, writes value r at out[offsets[r] ...] and never outside
// [offsets[r], offsets[r + 1]) cut to [0, out_bytes).  One launch each, no workspace, no atomics;
// only bytes of live values are read.  The launchers re-check the quote (-1..255), n <= 2^31 and
// the pointers and refuse with hipErrorInvalidValue.
hipError_t launch_text_measure(const TextColumnArgs& a, hipStream_t stream);
hipError_t launch_text_emit(const TextColumnArgs& a, hipStream_t stream);
// 0 = one lane per value (a serial byte walk), 1 (default) = sixteen lanes per value over 256-byte steps.
void set_text_column_variant(int variant);
int text_column_variant();

// JSON Lines columns (json_fields.hip): the values of requested top-level keys located and typed,
// and JSON string values unescaped into packed bytes.  JsonFieldsArgs, JsonTextArgs and the rules
// are in json_fields_host.h and json_text_host.h.  One launch each, no workspace, no atomics; only
// bytes of rows inside [data, data + data_bytes) and of live values are read; emit never writes
// outside [offsets[r], offsets[r + 1]) cut to [0, out_bytes).  The launchers re-check the scalars
// (terminator one byte, 1..32 columns, known types, names of 1..255 bytes inside the name buffer,
// at most 2^31 rows or values) and the pointers and refuse with hipErrorInvalidValue.
hipError_t launch_json_fields(const JsonFieldsArgs& a, hipStream_t stream);
hipError_t launch_json_text_measure(const JsonTextArgs& a, hipStream_t stream);
hipError_t launch_json_text_emit(const JsonTextArgs& a, hipStream_t stream);
// 0 = one lane per row or value (a serial byte walk), 1 (default) = sixteen lanes over 256-byte steps.
void set_json_fields_variant(int variant);
int json_fields_variant();
void set_json_text_variant(int variant);
int json_text_variant();

// Parquet pages (parquet_decode.hip): the passes of parquet_host.h, one launch each, no workspace,
// no atomics.  Only bytes inside the windows that the tables name, cut to [data, data + data_bytes),
// are read, and nothing is written outside the outputs' sizes.  hybrid: mode 0 decodes each stream
// serially, modes 1 to 3 are the cooperative form (count the runs, fill the run table, one thread
// per value).  The launchers re-check counts (at most 2^31), the value width and the pointers and
// refuse with hipErrorInvalidValue.
hipError_t launch_parquet_walk(const PqWalkArgs& a, hipStream_t stream);
hipError_t launch_parquet_lz4_plan(const PqLz4Args& a, hipStream_t stream);
hipError_t launch_parquet_hybrid(const PqStreamArgs& a, int mode, hipStream_t stream);
hipError_t launch_parquet_place(const PqPlaceArgs& a, hipStream_t stream);
hipError_t launch_parquet_bytes(const PqBytesArgs& a, hipStream_t stream);
// Which form callers of the hybrid pass should use: 0 = mode 0, 1 (default) = modes 1 to 3.
void set_parquet_decode_variant(int variant);
int parquet_decode_variant();

// Parquet page encode (parquet_encode.hip): pass `pass` (kPePass*) of parquet_encode_host.h over the
// pages [a.first, a.last), one launch; `largest` is the most rows (pack: value bytes) that a page of
// the range has and sizes the grid.  Only addresses that the page table names are read, and nothing
// is written outside the flat arrays, the measure table and [out, out + out_bytes).
hipError_t launch_parquet_encode(const PeArgs& a, int pass, uint64_t largest, hipStream_t stream);

// Parquet column statistics (parquet_stats.hip): pass `pass` (kPsPass*) of parquet_stats_host.h over
// the segments [a.first, a.last), one launch; `largest` is the most rows that a segment of the range
// has and sizes the grid.  Only addresses that the segment table names are read; writes go to the
// result rows, the alive bytes and, in the mark pass, the mark bytes that the table names.
hipError_t launch_parquet_stats(const PsArgs& a, int pass, uint64_t largest, hipStream_t stream);

// Text dictionaries (text_dict.hip): the passes of text_dict_host.h, one launch each.  probe uses
// global atomics on the table (compare-and-swap, min) and never waits on another lane or
// workgroup; the other passes are one lane per row (rehash: per entry) with plain loads and stores.
// The launchers re-check the scalars (text_dict_scalars_ok, and text_dict_probe_fits for probe) and
// the pointers and refuse with hipErrorInvalidValue.  n == 0 (rehash: D == 0) launches nothing.
hipError_t launch_text_dict_probe(const TextDictArgs& a, hipStream_t stream);
hipError_t launch_text_dict_first(const TextDictArgs& a, hipStream_t stream);
hipError_t launch_text_dict_codes(const TextDictArgs& a, hipStream_t stream);
hipError_t launch_text_dict_commit(const TextDictArgs& a, hipStream_t stream);
hipError_t launch_text_dict_rehash(const TextDictArgs& a, hipStream_t stream);
// probe: 0 (default) = one lane per value (a serial walk), 1 = sixteen lanes per value (hash and
// compares in 16-byte vectors, the group's lane 0 issues the atomics).
void set_text_dict_variant(int variant);
int text_dict_variant();

// CRC32C (Castagnoli, reflected, init/xorout 0xFFFFFFFF) of `n` equal-length pieces
// (piece i = base + i*piece_bytes, last may be shorter: total_bytes).  `out` device array.
hipError_t launch_crc32c_pieces(const uint8_t* base, uint64_t total_bytes, uint64_t piece_bytes,
                                uint32_t* out, uint32_t* scratch, uint64_t scratch_words,
                                hipStream_t stream);
// The same per-page CRC32Cs of a block whose pages are scattered in an arena: page i of the block
// is base + page_idx[i] * page_bytes (page_idx: device array).  One launch pair for the whole
// block; hipErrorNotSupported when the active CRC variant has no paged form (use per-run launches).
hipError_t launch_crc32c_pages(const uint8_t* base, const int64_t* page_idx, uint64_t total_bytes,
                               uint64_t page_bytes, uint32_t* out, uint32_t* scratch, uint64_t scratch_words,
                               hipStream_t stream);
// Scratch words launch_crc32c_pages needs.
uint64_t crc32c_pages_scratch_words(uint64_t total_bytes, uint64_t page_bytes);
// Standard CRC32C of n gathered pieces (device pointers/lengths in device memory, each piece
// <= crc32c_gather_max_piece() bytes), one workgroup per piece.
hipError_t launch_crc32c_gather(const uint64_t* ptrs, const uint32_t* lens, uint64_t n, uint32_t* out,
                                hipStream_t stream);
uint64_t crc32c_gather_max_piece();
// 0: per-lane contiguous strips, 1 (default): interleaved coalesced lanes.
void set_crc_variant(int v);
// Scratch words needed by launch_crc32c_pieces (an upper bound for every variant).
uint64_t crc32c_scratch_words(uint64_t total_bytes, uint64_t piece_bytes);

// LZ4 block decompression of `n` independent chunks.
struct Lz4Chunk {
  uint64_t src;       // compressed bytes (device)
  uint64_t dst;       // output (device)
  uint32_t src_bytes;
  uint32_t dst_capacity;
};
constexpr int kLzThreads = 64;                 // one wave per chunk, in the decoders and the encoders
constexpr uint32_t kLzWindow = 64 * 1024;      // the most bytes of a chunk
hipError_t launch_lz4_decompress(const Lz4Chunk* chunks, int n, int32_t* out_sizes,
                                 hipStream_t stream);
// 0: LDS-window decoder, 1: direct-to-HBM, 2 (default): direct + LDS-staged parse, 3: + LDS ring
// of recent output for near matches.
void set_lz4_decode_variant(int v);
void set_lz4_encode_variant(int v);
// LZ4 block compression (greedy, one wave per chunk, LDS hash table).  out_sizes[i] = -1 if
// the chunk does not fit dst_capacity (caller then stores it raw).
hipError_t launch_lz4_compress(const Lz4Chunk* chunks, int n, int32_t* out_sizes,
                               hipStream_t stream);
// Snappy raw decompression of `n` independent streams (snappy_decode.hip; snappy_host.h has the
// format and the codes): the chunk table of launch_lz4_decompress, out_sizes[i] the bytes produced
// (dst_capacity, which the stream's preamble has to equal) or a negative code.  One wave per stream.
// 0: one element per step; 1: a 64-byte window of the stream per step; -1: the default.
constexpr int kSnDefaultVariant = 1;
constexpr uint32_t kSnStage0 = 2048;           // variant 0: bytes of the stream staged in LDS
constexpr uint32_t kSnStage = 1024;            // variant 1: the stage,
constexpr uint32_t kSnRing = 4096;             //   the LDS ring of recent output,
constexpr uint32_t kSnWindow = 256;            //   the most output bytes of one step,
constexpr uint32_t kSnFlush = 1024;            //   and the bytes after which the ring goes to HBM
hipError_t launch_snappy_decompress(const Lz4Chunk* chunks, int n, int32_t* out_sizes, hipStream_t stream);
void set_snappy_decode_variant(int v);
// One LZ4 block per page body of any size below 2^31 (lz4_block_host.h has the tables and the
// rules): parse (one wave per segment row, sequences and records into scratch), link (one lane per
// page: the places of the segments and the sizes into `result`) and merge (one workgroup per
// segment row, blocks written at out + dst[page]).  Three launches whatever the pages; rows that do
// not fit their buffers are skipped and flagged in `result`.  Null arrays, counts of zero or above
// 2^31 and a scratch buffer shorter than its records are refused with hipErrorInvalidValue.
hipError_t launch_lz4_page_parse(const LbArgs& a, hipStream_t stream);
hipError_t launch_lz4_page_link(const LbArgs& a, hipStream_t stream);
hipError_t launch_lz4_page_merge(const LbArgs& a, hipStream_t stream);

// ---- device-resident annotations + grid-wide select (evict_alloc.hip) ----------------------
// Slot-indexed arrays in HBM.  dir[s] = storage dir of a committed, statically evictable block
// (not temp / pinned), -1 otherwise; fbytes = its page-rounded footprint.
struct EvictState {
  float* crf;
  uint64_t* last;
  uint64_t* fbytes;
  int32_t* dir;
  uint32_t n;            // slots in use (grid extent)
  uint64_t now;          // logical access clock
  float step;            // LRFU step factor
  float log2_inv_att;    // log2(1 / attenuation)
  int policy;            // 0 = LRU, 1 = LRFU
  uint64_t dir_mask;     // candidate dirs (bit d = dir d); 0 = the select's target dir only
  int unit;              // 1: every candidate weighs 1 (select by count, not bytes)
  int invert;            // 1: hottest first (select the largest keys)
};
constexpr uint32_t kSlotSetState = 1, kSlotReset = 2, kSlotTouch = 4;
// One coalesced host->device update per slot: state (dir, footprint) and/or annotations
// (reset: crf = crf, last = t; touch: crf = crf_dev * decay(t - last_dev) + crf, last = t).
struct SlotUpdate {
  uint32_t slot;
  uint32_t flags;
  int32_t dir;
  float crf;
  uint64_t fbytes;
  uint64_t t;
};
// Max selection grid (workgroups per pass).
constexpr unsigned kEvSlabRows = 128;
struct EvictCtl {
  unsigned long long hist[256];
  unsigned long long total;     // evictable footprint in the target dir
  unsigned long long acc;       // bytes of keys strictly below the current prefix
  unsigned long long tie_acc;
  unsigned long long freed;
  uint32_t prefix, mask;
  uint32_t all, done;
  uint32_t count, pad;
};
hipError_t launch_slot_update(const EvictState& st, const SlotUpdate* upd, uint32_t n, hipStream_t stream);
// Smallest-key-first victims of `target_dir` whose footprints add up to >= need (all of them if
// the dir holds less); `excl` (bitmap by slot, may be null) removes locked slots.  Victim slots
// go to out_slots (device-visible, e.g. mapped pinned host), their count/bytes to ctl->count/freed.
hipError_t launch_evict_select_grid(const EvictState& st, uint32_t target_dir, const uint32_t* excl,
                                    uint64_t need, uint32_t* keys, EvictCtl* ctl, uint32_t* out_slots,
                                    hipStream_t stream);
// K7: claim the `want` lowest free pages of a free-page bitmap (1 = free) in place; pages_out
// gets the page numbers, *claimed how many (< want if the bitmap ran out).  `partial` needs
// page_alloc_partials(nwords) words.
hipError_t launch_page_alloc(uint64_t* bits, uint32_t nwords, uint32_t want, uint32_t* partial,
                             int64_t* pages_out, uint32_t* claimed, hipStream_t stream);
uint32_t page_alloc_partials(uint32_t nwords);

// K7 device page magazine (evict_alloc.hip): an HBM dir keeps a device-resident bitmap of free
// pages it handed to the device ("magazine"); kernels claim pages from it with atomics, the host
// refills it by whole bitmap words and drains it back only when its own pool runs dry.
struct ClaimItem {
  uint64_t src;          // device source of the item's bytes (scatter) or 0 (claim only)
  uint64_t len;          // bytes
  uint32_t want;         // pages to claim
  uint32_t page_base;    // first index in pages_out
  uint32_t chunk_base;   // first 64 KiB chunk of this item in the scatter grid
  uint32_t pad;
};
// bits[upd[2i]] |= upd[2i+1] (atomic): pages moved into the magazine
hipError_t launch_mag_fill(uint64_t* bits, uint32_t nwords, const uint64_t* upd, uint32_t n, hipStream_t stream);
// out[w] = atomicExch(bits[w], 0): the magazine handed back (no claim can race it)
hipError_t launch_mag_drain(uint64_t* bits, uint32_t nwords, uint64_t* out, hipStream_t stream);
// One wave per item claims item.want pages (atomicAnd on the words, ballot/popcount ranking)
// into pages_out[page_base ...]; got[i] = pages claimed (< want when the magazine ran dry).
// When total_chunks > 0 a second launch copies each item's bytes into its claimed pages (one
// wave per 64 KiB chunk; items that came up short are skipped -- the host finishes them).
// win_lo/win_len: the words the magazine's bits live in (refills fill a contiguous arc of the
// bitmap); items search there first and fall back to the whole bitmap when it runs dry.
hipError_t launch_mag_claim_scatter(uint64_t* bits, uint32_t nwords, const ClaimItem* items, uint32_t nitems,
                                    int64_t* pages_out, uint32_t pages_cap, uint32_t* got, uint32_t total_chunks,
                                    uint8_t* arena, uint64_t page_size, hipStream_t stream, uint32_t win_lo = 0,
                                    uint32_t win_len = 0);

// K9: client page cache lookup.  Open-addressing (linear probing) table of page keys in HBM;
// `key` = (interned file id << 24) | page index, so keys are exact (no hash collisions to
// verify).  Empty slots hold kPageKeyEmpty, erased ones kPageKeyTomb (probing continues).
struct PageTableEntry {
  uint64_t key;
  int32_t slot;    // arena slot of the page
  uint32_t len;    // valid bytes in the page
};
constexpr uint64_t kPageKeyEmpty = ~0ull;
constexpr uint64_t kPageKeyTomb = ~0ull - 1;
__host__ __device__ inline uint64_t page_key_hash(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
// Fused lookup + gather of `n` pages whose keys live in device memory: request i copies the
// valid bytes of page keys[i] from arena slot to dst + i*dst_stride, writes slot_out[i] (-1 on a
// miss) and len_out[i], and stamps[slot] = epoch on a hit (device-side LRU recency).  One wave
// probes 64 table entries per step with a ballot; `chunk_bytes` splits big pages over gridDim.y.
struct PageGatherArgs {
  const PageTableEntry* table;
  uint64_t mask;           // table size - 1 (power of two)
  const uint64_t* keys;
  uint32_t n;
  const uint8_t* arena;
  uint64_t page_size;
  uint8_t* dst;
  uint64_t dst_stride;
  int32_t* slot_out;
  uint32_t* len_out;
  uint32_t* stamps;
  uint32_t epoch;
};
hipError_t launch_page_lookup_gather(const PageGatherArgs& a, hipStream_t stream);
// Largest page size served by the wave-per-request kernel (bigger pages: workgroup per chunk).
void set_page_gather_small_max(uint64_t bytes);
void set_page_gather_wave_variant(int variant);
void set_page_gather_chunk_variant(int v);
// The three settings above as they stand: small_max, wave variant, chunk variant.
void page_gather_config(uint64_t* small_max, int* wave_variant, int* chunk_variant);
// Apply table updates (idx, entry) pairs uploaded by the host mirror.
hipError_t launch_page_table_update(PageTableEntry* table, const uint64_t* idx,
                                    const PageTableEntry* entries, uint32_t n, hipStream_t stream);

// K9 put path on the GPU (page_cache_put.hip): probe/claim -> assign (free stack or CLOCK
// eviction) -> fill, for a batch of device-resident keys; the device table is authoritative.
struct PutCounters {
  int32_t free_top;        // entries left on the device free stack (may go negative)
  uint32_t hand;           // CLOCK hand
  uint32_t nfresh;         // keys this batch claimed new table entries for
  uint32_t nevicted;       // victims (their keys in `evicted`)
  uint32_t ntomb;          // tombstones this batch created
  uint32_t nfail;          // requests that got no slot
  uint32_t min_age;        // victims: slots not touched for >= this many epochs (threshold kernel)
  uint32_t pad;
};
constexpr uint32_t kPutAgeBuckets = 4096;   // recency histogram: age = epoch - stamp, clamped
struct PagePutArgs {
  PageTableEntry* table;
  uint64_t mask;
  const uint64_t* keys;
  uint32_t n;
  uint32_t* tidx;                // [n] table index of each request
  unsigned long long* tag;       // [table size] (batch << 32) | (request + 1) of the winner
  unsigned long long batch;
  uint32_t* stamps;              // [slots] recency (shared with the gather kernel)
  uint32_t* hist;                // [kPutAgeBuckets] slots per age (eviction threshold)
  uint32_t epoch;
  uint32_t nslots;
  uint64_t* slot_key;            // [slots] key held by each slot (kPageKeyEmpty = free)
  uint32_t* slot_tidx;           // [slots] table index of that key
  uint32_t* free_stack;          // [slots]
  PutCounters* ctr;
  uint64_t* evicted;             // [n]
  int32_t* slot_of;              // [n] slot to fill (-1: duplicate or failed)
  int evict;
  uint32_t len;
  const uint8_t* src;
  uint64_t src_stride;
  uint8_t* arena;
  uint64_t page_size;
};
hipError_t launch_page_put_probe(const PagePutArgs& a, hipStream_t stream);
hipError_t launch_page_put_assign(const PagePutArgs& a, hipStream_t stream);
hipError_t launch_page_put_fill(const PagePutArgs& a, hipStream_t stream);
hipError_t launch_page_put_revert(const PagePutArgs& a, hipStream_t stream);
// Age histogram of the evictable slots + the threshold age that frees enough of them.
hipError_t launch_page_put_threshold(const PagePutArgs& a, hipStream_t stream);
// Drop tombstones on the device: live entries of a.table are re-inserted into `fresh` (cleared
// first) and slot_tidx is repointed; the caller swaps the two tables afterwards.
hipError_t launch_page_table_rebuild(const PagePutArgs& a, PageTableEntry* fresh, hipStream_t stream);

// Fill `bytes` at dst with 64-bit words w[i] = splitmix64(seed ^ ((i + word_offset) * K)):
// synthetic bench/test data that is a pure function of the byte offset inside a block.
hipError_t launch_fill_pattern(uint8_t* dst, uint64_t bytes, uint64_t seed, uint64_t word_offset,
                               hipStream_t stream);

}  // namespace amdx
