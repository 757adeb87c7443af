"""Typed columns from Parquet files: what :mod:`.fields` does for CSV and :mod:`.json_fields` for
JSON Lines, for the table format that ``transformTable`` writes.  :func:`parquet_metadata` reads
the footer (a small Thrift compact-protocol reader, written from the format specification: no
``pyarrow`` here); :func:`read_parquet_columns` brings the bytes of the selected column chunks to
the device with the ragged gather and decodes their pages there (kernels for device memory, C++
loops for a file on a DRAM tier or read through the general path); :func:`parquet_row_groups`
yields one :class:`FieldColumns` per row group for a training loop.

The passes (``csrc/parquet_host.h`` has the rules in full): the page walk parses the
``PageHeader`` between the pages of every chunk into a page table; LZ4_RAW pages are decompressed
by the LZ4 block kernel into a second buffer; definition levels, dictionary indices and RLE
booleans are RLE / bit-packed hybrid streams decoded to int32; a row then takes value number
``rank`` of its page (``rank``: the exclusive prefix sum of validity within the page) from PLAIN
bytes or from the chunk's dictionary; a PLAIN BYTE_ARRAY page is walked into spans that
``extract_text`` packs.

Column types: ``"int64"``, ``"int32"``, ``"float64"``, ``"float32"``, ``"bool"`` give ``values``
and ``status`` (0 a value, 1 null, 2 a corrupt page or value; a null or corrupt row has value 0);
BYTE_ARRAY is ``"text"`` (a packed text column; ``""`` is a value of length 0 with status 0, a null
has status 1) or ``"category"`` (int32 codes of a :class:`TextDictionary`, -1 for nulls, in order of
first occurrence).  The requested type must be the one the physical type implies, except that INT32
widens to ``int64`` and FLOAT to ``float64``.  Logical types are not interpreted: a timestamp
column comes back as its ``int64``, a decimal as its integer, a date as its ``int32``.

Not supported (``NotImplementedError`` that names the column, before any launch unless noted):
columns with repetition or a definition level above 1 (lists, structs with optional parents),
INT96 and FIXED_LEN_BYTE_ARRAY, every codec but UNCOMPRESSED and LZ4_RAW (so SNAPPY, GZIP, ZSTD,
BROTLI and the Hadoop-framed LZ4), BIT_PACKED levels, encrypted files, and the DELTA_* and
BYTE_STREAM_SPLIT value encodings, which only a page header reveals and which are therefore
raised after the page walk.  Columns that are not selected may be of any kind.
"""
from __future__ import annotations

import struct
from collections import namedtuple

import numpy as np

from .dataset import DeviceBatchLoader, IndexedRecordDataset, RaggedBatch
from .fields import (BOOL, CATEGORY, FLOAT32, FLOAT64, INT32, INT64, TEXT, Column, FieldColumns,
                     _category_dictionaries, _queue, extract_text)

PHYSICAL = ["BOOLEAN", "INT32", "INT64", "INT96", "FLOAT", "DOUBLE", "BYTE_ARRAY", "FIXED_LEN_BYTE_ARRAY"]
CODECS = ["UNCOMPRESSED", "SNAPPY", "GZIP", "LZO", "BROTLI", "LZ4", "ZSTD", "LZ4_RAW"]
REPETITION = ["REQUIRED", "OPTIONAL", "REPEATED"]
ENCODINGS = {0: "PLAIN", 2: "PLAIN_DICTIONARY", 3: "RLE", 4: "BIT_PACKED", 5: "DELTA_BINARY_PACKED",
             6: "DELTA_LENGTH_BYTE_ARRAY", 7: "DELTA_BYTE_ARRAY", 8: "RLE_DICTIONARY", 9: "BYTE_STREAM_SPLIT"}

ParquetLeaf = namedtuple("ParquetLeaf", "name physical_type repetition max_definition_level max_repetition_level "
                                        "type_length")
ParquetChunk = namedtuple("ParquetChunk", "name physical_type codec num_values dictionary_page_offset "
                                          "data_page_offset total_compressed_size")
ParquetRowGroup = namedtuple("ParquetRowGroup", "num_rows columns")
ParquetMetadata = namedtuple("ParquetMetadata", "num_rows schema row_groups created_by")

_TYPE_NAMES = {"int64": INT64, "int32": INT32, "float64": FLOAT64, "float32": FLOAT32, "bool": BOOL, "text": TEXT,
               "category": CATEGORY, "int": INT64, "float": FLOAT64, "bytes": TEXT, "dict": CATEGORY}
_IMPLIED = {"BOOLEAN": BOOL, "INT32": INT32, "INT64": INT64, "FLOAT": FLOAT32, "DOUBLE": FLOAT64, "BYTE_ARRAY": TEXT}
_ALLOWED = {"BOOLEAN": (BOOL,), "INT32": (INT32, INT64), "INT64": (INT64,), "FLOAT": (FLOAT32, FLOAT64),
            "DOUBLE": (FLOAT64,), "BYTE_ARRAY": (TEXT, CATEGORY)}
_WIDTH = {"BOOLEAN": 1, "INT32": 4, "INT64": 8, "FLOAT": 4, "DOUBLE": 8}
# page-table, stream and data-page columns of csrc/parquet_host.h
_PQ_COLS, _PS_COLS, _PP_COLS = 12, 8, 10
(_T_TYPE, _T_PAYLOAD, _T_COMP, _T_UNCOMP, _T_NVAL, _T_ENC, _T_DEFLEN, _T_REPLEN, _T_NNULL, _T_ISCOMP, _T_CHUNK,
 _T_DEFENC) = range(12)


# ---- Thrift compact protocol ------------------------------------------------------------------------
class _Thrift:
    """A reader of the Thrift compact protocol over ``bytes``.  A struct becomes ``{field id: value}``
    with every field kept by its type alone, so unknown fields cost nothing and are ignored by the
    callers; a list becomes a ``list``, a binary ``bytes``."""

    def __init__(self, buf: bytes, pos: int = 0):
        self.b, self.p = buf, pos

    def byte(self) -> int:
        if self.p >= len(self.b):
            raise ValueError("the Thrift data ends early")
        self.p += 1
        return self.b[self.p - 1]

    def varint(self) -> int:
        v = s = 0
        while True:
            c = self.byte()
            v |= (c & 0x7F) << s
            if not c & 0x80:
                return v
            s += 7
            if s > 70:
                raise ValueError("a Thrift varint is too long")

    def zigzag(self) -> int:
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def take(self, n: int) -> bytes:
        if n < 0 or self.p + n > len(self.b):
            raise ValueError("the Thrift data ends early")
        self.p += n
        return self.b[self.p - n:self.p]

    def value(self, t: int, depth: int = 0):
        if depth > 32:
            raise ValueError("the Thrift data nests too deeply")
        if t in (1, 2):
            return t == 1
        if t == 3:
            return self.byte()
        if t in (4, 5, 6):
            return self.zigzag()
        if t == 7:
            return struct.unpack("<d", self.take(8))[0]
        if t == 8:
            return self.take(self.varint())
        if t in (9, 10):
            h = self.byte()
            n, et = h >> 4, h & 15
            if n == 15:
                n = self.varint()
            if n > len(self.b) - self.p:
                raise ValueError("a Thrift list is longer than the data")
            if et in (1, 2):
                return [self.byte() == 1 for _ in range(n)]
            return [self.value(et, depth + 1) for _ in range(n)]
        if t == 11:
            n = self.varint()
            if n == 0:
                return {}
            if n > len(self.b) - self.p:
                raise ValueError("a Thrift map is longer than the data")
            kv = self.byte()
            kt, vt = (3 if x in (1, 2) else x for x in (kv >> 4, kv & 15))
            return [(self.value(kt, depth + 1), self.value(vt, depth + 1)) for _ in range(n)]
        if t == 12:
            return self.struct(depth + 1)
        raise ValueError(f"unknown Thrift type {t}")

    def struct(self, depth: int = 0) -> dict:
        out, fid = {}, 0
        while True:
            h = self.byte()
            if h == 0:
                return out
            fid = fid + (h >> 4) if h >> 4 else self.zigzag()
            out[fid] = self.value(h & 15, depth)


def _pread(f, off: int, n: int) -> bytes:
    buf = np.empty(n, dtype=np.uint8)
    got = 0
    while got < n:
        k = f.pread(off + got, buf[got:])
        if k <= 0:
            raise ValueError("the file ends early")
        got += k
    return buf.tobytes()


def _name(codes, i):
    return codes[i] if isinstance(i, int) and 0 <= i < len(codes) else f"UNKNOWN({i})"


def parquet_metadata(fs, path: str) -> ParquetMetadata:
    """The footer of a Parquet file, read with positioned reads through the client stream (the last
    8 bytes, then the ``FileMetaData``): ``num_rows``, ``schema`` (one :class:`ParquetLeaf` per leaf
    column: dotted ``name``, ``physical_type``, ``repetition``, ``max_definition_level``,
    ``max_repetition_level``, ``type_length``) and ``row_groups`` (``num_rows`` and, per leaf in
    schema order, a :class:`ParquetChunk`: ``codec``, ``num_values``, ``dictionary_page_offset``
    (``None`` without one), ``data_page_offset``, ``total_compressed_size``).  Type, codec and
    repetition are the names of the format specification.  Unknown fields are skipped."""
    length = int(fs.get_status(path).length)
    with fs.open_file(path) as f:
        if length < 12:
            raise ValueError(f"{path}: not a Parquet file ({length} bytes)")
        tail = _pread(f, length - 8, 8)
        if tail[4:] == b"PARE":
            raise NotImplementedError(f"{path}: encrypted Parquet files (an encrypted footer) are not supported")
        if tail[4:] != b"PAR1":
            raise ValueError(f"{path}: not a Parquet file (no PAR1 at the end)")
        n = int.from_bytes(tail[:4], "little")
        if n <= 0 or n > length - 12:
            raise ValueError(f"{path}: the footer length {n} does not fit the file")
        raw = _pread(f, length - 8 - n, n)
    try:
        md = _Thrift(raw).struct()
    except (ValueError, RecursionError) as e:
        raise ValueError(f"{path}: the footer is malformed: {e}") from None
    if 8 in md:
        raise NotImplementedError(f"{path}: encrypted Parquet files (encrypted columns) are not supported")
    elems = md.get(2) or []
    leaves = []

    def walk(i, prefix, d, r):                          # depth first; returns the next element
        e = elems[i]
        rep = e.get(3, 0)
        nm = e.get(4, b"").decode("utf-8", "replace")
        d, r = d + (rep != 0), r + (rep == 2)
        kids = e.get(5) or 0
        full = prefix + [nm]
        i += 1
        if not kids:
            leaves.append(ParquetLeaf(".".join(full), _name(PHYSICAL, e.get(1)), _name(REPETITION, rep), d, r,
                                      e.get(2)))
            return i
        for _ in range(kids):
            i = walk(i, full, d, r)
        return i

    if elems:
        try:
            i = 1
            for _ in range(elems[0].get(5) or 0):
                i = walk(i, [], 0, 0)
        except IndexError:
            raise ValueError(f"{path}: the schema names more children than it has elements") from None
    groups = []
    for rg in md.get(4) or []:
        cols = []
        for cc in rg.get(1) or []:
            m = cc.get(3)
            if m is None:
                raise NotImplementedError(f"{path}: a column chunk without metadata (encrypted, or in another file) "
                                          f"is not supported")
            cols.append(ParquetChunk(".".join(x.decode("utf-8", "replace") for x in m.get(3) or []),
                                     _name(PHYSICAL, m.get(1)), _name(CODECS, m.get(4)), m.get(5, 0), m.get(11),
                                     m.get(9, 0), m.get(7, 0)))
        groups.append(ParquetRowGroup(rg.get(3, 0), cols))
    return ParquetMetadata(md.get(3, 0), leaves, groups, (md.get(6) or b"").decode("utf-8", "replace"))


# ---- what to read -----------------------------------------------------------------------------------
def _type_code(dtype) -> int:
    name = dtype.__name__ if isinstance(dtype, type) else str(dtype).replace("torch.", "")
    try:
        return _TYPE_NAMES[name]
    except KeyError:
        raise ValueError(f"unknown column type {dtype!r}: one of int64, int32, float64, float32, bool, text, "
                         f"category") from None


def _plan(path, md: ParquetMetadata, columns, row_groups):
    """[(name or None, leaf position, leaf, type code)] and the row group numbers, with everything
    that can be refused from the footer refused."""
    by_name = {lf.name: j for j, lf in enumerate(md.schema)}
    if columns is None:
        items = [(lf.name, (lf.name, None)) for lf in md.schema
                 if lf.physical_type in _IMPLIED and lf.max_repetition_level == 0 and lf.max_definition_level <= 1]
    elif isinstance(columns, dict):
        items = list(columns.items())
    else:
        items = [(spec[0], spec) if isinstance(spec, tuple) else (spec, (spec, None)) for spec in columns]
    specs = []
    for name, (leaf, dtype) in items:
        if not isinstance(leaf, str):
            raise TypeError(f"a column is named by its leaf name, got {leaf!r}")
        if leaf not in by_name:
            raise KeyError(f"{path}: no column {leaf!r}; the leaves are {sorted(by_name)}")
        j = by_name[leaf]
        lf = md.schema[j]
        if lf.max_repetition_level > 0:
            raise NotImplementedError(f"{path}: column {leaf!r} is repeated (a list or map); columns with "
                                      f"repetition levels are not supported")
        if lf.max_definition_level > 1:
            raise NotImplementedError(f"{path}: column {leaf!r} has definition levels up to "
                                      f"{lf.max_definition_level} (a nested optional); only flat columns are supported")
        if lf.physical_type not in _IMPLIED:
            raise NotImplementedError(f"{path}: column {leaf!r} has the physical type {lf.physical_type}, which is "
                                      f"not supported")
        t = _IMPLIED[lf.physical_type] if dtype is None else _type_code(dtype)
        if t not in _ALLOWED[lf.physical_type]:
            raise ValueError(f"{path}: column {leaf!r} is {lf.physical_type} and cannot be read as {dtype!r}")
        specs.append((name, j, lf, t))
    if not specs:
        raise ValueError("at least one column is required")
    if row_groups is None:
        groups = list(range(len(md.row_groups)))
    else:
        groups = [int(g) for g in row_groups]
        for g in groups:
            if not 0 <= g < len(md.row_groups):
                raise IndexError(f"{path}: no row group {g} (there are {len(md.row_groups)})")
    for g in groups:
        rg = md.row_groups[g]
        for _name_, j, lf, _t in specs:
            if j >= len(rg.columns):
                raise ValueError(f"{path}: row group {g} has no chunk for column {lf.name!r}")
            cc = rg.columns[j]
            if cc.codec not in ("UNCOMPRESSED", "LZ4_RAW"):
                raise NotImplementedError(f"{path}: column {lf.name!r} is compressed with {cc.codec}; only "
                                          f"UNCOMPRESSED and LZ4_RAW are supported")
    return specs, groups


def _chunk_range(cc: ParquetChunk):
    start = cc.data_page_offset
    if cc.dictionary_page_offset is not None and 0 < cc.dictionary_page_offset < start:
        start = cc.dictionary_page_offset
    return int(start), int(start) + int(cc.total_compressed_size)


# ---- the passes ---------------------------------------------------------------------------------------
def _dev_i64(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else 0


def parquet_page_table(data, chunk_off, chunk_len):
    """The page walk over the chunks ``data[chunk_off[c]:chunk_off[c] + chunk_len[c]]`` of a flat
    uint8 tensor, where it lies: ``(table, counts, errors)`` as numpy arrays on the host; ``table``
    has one int64 row of 12 columns per page in chunk order (the columns of
    ``csrc/parquet_host.h``), ``counts`` the pages per chunk and ``errors`` a code per chunk
    (0: none).  Two launches, count and fill, and two small readbacks."""
    import torch
    from ..ops.native import lib, native_errors
    dev = data.device
    device, stream = _queue(dev)
    n = len(chunk_off)
    off, ln = _dev_i64(chunk_off, dev), _dev_i64(chunk_len, dev)
    both = torch.zeros(2, max(n, 1), dtype=torch.int32, device=dev)
    with native_errors():
        lib().parquet_walk_raw(_ptr(data), data.numel(), _ptr(off), _ptr(ln), n, device, both[0].data_ptr(),
                               both[1].data_ptr(), stream=stream)
        host = both.cpu().numpy()
        counts, errors = host[0, :n].copy(), host[1, :n].copy()
        base = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
        total = int(base[-1])
        table = torch.zeros(max(total, 1), _PQ_COLS, dtype=torch.int64, device=dev)
        if total:
            pb = _dev_i64(base, dev)
            lib().parquet_walk_raw(_ptr(data), data.numel(), _ptr(off), _ptr(ln), n, device, 0, 0, pb.data_ptr(),
                                   table.data_ptr(), total, stream)
    return table[:total].cpu().numpy(), counts, errors


def _hybrid(data, streams, out_n):
    """The hybrid streams (a device int64 tensor of stream rows) decoded into int32 ``out_n`` slots:
    ``(out, errors)``.  On the host and in kernel variant 0 one call; in variant 1 the run table is
    counted, scanned, read back for its size and filled, and a third launch places the values."""
    import torch
    from ..ops.native import lib, native_errors
    C = lib()
    dev = data.device
    device, stream = _queue(dev)
    ns = int(streams.shape[0])
    out = torch.zeros(out_n, dtype=torch.int32, device=dev)
    errors = torch.zeros(ns, dtype=torch.int32, device=dev)
    if ns == 0 or out_n == 0:
        return out, errors
    with native_errors():
        if device < 0 or C.parquet_decode_variant() == 0:
            C.parquet_hybrid_raw(_ptr(data), data.numel(), streams.data_ptr(), ns, out.data_ptr(), out_n,
                                 errors.data_ptr(), device, 0, stream=stream)
            return out, errors
        counts = torch.zeros(ns, dtype=torch.int32, device=dev)
        C.parquet_hybrid_raw(_ptr(data), data.numel(), streams.data_ptr(), ns, out.data_ptr(), out_n,
                             errors.data_ptr(), device, 1, counts.data_ptr(), stream=stream)
        base = torch.zeros(ns + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, dtype=torch.int64, out=base[1:])
        total = int(base[-1].item())
        runs = torch.empty(max(total, 1), 4, dtype=torch.int64, device=dev)
        C.parquet_hybrid_raw(_ptr(data), data.numel(), streams.data_ptr(), ns, out.data_ptr(), out_n, 0, device, 2,
                             0, base.data_ptr(), runs.data_ptr(), total, stream)
        C.parquet_hybrid_raw(_ptr(data), data.numel(), streams.data_ptr(), ns, out.data_ptr(), out_n, 0, device, 3,
                             0, base.data_ptr(), runs.data_ptr(), total, stream)
    return out, errors


def _place(data, pages, excl, idx, dict_, stream_err, width, is_bool, rows):
    import torch
    from ..ops.native import lib, native_errors
    dev = data.device
    device, stream = _queue(dev)
    values = torch.zeros(rows * width, dtype=torch.uint8, device=dev)
    status = torch.full((rows,), 2, dtype=torch.uint8, device=dev)
    with native_errors():
        lib().parquet_place_raw(_ptr(data), data.numel(), _ptr(pages), int(pages.shape[0]), _ptr(excl), _ptr(idx),
                                0 if idx is None else idx.numel(), _ptr(dict_),
                                0 if dict_ is None else dict_.numel() // width, _ptr(stream_err),
                                0 if stream_err is None else stream_err.numel(), width, is_bool, values.data_ptr(),
                                status.data_ptr(), rows, device, stream)
    return values, status


def _byte_spans(data, pages, excl, rows, stream_err, nvalues):
    import torch
    from ..ops.native import lib, native_errors
    dev = data.device
    device, stream = _queue(dev)
    start = torch.zeros(nvalues, dtype=torch.int64, device=dev)
    length = torch.zeros(nvalues, dtype=torch.int32, device=dev)
    status = torch.full((nvalues,), 2, dtype=torch.uint8, device=dev)
    with native_errors():
        lib().parquet_bytes_raw(_ptr(data), data.numel(), _ptr(pages), int(pages.shape[0]), _ptr(excl), rows,
                                _ptr(stream_err), 0 if stream_err is None else stream_err.numel(), start.data_ptr(),
                                length.data_ptr(), status.data_ptr(), nvalues, device, stream)
    return start, length, status


def _decompress(data, table, sel):
    """The pages ``sel`` (rows of the host page table) of LZ4_RAW chunks decompressed into a second
    buffer: ``(buffer, rows)`` where ``rows`` are those pages' table rows rewritten to point into the
    buffer as uncompressed pages; a page whose LZ4 block is malformed gets type -1."""
    import torch
    from ..ops.native import lib, native_errors
    dev = data.device
    device, stream = _queue(dev)
    rows = table[sel].copy()
    n = len(rows)
    dst = np.concatenate([[0], np.cumsum(rows[:, _T_UNCOMP])]).astype(np.int64)
    out = torch.zeros(int(dst[-1]), dtype=torch.uint8, device=dev)
    if n == 0:
        return out, rows
    d_table, d_dst = _dev_i64(rows, dev), _dev_i64(dst[:-1], dev)
    chunks = torch.zeros(n * 3, dtype=torch.int64, device=dev)
    got = torch.zeros(2, n, dtype=torch.int32, device=dev)      # expected, produced
    with native_errors():
        lib().parquet_lz4_raw(_ptr(data), data.numel(), d_table.data_ptr(), n, d_dst.data_ptr(), _ptr(out), out.numel(),
                              chunks.data_ptr(), got[0].data_ptr(), got[1].data_ptr(), device, stream)
    bad = (got[0] != got[1]).cpu().numpy()
    rows[:, _T_PAYLOAD] = dst[:-1]
    rows[:, _T_COMP] = rows[:, _T_UNCOMP]
    rows[:, _T_ISCOMP] = 0
    rows[bad, _T_TYPE] = -1
    return out, rows


def _check_pages(path, lf, pages):
    for r in pages:
        enc = int(r[_T_ENC])
        if r[_T_TYPE] == 2:
            ok = enc in (0, 2)
        elif lf.physical_type == "BOOLEAN":
            ok = enc in (0, 3)
        else:
            ok = enc in (0, 2, 8)
        if r[_T_TYPE] >= 0 and not ok:
            raise NotImplementedError(f"{path}: column {lf.name!r} has a page in the "
                                      f"{ENCODINGS.get(enc, f'encoding {enc}')} encoding, which is not supported")
        if r[_T_TYPE] == 0 and lf.max_definition_level and int(r[_T_DEFENC]) != 3:
            raise NotImplementedError(f"{path}: column {lf.name!r} has BIT_PACKED levels, which are not supported")


def _chunk_tables(pages, lf, nrows):
    """One column chunk's pages (host table rows) as the tables of csrc/parquet_host.h:
    ``(data pages, definition-level streams, value streams, dictionary pages)``."""
    opt = lf.max_definition_level == 1
    dict_pages = [r for r in pages if r[_T_TYPE] == 2]
    data_pages = [r for r in pages if r[_T_TYPE] in (0, 3, -1)]
    # the data pages, cut to the rows the row group has
    pp = np.zeros((len(data_pages), _PP_COLS), dtype=np.int64)
    ds = np.zeros((len(data_pages), _PS_COLS), dtype=np.int64)      # definition-level streams
    vs = np.zeros((len(data_pages), _PS_COLS), dtype=np.int64)      # value streams (dictionary indices, RLE booleans)
    rb, nv_pages = 0, len(data_pages)
    for k, r in enumerate(data_pages):
        nv = int(min(r[_T_NVAL], nrows - rb))
        v2 = r[_T_TYPE] == 3
        enc = int(r[_T_ENC])
        lev = int(r[_T_DEFLEN] + r[_T_REPLEN]) if v2 else 0
        voff, vlen, skip = int(r[_T_PAYLOAD]) + lev, int(r[_T_COMP]) - lev, int(opt and not v2)
        src = 3 if r[_T_TYPE] < 0 or (v2 and bool(r[_T_DEFLEN]) != opt and nv) else 0 if enc == 0 else 1 if enc in (2, 8) else 2
        if src == 1 and not dict_pages:
            src = 3
        pp[k] = (rb, nv, src, voff, vlen, skip, rb, k if opt else -1, nv_pages + k if src in (1, 2) else -1, 0)
        if not opt or src == 3:
            ds[k] = (0, 0, 0, 0, 1, 0, rb, 0)           # no levels, or a corrupt page: nothing is read
        elif v2:
            ds[k] = (int(r[_T_PAYLOAD] + r[_T_REPLEN]), int(r[_T_DEFLEN]), 0, 0, 1, nv, rb, 0)
        else:
            ds[k] = (int(r[_T_PAYLOAD]), int(r[_T_COMP]), 1, 0, 1, nv, rb, 0)
        # bool RLE: a 4-byte length, then width 1; indices: a width byte.  No values: nothing is read.
        vs[k] = (voff, vlen, 1 if src == 2 else 2, skip, 1, nv if src in (1, 2) else 0, rb, 0)
        rb += nv
    return pp, ds, vs, dict_pages


def _levels_and_indices(buf, tabs, opts, nrows):
    """The hybrid streams of all the chunks of a row group that lie in ``buf``, in two calls: every
    definition-level stream, then (their counts now known) every value stream.  Chunk k's rows are
    [k * nrows, (k + 1) * nrows) of the arrays.  Returns per chunk ``(excl, idx, stream_err)``:
    the exclusive scan of validity (``None`` for a column without levels), the decoded indices
    (``None`` without dictionary-coded or RLE pages) and the error codes of its pages' streams."""
    import torch
    dev = buf.device
    n = len(tabs)
    counts = [len(pp) for pp, _ds, _vs, _d in tabs]
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    col = np.repeat(np.arange(n, dtype=np.int64), counts)
    pp_all = np.concatenate([t[0] for t in tabs]) if n else np.zeros((0, _PP_COLS), np.int64)
    ds_all, vs_all = np.concatenate([t[1] for t in tabs]), np.concatenate([t[2] for t in tabs])
    ds_all[:, 6] += col * nrows
    vs_all[:, 6] += col * nrows
    total = int(first[-1])
    excl2 = None
    if any(opts) and total:
        levels, def_err = _hybrid(buf, _dev_i64(ds_all, dev), n * nrows)
        excl2 = torch.zeros(n, nrows + 1, dtype=torch.int64, device=dev)
        torch.cumsum((levels == 1).view(n, nrows), 1, dtype=torch.int64, out=excl2[:, 1:])
    else:
        def_err = torch.zeros(total, dtype=torch.int32, device=dev)
    idx_all = None
    if total and bool((vs_all[:, 5] > 0).any()):
        d_vs = _dev_i64(vs_all, dev)
        if excl2 is not None:                           # a page holds as many values as it has valid rows
            lo = _dev_i64(col * (nrows + 1) + pp_all[:, 0], dev)
            hi = _dev_i64(col * (nrows + 1) + pp_all[:, 0] + pp_all[:, 1], dev)
            of_opt = torch.from_numpy(np.array(opts, dtype=bool)[col] & (vs_all[:, 5] > 0)).to(dev)
            flat = excl2.view(-1)
            d_vs[:, 5] = torch.where(of_opt, flat[hi] - flat[lo], d_vs[:, 5])
        idx_all, val_err = _hybrid(buf, d_vs, n * nrows)
    else:
        val_err = torch.zeros(total, dtype=torch.int32, device=dev)
    out = []
    for k, (pp, _ds, vs, _d) in enumerate(tabs):
        a, b = int(first[k]), int(first[k + 1])
        idx = idx_all[k * nrows:(k + 1) * nrows] if idx_all is not None and bool((vs[:, 5] > 0).any()) else None
        out.append((excl2[k] if opts[k] and excl2 is not None else None, idx, torch.cat([def_err[a:b], val_err[a:b]])))
    return out


def _decode_chunk(buf, tab, streams, lf, t, nrows, dictionary):
    """One column chunk (its tables and the decoded streams of its pages) as a Column's tensors."""
    import torch
    dev = buf.device
    pp, _ds, _vs, dict_pages = tab
    excl, idx, stream_err = streams
    opt = excl is not None
    byte_array = lf.physical_type == "BYTE_ARRAY"
    nv_pages = len(pp)
    d_pages = _dev_i64(pp, dev)
    arange = torch.arange(nrows + 1, dtype=torch.int64, device=dev)
    has_idx = idx is not None
    dict_n = int(dict_pages[0][_T_NVAL]) if dict_pages else 0
    dp = None
    if dict_pages:
        r = dict_pages[0]
        dp = _dev_i64(np.array([[0, dict_n, 0, r[_T_PAYLOAD], r[_T_COMP], 0, 0, -1, -1, 0]], dtype=np.int64), dev)

    if not byte_array:
        width, is_bool = _WIDTH[lf.physical_type], lf.physical_type == "BOOLEAN"
        dvals = None
        if dict_pages and dict_n and idx is not None:
            dvals, dstat = _place(buf, dp, None, None, None, None, width, False, dict_n)
            # a dictionary entry that its page does not hold is out of range for every row that names it
            dict_n_t = (dstat == 0).to(torch.int64).cumprod(0).sum()
            idx = torch.where(idx.to(torch.int64) < dict_n_t, idx, torch.full_like(idx, -1))
        values, status = _place(buf, d_pages, excl, idx, dvals, stream_err, width, is_bool, nrows)
        dt = {"BOOLEAN": torch.bool, "INT32": torch.int32, "INT64": torch.int64, "FLOAT": torch.float32,
              "DOUBLE": torch.float64}[lf.physical_type]
        values = values.view(dt)
        want = {INT64: torch.int64, INT32: torch.int32, FLOAT64: torch.float64, FLOAT32: torch.float32, BOOL: torch.bool}[t]
        return (values if want == dt else values.to(want)), status

    # BYTE_ARRAY: a span into buf per row, from the PLAIN pages' length chains or the dictionary's
    row_page = torch.from_numpy(np.repeat(np.arange(nv_pages, dtype=np.int64), pp[:, 1])).to(dev)
    covered = int(pp[:, 1].sum())
    src_row = d_pages[:, 2][row_page]
    base_row = d_pages[:, 0][row_page]
    pg_bad = (stream_err[:nv_pages] != 0) | (stream_err[nv_pages:] != 0) | (d_pages[:, 2] == 3)
    bad_row = pg_bad[row_page]
    slot = (excl if opt else arange)[:covered]
    valid = (excl[1:covered + 1] > excl[:covered]) if opt else torch.ones(covered, dtype=torch.bool, device=dev)
    vstart, vlen, vstat = _byte_spans(buf, d_pages, excl, nrows, stream_err, nrows)
    start = torch.zeros(nrows, dtype=torch.int64, device=dev)
    length = torch.zeros(nrows, dtype=torch.int32, device=dev)
    status = torch.full((nrows,), 2, dtype=torch.uint8, device=dev)
    sl = slot.clamp(max=max(nrows - 1, 0))
    st = vstat[sl] if nrows else vstat[:0]
    s_, l_ = (vstart[sl], vlen[sl]) if nrows else (vstart[:0], vlen[:0])
    ix = None
    if has_idx and dict_pages:
        dstart, dlen, dstat = _byte_spans(buf, dp, None, dict_n, None, max(dict_n, 1))
        rank = slot - (excl[base_row] if opt else base_row)
        ix = idx[(base_row + rank).clamp(0, max(nrows - 1, 0))].to(torch.int64)
        ok = (ix >= 0) & (ix < dict_n)
        ixc = ix.clamp(0, max(dict_n - 1, 0))
        from_dict = src_row == 1
        st = torch.where(from_dict, torch.where(ok, dstat[ixc], torch.full_like(st, 2)), st)
        s_ = torch.where(from_dict, dstart[ixc], s_)
        l_ = torch.where(from_dict, dlen[ixc], l_)
    st = torch.where(bad_row, torch.full_like(st, 2), torch.where(valid, st, torch.ones_like(st)))
    live = st == 0
    start[:covered] = torch.where(live, s_, torch.zeros_like(s_))
    length[:covered] = torch.where(live, l_, torch.zeros_like(l_))
    status[:covered] = st
    if t == TEXT:
        return start, length, status
    # category.  Codes are those of setdefault over the rows in order.  Where every dictionary-coded
    # page of the chunk comes before its PLAIN pages (what a writer's fallback produces), the
    # dictionary's entries that rows name are encoded once, in the order in which rows first name
    # them, and the rows take their codes from that small map; PLAIN rows are encoded directly, after
    # them.  Any other page order encodes every row directly, which gives the same codes.
    kinds = [int(k) for k in pp[:, 2] if k in (0, 1)]
    if ix is None or kinds != sorted(kinds, reverse=True) or dict_n == 0:
        return dictionary.encode(RaggedBatch(buf, start, length), status), None, status
    named = live & (src_row == 1)
    pos = torch.arange(covered, dtype=torch.int64, device=dev)
    first = torch.full((dict_n,), covered, dtype=torch.int64, device=dev)
    first.scatter_reduce_(0, ix[named], pos[named], reduce="amin")
    order = torch.argsort(first, stable=True)
    est = torch.where(first[order] < covered, dstat[order], torch.ones_like(dstat))
    ecodes = dictionary.encode(RaggedBatch(buf, dstart[order], dlen[order]), est)
    code_of = torch.empty(dict_n, dtype=torch.int32, device=dev)
    code_of[order] = ecodes
    codes = torch.full((nrows,), -1, dtype=torch.int32, device=dev)
    codes[:covered] = torch.where(named, code_of[ix.clamp(0, dict_n - 1)], codes[:covered])
    plain = live & (src_row == 0)
    pst = torch.where(plain, torch.zeros_like(st), torch.ones_like(st))
    if bool(kinds) and kinds[-1] == 0:
        pcodes = dictionary.encode(RaggedBatch(buf, start[:covered], length[:covered]), pst)
        codes[:covered] = torch.where(plain, pcodes, codes[:covered])
    return codes, None, status


def _empty_part(specs, dicts, dev):
    import torch
    cols = []
    for j, (name, _leaf, lf, t) in enumerate(specs):
        status = torch.empty(0, dtype=torch.uint8, device=dev)
        if t == TEXT:
            cols.append(Column(name, lf.name, TEXT, None, torch.empty(0, dtype=torch.int32, device=dev), status,
                               torch.empty(0, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)))
        elif t == CATEGORY:
            cols.append(Column(name, lf.name, CATEGORY, torch.empty(0, dtype=torch.int32, device=dev), None, status,
                               dictionary=dicts[j]))
        else:
            dt = {INT64: torch.int64, INT32: torch.int32, FLOAT64: torch.float64, FLOAT32: torch.float32, BOOL: torch.bool}[t]
            cols.append(Column(name, lf.name, t, torch.empty(0, dtype=dt, device=dev), None, status))
    return FieldColumns(cols)


def _row_group(path, dl, records, sizes, rg, specs, dicts):
    """The selected chunks of one row group: gather, walk, decompress, decode."""
    nrows = int(rg.num_rows)
    dev = dl.device
    if nrows == 0:
        return _empty_part(specs, dicts, dev)
    batch = dl.gather(records)
    data = batch.data.view(-1)
    off = batch.offsets.cpu().numpy()[:len(records)]
    ln = np.minimum(batch.lengths.cpu().numpy(), np.array(sizes, dtype=np.int64))
    table, counts, errors = parquet_page_table(data, off, ln)
    base = np.concatenate([[0], np.cumsum(counts)])
    for k, (_n, j, lf, _t) in enumerate(specs):
        _check_pages(path, lf, table[base[k]:base[k + 1]])
    packed = np.array([rg.columns[j].codec == "LZ4_RAW" for _n, j, _lf, _t in specs])
    sel = np.nonzero(packed[table[:, _T_CHUNK]])[0] if len(table) else np.zeros(0, np.int64)
    buf2 = None
    if len(sel):
        buf2, rows2 = _decompress(data, table, sel)
        table = table.copy()
        table[sel] = rows2
    bufs = [buf2 if packed[k] and buf2 is not None else data for k in range(len(specs))]
    tabs = [_chunk_tables(table[base[k]:base[k + 1]] if not errors[k] else table[:0], lf, nrows)
            for k, (_n, _j, lf, _t) in enumerate(specs)]    # a corrupt chunk: what the walk found before the error is dropped
    streams = [None] * len(specs)
    for buf in (data, buf2):                            # the chunks of one buffer share their launches
        ks = [k for k in range(len(specs)) if bufs[k] is buf]
        if buf is not None and ks:
            got = _levels_and_indices(buf, [tabs[k] for k in ks], [specs[k][2].max_definition_level == 1 for k in ks], nrows)
            for k, g in zip(ks, got):
                streams[k] = g
    cols = []
    for k, (name, j, lf, t) in enumerate(specs):
        buf = bufs[k]
        got = _decode_chunk(buf, tabs[k], streams[k], lf, t, nrows, dicts.get(k))
        if t == TEXT:
            start, length, status = got
            text = extract_text(buf, start, length, status)
            cols.append(Column(name, lf.name, TEXT, None, text.lengths, status, text.data, text.offsets))
        elif t == CATEGORY:
            codes, _none, status = got
            cols.append(Column(name, lf.name, CATEGORY, codes, None, status, dictionary=dicts[k]))
        else:
            values, status = got
            cols.append(Column(name, lf.name, t, values, None, status))
    return FieldColumns(cols)


def parquet_row_groups(fs, path: str, columns=None, row_groups=None, device=None, device_plan="auto",
                       dictionaries=None):
    """A generator of one :class:`FieldColumns` per row group (``row_groups``: their numbers, in the
    order wanted; ``None``: all), for a training loop that takes a file piece by piece.  Arguments
    are those of :func:`read_parquet_columns`; a category column's dictionary is shared by all row
    groups.  The footer is read and everything it can refuse is refused when the generator is
    created, not at the first ``next``."""
    md = parquet_metadata(fs, path)
    specs, groups = _plan(path, md, columns, row_groups)
    return _row_group_iter(fs, path, md, specs, groups, device, device_plan, dictionaries)


def _row_group_iter(fs, path, md, specs, groups, device, device_plan, dictionaries):
    # the file cut at the boundaries of the selected chunks: a chunk is one record of the dataset
    length = int(fs.get_status(path).length)
    ranges = {}
    for g in groups:
        for _n, j, lf, _t in specs:
            a, b = _chunk_range(md.row_groups[g].columns[j])
            if not 0 <= a <= b <= length:
                raise ValueError(f"{path}: the chunk of column {lf.name!r} in row group {g} lies outside the file")
            ranges[(g, j)] = (a, b)
    cuts = np.array(sorted({0, length} | {x for ab in ranges.values() for x in ab}), dtype=np.int64)
    for a, b in ranges.values():
        if np.searchsorted(cuts, b) - np.searchsorted(cuts, a) > 1:
            raise ValueError(f"{path}: column chunks overlap")
    ds = IndexedRecordDataset(fs, path, index=cuts, device=device)
    with DeviceBatchLoader(ds, batch_size=max(1, len(specs)), device=device, align=1, device_plan=device_plan) as dl:
        dicts = _category_dictionaries([(n, j, t) for n, j, _lf, t in specs], dictionaries, dl.device)
        if not groups:
            yield _empty_part(specs, dicts, dl.device)
            return
        for g in groups:
            records, sizes = [], []
            for _n, j, _lf, _t in specs:
                a, b = ranges[(g, j)]
                records.append(min(int(np.searchsorted(cuts, a)), len(cuts) - 2))
                sizes.append(b - a)                     # an empty chunk has no record of its own: cut to nothing
            yield _row_group(path, dl, records, sizes, md.row_groups[g], specs, dicts)


def read_parquet_columns(fs, path: str, columns=None, row_groups=None, device=None, device_plan="auto",
                         dictionaries=None) -> FieldColumns:
    """The selected columns of a Parquet file as tensors on ``device``, decoded where the bytes lie.

    ``columns``: ``None`` (every supported leaf, with the type its physical type implies), a list of
    leaf names (or of ``(leaf name, type)``), both named by the leaf name, or a dict
    ``name -> (leaf name, type)`` with the type names of :mod:`.fields` plus ``"bool"``; a type of
    ``None`` is the implied one.  A leaf of a nested schema is named by its dotted path.
    ``row_groups``: the numbers of the row groups to read, in the order wanted (``None``: all);
    their columns are joined with :meth:`FieldColumns.concat`.  ``dictionaries`` maps a category
    column's name to the :class:`TextDictionary` to encode into, so codes
    agree across files; a category column without one gets a fresh dictionary for the file.

    The bytes of the selected column chunks, and only those, come through a
    :class:`DeviceBatchLoader` over the file cut at chunk boundaries: one ragged gather per row group
    when the file is cached in device memory by one in-process worker (``device_plan="auto"``); a
    file on a DRAM tier, or ``device_plan=False``, is decoded by the host loops on CPU tensors.  Per
    row group the page table, a flag per LZ4 page and the sizes that text columns, dictionaries and
    (in kernel variant 1) run tables need are read back; everything else stays on torch's current
    stream.  See the module's documentation for types, statuses and what is refused."""
    parts = list(parquet_row_groups(fs, path, columns, row_groups, device, device_plan, dictionaries))
    return FieldColumns.concat(parts)
