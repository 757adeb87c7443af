"""Typed columns from Parquet files: what :mod:`.fields` does for CSV and :mod:`.json_fields` for
JSON Lines, for the table format that ``transformTable`` writes.  :func:`parquet_metadata` reads
the footer (a small Thrift compact-protocol reader, written from the format specification: no
``pyarrow`` here); :func:`read_parquet_columns` brings the bytes of the selected column chunks to
the device with the ragged gather and decodes their pages there (kernels for device memory, C++
loops for a file on a DRAM tier or read through the general path); :func:`parquet_row_groups`
yields one :class:`FieldColumns` per row group for a training loop.

The passes (``csrc/parquet_host.h`` has the rules in full): the page walk parses the
``PageHeader`` between the pages of every chunk into a page table; LZ4_RAW pages are decompressed
by the LZ4 block kernel and, where the call allows it (``codecs=``), SNAPPY pages by the Snappy
kernel (``csrc/snappy_host.h`` has the format) into a second buffer; definition levels, dictionary indices and RLE
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
INT96 and FIXED_LEN_BYTE_ARRAY, every codec but UNCOMPRESSED, LZ4_RAW and, only when the call names
it in ``codecs=`` (``codecs=("LZ4_RAW", "SNAPPY")`` or ``codecs="all"``), SNAPPY (so GZIP, ZSTD,
BROTLI and the Hadoop-framed LZ4 always), BIT_PACKED levels, encrypted files, and the DELTA_* and
BYTE_STREAM_SPLIT value encodings, which only a page header reveals and which are therefore
raised after the page walk.  Columns that are not selected may be of any kind.

The write side, :func:`write_parquet_columns` and :class:`ParquetWriter`, turns a
:class:`FieldColumns` back into a file (``csrc/parquet_encode_host.h`` has the rules): measure (a
flag per row and the sizes per page, the one readback), rank (``torch.cumsum``), emit (level bits,
PLAIN values, text, bit-packed booleans and dictionary indices, and the host-built headers, all into
one buffer per row group), then a footer from a small Thrift compact writer.  V1 data pages, flat
columns; uncompressed, or with ``compression="lz4_raw"`` every page body as one LZ4 block made on
the device (``csrc/lz4_block_host.h``: segments parsed by independent waves, linked and merged into
one standard block per page, whatever its size).  ``statistics=True`` has the device compute ``null_count``, ``min_value`` and
``max_value`` of every column chunk (``csrc/parquet_stats_host.h`` has the rules;
:func:`column_statistics` gives them for any :class:`FieldColumns`), and the readers take
``filters=`` to skip the row groups that the statistics of any file rule out.
"""
from __future__ import annotations

import struct
from collections import namedtuple

import numpy as np

from .dataset import DeviceBatchLoader, IndexedRecordDataset, RaggedBatch
from .fields import (BOOL, CATEGORY, FLOAT32, FLOAT64, INT32, INT64, SPAN, TEXT, Column, FieldColumns, TextDictionary,
                     _category_dictionaries, _queue, extract_text)

PHYSICAL = ["BOOLEAN", "INT32", "INT64", "INT96", "FLOAT", "DOUBLE", "BYTE_ARRAY", "FIXED_LEN_BYTE_ARRAY"]
CODECS = ["UNCOMPRESSED", "SNAPPY", "GZIP", "LZO", "BROTLI", "LZ4", "ZSTD", "LZ4_RAW"]
REPETITION = ["REQUIRED", "OPTIONAL", "REPEATED"]
ENCODINGS = {0: "PLAIN", 2: "PLAIN_DICTIONARY", 3: "RLE", 4: "BIT_PACKED", 5: "DELTA_BINARY_PACKED",
             6: "DELTA_LENGTH_BYTE_ARRAY", 7: "DELTA_BYTE_ARRAY", 8: "RLE_DICTIONARY", 9: "BYTE_STREAM_SPLIT"}

ParquetLeaf = namedtuple("ParquetLeaf", "name physical_type repetition max_definition_level max_repetition_level "
                                        "type_length")
ParquetChunk = namedtuple("ParquetChunk", "name physical_type codec num_values dictionary_page_offset "
                                          "data_page_offset total_compressed_size statistics", defaults=(None,))
ParquetStatistics = namedtuple("ParquetStatistics", "null_count min max")
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


# converted types and LogicalType union fields whose order is that of the physical type as our column
# types see it: UTF8, ENUM, DATE, TIME_*, TIMESTAMP_*, INT_8 .. INT_64, JSON; STRING, ENUM, DATE, TIME,
# TIMESTAMP, INTEGER (signed only), JSON
_OUR_CONVERTED = {0, 4, 6, 7, 8, 9, 10, 15, 16, 17, 18, 19}
_OUR_LOGICAL = {1, 4, 6, 7, 8, 10, 12}
_PLAIN_FORMAT = {"INT32": "<i", "INT64": "<q", "FLOAT": "<f", "DOUBLE": "<d"}


def _our_order(elem: dict) -> bool:
    """Whether min_value / max_value of a leaf (its SchemaElement) are in the order in which our
    column types compare: signed integers, IEEE floats, unsigned bytes."""
    conv, logical = elem.get(6), elem.get(10)
    if conv is not None and conv not in _OUR_CONVERTED:
        return False
    if logical is not None:
        if not isinstance(logical, dict) or len(logical) != 1 or next(iter(logical)) not in _OUR_LOGICAL:
            return False
        if 10 in logical and not (isinstance(logical[10], dict) and logical[10].get(2) is True):
            return False                                # an unsigned INTEGER
    return True


def _stat_value(physical: str, raw):
    """A PLAIN-encoded statistics value as a Python value; ``None`` when the bytes do not fit the type."""
    if not isinstance(raw, bytes):
        return None
    if physical == "BYTE_ARRAY":
        return raw
    if physical == "BOOLEAN":
        return bool(raw[0]) if len(raw) == 1 else None
    fmt = _PLAIN_FORMAT.get(physical)
    if fmt is None or len(raw) != struct.calcsize(fmt):
        return None
    return struct.unpack(fmt, raw)[0]


def _read_statistics(st, physical: str, ordered: bool):
    """The ``Statistics`` struct of a column chunk (``None`` without one) as ParquetStatistics."""
    if not isinstance(st, dict):
        return None
    lo = hi = None
    if ordered:
        lo, hi = _stat_value(physical, st.get(6)), _stat_value(physical, st.get(5))
        if lo is None or hi is None or lo != lo or hi != hi:        # one bound alone, or a NaN, says nothing
            lo = hi = None
    nulls = st.get(3)
    return ParquetStatistics(nulls if isinstance(nulls, int) and not isinstance(nulls, bool) else None, lo, hi)


def parquet_metadata(fs, path: str) -> ParquetMetadata:
    """The footer of a Parquet file, read with positioned reads through the client stream (the last
    8 bytes, then the ``FileMetaData``): ``num_rows``, ``schema`` (one :class:`ParquetLeaf` per leaf
    column: dotted ``name``, ``physical_type``, ``repetition``, ``max_definition_level``,
    ``max_repetition_level``, ``type_length``) and ``row_groups`` (``num_rows`` and, per leaf in
    schema order, a :class:`ParquetChunk`: ``codec``, ``num_values``, ``dictionary_page_offset``
    (``None`` without one), ``data_page_offset``, ``total_compressed_size``, ``statistics``).  Type,
    codec and repetition are the names of the format specification.  Unknown fields are skipped.

    ``statistics`` is ``None`` for a chunk without a ``Statistics`` struct (a file written without
    statistics), else a :class:`ParquetStatistics`: ``null_count`` (``None`` if the struct has
    none) and ``min`` / ``max`` from ``min_value`` / ``max_value`` as ``int``, ``float``, ``bool``
    or ``bytes``.  The bounds are taken only where the file's ``column_orders`` gives the leaf the
    type-defined order and that order is the one our column types use: a leaf without converted or
    logical type, or STRING / UTF8, ENUM, JSON, a signed INTEGER, DATE, TIME or TIMESTAMP.  For
    every other leaf (unsigned integers, DECIMAL, FLOAT16, INTERVAL, unknown types), for bytes that
    do not fit the physical type and for a NaN bound they are ``None``.  The deprecated ``min`` /
    ``max`` fields are never read."""
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
    leaves, ours = [], []                               # ours: the leaf's order is the one our types use

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
            ours.append(_our_order(e))
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
    orders = md.get(7) if isinstance(md.get(7), list) else []
    groups = []
    for rg in md.get(4) or []:
        cols = []
        for j, cc in enumerate(rg.get(1) or []):
            m = cc.get(3)
            if m is None:
                raise NotImplementedError(f"{path}: a column chunk without metadata (encrypted, or in another file) "
                                          f"is not supported")
            cols.append(ParquetChunk(".".join(x.decode("utf-8", "replace") for x in m.get(3) or []),
                                     _name(PHYSICAL, m.get(1)), _name(CODECS, m.get(4)), m.get(5, 0), m.get(11),
                                     m.get(9, 0), m.get(7, 0),
                                     _read_statistics(m.get(12), _name(PHYSICAL, m.get(1)),
                                                      j < len(ours) and ours[j] and j < len(orders)
                                                      and isinstance(orders[j], dict) and 1 in orders[j])))
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


# the codecs that have a decoder, by the names a caller may give (pyarrow calls codec 7 "LZ4")
_DECODERS = {"LZ4_RAW": "LZ4_RAW", "LZ4": "LZ4_RAW", "SNAPPY": "SNAPPY"}
_DEFAULT_CODECS = ("LZ4_RAW",)


def _allowed_codecs(codecs) -> tuple:
    """The ``codecs=`` argument as the names of :data:`CODECS` that a call may decode besides
    UNCOMPRESSED, LZ4_RAW first (the order in which a refusal lists them)."""
    if codecs is None:
        names = _DEFAULT_CODECS
    elif isinstance(codecs, str) and codecs.lower() == "all":
        names = tuple(_DECODERS.values())
    else:
        names = []
        for c in [codecs] if isinstance(codecs, str) else codecs:
            key = c.upper() if isinstance(c, str) else c
            if key == "UNCOMPRESSED":
                continue
            if key not in _DECODERS:
                raise ValueError(f"codecs names codecs that have a decoder, {sorted(_DECODERS)} (or 'all'), got {c!r}")
            names.append(_DECODERS[key])
    return tuple(sorted(set(names), key=CODECS.index, reverse=True))


def _plan(path, md: ParquetMetadata, columns, row_groups, codecs=None):
    """[(name or None, leaf position, leaf, type code)] and the row group numbers, with everything
    that can be refused from the footer refused.  ``codecs``: what :func:`_allowed_codecs` gave."""
    allowed = _allowed_codecs(None) if codecs is None else codecs
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
            if cc.codec != "UNCOMPRESSED" and cc.codec not in allowed:
                names = ("UNCOMPRESSED",) + allowed
                only = f"{', '.join(names[:-1])} and {names[-1]} are" if allowed else "UNCOMPRESSED is"
                hint = (f" (pass codecs=(..., {cc.codec!r}) or codecs='all' to have it decoded)"
                        if cc.codec in _DECODERS.values() else "")
                raise NotImplementedError(f"{path}: column {lf.name!r} is compressed with {cc.codec}; only "
                                          f"{only} supported{hint}")
    return specs, groups


def _chunk_range(cc: ParquetChunk):
    start = cc.data_page_offset
    if cc.dictionary_page_offset is not None and 0 < cc.dictionary_page_offset < start:
        start = cc.dictionary_page_offset
    return int(start), int(start) + int(cc.total_compressed_size)


# ---- pruning row groups by their statistics -------------------------------------------------------------
_FILTER_OPS = ("==", "!=", "<", "<=", ">", ">=", "in", "is_null")
_INT_TYPES, _FLOAT_TYPES = ("INT32", "INT64"), ("FLOAT", "DOUBLE")


def _filter_value(path, leaf: ParquetLeaf, v):
    """A filter's value as what the leaf's statistics compare with, or TypeError."""
    ph, ok = leaf.physical_type, True
    if ph in _INT_TYPES:
        ok = isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
        v = int(v) if ok else v
    elif ph in _FLOAT_TYPES:
        ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))
    elif ph == "BOOLEAN":
        ok = isinstance(v, (bool, np.bool_))
        v = bool(v) if ok else v
    elif ph == "BYTE_ARRAY":
        ok = isinstance(v, (bytes, str))
        v = v.encode("utf-8") if isinstance(v, str) else v
    if not ok:
        raise TypeError(f"{path}: a filter on column {leaf.name!r} ({ph}) cannot take the value {v!r}")
    return v


def _filters(path, md: ParquetMetadata, filters):
    """``filters`` as a list of alternatives, each a list of (leaf position, op, value), checked."""
    if filters is None:
        return None
    filters = list(filters)
    if filters and all(isinstance(f, tuple) for f in filters):
        filters = [filters]
    by_name = {lf.name: j for j, lf in enumerate(md.schema)}
    out = []
    for alt in filters:
        terms = []
        for term in alt:
            if not isinstance(term, (tuple, list)) or len(term) != 3:
                raise ValueError(f"a filter is (leaf name, op, value), got {term!r}")
            leaf, op, v = term
            if leaf not in by_name:
                raise KeyError(f"{path}: no column {leaf!r} to filter on; the leaves are {sorted(by_name)}")
            op = "==" if op == "=" else op
            if op not in _FILTER_OPS:
                raise ValueError(f"unknown filter op {op!r}: one of {', '.join(_FILTER_OPS)}")
            j = by_name[leaf]
            lf = md.schema[j]
            if op == "is_null":
                if not isinstance(v, (bool, np.bool_)):
                    raise TypeError(f"{path}: is_null on column {leaf!r} takes True or False, not {v!r}")
                v = bool(v)
            elif op == "in":
                if isinstance(v, (str, bytes)) or not hasattr(v, "__iter__"):
                    raise TypeError(f"{path}: 'in' on column {leaf!r} takes a collection, not {v!r}")
                v = [_filter_value(path, lf, x) for x in v]
            else:
                v = _filter_value(path, lf, v)
            terms.append((j, op, v))
        out.append(terms)
    return out


def _may_match(cc: ParquetChunk, op: str, v) -> bool:
    """False only when the chunk's statistics prove that no row of it satisfies ``op v``."""
    st = cc.statistics
    if st is None:
        return True
    all_null = st.null_count is not None and st.null_count == cc.num_values
    if op == "is_null":
        return st.null_count is None or (st.null_count != 0 if v else not all_null)
    lo, hi = st.min, st.max
    if op == "!=":                                      # NaNs are outside the bounds and satisfy !=
        return not (lo is not None and lo == hi == v and cc.physical_type not in _FLOAT_TYPES)
    if all_null:
        return False
    if lo is None or hi is None:
        return True
    vs = v if op == "in" else [v]
    if any(x != x for x in vs):                         # a NaN to compare with: nothing is proven
        return True
    if op in ("==", "in"):
        return any(lo <= x <= hi for x in vs)
    return {"<": lo < v, "<=": lo <= v, ">": hi > v, ">=": hi >= v}[op]


def _matching(path, md: ParquetMetadata, filters, row_groups):
    n = len(md.row_groups)
    groups = list(range(n)) if row_groups is None else [int(g) for g in row_groups]
    for g in groups:
        if not 0 <= g < n:
            raise IndexError(f"{path}: no row group {g} (there are {n})")
    if not filters:
        return groups
    return [g for g in groups
            if any(all(j >= len(md.row_groups[g].columns) or _may_match(md.row_groups[g].columns[j], op, v)
                       for j, op, v in alt) for alt in filters)]


def parquet_matching_row_groups(fs, path: str, filters, row_groups=None) -> list:
    """The numbers of the row groups (of ``row_groups``, in its order; ``None``: all) that the
    file's statistics cannot rule out for ``filters``: what :func:`read_parquet_columns` reads when
    given the same filters.  Only the footer is read."""
    md = parquet_metadata(fs, path)
    return _matching(path, md, _filters(path, md, filters), row_groups)


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


def _decompress(data, table, sel, codecs):
    """The pages ``sel`` (rows of the host page table) of compressed chunks decompressed into a second
    buffer: ``(buffer, rows)`` where ``rows`` are those pages' table rows rewritten to point into the
    buffer as uncompressed pages; a page whose stream is malformed, or gives another size than its
    header states, gets type -1.  ``codecs``: the codec number of every page of ``sel``; the pages of
    all codecs share the buffer, and each codec present takes one native call."""
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
    codecs = np.asarray(codecs, dtype=np.int64)
    order = np.argsort(codecs, kind="stable")           # the pages of one codec in a row
    d_table, d_dst = _dev_i64(rows[order], dev), _dev_i64(dst[:-1][order], dev)
    chunks = torch.zeros(n * 3, dtype=torch.int64, device=dev)
    got = torch.zeros(2, n, dtype=torch.int32, device=dev)      # expected, produced
    at = 0
    with native_errors():
        for codec in np.unique(codecs):
            m = int((codecs == codec).sum())
            lib().parquet_decompress_raw(int(codec), _ptr(data), data.numel(), d_table.data_ptr() + at * rows.shape[1] * 8,
                                         m, d_dst.data_ptr() + at * 8, _ptr(out), out.numel(),
                                         chunks.data_ptr() + at * 24, got[0].data_ptr() + at * 4,
                                         got[1].data_ptr() + at * 4, device, stream)
            at += m
    bad = np.zeros(n, dtype=bool)
    bad[order] = (got[0] != got[1]).cpu().numpy()
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
        if src in (1, 2):
            vs[k] = (voff, vlen, 1 if src == 2 else 2, skip, 1, nv, rb, 0)
        else:                                           # PLAIN values are no stream: their first byte is no bit width
            vs[k] = (0, 0, 0, 0, 1, 0, rb, 0)
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
    codec = np.array([CODECS.index(rg.columns[j].codec) for _n, j, _lf, _t in specs])
    packed = codec != 0                                 # not UNCOMPRESSED
    sel = np.nonzero(packed[table[:, _T_CHUNK]])[0] if len(table) else np.zeros(0, np.int64)
    buf2 = None
    if len(sel):
        buf2, rows2 = _decompress(data, table, sel, codec[table[sel, _T_CHUNK]])
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
                       dictionaries=None, filters=None, codecs=None):
    """A generator of one :class:`FieldColumns` per row group (``row_groups``: their numbers, in the
    order wanted; ``None``: all; with ``filters``, those of them that the statistics cannot rule
    out), for a training loop that takes a file piece by piece.  Arguments are those of
    :func:`read_parquet_columns`; a category column's dictionary is shared by all row groups.  The
    footer is read and everything it can refuse is refused when the generator is created, not at the
    first ``next``."""
    allowed = _allowed_codecs(codecs)
    md = parquet_metadata(fs, path)
    if filters is not None:
        row_groups = _matching(path, md, _filters(path, md, filters), row_groups)
    specs, groups = _plan(path, md, columns, row_groups, allowed)
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
                         dictionaries=None, filters=None, codecs=None) -> FieldColumns:
    """The selected columns of a Parquet file as tensors on ``device``, decoded where the bytes lie.

    ``columns``: ``None`` (every supported leaf, with the type its physical type implies), a list of
    leaf names (or of ``(leaf name, type)``), both named by the leaf name, or a dict
    ``name -> (leaf name, type)`` with the type names of :mod:`.fields` plus ``"bool"``; a type of
    ``None`` is the implied one.  A leaf of a nested schema is named by its dotted path.
    ``row_groups``: the numbers of the row groups to read, in the order wanted (``None``: all);
    their columns are joined with :meth:`FieldColumns.concat`.  ``dictionaries`` maps a category
    column's name to the :class:`TextDictionary` to encode into, so codes
    agree across files; a category column without one gets a fresh dictionary for the file.

    ``filters`` prunes whole row groups by the statistics in the footer (:func:`parquet_metadata`):
    a list of ``(leaf name, op, value)`` that must all hold, or a list of such lists of which any
    may hold (pyarrow's form).  The ops are ``==`` (also ``=``), ``!=``, ``<``, ``<=``, ``>``,
    ``>=``, ``in`` (a collection) and ``is_null`` (``True`` or ``False``); a value is an ``int`` for
    an integer column, an ``int`` or ``float`` for a float column, a ``bool`` for a boolean column
    and ``bytes`` or ``str`` (taken as UTF-8) for a BYTE_ARRAY column, else ``TypeError``; an unknown
    leaf is a ``KeyError``, an unknown op a ``ValueError``, all before any data is read.  The leaf
    need not be among ``columns``.  A row group is skipped only when its statistics prove that no
    row of it can match (a chunk without statistics, or without bounds, keeps its row group), and a
    row group that is kept comes back whole: rows are not filtered.  The bytes of a skipped row
    group are never gathered and none of its pages is walked, and what the footer refuses (codec,
    nesting, physical type) is refused for the kept row groups only.  With every row group pruned the
    result has no rows, the requested columns and types, and nothing is gathered or launched.

    ``codecs`` names the codecs the call may decode besides UNCOMPRESSED: ``None`` is
    ``("LZ4_RAW",)``; ``("LZ4_RAW", "SNAPPY")`` or ``"all"`` (every codec that has a decoder) also
    reads Snappy chunks, which Parquet writers make by default.  Names are case-insensitive and
    ``"LZ4"`` is pyarrow's name for LZ4_RAW; a name without a decoder (``"GZIP"``, ``"ZSTD"``, ...)
    is a ``ValueError``.  A row group may mix the codecs; every codec present costs two launches.

    The bytes of the selected column chunks, and only those, come through a
    :class:`DeviceBatchLoader` over the file cut at chunk boundaries: one ragged gather per row group
    when the file is cached in device memory by one in-process worker (``device_plan="auto"``); a
    file on a DRAM tier, or ``device_plan=False``, is decoded by the host loops on CPU tensors.  Per
    row group the page table, a flag per LZ4 page and the sizes that text columns, dictionaries and
    (in kernel variant 1) run tables need are read back; everything else stays on torch's current
    stream.  See the module's documentation for types, statuses and what is refused."""
    parts = list(parquet_row_groups(fs, path, columns, row_groups, device, device_plan, dictionaries, filters, codecs))
    return FieldColumns.concat(parts)


# ---- writing ------------------------------------------------------------------------------------------
# page-table and measure columns of csrc/parquet_encode_host.h
_PE_COLS, _PM_COLS = 16, 8
(_E_KIND, _E_WIDTH, _E_VALUES, _E_STATUS, _E_OFFSETS, _E_AUX, _E_ROW, _E_ROWS, _E_FLAT, _E_LEVEL, _E_VALOFF, _E_VALBYTES,
 _E_NVALID) = range(13)
_M_VALID, _M_BAD, _M_TEXT, _M_MAXCODE, _M_OUTSIDE = range(5)
_K_FIXED, _K_BOOL, _K_TEXT, _K_INDEX = range(4)
_PASS_ROWS, _PASS_TEXT, _PASS_PACK = 1, 2, 3
_KIND_ORDER = {_K_FIXED: 0, _K_BOOL: 1, _K_INDEX: 2, _K_TEXT: 3}      # the table's order: each pass takes a range
_MAX_BODY = 2 ** 31
CREATED_BY = "alluxio-amd parquet writer (device page encode)"
_WRITE_KINDS = {INT64: ("INT64", _K_FIXED, 8), INT32: ("INT32", _K_FIXED, 4), FLOAT64: ("DOUBLE", _K_FIXED, 8),
                FLOAT32: ("FLOAT", _K_FIXED, 4), BOOL: ("BOOLEAN", _K_BOOL, 1), TEXT: ("BYTE_ARRAY", _K_TEXT, 0),
                CATEGORY: ("BYTE_ARRAY", _K_INDEX, 0)}


def _varint(v: int) -> bytes:
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


class _ThriftOut:
    """A writer of the Thrift compact protocol, the counterpart of :class:`_Thrift`: fields are
    written in ascending id order inside ``struct`` / ``end``."""

    def __init__(self):
        self.b = bytearray()
        self._last = [0]

    def _field(self, fid: int, t: int):
        d = fid - self._last[-1]
        if 0 < d <= 15:
            self.b.append((d << 4) | t)
        else:
            self.b.append(t)
            self.b += _varint((fid << 1) ^ (fid >> 63))
        self._last[-1] = fid

    def i32(self, fid: int, v: int):
        self._field(fid, 5)
        self.b += _varint(((v << 1) ^ (v >> 63)) & 0xFFFFFFFFFFFFFFFF)

    def i64(self, fid: int, v: int):
        self._field(fid, 6)
        self.b += _varint(((v << 1) ^ (v >> 63)) & 0xFFFFFFFFFFFFFFFF)

    def binary(self, fid: int, v: bytes):
        self._field(fid, 8)
        self.b += _varint(len(v)) + v

    def list_(self, fid: int, etype: int, n: int):
        self._field(fid, 9)
        self.b += bytes([(n << 4) | etype]) if n < 15 else bytes([0xF0 | etype]) + _varint(n)

    def struct(self, fid=None):
        """Opens a struct: a field of the current one, or (``None``) a list element or the top."""
        if fid is not None:
            self._field(fid, 12)
        self._last.append(0)

    def end(self):
        self.b.append(0)
        self._last.pop()


def _page_header(page_type: int, size: int, num_values: int, encoding: int, compressed=None) -> bytes:
    t = _ThriftOut()
    t.struct()
    t.i32(1, page_type)
    t.i32(2, size)
    t.i32(3, size if compressed is None else compressed)
    t.struct(5 if page_type == 0 else 7)
    t.i32(1, num_values)
    t.i32(2, encoding)
    if page_type == 0:
        t.i32(3, 3)                                     # definition and repetition levels: RLE
        t.i32(4, 3)
    t.end()
    t.end()
    return bytes(t.b)


class _WriteColumn:
    __slots__ = ("name", "type", "physical", "kind", "width", "values", "status", "offsets", "data_bytes", "dictionary",
                 "required", "keep")


def _write_columns(columns, required):
    """The columns of a FieldColumns as the writer takes them: contiguous tensors of the expected
    types on one device.  Raises for what cannot be written."""
    import torch
    if not isinstance(columns, FieldColumns):
        raise TypeError(f"the columns are a FieldColumns, got {type(columns).__name__}")
    if len(columns) == 0:
        raise ValueError("at least one column is required")
    dev = columns[0].status.device
    want = {INT64: torch.int64, INT32: torch.int32, FLOAT64: torch.float64, FLOAT32: torch.float32, BOOL: torch.bool,
            CATEGORY: torch.int32}
    out, rows = [], columns.rows
    for j, c in enumerate(columns):
        name = c.name if c.name is not None else f"f{j}"
        if c.type == SPAN:
            raise TypeError(f"column {name!r} is a span column: its starts point into a batch that is gone; parse it "
                            f"as text")
        if c.type not in _WRITE_KINDS or (c.type == TEXT and c.data is None) or (c.type == CATEGORY and c.values is None):
            raise TypeError(f"column {name!r} cannot be written: it holds no values of a known type")
        w = _WriteColumn()
        w.name, w.type = name, c.type
        w.physical, w.kind, w.width = _WRITE_KINDS[c.type]
        w.required = name in required
        w.dictionary, w.offsets, w.data_bytes = None, None, 0
        tensors = [c.status] + ([c.data, c.offsets] if c.type == TEXT else [c.values])
        if any(t.device != dev for t in tensors) or len(c.status) != rows or c.status.dtype != torch.uint8:
            raise ValueError(f"column {name!r}: all columns have the same rows, on one device")
        w.status = c.status.contiguous()
        if c.type == TEXT:
            if c.data.dtype != torch.uint8 or c.offsets.dtype != torch.int64 or c.offsets.numel() != rows + 1:
                raise TypeError(f"column {name!r}: a text column has uint8 data and rows + 1 int64 offsets")
            w.values, w.offsets = c.data.contiguous().view(-1), c.offsets.contiguous()
            w.data_bytes = int(w.values.numel())
        else:
            if c.values.dtype != want[c.type] or c.values.numel() != rows:
                raise TypeError(f"column {name!r}: the values are {c.values.dtype}, not {want[c.type]}")
            w.values = c.values.contiguous()
            if c.type == BOOL:
                w.values = w.values.view(torch.uint8)
            if c.type == CATEGORY:
                if not isinstance(c.dictionary, TextDictionary) or c.dictionary.device != dev:
                    raise ValueError(f"column {name!r}: a category column has a TextDictionary on the columns' device")
                w.dictionary = c.dictionary
        out.append(w)
    if len({w.name for w in out}) != len(out):
        raise ValueError(f"the column names are not distinct: {[w.name for w in out]}")
    unknown = sorted(set(required) - {w.name for w in out})
    if unknown:
        raise ValueError(f"required names columns that are not there: {unknown}")
    return out, dev


# segment-table and result columns of csrc/parquet_stats_host.h
_E_ISFLOAT, _E_MARK = 13, 14
_SR_COLS, _S_NULLS, _S_MIN, _S_MAX, _S_ROUND_MIN, _S_ROUNDS = 28, 0, 2, 3, 8, 10


class _StatsPlan:
    """The statistics of rows [r0, r0 + n) of the writer's columns, one segment per column (and one
    per category column's dictionary): the segment table and the result rows as they start, both
    on the host, and the device arrays the passes need."""
    __slots__ = ("cols", "dev", "table", "init", "seg", "dict_seg", "mark_range", "text_first", "largest", "alive", "marks")

    def __init__(self, cols, r0, n, dev):
        import torch
        self.cols, self.dev = cols, dev
        order = sorted(range(len(cols)), key=lambda j: (_KIND_ORDER[cols[j].kind], j))
        cats = [j for j in order if cols[j].kind == _K_INDEX]
        entries = [len(cols[j].dictionary) for j in cats]
        self.marks = torch.ones(sum(entries), dtype=torch.uint8, device=dev) if cats else None
        self.table = np.zeros((len(cols) + len(cats), _PE_COLS), dtype=np.int64)
        self.seg, self.dict_seg = {}, {}
        flat = mark_at = 0
        for s, j in enumerate(order):
            c, row = cols[j], self.table[s]
            self.seg[j] = s
            row[_E_KIND], row[_E_WIDTH] = c.kind, c.width
            row[_E_VALUES], row[_E_STATUS] = _ptr(c.values), c.status.data_ptr() if n else 0
            row[_E_OFFSETS] = c.offsets.data_ptr() if c.offsets is not None else 0
            row[_E_AUX] = c.data_bytes if c.kind == _K_TEXT else len(c.dictionary) if c.kind == _K_INDEX else 0
            row[_E_ROW], row[_E_ROWS], row[_E_LEVEL] = r0, n, -1
            row[_E_ISFLOAT] = c.type in (FLOAT32, FLOAT64)
            if c.kind == _K_TEXT:
                row[_E_FLAT] = flat
                flat += n
        for k, j in enumerate(cats):                    # the dictionaries: text segments whose status is the marks
            d, row = cols[j].dictionary, self.table[len(cols) + k]
            self.dict_seg[j] = len(cols) + k
            mark = self.marks.data_ptr() + mark_at if entries[k] else 0
            self.table[self.seg[j], _E_MARK] = mark
            row[_E_KIND], row[_E_VALUES], row[_E_OFFSETS] = _K_TEXT, _ptr(d._data), d._off.data_ptr()
            row[_E_STATUS], row[_E_AUX], row[_E_ROWS], row[_E_LEVEL] = mark, d._nbytes, entries[k], -1
            row[_E_FLAT] = flat
            flat += entries[k]
            mark_at += entries[k]
        kinds = self.table[:, _E_KIND]
        marked = np.nonzero(kinds == _K_INDEX)[0]
        self.mark_range = (int(marked[0]), int(marked[-1]) + 1) if len(marked) else (0, 0)
        texts = np.nonzero(kinds == _K_TEXT)[0]
        self.text_first = int(texts[0]) if len(texts) else len(self.table)
        self.largest = int(self.table[:, _E_ROWS].max())
        self.alive = torch.empty(flat, dtype=torch.uint8, device=dev) if flat else None
        self.init = np.zeros((len(self.table), _SR_COLS), dtype=np.int64)
        self.init[:, _S_MIN], self.init[:, _S_MAX] = np.iinfo(np.int64).max, np.iinfo(np.int64).min
        self.init[:, _S_ROUND_MIN:_S_ROUND_MIN + _S_ROUNDS] = -1

    def launch(self, d_table: int, d_results: int) -> None:
        """All passes, queued: ``d_table`` and ``d_results`` are where ``table`` and ``init`` lie on the device."""
        from ..ops.native import lib, native_errors
        device, stream = _queue(self.dev)
        with native_errors():
            lib().parquet_stats_raw(d_table, len(self.table), *self.mark_range, self.text_first, self.largest,
                                    _ptr(self.alive), 0 if self.alive is None else self.alive.numel(), d_results, device,
                                    stream)

    def finish(self, results: np.ndarray) -> list:
        """Per column ``(null_count, min, max)`` with the bounds as PLAIN bytes or ``None``, from the
        result rows on the host."""
        from ..ops.native import lib
        C = lib()
        results = np.ascontiguousarray(results, dtype=np.int64)
        out = []
        for j, c in enumerate(self.cols):
            s = self.seg[j]
            if c.kind == _K_INDEX:
                lo, hi = C.parquet_stats_finish(results[self.dict_seg[j]].ctypes.data, _K_TEXT, 0, False)
            else:
                lo, hi = C.parquet_stats_finish(results[s].ctypes.data, c.kind, c.width, c.type in (FLOAT32, FLOAT64))
            out.append((int(results[s, _S_NULLS]), lo, hi))
        return out


def column_statistics(columns) -> list:
    """One :class:`ParquetStatistics` per column of a :class:`FieldColumns` (on a GPU or on the
    CPU), computed where the columns lie, over all rows as one segment: what
    ``write_parquet_columns(..., statistics=True)`` writes for a file of one row group.

    ``null_count`` counts the rows that the writer would write as nulls under ``invalid="null"``:
    every row whose status is not 0, a text value outside its data, a code outside its dictionary.
    ``min`` and ``max`` are ``None`` without a value.  Integers compare signed and ``False`` is less
    than ``True``.  Floats: NaNs take no part (only NaNs: no bounds), a minimum that equals zero is
    ``-0.0`` and a maximum that equals zero ``+0.0``.  Text and category values (``bytes``) compare
    byte by byte, unsigned, a proper prefix first; a category's bounds are taken over the dictionary
    entries that some row uses; with a value (a used entry) longer than 64 bytes there are no
    bounds.  One small readback."""
    cols, dev = _write_columns(columns, ())
    plan = _StatsPlan(cols, 0, columns.rows, dev)
    both = _dev_i64(np.concatenate([plan.table.ravel(), plan.init.ravel()]), dev)
    plan.launch(both.data_ptr(), both[plan.table.size:].data_ptr())
    got = plan.finish(both[plan.table.size:].cpu().numpy().reshape(-1, _SR_COLS))
    return [ParquetStatistics(nulls, _stat_value(c.physical, lo), _stat_value(c.physical, hi))
            for c, (nulls, lo, hi) in zip(cols, got)]


class _Group:
    """One row group on its way: the page table, the flat arrays and the measure table."""
    __slots__ = ("cols", "r0", "rows", "dev", "table", "index", "flags", "text_bytes", "measure", "flat_n", "layout",
                 "stats", "bodies")


def _measure_group(cols, r0, r1, page_rows, dev, statistics=False) -> _Group:
    """The measure pass over rows [r0, r1) of the columns: one launch and the one readback.  With
    ``statistics`` the statistics passes are queued behind it and their result rows come back in
    that readback: ``g.stats`` then holds ``(null_count, min, max)`` per column."""
    import torch
    from ..ops.native import lib, native_errors
    g = _Group()
    g.cols, g.r0, g.rows, g.dev = cols, r0, r1 - r0, dev
    n = g.rows
    pr = n if page_rows is None else min(int(page_rows), n)
    per_col = -(-n // pr)
    order = sorted(range(len(cols)), key=lambda j: (_KIND_ORDER[cols[j].kind], j))
    g.table = np.zeros((per_col * len(cols), _PE_COLS), dtype=np.int64)
    g.index = {}
    p = 0
    for j in order:
        c = cols[j]
        g.index[j] = list(range(p, p + per_col))
        for k in range(per_col):
            row = g.table[p]
            row[_E_KIND], row[_E_WIDTH] = c.kind, c.width
            row[_E_VALUES], row[_E_STATUS] = _ptr(c.values), c.status.data_ptr()
            row[_E_OFFSETS] = c.offsets.data_ptr() if c.offsets is not None else 0
            row[_E_AUX] = c.data_bytes if c.kind == _K_TEXT else len(c.dictionary) if c.kind == _K_INDEX else 0
            row[_E_ROW], row[_E_ROWS], row[_E_FLAT] = r0 + k * pr, min(pr, n - k * pr), j * n + k * pr
            row[_E_LEVEL] = -1
            p += 1
    g.flat_n = len(cols) * n
    g.flags = torch.empty(g.flat_n, dtype=torch.uint8, device=dev)
    g.text_bytes = torch.empty(g.flat_n, dtype=torch.int32, device=dev) if any(c.kind == _K_TEXT for c in cols) else None
    device, stream = _queue(dev)
    g.stats = None
    if statistics:                                      # both tables and both results: one copy each way
        plan = _StatsPlan(cols, r0, n, dev)
        m0 = np.zeros((len(g.table), _PM_COLS), dtype=np.int64)
        m0[:, _M_MAXCODE] = -1
        both = _dev_i64(np.concatenate([g.table.ravel(), plan.table.ravel(), m0.ravel(), plan.init.ravel()]), dev)
        a, b = g.table.size, g.table.size + plan.table.size
        with native_errors():
            lib().parquet_encode_measure_raw(both.data_ptr(), len(g.table), 0, len(g.table), pr, g.flags.data_ptr(),
                                             _ptr(g.text_bytes), g.flat_n, both[b:].data_ptr(), device, stream)
        plan.launch(both[a:].data_ptr(), both[b + m0.size:].data_ptr())
        host = both[b:].cpu().numpy()
        g.measure = host[:m0.size].reshape(-1, _PM_COLS)
        g.stats = plan.finish(host[m0.size:].reshape(-1, _SR_COLS))
        return g
    measure = torch.zeros(len(g.table), _PM_COLS, dtype=torch.int64, device=dev)
    measure[:, _M_MAXCODE] = -1
    d_table = _dev_i64(g.table, dev)
    with native_errors():
        lib().parquet_encode_measure_raw(d_table.data_ptr(), len(g.table), 0, len(g.table), pr, g.flags.data_ptr(),
                                         _ptr(g.text_bytes), g.flat_n, measure.data_ptr(), device, stream)
    g.measure = measure.cpu().numpy()
    return g


def _layout_group(g: _Group, invalid, dict_offsets, compressed=False) -> None:
    """The places of everything in the row group's buffer, from the measure table; everything that
    is refused from it is refused here.  ``g.layout``: the table with the dictionary pages added,
    the copy segments, the blob, the buffer's size and, per column, what the footer needs.
    ``g.bodies``: per page in file order ``(column, page type, values, encoding, where its header
    starts, where its body starts, the body's bytes)``, which compression works from."""
    m, cols = g.measure, g.cols
    table = g.table.copy()
    extra, segs, blob, chunks = [], [], bytearray(), []
    pos = 0
    g.bodies = []

    def body_of(j, page_type, values, enc, header, size):
        if compressed and _lz4_bound(size) >= _MAX_BODY:
            raise ValueError(f"column {cols[j].name!r}: a page of {size} bytes, whose LZ4 block may take 2^31 bytes or "
                             f"more; a page holds less than 2^31 (page_rows=)")
        g.bodies.append((j, page_type, values, enc, pos, pos + len(header), size))

    def put(b: bytes):
        nonlocal pos
        if b:
            segs.append((len(blob), pos, len(b)))
            blob.extend(b)
            pos += len(b)

    for j, c in enumerate(cols):
        ps = g.index[j]
        bad, outside = int(m[ps, _M_BAD].sum()), int(m[ps, _M_OUTSIDE].sum())
        if bad and invalid == "error":
            raise ValueError(f"column {c.name!r} has {bad} rows whose status is above 1 (malformed or deferred values); "
                             f"resolve them or pass invalid='null'")
        if outside:
            raise ValueError(f"column {c.name!r} has {outside} codes outside its dictionary of {len(c.dictionary)} entries")
        nulls = g.rows - int(m[ps, _M_VALID].sum())
        if c.required and nulls:
            raise ValueError(f"column {c.name!r} is required and has {nulls} nulls")
        start, dict_off, width, enc = pos, None, c.width, 0
        if c.kind == _K_INDEX:
            top = int(m[ps, _M_MAXCODE].max())
            entries, width, enc = top + 1, max(1, top.bit_length() if top > 0 else 1), 8
            off = dict_offsets(c.dictionary)
            body = int(off[entries] - off[0]) + 4 * entries
            if body >= _MAX_BODY:
                raise ValueError(f"column {c.name!r}: a dictionary page of {body} bytes; a page holds less than 2^31")
            dict_off = pos
            header = _page_header(2, body, entries, 0)
            body_of(j, 2, entries, 0, header, body)
            put(header)
            row = np.zeros(_PE_COLS, dtype=np.int64)
            row[_E_KIND], row[_E_VALUES], row[_E_OFFSETS] = _K_TEXT, c.dictionary._data.data_ptr(), c.dictionary._off.data_ptr()
            row[_E_AUX], row[_E_ROWS], row[_E_LEVEL] = c.dictionary._nbytes, entries, -1
            row[_E_VALOFF], row[_E_VALBYTES] = pos, body
            extra.append(row)
            pos += body
        data_off = pos
        for p in ps:
            rows, valid = int(table[p, _E_ROWS]), int(m[p, _M_VALID])
            lev, lev_bits = b"", 0
            if not c.required:
                if valid == rows:
                    run = _varint(rows << 1) + b"\x01"
                else:
                    lev_bits = (rows + 7) // 8
                    run = _varint((lev_bits << 1) | 1)
                lev = struct.pack("<I", len(run) + lev_bits) + run
            pre = b""
            if c.kind == _K_FIXED:
                vb = valid * c.width
            elif c.kind == _K_BOOL:
                vb = (valid + 7) // 8
            elif c.kind == _K_TEXT:
                vb = int(m[p, _M_TEXT])
            else:
                groups = (valid + 7) // 8
                pre = bytes([width]) + (_varint((groups << 1) | 1) if valid else b"")
                vb = groups * width
            body = len(lev) + lev_bits + len(pre) + vb
            if body >= _MAX_BODY:
                raise ValueError(f"column {c.name!r}: a page of {body} bytes; a page holds less than 2^31 (page_rows=)")
            header = _page_header(0, body, rows, enc)
            body_of(j, 0, rows, enc, header, body)
            put(header + lev)
            table[p, _E_LEVEL] = pos if lev_bits else -1
            pos += lev_bits
            put(pre)
            table[p, _E_WIDTH], table[p, _E_VALOFF], table[p, _E_VALBYTES], table[p, _E_NVALID] = width, pos, vb, valid
            pos += vb
        if pos - start >= _MAX_BODY:
            raise ValueError(f"column {c.name!r}: a chunk of {pos - start} bytes; a chunk holds less than 2^31 "
                             f"(row_group_rows=)")
        chunks.append((dict_off, data_off, pos - start, enc))
    if extra:
        table = np.concatenate([table, np.stack(extra)])
    g.layout = (table, np.array(segs, dtype=np.int64).reshape(-1, 3), bytes(blob), pos, chunks)


def _emit_group(g: _Group):
    """rank and emit: the row group's bytes as one uint8 tensor on the columns' device."""
    import torch
    from ..ops.native import lib, native_errors
    C = lib()
    dev = g.dev
    device, stream = _queue(dev)
    table, segs, blob, out_bytes, _chunks = g.layout
    ncol = len(g.table)
    kinds = table[:, _E_KIND]
    rank = torch.zeros(g.flat_n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(g.flags, 0, dtype=torch.int64, out=rank[1:])
    text_at = None
    if g.text_bytes is not None:
        text_at = torch.zeros(g.flat_n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(g.text_bytes, 0, dtype=torch.int64, out=text_at[1:])
    packed = np.nonzero((kinds[:ncol] == _K_BOOL) | (kinds[:ncol] == _K_INDEX))[0]
    texts = np.nonzero(kinds == _K_TEXT)[0]
    scratch = torch.empty(g.flat_n, dtype=torch.int32, device=dev) if len(packed) else None
    out = torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
    both = _dev_i64(np.concatenate([table.ravel(), segs.ravel()]), dev)
    d_table, d_segs = both[:table.size], both[table.size:]
    d_blob = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    n = len(table)

    def emit(pass_, first, last, largest):
        C.parquet_encode_emit_raw(pass_, d_table.data_ptr(), n, first, last, largest, g.flags.data_ptr(), rank.data_ptr(),
                                  _ptr(text_at), _ptr(scratch), g.flat_n, out.data_ptr(), out_bytes, device, stream)

    with native_errors():
        C.parquet_encode_copy_raw(d_blob.data_ptr(), d_blob.numel(), _ptr(d_segs), len(segs), out.data_ptr(), out_bytes,
                                  device, stream)
        emit(_PASS_ROWS, 0, ncol, int(table[:ncol, _E_ROWS].max()))
        if len(texts):
            emit(_PASS_TEXT, int(texts[0]), n, int(table[texts, _E_ROWS].max()))
        if len(packed):
            emit(_PASS_PACK, int(packed[0]), int(packed[-1]) + 1, int(table[packed, _E_VALBYTES].max()))
    return out


# page, segment and result columns of csrc/lz4_block_host.h
_LB_PAGE_COLS, _LB_SEG_COLS, _LB_RES_COLS = 4, 8, 4
_LB_SIZE, _LB_STATUS = 0, 3
_LB_SEGMENT, _LB_WARM = 32 * 1024, 4096
_COMPRESSIONS = {None: 0, "none": 0, "uncompressed": 0, "lz4_raw": 7, "lz4": 7}


def _lz4_bound(n: int) -> int:
    return n + n // 255 + 16


def _codec(compression) -> int:
    key = compression.lower() if isinstance(compression, str) else compression
    if key not in _COMPRESSIONS:
        raise ValueError(f"compression is None, 'none', 'uncompressed', 'lz4_raw' or 'lz4' (both LZ4_RAW), "
                         f"got {compression!r}")
    return _COMPRESSIONS[key]


def lz4_block_tables(bodies, segment=_LB_SEGMENT):
    """The page and segment tables of ``csrc/lz4_block_host.h`` for page bodies ``(offset, length)``
    of one source buffer, cut at ``segment`` bytes: ``(pages, segs, scratch_bytes)``, the tables as
    int64 numpy arrays.  The segments' scratch areas lie behind the records, each of its LZ4 bound."""
    bodies = [(int(o), int(n)) for o, n in bodies]
    counts = [max(1, -(-n // segment)) for _o, n in bodies]
    nsegs = sum(counts)
    pages = np.zeros((len(bodies), _LB_PAGE_COLS), dtype=np.int64)
    segs = np.zeros((nsegs, _LB_SEG_COLS), dtype=np.int64)
    at, s = (nsegs * 24 + 15) & ~15, 0
    for p, ((off, n), k) in enumerate(zip(bodies, counts)):
        pages[p] = (off, n, s, k)
        for i in range(k):
            b, e = min(n, i * segment), min(n, (i + 1) * segment)
            segs[s, :6] = (p, off, b, e, int(i + 1 == k), at)
            at += (_lz4_bound(e - b) + 15) & ~15
            s += 1
    return pages, segs, at


def _compress_group(g: _Group, staged, segment=_LB_SEGMENT, warm=_LB_WARM):
    """The row group's staged bytes with every page body as one LZ4 block: parse and link over all
    bodies, the second readback (the blocks' sizes), the page headers rebuilt on the host, and the
    merge straight into the final buffer.  Returns ``(buffer, chunks)`` with the chunks' places and
    compressed sizes in that buffer."""
    import torch
    from ..ops.native import lib, native_errors
    C = lib()
    dev = g.dev
    device, stream = _queue(dev)
    bodies = g.bodies
    n = len(bodies)
    pages, segs, scratch_bytes = lz4_block_tables([(b[5], b[6]) for b in bodies], segment)
    both = _dev_i64(np.concatenate([pages.ravel(), segs.ravel()]), dev)
    d_pages, d_segs = both[:pages.size], both[pages.size:]
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    result = torch.zeros(n, _LB_RES_COLS, dtype=torch.int64, device=dev)

    def run(mode, dst, out):
        C.parquet_encode_lz4_raw(mode, _ptr(staged), staged.numel(), d_pages.data_ptr(), n, d_segs.data_ptr(), len(segs),
                                 scratch.data_ptr(), scratch_bytes, result.data_ptr(), _ptr(dst), _ptr(out),
                                 0 if out is None else out.numel(), min(warm, 65535 - segment), segment, device, stream)

    with native_errors():
        run(0, None, None)
    host = result.cpu().numpy()                         # the second and last readback
    if host[:, _LB_STATUS].any() or (host[:, _LB_SIZE] < 1).any():
        p = int(np.nonzero((host[:, _LB_STATUS] != 0) | (host[:, _LB_SIZE] < 1))[0][0])
        raise RuntimeError(f"column {g.cols[bodies[p][0]].name!r}: the LZ4 block of a page of {bodies[p][6]} bytes was "
                           f"refused (status {int(host[p, _LB_STATUS])})")
    sizes = host[:, _LB_SIZE]
    blob, copies, dst = bytearray(), [], np.zeros(n, dtype=np.int64)
    chunks, pos = [], 0
    of_col = {}
    for p, b in enumerate(bodies):
        of_col.setdefault(b[0], []).append(p)
    for j, (_d, _o, _total, enc) in enumerate(g.layout[4]):
        start, dict_off, data_off = pos, None, None
        for p in of_col[j]:
            _col, page_type, values, penc, _h, _b, size = bodies[p]
            if page_type == 2:
                dict_off = pos
            elif data_off is None:
                data_off = pos
            header = _page_header(page_type, size, values, penc, int(sizes[p]))
            copies.append((len(blob), pos, len(header)))
            blob.extend(header)
            dst[p] = pos + len(header)
            pos += len(header) + int(sizes[p])
        if pos - start >= _MAX_BODY:
            raise ValueError(f"column {g.cols[j].name!r}: a chunk of {pos - start} bytes; a chunk holds less than 2^31 "
                             f"(row_group_rows=)")
        chunks.append((dict_off, data_off, pos - start, enc))
    out = torch.zeros(pos, dtype=torch.uint8, device=dev)
    tabs = _dev_i64(np.concatenate([np.array(copies, dtype=np.int64).ravel(), dst]), dev)
    d_blob = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).to(dev)
    with native_errors():
        C.parquet_encode_copy_raw(d_blob.data_ptr(), d_blob.numel(), tabs.data_ptr(), len(copies), out.data_ptr(), pos,
                                  device, stream)
        run(1, tabs[3 * len(copies):], out)
    return out, chunks


class ParquetWriter:
    """Writes :class:`FieldColumns` into one Parquet file, a row group per :meth:`write` call (or
    several, with ``row_group_rows``), encoded where the columns lie: device tensors by the kernels
    of ``csrc/parquet_encode.hip``, CPU tensors by host loops that follow the same rules and give the
    same bytes.  The schema is that of the first call; the footer is written by :meth:`close`, after
    which :attr:`metadata` holds what :func:`parquet_metadata` would read.  See
    :func:`write_parquet_columns` for the format."""

    def __init__(self, fs, path: str, required=(), page_rows=None, invalid="error", write_type=None, statistics=False,
                 compression=None):
        if invalid not in ("error", "null"):
            raise ValueError("invalid is 'error' or 'null'")
        self._codec = _codec(compression)
        if page_rows is not None and int(page_rows) < 1:
            raise ValueError("page_rows is at least 1")
        self.fs, self.path = fs, path
        self.required = (required,) if isinstance(required, str) else tuple(required)
        self.page_rows, self.invalid, self.write_type, self.statistics = page_rows, invalid, write_type, bool(statistics)
        self.metadata = None
        self._schema, self._cols, self._f, self._groups, self._rows, self._closed = None, None, None, [], 0, False
        self._offsets = {}

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *_):
        if exc_type is None:
            self.close()
        else:
            self.abort()

    def _dict_offsets(self, d):
        """The dictionary's offsets on the host, read again only when it has grown."""
        got = self._offsets.get(id(d))
        if got is None or len(got[1]) != len(d) + 1:
            got = (d, d._off[:len(d) + 1].cpu().numpy())
            self._offsets[id(d)] = got
        return got[1]

    def _open(self):
        if self._f is None:
            self._f = self.fs.create_file(self.path, write_type=self.write_type)
            self._f.write(b"PAR1")

    def write(self, columns, row_group_rows=None) -> None:
        """Appends the rows of ``columns`` as one row group (``row_group_rows``: as row groups of
        that many rows).  Everything that is refused is refused before a byte of the call is
        written; a call without rows adds no row group."""
        import torch
        if self._closed:
            raise ValueError("the writer is closed")
        if row_group_rows is not None and int(row_group_rows) < 1:
            raise ValueError("row_group_rows is at least 1")
        cols, dev = _write_columns(columns, self.required)
        schema = [(c.name, c.type) for c in cols]
        if self._schema is not None and schema != self._schema:
            raise ValueError(f"the columns differ from those of the first call: {schema} against {self._schema}")
        rows = columns.rows
        step = rows if row_group_rows is None else int(row_group_rows)
        groups = []
        for r0 in range(0, rows, max(step, 1)):
            g = _measure_group(cols, r0, min(rows, r0 + step), self.page_rows, dev, self.statistics)
            _layout_group(g, self.invalid, self._dict_offsets, bool(self._codec))
            groups.append(g)
        self._schema, self._cols = schema, [(c.name, c.physical, c.kind, c.required) for c in cols]
        self._open()
        for g in groups:
            out, chunks = _emit_group(g), g.layout[4]
            raw = [c[2] for c in chunks]                # the chunks' uncompressed bytes, headers included
            if self._codec:
                out, chunks = _compress_group(g, out)
            if dev.type == "cuda":
                torch.cuda.current_stream(dev).synchronize()
            base = self._f.tell()
            self._f.write(out)
            self._groups.append((g.rows, base, int(out.numel()), chunks, g.stats, raw))
            self._rows += g.rows

    def _footer(self) -> bytes:
        t = _ThriftOut()
        t.struct()
        t.i32(1, 2)
        t.list_(2, 12, len(self._cols) + 1)
        t.struct()
        t.binary(4, b"schema")
        t.i32(5, len(self._cols))
        t.end()
        for name, physical, _kind, required in self._cols:
            t.struct()
            t.i32(1, PHYSICAL.index(physical))
            t.i32(3, 0 if required else 1)
            t.binary(4, name.encode())
            if physical == "BYTE_ARRAY":
                t.i32(6, 0)                             # UTF8
                t.struct(10)                            # LogicalType: STRING
                t.struct(1)
                t.end()
                t.end()
            t.end()
        t.i64(3, self._rows)
        t.list_(4, 12, len(self._groups))
        for rows, base, size, chunks, stats, raw in self._groups:
            t.struct()
            t.list_(1, 12, len(chunks))
            for j, ((name, physical, kind, required), (dict_off, data_off, total, enc)) in enumerate(zip(self._cols, chunks)):
                t.struct()
                t.i64(2, base + (data_off if dict_off is None else dict_off))
                t.struct(3)
                t.i32(1, PHYSICAL.index(physical))
                encs = sorted({0, enc} | (set() if required else {3}))
                t.list_(2, 5, len(encs))
                for e in encs:
                    t.b += _varint(e << 1)
                t.list_(3, 8, 1)
                t.b += _varint(len(name.encode())) + name.encode()
                t.i32(4, self._codec)
                t.i64(5, rows)
                t.i64(6, raw[j])
                t.i64(7, total)
                t.i64(9, base + data_off)
                if dict_off is not None:
                    t.i64(11, base + dict_off)
                if stats is not None:                   # Statistics: null_count, max_value, min_value
                    nulls, lo, hi = stats[j]
                    t.struct(12)
                    t.i64(3, nulls)
                    if lo is not None:
                        t.binary(5, hi)
                        t.binary(6, lo)
                    t.end()
                t.end()
                t.end()
            t.i64(2, sum(raw))
            t.i64(3, rows)
            t.i64(5, base)
            t.i64(6, size)
            t.end()
        t.binary(6, CREATED_BY.encode())
        if self.statistics:                             # column_orders: TypeDefinedOrder for every leaf
            t.list_(7, 12, len(self._cols))
            for _ in self._cols:
                t.struct()
                t.struct(1)
                t.end()
                t.end()
        t.end()
        return bytes(t.b)

    def close(self) -> None:
        """Writes the footer and completes the file.  A writer that was given no columns has no
        schema and writes nothing."""
        if self._closed:
            return
        self._closed = True
        if self._schema is None:
            return
        self._open()
        footer = self._footer()
        self._f.write(footer + struct.pack("<I", len(footer)) + b"PAR1")
        self._f.close()
        leaves = [ParquetLeaf(name, physical, "REQUIRED" if required else "OPTIONAL", 0 if required else 1, 0, None)
                  for name, physical, _kind, required in self._cols]

        def read_back(physical, st):                    # what parquet_metadata makes of the bytes in the footer
            return None if st is None else ParquetStatistics(st[0], _stat_value(physical, st[1]), _stat_value(physical, st[2]))

        groups = [ParquetRowGroup(rows, [ParquetChunk(name, physical, CODECS[self._codec], rows,
                                                      None if d is None else base + d, base + o, total,
                                                      read_back(physical, stats and stats[j]))
                                         for j, ((name, physical, _k, _r), (d, o, total, _e))
                                         in enumerate(zip(self._cols, chunks))])
                  for rows, base, _size, chunks, stats, _raw in self._groups]
        self.metadata = ParquetMetadata(self._rows, leaves, groups, CREATED_BY)

    def abort(self) -> None:
        """Gives the file up: what was written is dropped and the path does not exist."""
        self._closed = True
        if self._f is not None:
            self._f.cancel()
            self._f = None


def write_parquet_columns(fs, path: str, columns, row_group_rows=None, page_rows=None, required=(), invalid="error",
                          write_type=None, statistics=False, compression=None) -> ParquetMetadata:
    """Writes ``columns`` (a :class:`FieldColumns` on a GPU or on the CPU) as the Parquet file
    ``path`` and returns its metadata.  The pages are encoded where the columns lie and each row
    group's bytes go to the output stream as one tensor on that device.

    ``row_group_rows`` cuts the rows into row groups (``None``: one), ``page_rows`` a chunk into data
    pages (``None``: one).  ``int64`` / ``int32`` / ``float64`` / ``float32`` columns become PLAIN
    INT64 / INT32 / DOUBLE / FLOAT, ``bool`` PLAIN BOOLEAN, ``text`` PLAIN BYTE_ARRAY (STRING) and
    ``category`` dictionary-coded BYTE_ARRAY (STRING): per chunk a PLAIN dictionary page with the
    dictionary's entries up to the largest code that the row group uses, and RLE_DICTIONARY data
    pages of one bit-packed run.  Columns are OPTIONAL (status 1 is a null; definition levels are one
    RLE run for a page without nulls, else one bit-packed run) unless named in ``required``.  Data
    pages are V1.

    ``compression``: ``None``, ``"none"`` or ``"uncompressed"`` write the pages as they are;
    ``"lz4_raw"`` or ``"lz4"`` (pyarrow's name for codec 7) write every page body, dictionary pages
    included, as one LZ4 block (codec LZ4_RAW), compressed where the columns lie; any other value is
    a ``ValueError`` before the file is created.  A body is cut into segments of 32 KiB that are
    parsed independently and stitched into one standard block (``csrc/lz4_block_host.h``), so the
    blocks are a little larger than a serial encoder's and, on a device, need not be the same
    bytes from run to run; what they decode to is.  An empty body is the one-byte block ``00``.  In
    the footer ``total_uncompressed_size`` is what the chunk takes without compression and
    ``total_compressed_size`` what it takes in the file.

    Refused before the file is created: a ``span`` column (``TypeError``); a status above 1, a
    deferred float included, unless ``invalid="null"`` writes such rows as nulls; a null in a
    required column; a live code outside its dictionary; a page or chunk of 2^31 bytes or more (all
    ``ValueError``); with compression, a page whose LZ4 bound reaches 2^31.

    ``statistics=True`` adds a ``Statistics`` struct to every column chunk (``null_count``, and
    ``min_value`` / ``max_value`` where :func:`column_statistics` gives bounds: PLAIN-encoded, so a
    text bound has no length prefix and a boolean is one byte) and ``column_orders`` to the footer,
    so that other readers can skip row groups; page headers carry none.  A chunk with a text value
    (or a used dictionary entry) of more than 64 bytes has a null count and no bounds.  The default
    writes exactly the file that was written before there were statistics.

    Per row group: one measure launch and one small readback (the sizes of the pages, which the
    host needs for the page headers), two ``torch.cumsum`` and up to four emit launches, however many
    columns there are; a category column's dictionary offsets are read once more when it has grown.
    With statistics: one more launch for numbers alone, ten with a text column and eleven with a
    category column (``csrc/parquet_stats.hip``), queued behind the measure launch, and their results
    come back in that one readback.  With compression the row group is emitted into a staging
    tensor and four more launches follow, however many pages and columns: parse and link, a second
    small readback (the blocks' sizes, for the page headers), the copy of the rebuilt headers and
    the merge of every block into its final place."""
    w = ParquetWriter(fs, path, required=required, page_rows=page_rows, invalid=invalid, write_type=write_type,
                      statistics=statistics, compression=compression)
    try:
        w.write(columns, row_group_rows)
        w.close()
    except BaseException:
        w.abort()
        raise
    return w.metadata
