"""Typed columns from batches of JSON Lines: what :mod:`.fields` does for CSV/TSV, for rows that are
JSON objects.  :func:`parse_json_fields` finds the values of the requested top-level keys in every
row of a :class:`RaggedBatch` where it lies (one kernel for a device batch, a C++ loop for a host
batch) and types them into tensors; :func:`unescape_json_text` undoes JSON string escapes into
packed bytes; :func:`read_json_columns` does both for a whole file.

The rule (``csrc/json_fields_host.h`` and ``csrc/json_text_host.h`` have it in full) is the record
structure of well-formed files, the same stance ``build_delimited_index(quote=)`` takes.  It is not
a JSON validator.  A row must be one object: its first non-whitespace byte is ``{``, the depth
first returns to 0 at a ``}`` and only whitespace follows; any other row has status 2 in every
column, a blank row status 1.  A member's key is compared byte for byte with ``"`` + the requested
name + ``"``, so a key written in the file with an escape sequence (``"caf\\u00e9"``) is never
matched; request keys as the file spells them.  When a key occurs more than once the last
occurrence wins, as with ``json.loads``; a key that no member has gives status 1, as does the value
``null``.

Column types are those of :func:`.fields.parse_fields` plus ``"bool"`` (``true`` / ``false``, a
``torch.bool`` tensor).  ``"span"`` is the value's bytes as they stand (a string with its quotes, a
nested object or array raw).  Integers must match ``-?(0|[1-9][0-9]*)`` and floats
``-?(0|[1-9][0-9]*)(\\.[0-9]+)?([eE][+-]?[0-9]+)?``: ``1.0`` is no integer, and ``NaN``,
``Infinity``, ``+1``, ``01``, ``1.`` and ``.5`` are malformed (status 2), which is stricter than
``json.loads``' defaults.  Floats outside the device's exact fast path are deferred and resolved on
the host with ``float()`` exactly as in the CSV path.  ``"text"`` and ``"category"`` take a JSON
string and hold its unescaped content: ``\\" \\\\ \\/ \\b \\f \\n \\r \\t`` and ``\\uXXXX`` (a
surrogate pair becomes one 4-byte sequence, a lone surrogate its 3-byte generalised encoding, which
is ``json.loads(...).encode("utf-8", "surrogatepass")``); any other escape makes the value
malformed.  Bytes that are not part of an escape are copied unchanged: there is no UTF-8
validation, and raw control bytes pass through.  Unlike CSV, JSON tells ``""`` (status 0, length 0)
from ``null`` (status 1).
"""
from __future__ import annotations

import numpy as np

from . import fields as _f
from .dataset import DeviceBatchLoader, IndexedRecordDataset, RaggedBatch, build_delimited_index
from .fields import (BOOL, CATEGORY, FLOAT32, FLOAT64, INT32, INT64, SPAN, TEXT, Column, FieldColumns,
                     _category_dictionaries, _one_byte, _queue, extract_text)

_TYPES = dict(_f._TYPES, bool=BOOL)
_MAX_COLS = 32
_RAW_BOOL, _RAW_STRING = 5, 6


def _type_code(dtype) -> int:
    name = dtype.__name__ if isinstance(dtype, type) else str(dtype).replace("torch.", "")
    try:
        return _TYPES[name]
    except KeyError:
        raise ValueError(f"unknown column type {dtype!r}: one of span, text, category, int64, int32, float64, "
                         f"float32, bool") from None


def _key_bytes(key) -> bytes:
    if not isinstance(key, str):
        raise TypeError(f"a key is a str, got {key!r}")
    try:
        b = key.encode("utf-8")
    except UnicodeEncodeError:
        raise ValueError(f"the key {key!r} is not valid UTF-8 text") from None
    if not 1 <= len(b) <= 255:
        raise ValueError(f"a key is 1 to 255 bytes of UTF-8, got {len(b)}")
    if any(c < 0x20 or c in (0x22, 0x5C) for c in b):
        raise ValueError(f"the key {key!r} holds a quote, a backslash or a control byte: keys are matched as the "
                         f"file spells them, and such a key is spelled with an escape there")
    return b


def _column_list(columns):
    """[(name or None, key, type code)]."""
    items = list(columns.items()) if isinstance(columns, dict) else [(None, spec) for spec in columns]
    out = []
    for name, spec in items:
        key, dtype = spec
        _key_bytes(key)
        out.append((name, key, _type_code(dtype)))
    return out


def _alloc(type_, n, device):
    import torch
    dt = {SPAN: torch.int64, TEXT: torch.int64, CATEGORY: torch.int64, INT64: torch.int64, INT32: torch.int32,
          FLOAT64: torch.float64, FLOAT32: torch.float32, BOOL: torch.bool}[type_]
    values = torch.empty(n, dtype=dt, device=device)
    length = torch.empty(n, dtype=torch.int32, device=device) if type_ in (SPAN, TEXT, CATEGORY) else None
    return values, length, torch.empty(n, dtype=torch.uint8, device=device)


def _launch(data, off, ln, specs, term):
    """One native call for up to 32 columns; returns the Column objects.  A text or category column
    is located as the span of the string's content here; :func:`_fill_text` unescapes it."""
    import torch
    from ..ops.native import lib, native_errors
    n = int(ln.numel())
    dev = data.device
    keys = [_key_bytes(k) for _, k, _t in specs]
    names = torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(dev)
    cols, raw, at = [], [], 0
    for (name, k, t), kb in zip(specs, keys):
        values, length, status = _alloc(t, n, dev)
        cols.append(Column(name, k, t, values, length, status))
        rt = _RAW_STRING if t in (TEXT, CATEGORY) else _RAW_BOOL if t == BOOL else t
        raw.append((at, len(kb), rt, values.data_ptr(), length.data_ptr() if length is not None else 0,
                    status.data_ptr()))
        at += len(kb)
    device, stream = _queue(dev)
    with native_errors():
        lib().json_fields_raw(data.data_ptr(), data.numel(), off.data_ptr(), ln.data_ptr(), ln.dtype == torch.int64, n,
                              device, names.data_ptr(), names.numel(), raw, term, stream)
    return cols


def _resolve(data, off, ln, cols, term):
    """Deferred floats, as in the CSV path: one small readback tells whether there are any; then
    only the bytes of those values travel to the host, ``float()`` parses them and value and status
    0 go back."""
    import torch
    floats = [c for c in cols if c.type in (FLOAT64, FLOAT32)]
    if not floats or floats[0].status.numel() == 0:
        return
    flags = torch.stack([(c.status == 3).any() for c in floats]).cpu().tolist()
    todo = [c for c, f in zip(floats, flags) if f]
    for i in range(0, len(todo), _MAX_COLS):
        group = todo[i:i + _MAX_COLS]
        spans = _launch(data, off, ln, [(None, c.field, SPAN) for c in group], term)
        for c, s in zip(group, spans):
            rows = torch.nonzero(c.status == 3).view(-1)
            got = extract_text(data, s.start[rows], s.length[rows])
            text, cuts = got.data.cpu().numpy().tobytes(), got.offsets.cpu().numpy()
            vals = np.array([float(text[cuts[j]:cuts[j + 1]]) for j in range(len(cuts) - 1)], dtype=np.float64)
            if c.type == FLOAT32:
                with np.errstate(over="ignore"):
                    vals = vals.astype(np.float32)
            c.values[rows] = torch.from_numpy(vals).to(c.values.device)
            c.status[rows] = 0


def _text_passes(flat, spans):
    """measure, cumsum, one readback of all totals, emit: [(data, offsets, lengths, status)] for the
    spans [(start int64, length int32, status uint8 or None)] into the flat uint8 ``flat``."""
    import torch
    from ..ops.native import lib, native_errors
    dev = flat.device
    device, stream = _queue(dev)
    measured = []
    with native_errors():
        for start, length, status in spans:
            n = int(start.numel())
            out_len = torch.empty(n, dtype=torch.int32, device=dev)
            out_status = torch.empty(n, dtype=torch.uint8, device=dev)
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            lib().json_text_measure_raw(flat.data_ptr(), flat.numel(), start.data_ptr(), length.data_ptr(),
                                        status.data_ptr() if status is not None else 0, n, device, out_len.data_ptr(),
                                        out_status.data_ptr(), stream)
            if n:
                torch.cumsum(out_len, 0, dtype=torch.int64, out=offsets[1:])
            measured.append((out_len, out_status, offsets))
        if not measured:
            return []
        totals = torch.stack([o[-1] for _, _, o in measured]).cpu().tolist()
        out = []
        for (start, length, _status), (out_len, out_status, offsets), total in zip(spans, measured, totals):
            packed = torch.empty(int(total), dtype=torch.uint8, device=dev)
            lib().json_text_emit_raw(flat.data_ptr(), flat.numel(), start.data_ptr(), length.data_ptr(),
                                     out_status.data_ptr(), int(start.numel()), device, offsets.data_ptr(),
                                     packed.data_ptr(), packed.numel(), stream)
            out.append((packed, offsets, out_len, out_status))
    return out


def unescape_json_text(data, start, length, status=None):
    """The JSON string contents ``data[start[r]:start[r] + length[r]]`` (without their quotes) of a
    flat uint8 tensor, unescaped and packed end to end on the device of ``data`` (a GPU or the
    CPU): ``(RaggedBatch(data, offsets, lengths), status)`` with ``offsets`` of ``len(start) + 1``
    entries.  ``status`` is 0 for a good value, 2 for one with a bad escape (an unknown code, a
    ``\\u`` without four hex digits, a backslash as the last byte) or outside ``data``, and the
    given status where that is not 0; every value whose status is not 0 has length 0.

    Two launches (measure, emit) around a ``torch.cumsum`` on torch's current stream, and one small
    readback, the total size, to allocate the output."""
    import torch
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8:
        raise ValueError("unescape_json_text takes uint8 data")
    dev = data.device
    flat = (data if data.is_contiguous() else data.contiguous()).view(-1)
    start = torch.as_tensor(start).to(device=dev, dtype=torch.int64).contiguous().view(-1)
    length = torch.as_tensor(length).to(dev).view(-1)
    if length.dtype != torch.int32:
        length = length.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    length = length.contiguous()
    if length.numel() != start.numel():
        raise ValueError("start and length differ in size")
    if status is not None:
        status = torch.as_tensor(status).to(device=dev, dtype=torch.uint8).contiguous().view(-1)
        if status.numel() != start.numel():
            raise ValueError("start and status differ in size")
    ((packed, offsets, out_len, out_status),) = _text_passes(flat, [(start, length, status)])
    return RaggedBatch(packed, offsets, out_len), out_status


def _fill_text(data, cols):
    """The text and category columns of a call: the spans of their strings become unescaped packed
    bytes; one readback for all of them.  The status is the locate status, and 2 where a bad escape
    was found.  A category column's bytes are then encoded by its dictionary and dropped."""
    todo = [c for c in cols if c.type in (TEXT, CATEGORY)]
    if not todo:
        return
    got = _text_passes(data.view(-1), [(c.start, c.length, c.status) for c in todo])
    for c, (packed, offsets, out_len, out_status) in zip(todo, got):
        c.status = out_status
        if c.type == CATEGORY:
            c.values = c.dictionary.encode(RaggedBatch(packed, offsets, out_len), c.status)
            c.start = c.length = None
            continue
        c.data, c.offsets, c.length, c.start = packed, offsets, out_len, None


def parse_json_fields(batch, columns, terminator=b"\n", resolve_deferred=True, dictionaries=None) -> FieldColumns:
    """The values of the requested top-level keys of every row of ``batch`` (a uint8
    :class:`RaggedBatch` of JSON Lines rows, packed or padded, on a device or on the CPU) as tensors
    on the batch's device.

    ``columns``: a list of ``(key, type)`` or a dict ``name -> (key, type)``; ``key`` is a ``str``
    of 1 to 255 UTF-8 bytes without ``"``, ``\\`` or control characters (``ValueError``), and the
    same key may be requested several times with different types.  More than 32 columns are handled
    in groups of 32.  A ``Column``'s ``field`` is its key here.

    Stream and readbacks are those of :func:`.fields.parse_fields`: everything runs on torch's
    current stream and is not waited for, except one small readback for deferred floats
    (``resolve_deferred=False`` leaves them NaN with status 3), one for the total sizes of all text
    columns, and one per category encode.  ``dictionaries`` is as in ``parse_fields``."""
    import torch
    data, off, ln = batch
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8:
        raise ValueError("parse_json_fields takes a uint8 batch")
    specs = _column_list(columns)
    if not specs:
        raise ValueError("at least one column is required")
    t = _one_byte(terminator, "terminator")
    dev = data.device
    data = data if data.is_contiguous() else data.contiguous()
    n = int(ln.numel())
    off = off.to(device=dev, dtype=torch.int64)[:n].contiguous()
    if ln.dtype not in (torch.int32, torch.int64):
        ln = ln.to(torch.int64)
    ln = ln.to(dev).contiguous()
    dicts = _category_dictionaries(specs, dictionaries, dev)
    cols = []
    for i in range(0, len(specs), _MAX_COLS):
        cols += _launch(data, off, ln, specs[i:i + _MAX_COLS], t)
    for j, d in dicts.items():
        cols[j].dictionary = d
    if resolve_deferred:
        _resolve(data, off, ln, cols, t)
    _fill_text(data, cols)
    return FieldColumns(cols)


def read_json_columns(fs, path: str, columns, delimiter=b"\n", skip_rows: int = 0, batch_size: int = 65536,
                      device=None, device_plan="auto", dictionaries=None) -> FieldColumns:
    """The requested columns of a whole JSON Lines file, concatenated over an unshuffled
    :class:`DeviceBatchLoader` of ``batch_size`` rows.  The record index needs no quote: a JSON
    string cannot hold a raw line break.  As in :func:`.fields.read_delimited_columns`, the
    ``start`` of a span column is an offset into the file, a text column is one packed column for
    the file and a category column has one dictionary for the file (the caller's, through
    ``dictionaries``, or a fresh one).  ``skip_rows`` drops leading records."""
    if skip_rows < 0:
        raise ValueError("skip_rows counts rows")
    _one_byte(delimiter, "delimiter")
    named = isinstance(columns, dict)
    specs = _column_list(columns)
    index = build_delimited_index(fs, path, delimiter, device_plan=device_plan)
    index = index[min(int(skip_rows), len(index) - 1):]
    ds = IndexedRecordDataset(fs, path, index=index, device=device)
    parts = []
    with DeviceBatchLoader(ds, batch_size=batch_size, device=device, align=1, device_plan=device_plan) as dl:
        import torch
        file_off = torch.from_numpy(np.ascontiguousarray(index[:-1])).to(dl.device)
        dicts = _category_dictionaries(specs, dictionaries, dl.device)
        dicts = {specs[j][0] if named else j: d for j, d in dicts.items()}
        done = 0
        for batch in dl:
            got = parse_json_fields(batch, columns, delimiter, dictionaries=dicts)
            n = got.rows
            for c in got:
                if c.type == SPAN:                      # batch offsets -> file offsets
                    rel = c.start - batch.offsets[:n].to(torch.int64) + file_off[done:done + n]
                    c.start = torch.where(c.status == 0, rel, torch.zeros_like(rel))
            done += n
            parts.append(got)
        if not parts:
            empty = RaggedBatch(torch.empty(0, dtype=torch.uint8, device=dl.device),
                                torch.zeros(1, dtype=torch.int64, device=dl.device),
                                torch.empty(0, dtype=torch.int64, device=dl.device))
            parts.append(parse_json_fields(empty, columns, delimiter, dictionaries=dicts))
    return FieldColumns.concat(parts)
