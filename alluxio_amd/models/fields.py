"""Typed columns from batches of delimited text: the step after ``IndexedRecordDataset.from_delimited``
and ``DeviceBatchLoader``, which deliver each CSV/TSV row as raw bytes.  :func:`parse_fields` splits
the rows of a :class:`RaggedBatch` where it lies (one kernel for a device batch, a C++ loop for a
host batch) and parses the requested fields into tensors; :func:`read_delimited_columns` does so
for a whole file.

The rule (``csrc/field_parse_host.h`` has it in full): a row is its bytes without the terminator
(and without the ``\\r`` before a ``\\n``); a separator splits where an even number of quote bytes
precedes it in the row; a field loses one pair of enclosing quotes, then blanks and tabs at both
ends.  Doubled quotes inside stay as they are: a ``span`` column returns them raw and a numeric
column calls them malformed; a ``text`` column undoes them (:func:`extract_text`).

Column types: ``"span"`` (``start`` into the batch's flat data and ``length``), ``"text"`` (the
unquoted bytes of all values packed into ``data``, with ``offsets`` and ``length``), ``"int64"``,
``"int32"``, ``"float64"``, ``"float32"``.  Status per value: 0 valid, 1 no value (field absent
or empty), 2 malformed or out of range, 3 deferred.  The device parses a float itself only where
one correctly rounded fp64 operation is exact (at most 19 significant digits, mantissa at most
2^53, decimal exponent within +-22); every other well-formed float is deferred and resolved on
the host with ``float()``, so every float64 equals ``float(text)`` bit for bit.  ``float32`` is
that float64 converted to float32: two roundings by definition, not ``numpy.float32(text)``.

``"category"`` (alias ``"dict"``) is a text column turned into int32 codes by a
:class:`TextDictionary` on the device: the code of a value is the number of distinct values seen
before its first occurrence, ``-1`` where the status is not 0, and the dictionary persists across
batches, files and calls.
"""
from __future__ import annotations

import numpy as np

from .dataset import DeviceBatchLoader, IndexedRecordDataset, RaggedBatch, build_delimited_index

SPAN, INT64, INT32, FLOAT64, FLOAT32, TEXT, CATEGORY = range(7)
_TYPES = {"span": SPAN, "int64": INT64, "int32": INT32, "float64": FLOAT64, "float32": FLOAT32, "text": TEXT,
          "category": CATEGORY, "int": INT64, "float": FLOAT64, "str": SPAN, "bytes": TEXT, "dict": CATEGORY}
BOOL = 7                                                # JSON columns only (json_fields.py)
_MAX_COLS = 32


def _type_code(dtype) -> int:
    # a name, a torch / numpy dtype (torch.int64, np.float32) or one of int, float, str, bytes
    name = dtype.__name__ if isinstance(dtype, type) else str(dtype).replace("torch.", "")
    try:
        return _TYPES[name]
    except KeyError:
        raise ValueError(f"unknown column type {dtype!r}: one of span, text, category, int64, int32, float64, "
                         f"float32") from None


def _one_byte(x, what: str) -> int:
    b = x.encode() if isinstance(x, str) else bytes(x)
    if len(b) != 1:
        raise ValueError(f"the {what} must be exactly one byte, got {len(b)}")
    return b[0]


def _scalars(sep, quote, terminator):
    s, t = _one_byte(sep, "separator"), _one_byte(terminator, "terminator")
    q = -1 if quote is None else _one_byte(quote, "quote")
    if s == t or q in (s, t):
        raise ValueError("separator, quote and terminator must differ")
    return s, q, t


class Column:
    """One parsed column: ``values`` and ``status``; a span column has ``start`` and ``length``
    instead of ``values``; a text column has ``data`` (the bytes of all values, packed), ``offsets``
    (rows + 1: value r is ``data[offsets[r]:offsets[r + 1]]``) and ``length``; a category column has
    int32 codes in ``values`` (-1 where the status is not 0) and the :class:`TextDictionary` they
    index in ``dictionary``."""

    __slots__ = ("name", "field", "type", "values", "start", "length", "status", "data", "offsets", "dictionary")

    def __init__(self, name, field, type_, values, length, status, data=None, offsets=None, dictionary=None):
        self.name, self.field, self.type = name, field, type_
        self.status = status
        self.data, self.offsets, self.dictionary = data, offsets, dictionary
        if type_ == SPAN:
            self.values, self.start, self.length = None, values, length
        elif type_ == TEXT or (type_ == CATEGORY and length is not None):
            # values: the span's start until the text is extracted (and, for a category, encoded)
            self.values, self.start, self.length = None, values, length
        else:
            self.values, self.start, self.length = values, None, None

    def _tensors(self):
        if self.type == TEXT:
            return (self.data, self.offsets, self.length, self.status)
        return (self.start, self.length, self.status) if self.type == SPAN else (self.values, self.status)

    def tolist(self) -> list:
        """The column on the host, ``None`` where the status is not 0: ``bytes`` for a text column
        (one device-to-host copy for the whole column), numbers for a numeric one, codes for a
        category, ``(start, length)`` for a span."""
        import torch
        if self.type == TEXT:
            n, nb = int(self.status.numel()), int(self.data.numel())
            blob = torch.cat([self.data, self.offsets.view(torch.uint8), self.status]).cpu().numpy()
            cuts = blob[nb:nb + 8 * (n + 1)].view(np.int64).tolist()
            text, st = blob[:nb].tobytes(), blob[nb + 8 * (n + 1):].tolist()
            return [text[cuts[r]:cuts[r + 1]] if st[r] == 0 else None for r in range(n)]
        st = self.status.cpu().tolist()
        if self.type == SPAN:
            vals = list(zip(self.start.cpu().tolist(), self.length.cpu().tolist()))
        else:
            vals = self.values.cpu().tolist()
        return [v if s == 0 else None for v, s in zip(vals, st)]

    def __repr__(self):
        kind = "bool" if self.type == BOOL else [k for k, v in _TYPES.items() if v == self.type][0]
        return f"Column({self.name!r}, field={self.field!r}, {kind}, rows={len(self.status)})"


class FieldColumns:
    """The columns of one :func:`parse_fields` call, by position or by name."""

    def __init__(self, columns):
        self._cols = list(columns)
        self._by_name = {c.name: c for c in self._cols if c.name is not None}

    def __getitem__(self, key):
        if isinstance(key, str):
            return self._by_name[key]
        return self._cols[key]

    def __len__(self):
        return len(self._cols)

    def __iter__(self):
        return iter(self._cols)

    @property
    def names(self):
        return [c.name for c in self._cols]

    @property
    def rows(self) -> int:
        return len(self._cols[0].status) if self._cols else 0

    @staticmethod
    def concat(parts):
        """Row-wise concatenation of the results of several calls with the same columns.  Span
        starts stay relative to each part's own batch; a text column's ``data`` is joined and its
        ``offsets`` are rebased, so the result is one packed column."""
        import torch
        parts = list(parts)
        cols = []
        for j, c in enumerate(parts[0]):
            if c.type == CATEGORY:
                if any(p[j].dictionary is not c.dictionary for p in parts):
                    raise ValueError(f"category column {c.name if c.name is not None else j}: the parts were encoded "
                                     f"with different dictionaries, so their codes cannot be joined; pass one "
                                     f"dictionary to every call (dictionaries=)")
                cols.append(Column(c.name, c.field, CATEGORY, torch.cat([p[j].values for p in parts]), None,
                                   torch.cat([p[j].status for p in parts]), dictionary=c.dictionary))
                continue
            if c.type == TEXT:
                base, offs = 0, []
                for p in parts:                         # the sizes are known on the host: no readback
                    offs.append(p[j].offsets[:-1] + base)
                    base += int(p[j].data.numel())
                offs.append(torch.full((1,), base, dtype=torch.int64, device=c.offsets.device))
                cols.append(Column(c.name, c.field, TEXT, None, torch.cat([p[j].length for p in parts]),
                                   torch.cat([p[j].status for p in parts]), torch.cat([p[j].data for p in parts]),
                                   torch.cat(offs)))
                continue
            ts = [torch.cat([p[j]._tensors()[i] for p in parts]) for i in range(len(c._tensors()))]
            if c.type == SPAN:
                cols.append(Column(c.name, c.field, c.type, ts[0], ts[1], ts[2]))
            else:
                cols.append(Column(c.name, c.field, c.type, ts[0], None, ts[1]))
        return FieldColumns(cols)


def _column_list(columns):
    """[(name or None, field number, type code)]."""
    if isinstance(columns, dict):
        items = [(name, spec) for name, spec in columns.items()]
    else:
        items = [(None, spec) for spec in columns]
    out = []
    for name, spec in items:
        k, dtype = spec
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"a field number is an integer, got {k!r}")
        if k < 0:
            raise ValueError("field numbers count from 0")
        out.append((name, int(k), _type_code(dtype)))
    return out


def _alloc(type_, n, device):
    import torch
    dt = {SPAN: torch.int64, TEXT: torch.int64, CATEGORY: torch.int64, INT64: torch.int64, INT32: torch.int32, FLOAT64: torch.float64,
          FLOAT32: torch.float32}[type_]
    values = torch.empty(n, dtype=dt, device=device)
    length = torch.empty(n, dtype=torch.int32, device=device) if type_ in (SPAN, TEXT, CATEGORY) else None
    return values, length, torch.empty(n, dtype=torch.uint8, device=device)


def _queue(dev):
    """(device number or -1 for the host, torch's current stream on it) for a native call."""
    import torch
    if dev.type == "cuda":
        return dev.index if dev.index is not None else torch.cuda.current_device(), \
            int(torch.cuda.current_stream(dev).cuda_stream)
    return -1, 0


def _launch(data, off, ln, specs, sep, quote, term):
    """One native call for up to 32 columns; returns the Column objects.  A text or category column
    is located as a span here; :func:`_fill_text` extracts it."""
    import torch
    from ..ops.native import lib, native_errors
    n = int(ln.numel())
    dev = data.device
    cols, raw = [], []
    for name, k, t in specs:
        values, length, status = _alloc(t, n, dev)
        cols.append(Column(name, k, t, values, length, status))
        raw.append((k, SPAN if t in (TEXT, CATEGORY) else t, values.data_ptr(), length.data_ptr() if length is not None else 0,
                    status.data_ptr()))
    device, stream = _queue(dev)
    with native_errors():
        lib().field_parse_raw(data.data_ptr(), data.numel(), off.data_ptr(), ln.data_ptr(), ln.dtype == torch.int64, n,
                              device, raw, sep, quote, term, stream)
    return cols


def _resolve(data, off, ln, cols, sep, quote, term):
    """Deferred floats: one small readback tells whether there are any; then only the bytes of
    those fields travel to the host, ``float()`` parses them and value and status 0 go back."""
    import torch
    floats = [c for c in cols if c.type in (FLOAT64, FLOAT32)]
    if not floats or floats[0].status.numel() == 0:
        return
    flags = torch.stack([(c.status == 3).any() for c in floats]).cpu().tolist()
    todo = [c for c, f in zip(floats, flags) if f]
    for i in range(0, len(todo), _MAX_COLS):
        group = todo[i:i + _MAX_COLS]
        spans = _launch(data, off, ln, [(None, c.field, SPAN) for c in group], sep, quote, term)
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


def _text_passes(flat, spans, quote):
    """measure, cumsum, one readback of all totals, emit: [(data, offsets, lengths)] for the spans
    [(start int64, length int32, status uint8 or None)] into the flat uint8 ``flat``."""
    import torch
    from ..ops.native import lib, native_errors
    dev = flat.device
    device, stream = _queue(dev)
    measured = []
    with native_errors():
        for start, length, status in spans:
            n = int(start.numel())
            out_len = torch.empty(n, dtype=torch.int32, device=dev)
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
            lib().text_measure_raw(flat.data_ptr(), flat.numel(), start.data_ptr(), length.data_ptr(),
                                   status.data_ptr() if status is not None else 0, n, device, quote, out_len.data_ptr(),
                                   stream)
            if n:
                torch.cumsum(out_len, 0, dtype=torch.int64, out=offsets[1:])
            measured.append((out_len, offsets))
        if not measured:
            return []
        totals = torch.stack([o[-1] for _, o in measured]).cpu().tolist()
        out = []
        for (start, length, status), (out_len, offsets), total in zip(spans, measured, totals):
            packed = torch.empty(int(total), dtype=torch.uint8, device=dev)
            lib().text_emit_raw(flat.data_ptr(), flat.numel(), start.data_ptr(), length.data_ptr(),
                                status.data_ptr() if status is not None else 0, int(start.numel()), device, quote,
                                offsets.data_ptr(), packed.data_ptr(), packed.numel(), stream)
            out.append((packed, offsets, out_len))
    return out


def extract_text(data, start, length, status=None, quote=None) -> RaggedBatch:
    """The values ``data[start[r]:start[r] + length[r]]`` of a flat uint8 tensor, packed end to end
    on the device of ``data`` (a GPU or the CPU): ``RaggedBatch(data, offsets, lengths)`` with
    ``offsets`` of ``len(start) + 1`` entries.  ``start``, ``length`` and ``status`` are what a
    ``span`` column holds (lengths are int32).

    With ``quote`` every doubled quote becomes one (a run of k quote bytes becomes ceil(k / 2)),
    which is ``value.replace(quote * 2, quote)``: the reading of well-formed files.  The rule is
    applied to the content whether or not the field was enclosed in quotes, and a lone quote is
    kept and is not an error.  ``quote=None`` copies the bytes unchanged.  A value whose status is
    not 0, or that does not lie inside ``data``, has length 0 and is not read.

    Two launches (measure, emit) around a ``torch.cumsum`` on torch's current stream, and one small
    readback, the total size, to allocate the output."""
    import torch
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8:
        raise ValueError("extract_text takes uint8 data")
    q = -1 if quote is None else _one_byte(quote, "quote")
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
    (got,) = _text_passes(flat, [(start, length, status)], q)
    return RaggedBatch(*got)


def _fill_text(data, cols, quote):
    """The text and category columns of a call: their spans become packed bytes; one readback for
    all of them.  The status is the span's, except that an empty value is 1 (no value) as in a
    numeric column.  A category column's bytes are then encoded by its dictionary and dropped."""
    import torch
    todo = [c for c in cols if c.type in (TEXT, CATEGORY)]
    if not todo:
        return
    got = _text_passes(data.view(-1), [(c.start, c.length, c.status) for c in todo], quote)
    for c, (packed, offsets, out_len) in zip(todo, got):
        c.status = torch.where((c.status == 0) & (out_len == 0), torch.ones_like(c.status), c.status)
        if c.type == CATEGORY:
            c.values = c.dictionary.encode(RaggedBatch(packed, offsets, out_len), c.status)
            c.start = c.length = None
            continue
        c.data, c.offsets, c.length, c.start = packed, offsets, out_len, None


def _pow2(x: int) -> int:
    return 1 << max(0, int(x) - 1).bit_length()


class TextDictionary:
    """A dictionary of byte strings on a device (a GPU or the CPU) that turns text values into int32
    codes.  The codes are those of ``[d.setdefault(v, len(d)) for v in values]`` over the values in
    row order with ``d`` kept across calls: first-occurrence order, as ``pandas.factorize`` gives.
    Keys are compared byte for byte (no trimming, no case folding); the empty value is a key like
    any other; a value whose status is not 0, or that does not lie inside its data, has code -1 and
    is not added.  The result depends neither on the hash, the table size nor on timing.

    The state is four tensors on ``device``: an open-addressing hash table (``capacity`` slots, a
    power of two, kept at most half full), the entries' hashes, and their bytes and offsets packed
    in code order, grown by doubling.  ``capacity`` is the initial table size."""

    def __init__(self, device=None, capacity: int = 1024):
        import torch
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if capacity < 1:
            raise ValueError("the capacity is at least 1")
        self._size, self._nbytes = 0, 0
        self._table = torch.full((_pow2(capacity),), -1, dtype=torch.int64, device=self.device)
        self._hash = torch.empty(16, dtype=torch.int64, device=self.device)
        self._off = torch.zeros(17, dtype=torch.int64, device=self.device)
        self._data = torch.empty(256, dtype=torch.uint8, device=self.device)

    @property
    def size(self) -> int:
        return self._size

    def __len__(self) -> int:
        return self._size

    @property
    def capacity(self) -> int:
        """Slots of the hash table now."""
        return int(self._table.numel())

    @property
    def values(self) -> RaggedBatch:
        """The entries packed in code order: entry c is ``data[offsets[c]:offsets[c + 1]]``."""
        off = self._off[:self._size + 1]
        return RaggedBatch(self._data[:self._nbytes], off, off[1:] - off[:-1])

    def tolist(self) -> list:
        """The entries as ``bytes``, in code order (one copy to the host)."""
        import torch
        nb = self._nbytes
        blob = torch.cat([self._data[:nb], self._off[:self._size + 1].view(torch.uint8)]).cpu().numpy()
        cuts, text = blob[nb:].view(np.int64).tolist(), blob[:nb].tobytes()
        return [text[cuts[c]:cuts[c + 1]] for c in range(self._size)]

    @classmethod
    def from_values(cls, values, device=None) -> "TextDictionary":
        """A dictionary whose entry c is ``values[c]`` (a saved vocabulary: distinct ``bytes``)."""
        import torch
        values = [bytes(v) for v in values]
        d = cls(device, capacity=max(1024, _pow2(2 * len(values))))
        lens = np.array([len(v) for v in values], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        data = np.frombuffer(b"".join(values), dtype=np.uint8).copy()
        d.encode(RaggedBatch(torch.from_numpy(data), torch.from_numpy(offs), torch.from_numpy(lens)))
        if d.size != len(values):
            raise ValueError("a vocabulary holds every value once")
        return d

    def _inputs(self, values, status):
        """(flat data, start int64, length int32, status uint8 or None, n) on the dictionary's device."""
        import torch
        if isinstance(values, Column):
            if values.type != TEXT:
                raise ValueError("a dictionary encodes text columns")
            if status is None:
                status = values.status
            values = (values.data, values.offsets, values.length)
        data, off, ln = values
        if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8:
            raise ValueError("a dictionary encodes uint8 values")
        dev = self.device
        data = data.to(dev).contiguous().view(-1)
        ln = torch.as_tensor(ln).to(dev).view(-1)
        n = int(ln.numel())
        if n > 2 ** 30:
            raise ValueError("at most 2^30 values in one call")
        if ln.dtype != torch.int32:
            ln = ln.clamp(-1, 2 ** 31 - 1).to(torch.int32)
        start = torch.as_tensor(off).to(device=dev, dtype=torch.int64).view(-1)[:n].contiguous()
        if start.numel() != n:
            raise ValueError("offsets and lengths differ in size")
        if status is not None:
            status = torch.as_tensor(status).to(device=dev, dtype=torch.uint8).contiguous().view(-1)
            if status.numel() != n:
                raise ValueError("values and status differ in size")
        return data, start, ln.contiguous(), status, n

    def _reserve_table(self, need: int):
        """A table of at least ``need`` slots: a larger one is filled from the entries' stored
        hashes (they are distinct: no byte compares)."""
        import torch
        from ..ops.native import lib
        if self.capacity >= need:
            return
        device, stream = _queue(self.device)
        table = torch.full((_pow2(need),), -1, dtype=torch.int64, device=self.device)
        lib().text_dict_rehash_raw(self._hash.data_ptr(), self._size, table.data_ptr(), table.numel(), device, stream)
        self._table = table

    def _reserve_entries(self, entries: int, nbytes: int):
        import torch
        if entries > self._hash.numel():
            cap = max(_pow2(entries), 2 * self._hash.numel())
            h = torch.empty(cap, dtype=torch.int64, device=self.device)
            o = torch.zeros(cap + 1, dtype=torch.int64, device=self.device)
            h[:self._size] = self._hash[:self._size]
            o[:self._size + 1] = self._off[:self._size + 1]
            self._hash, self._off = h, o
        if nbytes > self._data.numel():
            d = torch.empty(max(_pow2(nbytes), 2 * self._data.numel()), dtype=torch.uint8, device=self.device)
            d[:self._nbytes] = self._data[:self._nbytes]
            self._data = d

    def _probe(self, C, data, start, ln, status, n, insert, slot_of, hashes):
        device, stream = _queue(self.device)
        C.text_dict_probe_raw(data.data_ptr(), data.numel(), start.data_ptr(), ln.data_ptr(),
                              status.data_ptr() if status is not None else 0, n, device, self._data.data_ptr(),
                              self._nbytes, self._off.data_ptr(), self._size, self._table.data_ptr(), self.capacity,
                              insert, slot_of.data_ptr(), hashes.data_ptr(), stream)

    def encode(self, values, status=None):
        """The int32 codes of ``values`` (a ``RaggedBatch(data, offsets, lengths)`` of bytes, or a
        text :class:`Column`) on the dictionary's device; values not seen before are added.  Five
        launches and two ``torch.cumsum`` on torch's current stream, and one small readback (how
        many entries and bytes are new) to size the dictionary's storage."""
        import torch
        from ..ops.native import lib, native_errors
        data, start, ln, status, n = self._inputs(values, status)
        dev = self.device
        if n == 0:
            return torch.empty(0, dtype=torch.int32, device=dev)
        C = lib()
        device, stream = _queue(dev)
        D = self._size
        slot_of, first, first_len, codes = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
        hashes = torch.empty(n, dtype=torch.int64, device=dev)
        byte_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        with native_errors():
            self._reserve_table(2 * (D + n))
            cap, table = self.capacity, self._table.data_ptr()
            self._probe(C, data, start, ln, status, n, True, slot_of, hashes)
            C.text_dict_first_raw(table, cap, slot_of.data_ptr(), ln.data_ptr(), n, device, first.data_ptr(),
                                  first_len.data_ptr(), stream)
            rank = torch.cumsum(first, 0, dtype=torch.int64)
            torch.cumsum(first_len, 0, dtype=torch.int64, out=byte_off[1:])
            new, nb = torch.stack([rank[-1], byte_off[-1]]).cpu().tolist()
            C.text_dict_codes_raw(table, cap, slot_of.data_ptr(), rank.data_ptr(), n, D, device, codes.data_ptr(), stream)
            if new:
                self._reserve_entries(D + new, self._nbytes + nb)
                C.text_dict_commit_raw(table, cap, slot_of.data_ptr(), hashes.data_ptr(), first.data_ptr(),
                                       rank.data_ptr(), byte_off.data_ptr(), n, D, self._hash.data_ptr(),
                                       self._off.data_ptr(), self._hash.numel(), self._nbytes, device, stream)
                if nb:                                  # the first rows' bytes, in code order
                    C.text_emit_raw(data.data_ptr(), data.numel(), start.data_ptr(), ln.data_ptr(),
                                    status.data_ptr() if status is not None else 0, n, device, -1, byte_off.data_ptr(),
                                    self._data.data_ptr() + self._nbytes, nb, stream)
                self._size, self._nbytes = D + new, self._nbytes + nb
        return codes

    def lookup(self, values, status=None):
        """The int32 codes of ``values`` with nothing added: -1 for a value the dictionary does not
        hold (a frozen vocabulary, for a validation set).  Two launches, no readback."""
        import torch
        from ..ops.native import lib, native_errors
        data, start, ln, status, n = self._inputs(values, status)
        dev = self.device
        codes = torch.empty(n, dtype=torch.int32, device=dev)
        if n == 0:
            return codes
        C = lib()
        device, stream = _queue(dev)
        slot_of = torch.empty(n, dtype=torch.int32, device=dev)
        hashes = torch.empty(n, dtype=torch.int64, device=dev)
        with native_errors():
            self._probe(C, data, start, ln, status, n, False, slot_of, hashes)
            C.text_dict_codes_raw(self._table.data_ptr(), self.capacity, slot_of.data_ptr(), 0, n, self._size, device,
                                  codes.data_ptr(), stream)
        return codes

    def __repr__(self):
        return f"TextDictionary(size={self._size}, capacity={self.capacity}, device={self.device})"


def _category_dictionaries(specs, dictionaries, device) -> dict:
    """{column position: TextDictionary} for the category columns of ``specs``: the caller's (by
    column name, or by position for a list of columns) or a fresh one on ``device``."""
    given = dict(dictionaries or {})
    out = {}
    for j, (name, _k, t) in enumerate(specs):
        key = name if name is not None else j
        if t != CATEGORY:
            if key in given:
                raise ValueError(f"column {key!r} is given a dictionary but is not a category column")
            continue
        d = given.pop(key, None)
        if d is None:
            d = TextDictionary(device)
        elif not isinstance(d, TextDictionary):
            raise TypeError(f"the dictionary of column {key!r} is a TextDictionary, got {type(d).__name__}")
        out[j] = d
    if given:
        raise KeyError(f"dictionaries for unknown columns: {sorted(map(str, given))}")
    return out


def parse_fields(batch, columns, sep=",", quote=None, terminator=b"\n", resolve_deferred=True,
                 dictionaries=None) -> FieldColumns:
    """Parse the requested fields of every row of ``batch`` (a uint8 :class:`RaggedBatch`, packed
    or padded, on a device or on the CPU) into tensors on the batch's device.

    ``columns``: a list of ``(field number, type)`` or a dict ``name -> (field number, type)``.
    The work runs on torch's current stream and is not waited for, except that
    ``resolve_deferred=True`` reads one small flag back to learn whether any float was deferred;
    ``resolve_deferred=False`` leaves such values NaN with status 3, and that the ``"text"``
    columns of a call (alias ``"bytes"``) read their total sizes back, all in one copy, to allocate
    their ``data``.  A text column holds what :func:`extract_text` gives for the field's span, with
    ``quote`` as its quote; its status is the span's, except that an empty value has status 1 as in
    a numeric column, so ``tolist()`` gives ``None`` for absent and for empty fields.

    A ``"category"`` column (alias ``"dict"``) is that text column encoded by a
    :class:`TextDictionary`: ``values`` are int32 codes, -1 where the status is not 0, and
    ``dictionary`` is the dictionary.  ``dictionaries`` maps a column's name (its position, for a
    list of columns) to the dictionary to encode into, so that codes agree across calls; a category
    column without an entry gets a fresh one.  Each encode reads one more small tensor back."""
    import torch
    data, off, ln = batch
    if not isinstance(data, torch.Tensor) or data.dtype != torch.uint8:
        raise ValueError("parse_fields takes a uint8 batch")
    specs = _column_list(columns)
    if not specs:
        raise ValueError("at least one column is required")
    for _, k, _t in specs:
        if k > 65535:
            raise ValueError("field numbers above 65535 are not supported")
    s, q, t = _scalars(sep, quote, terminator)
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
        cols += _launch(data, off, ln, specs[i:i + _MAX_COLS], s, q, t)
    for j, d in dicts.items():
        cols[j].dictionary = d
    if resolve_deferred:
        _resolve(data, off, ln, cols, s, q, t)
    _fill_text(data, cols, q)
    return FieldColumns(cols)


def split_row(row: bytes, sep=",", quote=None, terminator=b"\n") -> list:
    """The contents of the fields of one row, by the rule above, on the host."""
    s, q, t = _scalars(sep, quote, terminator)
    if row.endswith(bytes([t])):
        row = row[:-1]
        if t == 0x0A and row.endswith(b"\r"):
            row = row[:-1]
    fields, start, inside = [], 0, False
    for i, c in enumerate(row):
        if c == q:
            inside = not inside
        elif c == s and not inside:
            fields.append(row[start:i])
            start = i + 1
    fields.append(row[start:])
    out = []
    for f in fields:
        if q >= 0 and len(f) >= 2 and f[0] == q and f[-1] == q:
            f = f[1:-1]
        out.append(f.strip(b" \t"))
    return out


def read_delimited_columns(fs, path: str, columns, sep=",", quote=None, delimiter=b"\n", header: bool = False,
                           skip_rows: int = 0, batch_size: int = 65536, device=None, device_plan="auto",
                           dictionaries=None) -> FieldColumns:
    """The requested columns of a whole delimited text file, concatenated over an unshuffled
    :class:`DeviceBatchLoader` of ``batch_size`` rows.  The ``start`` of a span column is an offset
    into the file here (into the batch's data in :func:`parse_fields`); a text column is one packed
    column for the file; a category column has one dictionary for the file (the caller's, through
    ``dictionaries`` as in :func:`parse_fields`, or a fresh one), so its codes are file-global.

    ``header=True``: the first record is read through the client stream and split by the same rule
    on the host; ``columns`` may then name a field by its header text instead of its number (an
    unknown name is a ``KeyError``, a header with the same name twice a ``ValueError``), and the
    header row is dropped.  ``skip_rows`` drops further leading records."""
    if skip_rows < 0:
        raise ValueError("skip_rows counts rows")
    s, q, t = _scalars(sep, quote, delimiter)
    index = build_delimited_index(fs, path, delimiter, quote=quote, device_plan=device_plan)
    named = isinstance(columns, dict)
    items = list(columns.items()) if named else [(None, spec) for spec in columns]
    drop = int(skip_rows)
    if header:
        if len(index) < 2:
            raise ValueError(f"{path}: no header row")
        with fs.open_file(path) as f:
            buf = np.empty(int(index[1]), dtype=np.uint8)
            got = 0
            while got < len(buf):
                k = f.readinto(buf[got:])
                if k <= 0:
                    break
                got += k
        names = [x.decode("utf-8", "replace") for x in split_row(buf[:got].tobytes(), sep, quote, delimiter)]
        if len(set(names)) != len(names):
            raise ValueError(f"{path}: the header names a column twice")
        where = {nm: i for i, nm in enumerate(names)}
        resolved = []
        for name, (k, dtype) in items:
            if isinstance(k, str):
                if k not in where:
                    raise KeyError(k)
                k = where[k]
            resolved.append((name, (k, dtype)))
        items = resolved
        drop += 1
    elif any(isinstance(k, str) for _, (k, _d) in items):
        raise ValueError("columns are named by header text only with header=True")
    spec = dict(items) if named else [sp for _, sp in items]
    index = index[min(drop, len(index) - 1):]
    ds = IndexedRecordDataset(fs, path, index=index, device=device)
    parts = []
    with DeviceBatchLoader(ds, batch_size=batch_size, device=device, align=1, device_plan=device_plan) as dl:
        import torch
        file_off = torch.from_numpy(np.ascontiguousarray(index[:-1])).to(dl.device)
        specs = _column_list(spec)
        dicts = _category_dictionaries(specs, dictionaries, dl.device)
        dicts = {specs[j][0] if named else j: d for j, d in dicts.items()}
        done = 0
        for batch in dl:
            got = parse_fields(batch, spec, sep, quote, delimiter, dictionaries=dicts)
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
            parts.append(parse_fields(empty, spec, sep, quote, delimiter, dictionaries=dicts))
    return FieldColumns.concat(parts)
