"""parquet_walk_raw: the PageHeaders between the pages of column chunks become page-table rows.
The yardstick is a Thrift-compact walker written here from the format specification; the chunks
come from files that pyarrow wrote (V1 and V2 pages, with and without a dictionary page, with and
without statistics, with long string statistics, many pages per chunk).

Ids: `cpu` runs the host loop over numpy buffers (device=-1); `gpu-v0` and `gpu-v1` run the kernel
(the walk is the same in both variants).  On the GPU the data is a slice in the middle of a larger
device tensor at an odd byte phase whose other bytes are field headers, varints and run headers, so
a read outside a chunk changes a result instead of going unseen.  Every output array has guard
elements on both sides and is filled before the call, so a write outside shows."""
import io

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

from alluxio_amd.ops.native import lib

PAD = 4099
GUARD = 5
COLS = 12
FILL = bytes([0x15, 0x00, 0x15, 0x90, 0x01, 0x15, 0x20, 0x2C, 0x15, 0x10, 0x18, 0x04, 0x03, 0x08, 0x00])


@pytest.fixture(params=[pytest.param(("cpu", 0), id="cpu"),
                        pytest.param(("gpu", 0), marks=pytest.mark.gpu, id="gpu-v0"),
                        pytest.param(("gpu", 1), marks=pytest.mark.gpu, id="gpu-v1")])
def env(request):
    mode, variant = request.param
    if mode == "cpu":
        yield _Env(False)
        return
    request.getfixturevalue("gpu")
    default = lib().parquet_decode_variant()
    lib().set_parquet_decode_variant(variant)
    assert lib().parquet_decode_variant() == variant
    yield _Env(True)
    lib().set_parquet_decode_variant(default)


# ---- the rule, in Python -------------------------------------------------------------------------
class _Reader:
    def __init__(self, b, p, end):
        self.b, self.p, self.end, self.binaries = b, p, end, []

    def byte(self):
        if self.p >= self.end:
            raise EOFError
        self.p += 1
        return self.b[self.p - 1]

    def varint(self):
        v = s = 0
        while s < 70:
            c = self.byte()
            v |= (c & 0x7F) << s
            if not c & 0x80:
                return v
            s += 7
        raise EOFError

    def zz(self):
        v = self.varint()
        return (v >> 1) ^ -(v & 1)

    def value(self, t, depth=0):
        """One value; `depth` counts the containers open around it since the last field the walk knows
        (the skip of csrc/parquet_host.h keeps a stack of 8)."""
        if t in (9, 10, 12):
            depth += 1
            if depth > 8:
                raise EOFError
        if t in (1, 2):
            return t == 1
        if t == 3:
            return self.byte()
        if t in (4, 5, 6):
            return self.zz()
        if t == 7:
            self.p += 8
            if self.p > self.end:
                raise EOFError
            return None
        if t == 8:
            n = self.varint()
            if n > self.end - self.p:
                raise EOFError
            self.binaries.append((self.p, n))
            self.p += n
            return None
        if t in (9, 10):
            h = self.byte()
            n = h >> 4 if h >> 4 != 15 else self.varint()
            if n > self.end - self.p:
                raise EOFError
            et = 3 if h & 15 in (1, 2) else h & 15
            return [self.value(et, depth) for _ in range(n)]
        if t == 12:
            return self.struct(depth)
        raise EOFError

    def struct(self, depth=0, known=()):
        out, fid = {}, 0
        while True:
            h = self.byte()
            if h == 0:
                return out
            fid = fid + (h >> 4) if h >> 4 else self.zz()
            if fid in known and h & 15 == 12:
                out[fid] = self.struct(0)               # a header the walk reads field by field
            else:
                out[fid] = self.value(h & 15, depth)


def ref_walk(data: bytes, off: int, ln: int, chunk: int):
    """([rows], error code, [(header start, payload start, payload end, binaries of the header)])."""
    rows, marks, pos, end = [], [], off, off + ln
    while pos < end:
        r = _Reader(data, pos, end)
        try:
            h = r.struct(0, known=(5, 7, 8))
        except EOFError:
            return rows, 1, marks
        comp, unc, typ = h.get(3, -1), h.get(2, -1), h.get(1, -1)
        v1, dc, v2 = h.get(5) or {}, h.get(7) or {}, h.get(8) or {}
        sub = v1 if 5 in h else dc if 7 in h else v2
        nv = sub.get(1, 0)
        if min(comp, unc, typ, nv) < 0:
            return rows, 3, marks
        if comp > end - r.p:
            return rows, 4, marks
        marks.append((pos, r.p, r.p + comp, r.binaries))
        pos = r.p + comp
        if typ == 1:
            continue
        if typ not in (0, 2, 3):
            return rows, 2, marks
        enc = v2.get(4, -1) if 8 in h else sub.get(2, -1)
        rows.append([typ, r.p, comp, unc, nv, enc, v2.get(5, 0), v2.get(6, 0), v2.get(2, -1) if 8 in h else -1,
                     int(v2.get(7, True)) if 8 in h else 1, chunk, v1.get(3, 3) if 5 in h else 3])
    return rows, 0, marks


# ---- chunks ----------------------------------------------------------------------------------------
def _chunks():
    n = 3000
    rng = np.random.default_rng(3)
    long_ = ["x" * 300 + str(i) for i in range(n)]
    tbl = pa.table({"a": pa.array(np.arange(n) * 3, pa.int64()),
                    "b": pa.array([None if i % 7 == 0 else f"k{i % 19}" for i in range(n)], pa.string()),
                    "c": pa.array(rng.standard_normal(n)),
                    "d": pa.array(long_, pa.string())})
    out = []
    for kw in (dict(data_page_version="1.0"), dict(data_page_version="2.0"),
               dict(data_page_version="1.0", use_dictionary=False), dict(data_page_version="2.0", write_statistics=False),
               dict(data_page_version="1.0", write_statistics=False, use_dictionary=False),
               dict(data_page_version="2.0", compression="lz4")):
        kw.setdefault("compression", "none")
        buf = io.BytesIO()
        pq.write_table(tbl, buf, data_page_size=4096, write_batch_size=64, **kw)
        blob = buf.getvalue()
        md = pq.ParquetFile(io.BytesIO(blob)).metadata
        for g in range(md.num_row_groups):
            for j in range(md.num_columns):
                c = md.row_group(g).column(j)
                start = c.data_page_offset
                if c.dictionary_page_offset is not None and 0 < c.dictionary_page_offset < start:
                    start = c.dictionary_page_offset
                out.append(blob[start:start + c.total_compressed_size])
    return out


_POOL = None


def pool():
    global _POOL
    if _POOL is None:
        _POOL = _chunks()
    return _POOL


class _Env:
    def __init__(self, gpu):
        self.gpu = gpu

    def walk(self, data: bytes, offs, lens, rows_cap=None):
        """count, then fill.  Returns (table, counts, errors); the guards are checked."""
        C = lib()
        n = len(offs)
        offs, lens = np.array(offs, dtype=np.int64), np.array(lens, dtype=np.int64)
        counts = np.full(n + 2 * GUARD, -7, np.int32)
        errors = np.full(n + 2 * GUARD, -7, np.int32)
        if self.gpu:
            import torch
            big = np.resize(np.frombuffer(FILL, dtype=np.uint8), PAD + len(data) + PAD)
            big[PAD:PAD + len(data)] = np.frombuffer(data, dtype=np.uint8)
            dev = torch.from_numpy(big).cuda()
            base, up, down, device = dev.data_ptr() + PAD, (lambda a: torch.from_numpy(a).cuda()), (lambda t: t.cpu().numpy()), 0
            ptr = lambda t, g=GUARD: t.data_ptr() + g * t.element_size()     # noqa: E731
            sync = torch.cuda.synchronize
        else:
            host = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(1, np.uint8)
            base, up, down, device = host.ctypes.data, (lambda a: a), (lambda t: t), -1
            ptr = lambda t, g=GUARD: t.ctypes.data + g * t.itemsize          # noqa: E731
            sync = lambda: None                                              # noqa: E731
        d_off, d_len, d_counts, d_errors = up(offs), up(lens), up(counts), up(errors)
        C.parquet_walk_raw(base, len(data), ptr(d_off, 0) if n else 0, ptr(d_len, 0) if n else 0, n, device,
                           ptr(d_counts), ptr(d_errors))
        sync()
        counts, errors = down(d_counts), down(d_errors)
        for a in (counts, errors):
            assert (a[:GUARD] == -7).all() and (a[GUARD + n:] == -7).all(), "a guard was written"
        counts, errors = counts[GUARD:GUARD + n].copy(), errors[GUARD:GUARD + n].copy()
        pbase = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        total = int(pbase[-1]) if rows_cap is None else rows_cap
        table = np.full((total + 2 * GUARD) * COLS, -7, np.int64)
        d_table, d_pbase = up(table), up(pbase)
        C.parquet_walk_raw(base, len(data), ptr(d_off, 0) if n else 0, ptr(d_len, 0) if n else 0, n, device, 0, 0,
                           ptr(d_pbase, 0), ptr(d_table, GUARD * COLS), total)
        sync()
        table = down(d_table).reshape(-1, COLS)
        assert (table[:GUARD] == -7).all() and (table[GUARD + total:] == -7).all(), "a table guard was written"
        return table[GUARD:GUARD + total], counts, errors


def _lay(chunks, gap=b"\x15\x00\x15"):
    data, offs, lens = bytearray(b"\x2c"), [], []
    for c in chunks:
        offs.append(len(data))
        lens.append(len(c))
        data += c + gap
    return bytes(data), offs, lens


def _expect(data, offs, lens):
    rows, errs, counts = [], [], []
    for k, (o, n) in enumerate(zip(offs, lens)):
        r, e, _ = ref_walk(data, o, n, k)
        rows += r
        errs.append(e)
        counts.append(len(r))
    return np.array(rows, dtype=np.int64).reshape(-1, COLS), counts, errs


@pytest.mark.parametrize("nchunks", [0, 1, 2, 63, 64, 65])
def test_walk_chunks(env, nchunks):
    p = pool()
    chunks = [p[(i * 5 + nchunks) % len(p)] for i in range(nchunks)]
    data, offs, lens = _lay(chunks)
    table, counts, errors = env.walk(data, offs, lens)
    want, wcounts, werrs = _expect(data, offs, lens)
    assert counts.tolist() == wcounts and errors.tolist() == werrs == [0] * nchunks
    assert np.array_equal(table, want)


def test_walk_covers_the_forms(env):
    """Every chunk of the pool, one call: the pool holds V1 and V2 pages, dictionary pages, chunks of
    many pages, headers with and without statistics and with statistics of 300 bytes."""
    p = pool()
    data, offs, lens = _lay(p)
    table, counts, errors = env.walk(data, offs, lens)
    want, wcounts, werrs = _expect(data, offs, lens)
    assert np.array_equal(table, want) and counts.tolist() == wcounts and not errors.any()
    assert {0, 2, 3} <= set(table[:, 0].tolist()) and max(wcounts) > 20
    marks = [m for o, n in zip(offs, lens) for m in ref_walk(data, o, n, 0)[2]]
    assert max((b[1] for m in marks for b in m[3]), default=0) >= 300      # long statistics were walked over
    assert any(not m[3] for m in marks)                                    # and headers without any


def test_walk_truncated(env):
    """A chunk cut inside a header, inside a statistics binary and inside a payload: the pages
    before the cut are found, the error code is set and nothing outside the outputs is written."""
    p = pool()
    big = max(p, key=len)
    data, offs, lens = _lay([big])
    _, _, marks = ref_walk(data, offs[0], lens[0], 0)
    k = len(marks) // 2
    hstart, pstart, pend, bins = marks[k]
    assert bins and max(b[1] for b in bins) >= 300
    binary = max(bins, key=lambda b: b[1])
    cuts = {"header": hstart + 3, "binary": binary[0] + binary[1] // 2, "payload": pstart + (pend - pstart) // 2,
            "first byte": hstart + 1}
    assert pend - pstart > 2
    chunks, want_err = [], []
    for what, cut in cuts.items():
        chunks.append(data[offs[0]:cut])
        want_err.append(4 if what == "payload" else 1)
    chunks.append(big)
    want_err.append(0)
    data2, offs2, lens2 = _lay(chunks, gap=big[:200])          # what follows a cut chunk looks like a chunk
    table, counts, errors = env.walk(data2, offs2, lens2)
    want, wcounts, werrs = _expect(data2, offs2, lens2)
    assert errors.tolist() == want_err == werrs
    assert counts.tolist() == wcounts == [k] * 4 + [len(marks)]
    assert np.array_equal(table, want)
    # a table with fewer rows than pages is filled as far as it goes
    small, _, _ = env.walk(data2, offs2, lens2, rows_cap=k + 1)
    assert np.array_equal(small, want[:k + 1])


def test_walk_hostile(env):
    """Headers written by hand: a negative size, an unknown page type, an index page, a size past
    the chunk, a list that claims more elements than bytes, nesting deeper than the skip stack, and
    a chunk outside the buffer."""
    def header(typ, unc, comp, extra=b""):
        zz = lambda v: _varint((v << 1) ^ (v >> 63))            # noqa: E731
        return b"\x15" + zz(typ) + b"\x15" + zz(unc) + b"\x15" + zz(comp) + extra + b"\x00"

    def _varint(v):
        v &= (1 << 64) - 1
        out = bytearray()
        while True:
            if v < 0x80:
                return bytes(out + bytes([v]))
            out.append((v & 0x7F) | 0x80)
            v >>= 7

    data_hdr = b"\x2c\x15\x08\x15\x00\x15\x06\x15\x06\x00"       # field 5: DataPageHeader{4 values, PLAIN, RLE, RLE}
    good = header(0, 4, 4, data_hdr) + b"abcd"
    cases = [(good, 0, 1), (header(0, 4, -4, data_hdr) + b"abcd", 3, 0), (header(9, 4, 4, data_hdr) + b"abcd", 2, 0),
             (header(1, 2, 2) + b"zz" + good, 0, 1), (header(0, 4, 400, data_hdr) + b"abcd", 4, 0),
             (good + header(0, 4, 4, data_hdr + b"\x99\xff\xff\x03") + b"abcd", 1, 1),
             (good + header(0, 4, 4, data_hdr + b"\x1c" * 12 + b"\x00" * 12) + b"abcd", 1, 1),
             (good + header(0, 4, 4, data_hdr + b"\x1c" * 6 + b"\x00" * 6) + b"abcd", 0, 2),
             (good + b"\xff" * 12, 1, 1)]
    data, offs, lens = _lay([c for c, _e, _n in cases])
    offs += [len(data) - 2, -1, 5]
    lens += [10, 4, -1]
    table, counts, errors = env.walk(data, offs, lens)
    assert errors.tolist() == [e for _c, e, _n in cases] + [5, 5, 5]
    assert counts.tolist() == [n for _c, _e, n in cases] + [0, 0, 0]
    want, wcounts, werrs = _expect(data, offs[:len(cases)], lens[:len(cases)])
    assert np.array_equal(table, want)


def test_walk_rejects(env):
    C = lib()
    before = C.parquet_decode_launches()
    a = np.zeros(4, np.int64)
    with pytest.raises(C.StoreError):
        C.parquet_walk_raw(0, 16, a.ctypes.data, a.ctypes.data, 1, -1, a.ctypes.data, a.ctypes.data)
    with pytest.raises(C.StoreError):
        C.parquet_walk_raw(a.ctypes.data, 16, a.ctypes.data, a.ctypes.data, 1, -1, 0, 0)
    with pytest.raises(C.StoreError):
        C.parquet_walk_raw(a.ctypes.data, 16, a.ctypes.data, a.ctypes.data, 2 ** 31 + 1, -1, a.ctypes.data, a.ctypes.data)
    assert C.parquet_decode_launches() == before
