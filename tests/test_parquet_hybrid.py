"""parquet_hybrid_raw, parquet_place_raw and parquet_bytes_raw: RLE / bit-packed hybrid streams into
int32 values, rows placed from PLAIN bytes or through a dictionary, and PLAIN BYTE_ARRAY pages
walked into spans.  The yardsticks are a decoder, a placer and a walker written here in Python from
the rules in csrc/parquet_host.h; the streams come from an encoder written here, which mixes RLE
and bit-packed runs, bit-packed runs of a single group and a last group padded past the count.

Ids: `cpu` runs the host loops over numpy buffers (device=-1; the run-table form is run on the
host as well and must agree); `gpu-v0` runs the serial kernel, `gpu-v1` the cooperative form (count
the runs, fill the run table, one thread per value).  On the GPU the data is a slice in the middle
of a larger device tensor at an odd byte phase whose other bytes are run headers and length
prefixes.  Every output array has guard elements on both sides and is filled before the call."""
import numpy as np
import pytest

from alluxio_amd.ops.native import lib

PAD = 4099
GUARD = 5
FILL = bytes([0x03, 0xFF, 0x10, 0x07, 0x00, 0x00, 0x00, 0x21, 0xAA, 0x55, 0x02, 0x01, 0x08])
WIDTHS = [0, 1, 2, 3, 5, 8, 11, 16, 17, 24, 31, 32]
COUNTS = [0, 1, 7, 8, 9, 63, 64, 65, 503, 504, 505, 1000, 4099]
SC, PC = 8, 10                                           # columns of a stream row and of a data-page row


@pytest.fixture(params=[pytest.param(("cpu", 0), id="cpu"),
                        pytest.param(("gpu", 0), marks=pytest.mark.gpu, id="gpu-v0"),
                        pytest.param(("gpu", 1), marks=pytest.mark.gpu, id="gpu-v1")])
def env(request):
    mode, variant = request.param
    if mode == "cpu":
        yield _Env(False, 0)
        return
    request.getfixturevalue("gpu")
    default = lib().parquet_decode_variant()
    lib().set_parquet_decode_variant(variant)
    assert lib().parquet_decode_variant() == variant
    yield _Env(True, variant)
    lib().set_parquet_decode_variant(default)


# ---- the encoder -----------------------------------------------------------------------------------
def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    return bytes(out + bytes([v]))


def make_values(rng, n, bw):
    """n values below 2^bw: stretches of one value and stretches of random ones."""
    top = (1 << bw) - 1
    vals = []
    while len(vals) < n:
        k = int(rng.integers(1, 40))
        if rng.random() < 0.5:
            vals += [int(rng.integers(0, top + 1))] * k
        else:
            vals += [int(x) for x in rng.integers(0, top + 1, k)]
    vals = vals[:n]
    if n > 2 and bw:
        vals[0], vals[-1] = top, top                    # every bit of the first and the last value
    return vals


def encode_hybrid(vals, bw, rng):
    """(bytes, [run kinds]): RLE runs where values repeat (not always), bit-packed runs of 1 to 4
    groups otherwise; the last group of a bit-packed run is padded with ones past the values."""
    out, kinds, i, n, nb = bytearray(), [], 0, len(vals), (bw + 7) // 8
    top = (1 << bw) - 1
    while i < n:
        j = i
        while j < n and vals[j] == vals[i]:
            j += 1
        if j - i >= 2 and (j - i >= 8 or rng.random() < 0.6):
            out += varint((j - i) << 1) + vals[i].to_bytes(nb, "little")
            kinds.append("rle")
            i = j
            continue
        groups = 1 if rng.random() < 0.4 else int(rng.integers(2, 5))
        take = min(n - i, groups * 8)
        groups = (take + 7) // 8
        chunk = vals[i:i + take] + [top] * (groups * 8 - take)
        bits = 0
        for k, v in enumerate(chunk):
            bits |= v << (k * bw)
        out += varint((groups << 1) | 1) + bits.to_bytes(groups * bw, "little")
        kinds.append("packed1" if groups == 1 else "padded" if take % 8 else "packed")
        i += take
    return bytes(out), kinds


# ---- the rules, in Python --------------------------------------------------------------------------
def le32(b, p):
    return int.from_bytes(b[p:p + 4], "little")


def ref_window(data, off, ln, skip):
    """(start, length) or None."""
    if off < 0 or ln < 0 or off > len(data) or ln > len(data) - off:
        return None
    if skip:
        if ln < 4 or le32(data, off) > ln - 4:
            return None
        k = 4 + le32(data, off)
        off, ln = off + k, ln - k
    return off, ln


def ref_stream(data, row, out_n):
    """(values, error) of one stream row."""
    off, ln, kind, skip, bw, cnt, ob, _ = (int(x) for x in row)
    n = min(cnt, out_n - ob) if 0 <= ob < out_n and cnt > 0 else 0
    w = ref_window(data, off, ln, skip)
    if w is None:
        return [0] * n, 6
    p, ln = w
    if kind == 1:
        if ln < 4 or le32(data, p) > ln - 4:
            return [0] * n, 6
        p, ln = p + 4, le32(data, p)
    elif kind == 2:
        if ln < 1:
            return [0] * n, (6 if n else 0)
        bw, p, ln = data[p], p + 1, ln - 1
    elif kind != 0:
        return [0] * n, 6
    if not 0 <= bw <= 32:
        return [0] * n, 6
    s, pos, vals, nb = data[p:p + ln], 0, [], (bw + 7) // 8
    while len(vals) < n:
        if pos >= len(s):
            return vals + [0] * (n - len(vals)), 7
        h = sh = 0
        while True:
            if pos >= len(s) or sh > 63:
                return vals + [0] * (n - len(vals)), 7
            c = s[pos]
            pos += 1
            h |= (c & 0x7F) << sh
            sh += 7
            if not c & 0x80:
                break
        h &= (1 << 64) - 1
        if h & 1:
            groups = h >> 1
            if bw and (groups > len(s) - pos or groups * bw > len(s) - pos):
                return vals + [0] * (n - len(vals)), 7
            bits = int.from_bytes(s[pos:pos + groups * bw], "little")
            m = min(groups * 8, n - len(vals))
            vals += [(bits >> (k * bw)) & ((1 << bw) - 1) for k in range(m)]
            pos += groups * bw
        else:
            if nb > len(s) - pos:
                return vals + [0] * (n - len(vals)), 7
            v = int.from_bytes(s[pos:pos + nb], "little") & ((1 << bw) - 1)
            vals += [v] * min(h >> 1, n - len(vals))
            pos += nb
    return vals, 0


def ref_place(data, pages, excl, idx, dict_, stream_err, width, is_bool, rows):
    """(values as bytes per row, status)."""
    vals, st = [bytes(width)] * rows, [2] * rows
    for r in range(rows):
        pg = None
        for p in pages:
            if p[0] <= r:
                pg = p
        if pg is None or pg[1] < 0 or r - pg[0] >= pg[1]:
            continue
        bad = pg[2] == 3 or any(0 <= s < len(stream_err) and stream_err[s] for s in (pg[7], pg[8]))
        if bad:
            continue
        if excl is not None and excl[r + 1] <= excl[r]:
            st[r] = 1
            continue
        rank = excl[r] - excl[pg[0]] if excl is not None else r - pg[0]
        if rank < 0:
            continue
        if pg[2] == 0:
            w = ref_window(data, pg[3], pg[4], pg[5])
            if w is None:
                continue
            q, n = w
            if is_bool:
                if rank // 8 < n:
                    vals[r], st[r] = bytes([(data[q + rank // 8] >> (rank % 8)) & 1]), 0
            elif rank < n // width:
                vals[r], st[r] = data[q + rank * width:q + (rank + 1) * width], 0
        elif pg[2] in (1, 2):
            j = pg[6] + rank
            if pg[6] >= 0 and j < len(idx):
                ix = idx[j] & 0xFFFFFFFF
                if pg[2] == 2:
                    vals[r], st[r] = bytes([ix & 1]), 0
                elif ix < len(dict_) // width:
                    vals[r], st[r] = dict_[ix * width:(ix + 1) * width], 0
    return vals, st


def ref_bytes(data, pages, excl, rows, stream_err, nvalues, fill):
    start, length, status = [fill[0]] * nvalues, [fill[1]] * nvalues, [fill[2]] * nvalues
    for pg in pages:
        if pg[2] not in (0, 3):
            continue
        rb, nv = pg[0], pg[1]
        if rb < 0 or nv < 0 or rb > rows or nv > rows - rb:
            continue
        base, n = rb, nv
        if excl is not None:
            base, n = excl[rb], excl[rb + nv] - excl[rb]
        if base >= nvalues:
            continue
        n = min(n, nvalues - base)
        w = ref_window(data, pg[3], pg[4], pg[5])
        bad = pg[2] == 3 or (0 <= pg[7] < len(stream_err) and stream_err[pg[7]] != 0) or w is None
        q, ln = w if w is not None else (0, 0)
        pos = 0
        for k in range(n):
            if not bad:
                if ln - pos < 4:
                    bad = True
                else:
                    v = le32(data, q + pos)
                    v -= (v >> 31) << 32
                    if v < 0 or v > ln - pos - 4:
                        bad = True
            if bad:
                start[base + k], length[base + k], status[base + k] = 0, 0, 2
                continue
            start[base + k], length[base + k], status[base + k] = q + pos + 4, v, 0
            pos += 4 + v
    return start, length, status


# ---- calls -----------------------------------------------------------------------------------------
class _Env:
    def __init__(self, gpu, variant):
        self.gpu, self.variant, self.keep = gpu, variant, []
        self.device = 0 if gpu else -1

    def data(self, b: bytes) -> int:
        if self.gpu:
            import torch
            big = np.resize(np.frombuffer(FILL, dtype=np.uint8), PAD + len(b) + PAD)
            big[PAD:PAD + len(b)] = np.frombuffer(b, dtype=np.uint8)
            t = torch.from_numpy(big).cuda()
            self.keep.append(t)
            return t.data_ptr() + PAD
        a = np.frombuffer(b, dtype=np.uint8).copy() if b else np.zeros(1, np.uint8)
        self.keep.append(a)
        return a.ctypes.data

    def arr(self, a, dtype) -> int:
        if a is None:
            return 0
        a = np.array(a, dtype=dtype)
        if a.size == 0:
            a = np.zeros(1, dtype)
        if self.gpu:
            import torch
            t = torch.from_numpy(a).cuda()
            self.keep.append(t)
            return t.data_ptr()
        self.keep.append(a)
        return a.ctypes.data

    def out(self, n, dtype, fill):
        a = np.full(n + 2 * GUARD, fill, dtype)
        if self.gpu:
            import torch
            t = torch.from_numpy(a).cuda()
            return (t, t.data_ptr() + GUARD * a.itemsize, n, fill)
        return (a, a.ctypes.data + GUARD * a.itemsize, n, fill)

    def fetch(self, h):
        t, _p, n, fill = h
        if self.gpu:
            import torch
            torch.cuda.synchronize()
            t = t.cpu().numpy()
        assert (t[:GUARD] == fill).all() and (t[GUARD + n:] == fill).all(), "a guard was written"
        return t[GUARD:GUARD + n].copy()

    def hybrid(self, data: bytes, streams, out_n, fill=-7):
        """(out, errors).  cpu: the serial loop, and the run-table form on the host, which must agree."""
        C = lib()
        streams = np.array(streams, dtype=np.int64).reshape(-1, SC)
        ns = len(streams)
        results = []
        for form in ([0, 1] if not self.gpu else [self.variant]):
            base, d_streams = self.data(data), self.arr(streams, np.int64)
            out, err = self.out(out_n, np.int32, fill), self.out(ns, np.int32, -9)
            if form == 0:
                C.parquet_hybrid_raw(base, len(data), d_streams, ns, out[1], out_n, err[1], self.device, 0)
            else:
                cnt = self.out(ns, np.int32, -9)
                C.parquet_hybrid_raw(base, len(data), d_streams, ns, out[1], out_n, err[1], self.device, 1, cnt[1])
                counts = self.fetch(cnt)
                rb = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) if ns else np.zeros(1, np.int64)
                total = int(rb[-1])
                runs = self.out(total * 4, np.int64, -9)
                d_rb = self.arr(rb, np.int64)
                C.parquet_hybrid_raw(base, len(data), d_streams, ns, out[1], out_n, 0, self.device, 2, 0, d_rb, runs[1], total)
                self.fetch(runs)
                C.parquet_hybrid_raw(base, len(data), d_streams, ns, out[1], out_n, 0, self.device, 3, 0, d_rb, runs[1], total)
            results.append((self.fetch(out), self.fetch(err)))
            self.keep.clear()
        for o, e in results[1:]:
            assert np.array_equal(o, results[0][0]) and np.array_equal(e, results[0][1])
        return results[0]

    def place(self, data, pages, excl, idx, dict_, stream_err, width, is_bool, rows):
        C = lib()
        pages = np.array(pages, dtype=np.int64).reshape(-1, PC)
        values, status = self.out(rows * width, np.uint8, 0x55), self.out(rows, np.uint8, 9)
        C.parquet_place_raw(self.data(data), len(data), self.arr(pages, np.int64), len(pages),
                            self.arr(excl, np.int64), self.arr(idx, np.int32), 0 if idx is None else len(idx),
                            self.arr(None if dict_ is None else np.frombuffer(dict_, dtype=np.uint8), np.uint8),
                            0 if dict_ is None else len(dict_) // width, self.arr(stream_err, np.int32),
                            0 if stream_err is None else len(stream_err), width, is_bool, values[1], status[1], rows,
                            self.device)
        v, s = self.fetch(values), self.fetch(status)
        self.keep.clear()
        return [v[r * width:(r + 1) * width].tobytes() for r in range(rows)], s.tolist()

    def bytes_(self, data, pages, excl, rows, stream_err, nvalues):
        C = lib()
        pages = np.array(pages, dtype=np.int64).reshape(-1, PC)
        start, length, status = self.out(nvalues, np.int64, -3), self.out(nvalues, np.int32, -5), self.out(nvalues, np.uint8, 7)
        C.parquet_bytes_raw(self.data(data), len(data), self.arr(pages, np.int64), len(pages), self.arr(excl, np.int64),
                            rows, self.arr(stream_err, np.int32), 0 if stream_err is None else len(stream_err), start[1],
                            length[1], status[1], nvalues, self.device)
        got = self.fetch(start).tolist(), self.fetch(length).tolist(), self.fetch(status).tolist()
        self.keep.clear()
        return got


def _check_streams(env, data, streams, out_n, want_err=None):
    out, err = env.hybrid(data, streams, out_n)
    want = np.full(out_n, -7, np.int64)
    werr = []
    for row in streams:
        vals, e = ref_stream(data, row, out_n)
        ob = int(row[6])
        want[ob:ob + len(vals)] = np.array(vals, dtype=np.uint32).astype(np.int32) if vals else []
        werr.append(e)
    assert err.tolist() == werr
    if want_err is not None:
        assert werr == want_err
    assert np.array_equal(out.astype(np.int64), want)
    return out, err


# ---- hybrid streams ----------------------------------------------------------------------------------
def test_hybrid_widths_and_counts(env):
    """Every bit width with every value count, each pair a stream of one call; a slot between
    streams belongs to none and stays as it was."""
    rng = np.random.default_rng(7)
    data, streams, at, kinds, truth = bytearray(b"\x07"), [], 0, set(), []
    for bw in WIDTHS:
        for n in COUNTS:
            vals = make_values(rng, n, bw)
            enc, k = encode_hybrid(vals, bw, rng)
            kinds |= set(k)
            streams.append([len(data), len(enc), 0, 0, bw, n, at, 0])
            truth.append((at, vals))
            data += enc + b"\x03"
            at += n + 1
    assert kinds == {"rle", "packed1", "packed", "padded"}
    out, err = _check_streams(env, bytes(data), streams, at, [0] * len(streams))
    for ob, vals in truth:                              # the Python decoder agrees with what was encoded
        assert (out[ob:ob + len(vals)].astype(np.int64) & 0xFFFFFFFF).tolist() == vals


@pytest.mark.parametrize("npages", [1, 2, 17])
def test_hybrid_page_streams(env, npages):
    """The streams of pages as they lie in a file: a V1 definition-level stream behind its 4-byte
    length (kind 1), then a dictionary-index stream that starts with its bit width (kind 2, after
    the skipped level block), and V2-style raw level streams (kind 0)."""
    rng = np.random.default_rng(npages)
    data, defs, idxs, at = bytearray(b"\x00\x01"), [], [], 0
    for p in range(npages):
        n = [4099, 1, 65, 0, 504][p % 5]
        bw = WIDTHS[1 + p % 11]
        lev, _ = encode_hybrid(make_values(rng, n, 1), 1, rng)
        ix, _ = encode_hybrid(make_values(rng, n, bw), bw, rng)
        page = len(lev).to_bytes(4, "little") + lev + bytes([bw]) + ix
        if p % 3 == 2:                                  # V2: levels raw, no prefix, widths from the caller
            page = lev + bytes([bw]) + ix
            defs.append([len(data), len(lev), 0, 0, 1, n, at, 0])
            idxs.append([len(data) + len(lev), len(page) - len(lev), 2, 0, 0, n, at, 0])
        else:
            defs.append([len(data), len(page), 1, 0, 1, n, at, 0])
            idxs.append([len(data), len(page), 2, 1, 0, n, at, 0])
        data += page
        at += n
    _check_streams(env, bytes(data), defs, at, [0] * npages)
    _check_streams(env, bytes(data), idxs, at, [0] * npages)


def test_hybrid_cut_short_and_hostile(env):
    """Streams that end inside a bit-packed run, inside a repeated value, after a run header or
    before any run; a length prefix past its window; a bit width of 33; a window outside the buffer;
    a run header that claims 2^40 groups; more values asked for than the output holds.  The values
    of the runs before the bad one are produced, the rest are 0, the error code is set."""
    rng = np.random.default_rng(11)
    vals = make_values(rng, 600, 11)
    enc, _ = encode_hybrid(vals, 11, rng)
    packed = varint((3 << 1) | 1) + bytes(range(1, 34))         # three groups of width 11: 33 bytes
    rle = varint(500 << 1) + b"\x05\x01"
    data, streams, want_err, at = bytearray(b"\x09"), [], [], 0

    def add(b, n, err, kind=0, skip=0, bw=11, ln=None, off=None):
        nonlocal at
        streams.append([len(data) if off is None else off, len(b) if ln is None else ln, kind, skip, bw, n, at, 0])
        want_err.append(err)
        data.extend(b + b"\x03\x55")
        at += n + 2

    add(enc, 600, 0)
    add(enc[:len(enc) // 2], 600, 7)
    add(enc[:-1], 600, 7)
    add(rle + packed[:20], 524, 7)                      # cut inside a bit-packed run: the run is not read at all
    add(rle + packed, 524, 0)
    add(rle + packed, 525, 7)                           # one value more than the runs hold
    add(rle[:-1], 500, 7)                               # cut inside the repeated value
    add(rle[:1], 500, 7)                                # cut inside the run header
    add(b"", 5, 7)
    add(b"", 0, 0)
    add(varint(((1 << 40) << 1) | 1) + packed, 24, 7)
    add(varint(((1 << 62) << 1) | 1), 100, 0, bw=0)     # width 0: no bytes at all, every value 0
    add((40).to_bytes(4, "little") + rle, 10, 6, kind=1)
    add((2).to_bytes(4, "little") + rle, 10, 7, kind=1)          # the prefix cuts the stream short
    add((len(rle)).to_bytes(4, "little") + rle + b"\x0b" + enc, 600, 0, kind=2, skip=1, bw=0)
    add((200000).to_bytes(4, "little") + rle + b"\x0b" + enc, 600, 6, kind=2, skip=1, bw=0)
    add(b"\x21" + enc, 600, 6, kind=2, bw=0)
    add(enc, 600, 6, bw=33)
    add(enc, 600, 6, bw=-1)
    add(enc, 600, 6, kind=5)
    add(enc, 600, 6, off=-4)
    add(enc, 600, 6, ln=-1)
    add(enc, 600, 6, off=1 << 40)
    add(enc, 600, 6, ln=1 << 40)
    streams.append([streams[0][0], len(enc), 0, 0, 11, 600, at, 0])      # the output ends 100 values later
    want_err.append(0)
    _check_streams(env, bytes(data), streams, at + 100, want_err)


def test_hybrid_empty_and_rejected(env):
    C = lib()
    before = C.parquet_decode_launches()
    out, err = env.hybrid(b"\x02\x01", [], 4)
    assert (out == -7).all() and len(err) == 0
    a = np.zeros(8, np.int64)
    for args in ((a.ctypes.data, 4, 0, 1, a.ctypes.data, 1, a.ctypes.data, -1, 0),
                 (a.ctypes.data, 4, a.ctypes.data, 1, a.ctypes.data, 1, 0, -1, 0),
                 (a.ctypes.data, 4, a.ctypes.data, 1, a.ctypes.data, 1, a.ctypes.data, -1, 4),
                 (a.ctypes.data, 4, a.ctypes.data, 1, a.ctypes.data, 2 ** 31 + 1, a.ctypes.data, -1, 0),
                 (a.ctypes.data, 4, a.ctypes.data, 1, a.ctypes.data, 1, a.ctypes.data, -1, 3)):
        with pytest.raises(C.StoreError):
            C.parquet_hybrid_raw(*args)
    with pytest.raises(C.StoreError):
        C.parquet_place_raw(a.ctypes.data, 8, a.ctypes.data, 1, 0, 0, 0, 0, 0, 0, 0, 3, False, a.ctypes.data, a.ctypes.data, 1, -1)
    with pytest.raises(C.StoreError):
        C.parquet_place_raw(a.ctypes.data, 8, a.ctypes.data, 1, 0, 0, 0, 0, 0, 0, 0, 8, False, 0, a.ctypes.data, 1, -1)
    with pytest.raises(C.StoreError):
        C.parquet_bytes_raw(a.ctypes.data, 8, a.ctypes.data, 1, 0, 1, 0, 0, 0, a.ctypes.data, a.ctypes.data, 1, -1)
    assert C.parquet_decode_launches() == before


# ---- place ---------------------------------------------------------------------------------------------
TYPES = [("bool", 1, True), ("int32", 4, False), ("int64", 8, False), ("float32", 4, False), ("float64", 8, False)]
SIZES = [1, 7, 8, 9, 63, 64, 65, 2, 100, 11, 5, 33, 1, 16, 17, 3, 40]          # 17 pages, 475 rows


def _validity(nulls, rows):
    if nulls == "none":
        return None
    return [0] * rows if nulls == "all" else [0 if r % 11 == 5 else 1 for r in range(rows)]


@pytest.mark.parametrize("nulls", ["none", "all", "eleventh"])
@pytest.mark.parametrize("name,width,is_bool", TYPES, ids=[t[0] for t in TYPES])
@pytest.mark.parametrize("npages", [1, 2, 17])
def test_place_plain(env, name, width, is_bool, nulls, npages):
    """PLAIN pages of each fixed type, each page starting at the next byte phase (all 8 occur with
    17 pages), every third behind a skipped level block; nulls none, all, every 11th."""
    rng = np.random.default_rng(width * 31 + npages)
    sizes = SIZES[:npages]
    rows = sum(sizes)
    valid = _validity(nulls, rows)
    excl = None if valid is None else np.concatenate([[0], np.cumsum(valid)]).tolist()
    data, pages, rb = bytearray(b"\x01" * 3), [], 0
    for p, nv in enumerate(sizes):
        while len(data) % 8 != (p + 3) % 8:
            data += b"\xee"
        k = nv if valid is None else sum(valid[rb:rb + nv])
        body = bytes(rng.integers(0, 256, (k + 7) // 8 if is_bool else k * width, dtype=np.uint8))
        skip = int(p % 3 == 1)
        page = ((6).to_bytes(4, "little") + b"\x03\x0c\xff\xff\x01\x02" if skip else b"") + body
        pages.append([rb, nv, 0, len(data), len(page), skip, -1, -1, -1, 0])
        data += page
        rb += nv
    got = env.place(bytes(data), pages, excl, None, None, None, width, is_bool, rows)
    want = ref_place(bytes(data), pages, excl, None, None, [], width, is_bool, rows)
    assert got[1] == want[1] and got[0] == want[0]
    wst = [0] * rows if valid is None else [0 if v else 1 for v in valid]
    assert got[1] == wst


def test_place_sources_and_corruption(env):
    """Dictionary indices (in range, equal to the size, negative), decoded booleans, a corrupt page, a
    page whose stream failed, a PLAIN page shorter than its rows, a window outside the buffer, a
    level block whose length runs past the page, and rows that no page holds."""
    rows = 90
    valid = [0 if r % 7 == 3 else 1 for r in range(rows)]
    excl = np.concatenate([[0], np.cumsum(valid)]).tolist()
    dict_ = bytes(range(40))                            # 10 entries of 4 bytes
    rng = np.random.default_rng(5)
    idx = [int(x) for x in rng.integers(0, 10, 100)]
    idx[3], idx[8], idx[15] = 10, -1, 2 ** 31 - 1
    data = bytes(rng.integers(0, 256, 400, dtype=np.uint8))
    pages = [[0, 10, 1, 0, 0, 0, 0, -1, -1, 0],         # dictionary
             [10, 10, 1, 0, 0, 0, 10, 0, 1, 0],         # its value stream failed
             [20, 10, 3, 0, 400, 0, 0, -1, -1, 0],      # corrupt
             [30, 10, 0, 7, 21, 0, 0, -1, -1, 0],       # 21 bytes: five values of 4, then status 2
             [40, 10, 0, 390, 20, 0, 0, -1, -1, 0],     # outside the buffer
             [50, 10, 0, 3, 100, 1, 0, 2, -1, 0],       # the level block's length is garbage
             [60, 10, 1, 0, 0, 0, 95, -1, -1, 0],       # indices past the index array
             [70, 10, 1, 0, 0, 0, -5, -1, -1, 0]]       # a negative index base
    stream_err = [0, 7, 0]
    got = env.place(data, pages, excl, idx, dict_, stream_err, 4, False, rows)
    want = ref_place(data, pages, excl, idx, dict_, stream_err, 4, False, rows)
    assert got[1] == want[1] and got[0] == want[0]
    assert set(got[1][:10]) == {0, 1, 2} and set(got[1][10:30]) == {2} and set(got[1][80:]) == {2}
    assert got[1][30:40].count(0) == 5 and set(got[1][40:50]) <= {1, 2}
    # decoded booleans (an RLE boolean page) and no validity
    pages = [[0, 50, 2, 0, 0, 0, 0, -1, -1, 0], [50, 40, 2, 0, 0, 0, 60, -1, -1, 0]]
    got = env.place(data, pages, None, idx, None, None, 1, True, rows)
    want = ref_place(data, pages, None, idx, None, [], 1, True, rows)
    assert got == want and got[1] == [0] * rows and got[0][3] == b"\x00" and got[0][8] == b"\x01"
    # no pages at all: every row is corrupt
    got = env.place(data, [], None, None, None, None, 8, False, 5)
    assert got[1] == [2] * 5 and got[0] == [bytes(8)] * 5


# ---- PLAIN BYTE_ARRAY pages -----------------------------------------------------------------------------
def _ba_page(values):
    return b"".join(len(v).to_bytes(4, "little") + v for v in values)


def test_bytes_pages(env):
    """Lengths 0, 1, 15, 16, 17 and 4099 over several pages, with and without validity; a negative
    length and a length past the page make that value and all later ones of the page corrupt."""
    rng = np.random.default_rng(9)
    lens = [0, 1, 15, 16, 17, 4099, 3, 0, 16]
    vals = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in lens]
    p0, p1, p2 = _ba_page(vals[:4]), _ba_page(vals[4:6]), _ba_page(vals[6:])
    neg = _ba_page(vals[:2]) + (2 ** 32 - 4).to_bytes(4, "little") + b"abcd" + _ba_page(vals[2:3])
    past = _ba_page(vals[:3]) + (17).to_bytes(4, "little") + b"x" * 16
    short = _ba_page(vals[:2]) + b"\x01\x00"
    lead = (5).to_bytes(4, "little") + b"\x03\x01\x02\x03\x04"
    data = bytearray(b"\x04\x00\x00")
    pages, rb = [], 0
    for body, nv, skip in ((p0, 4, 0), (lead + p1, 2, 1), (p2, 3, 0), (neg, 4, 0), (past, 4, 0), (short, 3, 0),
                           (b"", 2, 0), (p0, 4, 0)):
        pages.append([rb, nv, 0, len(data), len(body), skip, 0, -1, -1, 0])
        data += body + b"\x02\x00\x00\x00zz"
        rb += nv
    pages[-1][2] = 3                                    # a corrupt page: every value status 2
    pages.append([rb, 3, 1, 0, 0, 0, 0, -1, -1, 0])     # a dictionary-coded page is left alone
    rows = rb + 3
    data = bytes(data)
    got = env.bytes_(data, pages, None, rows, None, rows)
    want = ref_bytes(data, pages, None, rows, [], rows, (-3, -5, 7))
    assert got == tuple(want)
    st = got[2]
    assert st[:9] == [0] * 9 and got[1][:9] == lens and [data[s:s + n] for s, n in zip(got[0][:9], got[1][:9])] == vals
    assert st[9:13] == [0, 0, 2, 2] and st[13:17] == [0, 0, 0, 2] and st[17:20] == [0, 0, 2] and st[20:22] == [2, 2]
    assert st[22:26] == [2] * 4 and st[26:] == [7] * 3
    # with validity: value slots are numbered by the exclusive scan, a page holds as many values as it has valid rows
    valid = [1, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0]
    excl = np.concatenate([[0], np.cumsum(valid)]).tolist()
    pv = [[0, 5, 0, pages[0][3], pages[0][4], 0, 0, 0, -1, 0], [5, 4, 0, pages[2][3], pages[2][4], 0, 0, 1, -1, 0],
          [9, 4, 0, pages[0][3], pages[0][4], 0, 0, 2, -1, 0]]
    for errs in ([0, 0, 0], [0, 5, 0]):
        got = env.bytes_(data, pv, excl, 13, errs, 9)
        want = ref_bytes(data, pv, excl, 13, errs, 9, (-3, -5, 7))
        assert got == tuple(want)
        assert got[2] == ([0] * 9 if not errs[1] else [0, 0, 0, 2, 2, 2, 0, 0, 0])
    # pages whose rows or slots lie outside are skipped; fewer slots than values cut the page
    for pg, nvalues in (([0, 14, 0, pages[0][3], pages[0][4], 0, 0, -1, -1, 0], 9), ([-1, 2, 0, 0, 8, 0, 0, -1, -1, 0], 9),
                        ([0, 4, 0, pages[0][3], pages[0][4], 0, 0, -1, -1, 0], 2)):
        got = env.bytes_(data, [pg], None, 13, None, nvalues)
        assert got == tuple(ref_bytes(data, [pg], None, 13, [], nvalues, (-3, -5, 7)))
