"""Parquet statistics: min / max / null_count computed where the columns lie
(``column_statistics``, the raw binding), written with ``statistics=True`` and checked through
``pyarrow``, read by ``parquet_metadata`` from any file, and used by ``filters=`` to prune row
groups.  Every comparison is exact, floats as bit patterns.  CPU variants run on a DRAM-tier cluster
with CPU columns (the host loops), gpu variants on the HBM tier with CUDA columns (the kernels)."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest
from test_parquet_columns import _cluster
from test_parquet_write import _arrow, _col, _read, _same, _to

from alluxio_amd.models import (FieldColumns, ParquetStatistics, ParquetWriter, column_statistics,
                                parquet_matching_row_groups, parquet_metadata, parquet_row_groups, read_parquet_columns,
                                write_parquet_columns)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025]
NUMERIC = {"int32": (0, 4, 0, np.int32, "<i"), "int64": (0, 8, 0, np.int64, "<q"), "float32": (0, 4, 1, np.float32, "<f"),
           "float64": (0, 8, 1, np.float64, "<d"), "bool": (1, 1, 0, np.uint8, "<?")}
PE_COLS, PS_COLS = 16, 28                               # csrc/parquet_encode_host.h, csrc/parquet_stats_host.h


def _lib():
    from alluxio_amd.ops.native import lib
    return lib()


def _stats_launches():
    return _lib().parquet_stats_launches()


# ---- the rules, serially ------------------------------------------------------------------------------
def _ref(kind, values, status, vocab=None):
    """(null_count, min, max) of one segment with the bounds as PLAIN bytes or None, from the rules
    of csrc/parquet_stats_host.h written out row by row."""
    live = [v for v, s in zip(values, status) if s == 0]
    if kind == "category":
        live = [vocab[c] for c in live if 0 <= c < len(vocab)]
    nulls = len(values) - len(live)
    if kind in ("text", "category"):
        if not live or max(len(v) for v in live) > 64:
            return nulls, None, None
        return nulls, min(live), max(live)              # bytes compare unsigned, a proper prefix first
    fmt = NUMERIC[kind][4]
    if kind == "bool":
        live = [bool(v) for v in live]
    if kind in ("float32", "float64"):
        live = [float(v) for v in live if v == v]
        if not live:
            return nulls, None, None
        lo, hi = min(live), max(live)
        return nulls, struct.pack(fmt, -0.0 if lo == 0 else lo), struct.pack(fmt, 0.0 if hi == 0 else hi)
    if not live:
        return nulls, None, None
    return nulls, struct.pack(fmt, min(live)), struct.pack(fmt, max(live))


# ---- the raw binding ------------------------------------------------------------------------------------
def _run_segments(columns, device):
    """``columns``: dicts with ``kind``, ``values`` (a numpy array; text: a list of bytes; category:
    codes), ``status``, ``cuts`` (the segments: (first row, rows)) and for a category ``vocab``.
    Lays the segment table out, runs parquet_stats_raw on ``device`` and returns
    ``(result rows, [(column, first row, rows, (null_count, min, max))])``."""
    import torch
    C = _lib()
    keep, rows, segs = [], [], []
    rank = {"bool": 1, "category": 2, "text": 3}

    def text_arrays(vals):
        lens = np.array([len(b) for b in vals], dtype=np.int64)
        offs = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(device)
        data = torch.from_numpy(np.frombuffer(b"".join(vals) + b"\0", dtype=np.uint8).copy()).to(device)
        keep.extend([offs, data])
        return data.data_ptr(), offs.data_ptr(), int(lens.sum())

    dict_rows, flat = [], 0
    for c in sorted(columns, key=lambda c: rank.get(c["kind"], 0)):
        kind = c["kind"]
        st = torch.tensor(c["status"], dtype=torch.uint8).to(device)
        keep.append(st)
        base = np.zeros(PE_COLS, dtype=np.int64)
        base[3] = st.data_ptr() if len(c["status"]) else 0
        if kind == "text":
            base[0] = 2
            base[2], base[4], base[5] = text_arrays(c["values"])
        elif kind == "category":
            codes = torch.tensor(c["values"], dtype=torch.int32).to(device)
            keep.append(codes)
            base[0], base[2], base[5] = 3, codes.data_ptr() if len(c["values"]) else 0, len(c["vocab"])
        else:
            k, w, fl, dt, _fmt = NUMERIC[kind]
            vals = torch.from_numpy(np.ascontiguousarray(c["values"], dtype=dt)).to(device)
            keep.append(vals)
            base[0], base[1], base[2], base[13] = k, w, vals.data_ptr() if len(vals) else 0, fl
        for r0, n in c["cuts"]:
            row = base.copy()
            row[6], row[7], row[9] = r0, n, -1
            if kind == "text":
                row[8] = flat
                flat += n
            if kind == "category":                      # every segment has marks and a dictionary segment of its own
                marks = torch.ones(len(c["vocab"]), dtype=torch.uint8, device=device)
                keep.append(marks)
                row[14] = marks.data_ptr()
                d = np.zeros(PE_COLS, dtype=np.int64)
                d[0], d[3], d[7], d[9] = 2, marks.data_ptr(), len(c["vocab"]), -1
                d[2], d[4], d[5] = text_arrays(c["vocab"])
                dict_rows.append((len(rows), d))
            rows.append(row)
            segs.append((c, r0, n))
    dict_of = {}
    for s, d in dict_rows:
        d[8] = flat
        flat += int(d[7])
        dict_of[s] = len(rows)
        rows.append(d)
    table = np.stack(rows)
    kinds = table[:, 0]
    marked, texts = np.nonzero(kinds == 3)[0], np.nonzero(kinds == 2)[0]
    mark_range = (int(marked[0]), int(marked[-1]) + 1) if len(marked) else (0, 0)
    init = np.zeros((len(table), PS_COLS), dtype=np.int64)
    init[:, 2], init[:, 3], init[:, 8:18] = np.iinfo(np.int64).max, np.iinfo(np.int64).min, -1
    d_table, results = torch.from_numpy(table).to(device), torch.from_numpy(init).to(device)
    alive = torch.zeros(max(flat, 1), dtype=torch.uint8, device=device)
    dev = torch.device(device)
    C.parquet_stats_raw(d_table.data_ptr(), len(table), *mark_range, int(texts[0]) if len(texts) else len(table),
                        int(table[:, 7].max()), alive.data_ptr(), flat, results.data_ptr(),
                        torch.cuda.current_device() if dev.type == "cuda" else -1,
                        int(torch.cuda.current_stream().cuda_stream) if dev.type == "cuda" else 0)
    host = results.cpu().numpy()
    out = []
    for s, (c, r0, n) in enumerate(segs):
        kind = c["kind"]
        if kind == "category":
            lo, hi = C.parquet_stats_finish(host[dict_of[s]].ctypes.data, 2, 0, False)
        elif kind == "text":
            lo, hi = C.parquet_stats_finish(host[s].ctypes.data, 2, 0, False)
        else:
            k, w, fl, _dt, _fmt = NUMERIC[kind]
            lo, hi = C.parquet_stats_finish(host[s].ctypes.data, k, w, bool(fl))
        out.append((c, r0, n, (int(host[s, 0]), lo, hi)))
    return host, out


def _cuts(sizes):
    at, out = 0, []
    for n in sizes:
        out.append((at, n))
        at += n
    return out


def _sized_column(kind, seed):
    """Segments of every size of SIZES, one after the other in one column, so a neighbour's extreme
    lies one row away.  The extremes of a segment stand at its first and last row, or (from 128
    rows) in lane 0 and lane 63 of its second wave; a row beyond both extremes has status 1."""
    rng = np.random.default_rng(seed)
    total = sum(SIZES)
    status = (rng.integers(0, 7, total) == 0).astype(np.uint8)
    if kind == "text":
        values = [bytes(rng.integers(97, 123, int(rng.integers(0, 20))).astype(np.uint8)) for _ in range(total)]
        small, large, beyond = b"A" + bytes([seed]), b"~" + bytes([seed]), b"\xff\xff"
    elif kind == "bool":
        values = np.ones(total, dtype=np.uint8)
        small, large, beyond = 0, 1, 0
    else:
        dt = NUMERIC[kind][3]
        values = rng.integers(-1000, 1000, total).astype(dt)
        small, large, beyond = -5000, 5000, 9000
    for k, (r0, n) in enumerate(_cuts(SIZES)):
        if n == 0:
            continue
        lo, hi = (r0 + 64, r0 + 127) if n >= 128 else (r0, r0 + n - 1)
        if kind == "text":
            values[lo], values[hi] = small + bytes([k]), large + bytes([k])
            if hi == lo:
                values[lo] = small + bytes([k])
        elif kind == "bool":
            values[lo] = 0 if k % 2 else 1
        else:
            values[hi], values[lo] = large + k, small - k
        status[lo] = status[hi] = 0
        if n >= 3:
            values[lo + 1], status[lo + 1] = beyond, 1  # an extreme in a null row is ignored
    return dict(kind=kind, values=values, status=status.tolist(), cuts=_cuts(SIZES))


def _pair(k):
    """Two values that agree up to byte k and differ at byte k."""
    head = bytes((7 * j + 1) % 251 for j in range(k))
    return [head + b"\x02", head + b"\x01"]


def _edge_columns():
    f64 = lambda *v: np.array(v, dtype=np.float64)      # noqa: E731
    neg_nan64 = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]
    neg_nan32 = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]
    floats = [f64(NAN, np.inf, -np.inf, 1.0), f64(NAN, 1.5, -2.0, 7.0, NAN), f64(-0.0, 0.0), f64(0.0, -0.0), f64(0.0, 0.0),
              f64(-0.0, -0.0), f64(5e-324, 0.0), f64(-5e-324, 0.0, 5e-324), f64(NAN, NAN, NAN), f64(neg_nan64, 1.0, 2.0),
              f64(neg_nan64), f64(np.inf), f64(-np.inf, NAN), f64(-1.0, -0.0), f64(0.0, 3.0)]
    f32 = [np.where(np.abs(a) == 5e-324, np.sign(a) * 1e-45, a).astype(np.float32) for a in floats]
    f32[9], f32[10] = np.array([neg_nan32, 1.0, 2.0], np.float32), np.array([neg_nan32], np.float32)

    def numeric(kind, parts, status=None):
        vals = np.concatenate(parts)
        return dict(kind=kind, values=vals, status=[0] * len(vals) if status is None else status,
                    cuts=_cuts([len(p) for p in parts]))

    texts = [[b"", b"\0"], [b"\0", b""], [b"abc", b"ab", b"abcd"], [b"\x7f\x00", b"\x80"], [b"\x80", b"\x7f\xff\xff"],
             *[_pair(k) for k in (6, 7, 8, 13, 14, 62, 63)], *[_pair(k)[::-1] for k in (6, 7, 63)],
             [b"zz", b"a", b"zz", b"a", b"m"], [b"x" * 64, b"x" * 63, b"x" * 64], [b"x" * 65, b"a"], [b"a" * 70, b"a" * 71],
             [b"abcdefg", b"abcdefg\0", b"abcdefg"], [b""], [b"same"] * 3]
    flat = [v for part in texts for v in part]
    text = dict(kind="text", values=flat, status=[0] * len(flat), cuts=_cuts([len(p) for p in texts]))
    nulls = dict(kind="text", values=[b"\xff", b"b", b"c", b"\x00"], status=[1, 0, 0, 2], cuts=[(0, 4), (0, 1), (3, 1)])
    vocab = [b"a", b"m", b"q", b"mm", b"zz", b"y" * 65]
    cat = dict(kind="category", vocab=vocab, values=[1, 2, -1, 3, 2, 1, 0, 4, 5, 1, 6, -1, 2, 2],
               status=[0, 0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 1, 0, 1],
               cuts=[(0, 6), (0, 8), (8, 2), (9, 3), (11, 1), (12, 2), (0, 0)])
    return [numeric("float64", floats), numeric("float32", f32),
            numeric("int32", [np.array([-2 ** 31, 2 ** 31 - 1, 0], np.int32), np.array([2 ** 31 - 1], np.int32),
                              np.array([-2 ** 31, -1], np.int32)]),
            numeric("int64", [np.array([-2 ** 63, 2 ** 63 - 1, 0], np.int64), np.array([2 ** 63 - 1], np.int64),
                              np.array([-2 ** 63, -1], np.int64), np.array([5, -9, 7], np.int64)],
                    status=[0, 0, 0, 0, 0, 0, 1, 1, 1]),         # the last segment: all null
            numeric("bool", [np.array([0, 1, 0], np.uint8), np.array([1, 1], np.uint8), np.array([0], np.uint8),
                             np.array([2, 255], np.uint8)]),
            text, nulls, cat]


def _all_columns():
    return [_sized_column(kind, seed) for seed, kind in enumerate(("int64", "int32", "float64", "float32", "bool", "text"))] \
        + _edge_columns()


def _check_segments(out):
    for c, r0, n, got in out:
        want = _ref(c["kind"], list(c["values"][r0:r0 + n]), c["status"][r0:r0 + n], c.get("vocab"))
        assert got == want, (c["kind"], r0, n, got, want)


def test_stats_raw_cpu():
    before = _stats_launches()
    _host, out = _run_segments(_all_columns(), "cpu")
    assert len(out) > 100
    _check_segments(out)
    assert _stats_launches() == before                  # the host loops


@pytest.mark.gpu
def test_stats_raw(gpu):
    before = _stats_launches()
    dev_rows, out = _run_segments(_all_columns(), "cuda")
    assert _stats_launches() - before == 11             # mark, first, nine rounds: whatever the segments
    _check_segments(out)
    host_rows, _ = _run_segments(_all_columns(), "cpu")
    assert dev_rows.tobytes() == host_rows.tobytes()    # the kernels and the host loops: the same result rows


def test_stats_raw_refusals():
    C = _lib()
    table = np.zeros((1, PE_COLS), dtype=np.int64)
    res = np.zeros((1, PS_COLS), dtype=np.int64)
    before = _stats_launches()
    for args in ((0, 1, 0, 0, 1, 4, 0, 0, res.ctypes.data), (table.ctypes.data, 1, 0, 0, 1, 4, 0, 0, 0),
                 (table.ctypes.data, 2 ** 31 + 1, 0, 0, 1, 4, 0, 0, res.ctypes.data),
                 (table.ctypes.data, 1, 0, 0, 1, 2 ** 31 + 1, 0, 0, res.ctypes.data),
                 (table.ctypes.data, 1, 0, 2, 1, 4, 0, 0, res.ctypes.data),
                 (table.ctypes.data, 1, 0, 0, 0, 4, 0, 4, res.ctypes.data)):       # a text range and no alive bytes
        with pytest.raises(Exception, match="parquet stats"):
            C.parquet_stats_raw(*args, -1, 0)
    with pytest.raises(Exception, match="parquet stats"):
        C.parquet_stats_finish(0, 0, 8, False)
    assert _stats_launches() == before and not res.any()


def test_stats_check_program(tmp_path):
    """tools/parquet_stats_check.cpp builds with the command in its header and prints ok."""
    from alluxio_amd.ops.build import ROCM
    cxx = shutil.which("clang++") or os.path.join(ROCM, "lib", "llvm", "bin", "clang++")
    exe = str(tmp_path / "parquet_stats_check")
    header = open(os.path.join(ROOT, "tools", "parquet_stats_check.cpp")).read().split("#include")[0]
    flags = "-std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined"
    assert flags in header and "-Ialluxio_amd/csrc tools/parquet_stats_check.cpp" in header
    subprocess.run([cxx, *flags.split(), "-Ialluxio_amd/csrc", "tools/parquet_stats_check.cpp", "-o", exe], cwd=ROOT,
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- column_statistics -----------------------------------------------------------------------------------
def _run_column_statistics(device):
    cols = FieldColumns([_col("f", "float64", [NAN, 1.5, -2.0, None, NAN], device),
                         _col("g", "float32", [NAN, None, NAN, NAN, NAN], device),
                         _col("z", "float64", [0.0, 0.0, None, 0.0, 0.0], device),
                         _col("i", "int64", [5, None, -3, 7, 2 ** 63 - 1], device),
                         _col("q", "int32", [None, None, None, None, None], device),
                         _col("b", "bool", [None, True, True, None, True], device),
                         _col("t", "text", ["ab", "ab\0", "", None, "b"], device),
                         _col("c", "category", ["m", None, "q", "m", "m"], device, vocab=["a", "m", "q", "zz"])])
    got = column_statistics(cols)
    assert all(isinstance(s, ParquetStatistics) for s in got)
    assert got[0] == (1, -2.0, 1.5) and got[1] == (1, None, None) and got[3] == (1, -3, 2 ** 63 - 1)
    assert got[2][0] == 1 and [struct.pack("<d", v) for v in got[2][1:]] == [struct.pack("<d", -0.0), struct.pack("<d", 0.0)]
    assert got[4] == (5, None, None) and got[5] == (2, True, True) and got[5].min is True
    assert got[6] == (1, b"", b"b") and got[7] == (1, b"m", b"q")
    assert type(got[3].min) is int and type(got[0].min) is float and type(got[6].min) is bytes
    none = column_statistics(FieldColumns([_col("a", "int64", [], device), _col("t", "text", [], device)]))
    assert none == [(0, None, None), (0, None, None)]


def test_column_statistics_cpu():
    _run_column_statistics("cpu")


@pytest.mark.gpu
def test_column_statistics(gpu):
    before = _stats_launches()
    _run_column_statistics("cuda")
    assert _stats_launches() > before


# ---- the written file -------------------------------------------------------------------------------------
def _file_spec(n=700):
    rng = np.random.default_rng(11)
    vocab = ["aa", "m", "mm", "q", "zz", "unused-first", "~unused-last"]
    words = ["", "a", "ab", "ab\0", "é", "x" * 64, "日本", "zz", "\x7f", "~"]
    fl = [NAN, 0.0, -0.0, np.inf, -np.inf, 5e-324]
    spec = [("i", "int64", [None if r % 7 == 3 else int(rng.integers(-2 ** 62, 2 ** 62)) for r in range(n)]),
            ("q", "int32", [None if 250 <= r < 500 else int(rng.integers(-2 ** 31, 2 ** 31)) for r in range(n)]),
            ("d", "float64", [None if r % 5 == 1 else fl[r % 6] if r % 3 == 0 else float(rng.standard_normal())
                              for r in range(n)]),
            ("f", "float32", [NAN if r < 250 else None if r % 9 == 0 else float(np.float32(rng.standard_normal()))
                              for r in range(n)]),
            ("b", "bool", [None if r % 4 == 0 else bool(r >= 500 or rng.integers(0, 2)) for r in range(n)]),
            ("t", "text", [None if r % 6 == 5 else (words[int(rng.integers(0, len(words)))] + str(r % 13) * (r % 2))[:64]
                           for r in range(n)]),
            ("c", "category", [None if r % 8 == 0 else vocab[int(rng.integers(0, 5))] for r in range(n)]),
            ("rq", "int64", [r * 3 - 1000 for r in range(n)]),
            ("rt", "text", [words[r % len(words)] for r in range(n)])]
    assert max(len(v.encode()) for v in spec[5][2] + spec[8][2] if v is not None) == 64      # at the cap, not above
    return spec, vocab, ["rq", "rt"]


def _plain(stats, physical):
    """pyarrow's (has_min_max, min, max, null_count) with the bounds as bytes, floats by their bits."""
    if not stats.has_min_max:
        return False, None, None, stats.null_count
    enc = {"DOUBLE": lambda v: struct.pack("<d", v), "FLOAT": lambda v: struct.pack("<f", v),
           "BYTE_ARRAY": lambda v: v.encode() if isinstance(v, str) else v}.get(physical, lambda v: v)
    return True, enc(stats.min), enc(stats.max), stats.null_count


def _ours(st, physical):
    if st.min is None:
        return False, None, None, st.null_count
    enc = {"DOUBLE": lambda v: struct.pack("<d", v), "FLOAT": lambda v: struct.pack("<f", v)}.get(physical, lambda v: v)
    return True, enc(st.min), enc(st.max), st.null_count


def _run_file(c, device):
    fs = c.client()
    spec, vocab, required = _file_spec()
    cols = FieldColumns([_col(name, kind, vals, device, vocab) for name, kind, vals in spec])
    want = _arrow(spec, required)
    buf = io.BytesIO()
    pq.write_table(want, buf, row_group_size=250, compression="none")
    ref = pq.ParquetFile(buf).metadata
    with ParquetWriter(fs, "/s/out.parquet", required=required, page_rows=100, write_type="MUST_CACHE", statistics=True) as w:
        w.write(cols, row_group_rows=250)
    blob = _read(fs, "/s/out.parquet")
    assert w.metadata == parquet_metadata(fs, "/s/out.parquet")
    got = pq.ParquetFile(io.BytesIO(blob)).metadata
    assert got.num_row_groups == ref.num_row_groups == 3
    seen = set()
    for g in range(3):
        for j, (name, _kind, _vals) in enumerate(spec):
            a, b, ours = got.row_group(g).column(j), ref.row_group(g).column(j), w.metadata.row_groups[g].columns[j]
            assert a.statistics is not None, name
            assert _plain(a.statistics, a.physical_type) == _plain(b.statistics, b.physical_type), (g, name)
            assert _ours(ours.statistics, ours.physical_type) == _plain(b.statistics, b.physical_type), (g, name)
            seen.add((a.statistics.has_min_max, a.statistics.null_count > 0))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}     # the last: only NaNs
    _same(pq.read_table(io.BytesIO(blob)), want)
    kept = pq.read_table(io.BytesIO(blob), filters=[("rq", ">=", 500)])        # pyarrow prunes by what we wrote
    assert kept["rq"].to_pylist() == [v for v in want["rq"].to_pylist() if v >= 500]
    # statistics=False, and the argument left out: the same bytes as each other, and none of the new fields
    write_parquet_columns(fs, "/s/off.parquet", cols, row_group_rows=250, page_rows=100, required=required,
                          write_type="MUST_CACHE", statistics=False)
    md = write_parquet_columns(fs, "/s/plain.parquet", cols, row_group_rows=250, page_rows=100, required=required,
                               write_type="MUST_CACHE")
    assert _read(fs, "/s/off.parquet") == _read(fs, "/s/plain.parquet") and len(blob) > len(_read(fs, "/s/plain.parquet"))
    assert all(cc.statistics is None for rg in md.row_groups for cc in rg.columns)
    assert pq.ParquetFile(io.BytesIO(_read(fs, "/s/plain.parquet"))).metadata.row_group(0).column(0).statistics is None
    # a text value above the cap: a null count and no bounds, for the text column and for the category
    long_ = FieldColumns([_col("t", "text", ["a", None, "y" * 65], device),
                          _col("c", "category", ["y" * 65, "b", None], device, vocab=["b", "y" * 65, "z" * 80])])
    md = write_parquet_columns(fs, "/s/long.parquet", long_, write_type="MUST_CACHE", statistics=True)
    assert [cc.statistics for cc in md.row_groups[0].columns] == [(1, None, None), (1, None, None)]
    assert md == parquet_metadata(fs, "/s/long.parquet")
    st = pq.ParquetFile(io.BytesIO(_read(fs, "/s/long.parquet"))).metadata.row_group(0).column(0).statistics
    assert not st.has_min_max and st.null_count == 1
    fs.close()
    return blob


def test_statistics_file_cpu():
    before = _stats_launches()
    with _cluster("dram") as c:
        _run_file(c, "cpu")
    assert _stats_launches() == before


@pytest.mark.gpu
def test_statistics_file(gpu):
    before = _stats_launches()
    with _cluster("hbm:0") as c:
        blob = _run_file(c, "cuda")
        assert _stats_launches() > before
        mid = _stats_launches()
        fs = c.client()
        spec, vocab, required = _file_spec()
        cols = FieldColumns([_col(name, kind, vals, "cuda", vocab) for name, kind, vals in spec])
        write_parquet_columns(fs, "/s/host.parquet", _to(cols, "cpu"), row_group_rows=250, page_rows=100, required=required,
                              write_type="MUST_CACHE", statistics=True)
        assert _stats_launches() == mid and _read(fs, "/s/host.parquet") == blob
        fs.close()


@pytest.mark.gpu
def test_statistics_launch_counter(gpu):
    """The statistics launches of a row group do not grow with its columns; none without rows."""
    n = 600
    kinds = ["category", "int64", "text", "int32", "float64", "float32", "bool", "text", "category", "int64", "float64", "bool"]
    vocab = ["a", "b", "c"]

    def column(k, kind, rows):
        vals = [None if (r + k) % 9 == 0 else r for r in range(rows)]
        if kind in ("text", "category"):
            vals = [None if v is None else vocab[v % 3] for v in vals]
        elif kind == "bool":
            vals = [None if v is None else bool(v % 2) for v in vals]
        return _col(f"c{k}", kind, vals, "cuda", vocab)

    with _cluster("hbm:0") as c:
        fs = c.client()
        twelve = FieldColumns([column(k, kind, n) for k, kind in enumerate(kinds)])
        before = _stats_launches()
        write_parquet_columns(fs, "/s/none.parquet", FieldColumns([column(k, kind, 0) for k, kind in enumerate(kinds[:3])]),
                              write_type="MUST_CACHE", statistics=True)
        assert _stats_launches() == before
        write_parquet_columns(fs, "/s/twelve.parquet", twelve, write_type="MUST_CACHE", statistics=True)
        mid = _stats_launches()
        write_parquet_columns(fs, "/s/two.parquet", FieldColumns([twelve[0], twelve[1]]), write_type="MUST_CACHE",
                              statistics=True)
        assert mid - before == _stats_launches() - mid == 11
        end = _stats_launches()
        write_parquet_columns(fs, "/s/off.parquet", twelve, write_type="MUST_CACHE")
        assert _stats_launches() == end
        fs.close()


# ---- the reader's view --------------------------------------------------------------------------------------
def _run_reader_view(c):
    fs = c.client()
    n = 300
    tbl = pa.table({"i": pa.array([None if r % 7 == 0 else r - 100 for r in range(n)], pa.int64()),
                    "q": pa.array([r * 5 - 700 for r in range(n)], pa.int32()),
                    "d": pa.array([NAN if r % 11 == 0 else r / 3 - 20 for r in range(n)], pa.float64()),
                    "f": pa.array([None if r % 2 else np.float32(r) / 7 for r in range(n)], pa.float32()),
                    "b": pa.array([None if r % 3 == 0 else r > 200 for r in range(n)], pa.bool_()),
                    "s": pa.array([None if r % 5 == 0 else f"v{r % 17}é" for r in range(n)], pa.string()),
                    "u": pa.array([None if r % 4 == 0 else 2 ** 31 + r for r in range(n)], pa.uint32()),
                    "ts": pa.array([r * 10 ** 6 for r in range(n)], pa.timestamp("us")),
                    "dec": pa.array([None if r % 6 == 0 else r for r in range(n)], pa.decimal128(9, 0)),
                    "day": pa.array([r for r in range(n)], pa.date32()),
                    "i8": pa.array([r % 100 - 50 for r in range(n)], pa.int8())})
    buf = io.BytesIO()
    pq.write_table(tbl, buf, row_group_size=100)
    fs.write_file("/s/arrow.parquet", buf.getvalue(), write_type="MUST_CACHE")
    md, ref = parquet_metadata(fs, "/s/arrow.parquet"), pq.ParquetFile(buf).metadata
    for g, rg in enumerate(md.row_groups):
        for j, cc in enumerate(rg.columns):
            rs = ref.row_group(g).column(j).statistics
            if cc.name in ("u", "dec"):                 # unsigned order, DECIMAL: the bounds are not ours to read
                assert cc.statistics == (rs.null_count, None, None), cc.name
                continue
            lo, hi = rs.min, rs.max
            if cc.name == "s":
                lo, hi = lo.encode(), hi.encode()
            elif cc.name in ("ts", "day"):              # logical types are not interpreted: the physical integer
                unit = 10 ** 6 if cc.name == "ts" else 1
                lo, hi = g * 100 * unit, (g * 100 + 99) * unit
            assert cc.statistics == (rs.null_count, lo, hi), cc.name
            assert type(cc.statistics.min) is {"INT32": int, "INT64": int, "FLOAT": float, "DOUBLE": float, "BOOLEAN": bool,
                                               "BYTE_ARRAY": bytes}[cc.physical_type]
    # a file written without statistics: ``statistics is None``
    buf = io.BytesIO()
    pq.write_table(tbl, buf, write_statistics=False)
    fs.write_file("/s/bare.parquet", buf.getvalue(), write_type="MUST_CACHE")
    assert all(cc.statistics is None for rg in parquet_metadata(fs, "/s/bare.parquet").row_groups for cc in rg.columns)
    assert parquet_matching_row_groups(fs, "/s/bare.parquet", [("i", ">", 10 ** 9)]) == [0]
    fs.close()


def test_statistics_reader_view_cpu():
    with _cluster("dram") as c:
        _run_reader_view(c)


# ---- pruning ---------------------------------------------------------------------------------------------------
GROUPS, GROUP_ROWS = 6, 50


def _prune_rows():
    n = GROUPS * GROUP_ROWS
    rng = np.random.default_rng(5)
    return {"k": [r * 2 for r in range(n)],
            "name": [None if r % 10 == 9 else f"n{r // GROUP_ROWS}{chr(97 + r % 7)}" for r in range(n)],
            "x": [NAN if r % 8 == 0 else None if r % 8 == 1 else float(r // GROUP_ROWS * 10 + rng.integers(0, 10))
                  for r in range(n)],
            "hole": [None if 100 <= r < 150 or r % 3 == 0 else r % 50 for r in range(n)],
            "flag": [r >= 200 for r in range(n)],
            "full": [r % 5 for r in range(n)]}


def _prune_table():
    rows = _prune_rows()
    types = {"k": pa.int64(), "name": pa.string(), "x": pa.float64(), "hole": pa.int32(), "flag": pa.bool_(), "full": pa.int32()}
    return pa.table({k: pa.array(v, types[k]) for k, v in rows.items()})


FILTERS = [[("k", "==", 120)], [("k", "=", 121)], [("k", "==", -1)], [("k", "!=", 0)], [("k", "<", 100)], [("k", "<=", 100)],
           [("k", "<", 0)], [("k", ">", 498)], [("k", ">=", 598)], [("k", ">", 598)], [("k", "in", [98, 100, 401])],
           [("k", "in", [])], [("k", "in", {-5, 1000})], [("k", ">=", 150), ("k", "<", 250)],
           [("name", "==", "n3c")], [("name", ">=", "n5")], [("name", "<", "n1")], [("name", "in", ["n0a", "n4g", "zz"])],
           [("name", "!=", "n0a")], [("name", "is_null", True)], [("name", "is_null", False)],
           [("x", ">", 45.0)], [("x", "<=", 9)], [("x", "==", 25.0)], [("x", "!=", 25.0)], [("x", "==", NAN)],
           [("x", "is_null", True)], [("x", ">=", 1e9)],
           [("hole", "==", 7)], [("hole", "<", 1000)], [("hole", "is_null", True)], [("hole", "is_null", False)],
           [("hole", "!=", 7)], [("hole", ">", 48)],
           [("flag", "==", True)], [("flag", "==", False)], [("flag", "!=", True)], [("flag", "!=", False)],
           [("full", "is_null", True)], [("full", "is_null", False)], [("full", "!=", 3)],
           [("k", ">", 300), ("name", "<", "n7"), ("x", "<", 45)],
           [[("k", "<", 50)], [("k", ">", 550)]], [[("k", "<", 0)], [("name", "==", "n2a"), ("flag", "==", False)]]]


def _cannot_rule_out(rows, op, v):
    """Whether a row group's true min, max and null count leave a match possible: the pruning rules
    written out over the rows themselves."""
    live = [x for x in rows if x is not None]
    nulls = len(rows) - len(live)
    is_float = any(isinstance(x, float) for x in live)
    ordered = [x for x in live if x == x]
    if op == "is_null":
        return nulls > 0 if v else nulls < len(rows)
    if isinstance(v, str):
        v = v.encode()
    ordered = [x.encode() if isinstance(x, str) else x for x in ordered]
    if op == "!=":
        return not (ordered and min(ordered) == max(ordered) == v and not is_float)
    if nulls == len(rows):
        return False
    if not ordered:
        return True
    lo, hi = min(ordered), max(ordered)
    if op == "in":
        return any(lo <= (x.encode() if isinstance(x, str) else x) <= hi for x in v)
    if v != v:
        return True
    return {"==": lo <= v <= hi, "=": lo <= v <= hi, "<": lo < v, "<=": lo <= v, ">": hi > v, ">=": hi >= v}[op]


def _expected(filt):
    rows = _prune_rows()
    alts = filt if isinstance(filt[0], list) else [filt]
    return [g for g in range(GROUPS)
            if any(all(_cannot_rule_out(rows[name][g * GROUP_ROWS:(g + 1) * GROUP_ROWS], op, v) for name, op, v in alt)
                   for alt in alts)]


def _columns_equal(a: FieldColumns, b: FieldColumns):
    assert a.names == b.names and a.rows == b.rows
    for x, y in zip(a, b):
        assert x.type == y.type and x.status.cpu().tolist() == y.status.cpu().tolist(), x.name
        assert x.tolist() == y.tolist() or all(p == q or (p != p and q != q) for p, q in zip(x.tolist(), y.tolist())), x.name


def _run_pruning(c, device):
    fs = c.client()
    tbl = _prune_table()
    buf = io.BytesIO()
    pq.write_table(tbl, buf, row_group_size=GROUP_ROWS, compression="none")
    fs.write_file("/s/prune.parquet", buf.getvalue(), write_type="MUST_CACHE")
    path = "/s/prune.parquet"
    decode = _lib().parquet_decode_launches
    key = tbl["k"].to_pylist()
    some_pruned = 0
    for filt in FILTERS:
        kept = parquet_matching_row_groups(fs, path, filt)
        assert kept == _expected(filt), filt
        some_pruned += len(kept) < GROUPS
        terms = [t for alt in (filt if isinstance(filt[0], list) else [filt]) for t in alt]
        # pyarrow has no is_null op, and a NaN or an empty collection to compare with is not worth its while
        if not any(t[1] == "is_null" or (t[1] == "in" and not t[2]) or t[2] != t[2] for t in terms):
            theirs = pq.read_table(io.BytesIO(buf.getvalue()), filters=filt)["k"].to_pylist()
            ours = {k for g in kept for k in key[g * GROUP_ROWS:(g + 1) * GROUP_ROWS]}
            assert set(theirs) <= ours, filt             # every row pyarrow returns is among ours
    assert some_pruned > 20
    assert parquet_matching_row_groups(fs, path, [("name", "<", b"n1")]) == [0]      # bytes as well as str
    assert parquet_matching_row_groups(fs, path, [("flag", ">", False)]) == [4, 5]
    for filt in ([("k", ">=", 150), ("k", "<", 250)], [("hole", "is_null", False), ("name", ">=", "n2")], [("k", "==", 120)]):
        kept = parquet_matching_row_groups(fs, path, filt)
        assert 0 < len(kept) < GROUPS
        a = decode()
        got = read_parquet_columns(fs, path, filters=filt, device=device)
        b = decode()
        want = read_parquet_columns(fs, path, row_groups=kept, device=device)
        assert b - a == decode() - b
        _columns_equal(got, want)
        parts = list(parquet_row_groups(fs, path, ["k"], filters=filt, device=device))
        assert [p["k"].tolist() for p in parts] == [key[g * GROUP_ROWS:(g + 1) * GROUP_ROWS] for g in kept]
    # row_groups and filters together: the filter prunes among the row groups named, in their order
    assert parquet_matching_row_groups(fs, path, [("k", "<", 250)], row_groups=[5, 2, 0, 2]) == [2, 0, 2]
    # a filter on a column that is not selected still prunes; a kept row group comes back whole
    got = read_parquet_columns(fs, path, ["name"], filters=[("k", "==", 120)], device=device)
    assert got.names == ["name"] and got["name"].tolist() == [None if v is None else v.encode()
                                                             for v in tbl["name"].to_pylist()[50:100]]
    # everything pruned: no rows, the right types, nothing launched
    import torch
    a = decode()
    none = read_parquet_columns(fs, path, {"k": ("k", None), "x": ("x", None), "name": ("name", "category"), "t": ("name", None),
                                           "h": ("hole", "int64"), "flag": ("flag", None)}, filters=[("k", "<", 0)],
                                device=device)
    assert decode() == a and none.rows == 0 and none.names == ["k", "x", "name", "t", "h", "flag"]
    assert [c_.values.dtype for c_ in (none["k"], none["x"], none["h"], none["flag"])] == \
           [torch.int64, torch.float64, torch.int64, torch.bool]
    assert none["name"].values.dtype == torch.int32 and none["t"].tolist() == []
    assert list(parquet_row_groups(fs, path, ["k"], filters=[("k", "<", 0)], device=device))[0].rows == 0
    # a file without statistics prunes nothing
    bare = io.BytesIO()
    pq.write_table(tbl, bare, row_group_size=GROUP_ROWS, compression="none", write_statistics=False)
    fs.write_file("/s/bare.parquet", bare.getvalue(), write_type="MUST_CACHE")
    for filt in FILTERS:
        assert parquet_matching_row_groups(fs, "/s/bare.parquet", filt) == list(range(GROUPS))
    assert read_parquet_columns(fs, "/s/bare.parquet", ["k"], filters=[("k", "<", 0)], device=device).rows == len(key)
    # pruning comes first: a row group that is ruled out may hold what the reader refuses
    snappy = io.BytesIO()
    with pq.ParquetWriter(snappy, tbl.schema, compression="snappy") as w:
        w.write_table(tbl.slice(0, 50))
    fs.write_file("/s/snappy.parquet", snappy.getvalue(), write_type="MUST_CACHE")
    assert read_parquet_columns(fs, "/s/snappy.parquet", ["k"], filters=[("k", ">", 10 ** 6)], device=device).rows == 0
    with pytest.raises(NotImplementedError, match="SNAPPY"):
        read_parquet_columns(fs, "/s/snappy.parquet", ["k"], filters=[("k", ">", 10)], device=device)
    # our own files prune the same way
    spec = {k: (k, None) for k in tbl.column_names}
    cols = read_parquet_columns(fs, path, spec, device=device)
    write_parquet_columns(fs, "/s/ours.parquet", cols, row_group_rows=GROUP_ROWS, write_type="MUST_CACHE", statistics=True)
    write_parquet_columns(fs, "/s/ours-bare.parquet", cols, row_group_rows=GROUP_ROWS, write_type="MUST_CACHE")
    for filt in FILTERS:
        assert parquet_matching_row_groups(fs, "/s/ours.parquet", filt) == _expected(filt), filt
        assert parquet_matching_row_groups(fs, "/s/ours-bare.parquet", filt) == list(range(GROUPS))
    # the errors, before anything is read
    a = decode()
    with pytest.raises(KeyError, match="nope"):
        read_parquet_columns(fs, path, filters=[("nope", "==", 1)], device=device)
    with pytest.raises(ValueError, match="like"):
        read_parquet_columns(fs, path, filters=[("k", "like", 1)], device=device)
    for bad in (("k", "==", 1.5), ("k", "==", "1"), ("k", "==", True), ("x", "<", "1"), ("flag", "==", 1), ("name", "==", 3),
                ("name", "in", [b"a", 3]), ("k", "in", 5), ("k", "is_null", 1), ("name", "in", "n0a")):
        with pytest.raises(TypeError, match=bad[0]):
            parquet_matching_row_groups(fs, path, [bad])
    with pytest.raises(TypeError, match="'k'"):
        parquet_row_groups(fs, path, filters=[[("k", "<", 5)], [("k", ">", None)]], device=device)
    with pytest.raises(IndexError):
        parquet_matching_row_groups(fs, path, [("k", "<", 5)], row_groups=[6])
    assert decode() == a
    # no filters: nothing changes
    assert parquet_matching_row_groups(fs, path, None) == list(range(GROUPS)) == parquet_matching_row_groups(fs, path, [])
    _columns_equal(read_parquet_columns(fs, path, device=device, filters=None), read_parquet_columns(fs, path, device=device))
    fs.close()


def test_pruning_cpu():
    with _cluster("dram") as c:
        _run_pruning(c, "cpu")


@pytest.fixture(params=[pytest.param(0, id="gpu-v0"), pytest.param(1, id="gpu-v1")])
def variant(request, gpu):
    default = _lib().parquet_decode_variant()
    _lib().set_parquet_decode_variant(request.param)
    yield request.param
    _lib().set_parquet_decode_variant(default)


@pytest.mark.gpu
def test_pruning(variant):
    before = _lib().parquet_decode_launches()
    with _cluster("hbm:0") as c:
        _run_pruning(c, "cuda")
    assert _lib().parquet_decode_launches() > before
