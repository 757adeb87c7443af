"""json_text_measure_raw / json_text_emit_raw: JSON string contents unescaped into packed bytes.
The yardstick is ``json.loads(b'"' + content + b'"')`` encoded with ``"surrogatepass"``, compared
byte for byte; a content that ``json.loads`` cannot read for its escapes is bad (status 2, length
0).  Lengths, status and offsets are compared exactly.

Ids: `cpu` runs the host loops over numpy buffers (device=-1); `gpu-v0` (one lane per value) and
`gpu-v1` (sixteen lanes per value, 256-byte steps of 16-byte vectors) run the kernels.  On the GPU
the data is a slice in the middle of a larger device tensor whose other bytes are ``{ } " \\ , :``,
at an odd phase, so a read outside a value changes a result instead of going unseen.  The output
buffer has guard bytes on both sides and is filled before the call, so a write outside a value's
range shows."""
import json

import numpy as np
import pytest

from alluxio_amd.ops.native import lib

STEP = 256          # variant 1: bytes of a value that a 16-lane group takes per step
VEC = 16            # and per lane
PAD = 4099          # bytes before the slice on the device: an odd phase
GUARD = 67          # bytes on either side of the output
FILL = 0xEE         # the output and its guards before the call
LENGTHS = [0, 1, 2, 15, 16, 17, 255, 256, 257, 511, 512, 513, 4099]
POSITIONS = list(range(0, 34)) + list(range(250, 261))
SIMPLE = [b'\\"', b"\\\\", b"\\/", b"\\b", b"\\f", b"\\n", b"\\r", b"\\t"]


def _yard(v: bytes):
    """The yardstick: the unescaped bytes of a content that is UTF-8 (lone surrogates included), or
    None for a value with a bad escape.  Raw control bytes pass through (strict=False)."""
    try:
        s = json.loads('"' + v.decode("utf-8", "surrogatepass") + '"', strict=False)
    except ValueError:
        return None
    return s.encode("utf-8", "surrogatepass")


def test_the_yardstick_on_small_examples():
    assert _yard(b"") == b"" and _yard(b"a\\nb") == b"a\nb" and _yard(b'\\"\\\\\\/') == b'"\\/'
    assert _yard(b"\\ud800") == b"\xed\xa0\x80" and _yard(b"\\ud83d\\ude00") == b"\xf0\x9f\x98\x80"
    assert _yard(b"\\ude00\\ud83d") == b"\xed\xb8\x80\xed\xa0\xbd" and _yard(b"\\u00E9\\u00e9") == "éé".encode()
    assert _yard(b"\\") is None and _yard(b"\\x") is None and _yard(b"\\u12") is None and _yard(b"\\u12g4") is None
    assert _yard("é\x01\\t".encode()) == "é\x01\t".encode() and _yard(b"\xed\xa0\xbd\\ude00") == b"\xed\xa0\xbd\xed\xb8\x80"


class _Env:
    def __init__(self, mode):
        self.mode, self.gpu = mode, mode != "cpu"

    def run(self, data: bytes, start, length, status=None, offsets=None, out_bytes=None, emit_status="measured"):
        """measure, then emit with the exclusive scan of the measured lengths (or with `offsets` /
        `out_bytes` as given) and the measured status (or the input status).  Returns (lengths, status,
        offsets, the output bytes); the guards are checked."""
        start = np.ascontiguousarray(start, dtype=np.int64)
        length = np.ascontiguousarray(length, dtype=np.int32)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.uint8)
        n = len(start)
        C = lib()
        if self.gpu:
            import torch
            fill = np.frombuffer(b'{}"\\,:', dtype=np.uint8)
            big = np.resize(fill, PAD + len(data) + PAD)
            big[PAD:PAD + len(data)] = np.frombuffer(data, dtype=np.uint8)
            dev = torch.from_numpy(big).cuda()
            d_start, d_length = torch.from_numpy(start).cuda(), torch.from_numpy(length).cuda()
            d_status = None if status is None else torch.from_numpy(status).cuda()
            sp = 0 if d_status is None else d_status.data_ptr()
            d_len = torch.full((n + 2,), 77, dtype=torch.int32, device="cuda")
            d_st = torch.full((n + 2,), 9, dtype=torch.uint8, device="cuda")
            C.json_text_measure_raw(dev.data_ptr() + PAD, len(data), d_start.data_ptr(), d_length.data_ptr(), sp, n, 0,
                                    d_len.data_ptr() + 4, d_st.data_ptr() + 1)
            torch.cuda.synchronize()
            lens, st = d_len.cpu().numpy(), d_st.cpu().numpy()
        else:
            buf = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(1, np.uint8)
            sp = 0 if status is None else status.ctypes.data
            lens, st = np.full(n + 2, 77, np.int32), np.full(n + 2, 9, np.uint8)
            C.json_text_measure_raw(buf.ctypes.data, len(data), start.ctypes.data, length.ctypes.data, sp, n, -1,
                                    lens.ctypes.data + 4, st.ctypes.data + 1)
        assert lens[0] == 77 and lens[-1] == 77 and st[0] == 9 and st[-1] == 9, "a guard element was written"
        lens, st = lens[1:-1].copy(), st[1:-1].copy()
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        total = int(offsets[-1]) if out_bytes is None else out_bytes
        if self.gpu:
            d_out = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            d_off = torch.from_numpy(offsets).cuda()
            ep = sp if emit_status == "input" else (d_st.data_ptr() + 1)
            C.json_text_emit_raw(dev.data_ptr() + PAD, len(data), d_start.data_ptr(), d_length.data_ptr(), ep, n, 0,
                                 d_off.data_ptr(), d_out.data_ptr() + GUARD, total)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
        else:
            out = np.full(GUARD + total + GUARD, FILL, np.uint8)
            ep = sp if emit_status == "input" else st.ctypes.data
            C.json_text_emit_raw(buf.ctypes.data, len(data), start.ctypes.data, length.ctypes.data, ep, n, -1,
                                 offsets.ctypes.data, out.ctypes.data + GUARD, total)
        assert (out[:GUARD] == FILL).all() and (out[GUARD + total:] == FILL).all(), "a guard byte was written"
        return lens, st, offsets, out[GUARD:GUARD + total].tobytes()

    def check(self, data, start, length, status=None, emit_status="measured"):
        n = len(start)
        want, wst = [], []
        for r in range(n):
            s, l = int(start[r]), int(length[r])
            if status is not None and status[r] != 0:
                want.append(b"")
                wst.append(int(status[r]))
            elif not (s >= 0 and l >= 0 and s + l <= len(data)):
                want.append(b"")
                wst.append(2)
            else:
                w = _yard(data[s:s + l])
                want.append(w or b"")
                wst.append(2 if w is None else 0)
        lens, st, offsets, out = self.run(data, start, length, status, emit_status=emit_status)
        assert st.tolist() == wst
        assert lens.tolist() == [len(w) for w in want]
        assert out == b"".join(want)
        return want, wst

    def check_values(self, values, lead=0, emit_status="measured"):
        """Each value after `lead` bytes that belong to none (backslashes: a carry from them would show)."""
        data, start = b"", []
        for v in values:
            data += b"\\" * lead
            start.append(len(data))
            data += v
        return self.check(data + b"\\", start, [len(v) for v in values], None, emit_status)


@pytest.fixture(params=[pytest.param(("cpu", 0), id="cpu"),
                        pytest.param(("gpu", 0), marks=pytest.mark.gpu, id="gpu-v0"),
                        pytest.param(("gpu", 1), marks=pytest.mark.gpu, id="gpu-v1")])
def env(request):
    mode, variant = request.param
    if mode == "cpu":
        yield _Env(mode)
        return
    request.getfixturevalue("gpu")
    default = lib().json_text_variant()
    lib().set_json_text_variant(variant)
    assert lib().json_text_variant() == variant
    yield _Env(mode)
    lib().set_json_text_variant(default)


def _letters(n, seed=0):
    return bytes(0x61 + (i * 7 + seed) % 23 for i in range(n))


def _with_escapes(n, seed=0):
    """n bytes with a simple escape every 11 bytes or so; never cut inside one."""
    v = bytearray(_letters(n, seed))
    for k, i in enumerate(range(3 + seed % 5, n - 1, 11)):
        v[i:i + 2] = SIMPLE[(k + seed) % len(SIMPLE)]
    return bytes(v)


def _put(n, p, piece, seed=0):
    v = bytearray(_letters(max(n, p + len(piece)), seed))
    v[p:p + len(piece)] = piece
    return bytes(v)


# ---- cases ---------------------------------------------------------------------------------------
def test_lengths_at_every_start_phase(env):
    for lead in (0, 1, 7, 15):
        env.check_values([_letters(n, lead) for n in LENGTHS], lead=lead)
        want, st = env.check_values([_with_escapes(n, lead) for n in LENGTHS], lead=lead)
        assert set(st) == {0} and sum(len(w) for w in want) < sum(LENGTHS)
        env.check_values([_with_escapes(n, lead)[:-1] + b"\\" for n in LENGTHS if n], lead=lead)   # all bad


def test_simple_escapes_at_every_phase(env):
    values = [_put(300, p, e, p) for e in SIMPLE for p in POSITIONS]
    want, st = env.check_values(values)
    assert set(st) == {0} and all(len(w) == 299 for w in want)
    env.check_values(values, lead=3)
    # the backslash as the last byte of a vector and of a step, its code first in the next; runs
    values = [_put(600, p - 1, e) for e in SIMPLE for p in (VEC, 2 * VEC, STEP - VEC, STEP, STEP + VEC, 2 * STEP)]
    values += [_put(600, p - k, b"\\" * k + b"n") for k in range(1, 36) for p in (VEC, STEP, STEP + 7)]
    values += [_put(600, p - k, b"\\" * k) for k in range(2, 36, 2) for p in (VEC, STEP, STEP + 7)]
    values += [_put(600, p - k, b"\\" * k + b"q") for k in range(1, 36) for p in (VEC, STEP)]      # odd runs: bad
    values += [b"\\" * k for k in (2, 16, 32, 256, 258, 512, 1024)] + [b"\\" * k + b"t" for k in (15, 17, 255, 257, 511)]
    want, st = env.check_values(values)
    assert 0 in st and 2 in st
    env.check_values(values, lead=5)


def _u_pieces():
    return [b"\\u0041", b"\\u007f", b"\\u00e9", b"\\u07FF", b"\\u0800", b"\\u20AC", b"\\uffff", b"\\uFFFF", b"\\u0000",
            b"\\ud83d\\ude00", b"\\uD83D\\uDE00", b"\\udbff\\udfff", b"\\ud800\\udc00", b"\\ud800", b"\\udbff", b"\\udc00",
            b"\\udfff", b"\\ude00\\ud83d", b"\\ud83d\\ud83d\\ude00", b"\\ud83dx\\ude00", b"\\ud83d\\n\\ude00",
            b"\\ud83d\\u00e9", b"\\ud83d\\\\ude00"]


def test_u_escapes_around_vector_and_step_edges(env):
    values = []
    for piece in _u_pieces():
        for edge in (VEC, STEP, 2 * STEP):
            for p in range(max(0, edge - 12), edge + 2):
                values.append(_put(edge + 40, p, piece, p))
                values.append(_put(0, p, piece, p))                   # the value ends with the escape
    want, st = env.check_values(values)
    assert set(st) == {0}
    env.check_values(values, lead=1)
    # a step with a \u escape between steps without, and simple escapes around it
    env.check_values([_with_escapes(256, 1) + b"\\u00e9" + _with_escapes(700, 2) + b"\\ud83d\\ude00" + _with_escapes(300, 3),
                      _with_escapes(250, 4) + b"\\ud83d\\ude00" * 30 + _with_escapes(20, 5)])


def test_bad_escapes(env):
    bad = [b"\\x", b"\\a", b"\\U0041", b"\\'", b"\\0", b"\\ ", b"\\u", b"\\u0", b"\\u00", b"\\u004", b"\\u004g", b"\\uz041",
           b"\\u00 1", b"\\u-123", b"\\u+123"]
    values = []
    for n in (40, 300, 600):
        for piece in bad:
            values += [piece + _letters(n), _put(n, n // 2, piece), _letters(n) + piece, _put(n, 255, piece)]
            values += [_with_escapes(n) + b"z", _letters(n) + piece[:-1] if len(piece) > 2 else b"\\"]
        values += [_letters(n) + b"\\", _letters(n) + b"\\\\\\", _put(n + 20, n, b"\\ud83d\\ude0"), _put(n + 20, n, b"\\ud83d\\u")]
    want, st = env.check_values(values)
    assert st.count(2) > len(values) // 2 and st.count(0) > len(values) // 8   # the good neighbours are untouched
    env.check_values(values, lead=2)


def test_bytes_that_are_no_utf8_and_raw_quotes_pass_through(env):
    vals = [b'\xff\\n\xfe"', b'"\\""', b"\x80" * 300 + b"\\t" + b"\xc3", b'a"b\\u00e9"']
    data = b"".join(vals)
    start = np.concatenate([[0], np.cumsum([len(v) for v in vals])[:-1]])
    lens, st, _, out = env.run(data, start, [len(v) for v in vals])
    assert st.tolist() == [0, 0, 0, 0] and lens.tolist() == [4, 3, 302, 6]
    assert out == b'\xff\n\xfe"' + b'"""' + b"\x80" * 300 + b"\t\xc3" + b'a"b\xc3\xa9"'


def test_values_that_are_not_live(env):
    vals = [b"a\\nb", b"zzzz", b"zzzz", b"zzzz", b"zzzz", b"c\\u00e9d", b"zz\\q", _with_escapes(300), b"zzzz"]
    data = b"".join(vals)
    start = np.concatenate([[0], np.cumsum([len(v) for v in vals])[:-1]]).astype(np.int64)
    length = np.array([len(v) for v in vals], dtype=np.int32)
    status = np.zeros(len(vals), np.uint8)
    status[1], status[2] = 1, 3
    start[3] = -1
    length[4] = -1
    start[8] = len(data) - 3                            # start + length = data_bytes + 1
    want, st = env.check(data, start, length, status)
    assert st == [0, 1, 3, 2, 2, 0, 2, 0, 2] and [len(w) for w in want[:7]] == [3, 0, 0, 0, 0, 4, 0]
    env.check(data, start, length, status, emit_status="input")      # emit finds the bad value itself
    start[1], length[2] = 2 ** 62, 2 ** 31 - 1          # far outside, without a status array
    want, st = env.check(data, start, length, None)
    assert st[:5] == [0, 2, 2, 2, 2]
    start[8] = len(data) - 4                            # the value that ends with the data is live
    assert env.check(data, start, length, None)[0][8] == b"zzzz"


def _windowed(want, offsets, out_bytes):
    """What emit may write: value r inside [offsets[r], offsets[r + 1]) cut to [0, out_bytes)."""
    out = bytearray([FILL]) * out_bytes
    for r, w in enumerate(want):
        b, e = int(offsets[r]), min(int(offsets[r + 1]), out_bytes)
        for j, c in enumerate(w):
            if 0 <= b + j < e:
                out[b + j] = c
    return bytes(out)


@pytest.mark.parametrize("offsets,out_bytes", [
    ([0, 3, 8, 12, 500, 510], 600),                     # too small for values 0 and 3
    ([-5, 3, 5, 40, 50, 60], 45),                       # before the buffer, and cut by its end
    ([700, 800, 900, 1000, 1100, 1200], 600),           # past out_bytes altogether
    ([9, 4, 4, 0, 0, 0], 600),                          # decreasing: empty windows
    ([-2 ** 63, -2 ** 62, 0, 0, 2 ** 63 - 1, 2 ** 63 - 1], 600),   # as far out as int64 goes
    ([0, 8, 13, 17, 17 + 300, 17 + 310], 17 + 129),     # value 3 is cut by its window and by the buffer
    ([-301, 7, 12, 16, 16 + 530, 16 + 540], 600),       # the long value first, 301 bytes before the buffer
], ids=["small", "straddle", "past", "decreasing", "extreme", "short-buffer", "negative-long"])
@pytest.mark.parametrize("emit_status", ["measured", "input"])
def test_emit_with_inconsistent_offsets(env, offsets, out_bytes, emit_status):
    vals = [b"abcdefgh", b"ij\\nkl", b"m\\u00e9p", _with_escapes(530, 3) + b"\\ud83d\\ude00" + _with_escapes(200, 1), b"x\\qyz"]
    if offsets[0] == -301:
        vals[0], vals[3] = vals[3], vals[0]
    data = b"".join(vals)
    start = np.concatenate([[0], np.cumsum([len(v) for v in vals])[:-1]])
    want = [_yard(v) or b"" for v in vals]
    before = lib().json_text_launches()
    lens, st, _, out = env.run(data, start, [len(v) for v in vals], None, offsets=offsets, out_bytes=out_bytes,
                               emit_status=emit_status)
    assert lens.tolist() == [len(w) for w in want] and st.tolist() == [0, 0, 0, 0, 2]
    assert out == _windowed(want, offsets, out_bytes)   # no error, nothing outside the windows, nothing for the bad value
    assert lib().json_text_launches() == before + (2 if env.gpu else 0)


def test_argument_errors_and_empty_calls(env):
    C = lib()
    before = C.json_text_launches()
    one = np.zeros(2, np.int64)
    p = one.ctypes.data                                 # any non-null address: a rejected call touches nothing
    device = 0 if env.gpu else -1
    for args in ((p, 4, 0, p, 0, 1, device, p, p), (p, 4, p, 0, 0, 1, device, p, p), (0, 4, p, p, 0, 1, device, p, p),
                 (p, 4, p, p, 0, 1, device, 0, p), (p, 4, p, p, 0, 1, device, p, 0), (p, 4, p, p, 0, 2 ** 31 + 1, device, p, p)):
        with pytest.raises(C.StoreError) as e:
            C.json_text_measure_raw(*args)
        assert e.value.args[0] == 6                     # the store's invalid-argument code
    for args in ((p, 4, 0, p, 0, 1, device, p, p, 8), (p, 4, p, 0, 0, 1, device, p, p, 8), (p, 4, p, p, 0, 1, device, 0, p, 8),
                 (p, 4, p, p, 0, 1, device, p, 0, 8), (0, 4, p, p, 0, 1, device, p, p, 8)):
        with pytest.raises(C.StoreError) as e:
            C.json_text_emit_raw(*args)
        assert e.value.args[0] == 6
    assert C.json_text_launches() == before             # nothing was launched
    C.json_text_measure_raw(0, 0, 0, 0, 0, 0, device, 0, 0)   # n = 0: null arrays are fine and nothing is launched
    C.json_text_emit_raw(0, 0, 0, 0, 0, 0, device, 0, 0, 0)
    lens, st, offsets, out = env.run(b"", [], [])
    assert lens.size == 0 and offsets.tolist() == [0] and out == b"" and C.json_text_launches() == before
    env.check_values([b"a\\nb"])
    assert C.json_text_launches() == before + (2 if env.gpu else 0)


# ---- seeded random strings through json.dumps ----------------------------------------------------
PIECES = ["a", "bc", " ", "\n", "\t", "\r", "\b", "\f", '"', "\\", "/", "{", "}", "é", "€", "中", "\U0001f600", "\U0010ffff",
          "\ud83d", "\udc00", "\x00", "\x1f", "\x7f", "\\n", "\\u0041", "x" * 40]


def _random_strings(n, seed):
    rng = np.random.default_rng(seed)
    lens = np.minimum(rng.geometric(0.05, n) - 1, 400)
    lens[rng.integers(0, n, 20)] = rng.integers(300, 401, 20)
    lens[0], lens[1] = 400, 0
    return ["".join(PIECES[i] for i in rng.integers(0, len(PIECES), int(k))) for k in lens]


def test_random_strings_and_determinism(env):
    strings = _random_strings(2000, 31)
    values, want = [], []
    for i, s in enumerate(strings):
        values.append(json.dumps(s, ensure_ascii=bool(i % 2)).encode("utf-8", "surrogatepass")[1:-1])
        # json.loads joins an escaped high surrogate and an escaped low one that follows it
        want.append(json.loads('"' + values[-1].decode("utf-8", "surrogatepass") + '"').encode("utf-8", "surrogatepass"))
    assert max(len(v) for v in values) > 1200 and min(len(v) for v in values) == 0
    data, start = b"", []
    for v in values:
        start.append(len(data) + 1)
        data += b"\\" + v
    length = [len(v) for v in values]
    lens, st, offsets, out = env.run(data, start, length)
    assert st.tolist() == [0] * len(values) and lens.tolist() == [len(w) for w in want]
    assert out == b"".join(want)
    again = env.run(data, start, length)
    assert again[3] == out and again[0].tolist() == lens.tolist()     # two runs give identical bytes
