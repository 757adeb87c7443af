"""text_measure_raw / text_emit_raw: the bytes of span values with doubled quotes collapsed, packed.
The yardstick is ``bytes.replace(q + q, q)`` in Python, compared byte for byte; lengths and offsets
are compared exactly.

Ids: `cpu` runs the host loops over numpy buffers (device=-1); `gpu-v0` (one lane per value) and
`gpu-v1` (sixteen lanes per value, 256-byte steps of 16-byte vectors) run the kernels.  On the GPU
the data is a slice in the middle of a larger device tensor whose other bytes are quotes and
letters, at an odd phase, so a read outside a value changes a result instead of going unseen.  The
output buffer has guard bytes on both sides and is filled before the call, so a write outside a
value's range shows."""
import numpy as np
import pytest

from alluxio_amd.ops.native import lib

Q = 0x22
STEP = 256          # variant 1: bytes of a value that a 16-lane group takes per step
VEC = 16            # and per lane
PAD = 4099          # bytes before the slice on the device: an odd phase
GUARD = 67          # bytes on either side of the output
FILL = 0xEE         # the output and its guards before the call

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 511, 512, 513, 4099]
RUNS = [1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 35]
COUNTS = [0, 1, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1000]


def collapse(v: bytes, quote) -> bytes:
    return v if quote is None else v.replace(bytes([quote, quote]), bytes([quote]))


def test_the_rule_on_small_examples():
    assert collapse(b'say ""hi""', Q) == b'say "hi"' and collapse(b'"', Q) == b'"' and collapse(b'"""', Q) == b'""'
    assert collapse(b'""""', Q) == b'""' and collapse(b'a""', None) == b'a""' and collapse(b"", Q) == b""
    for k in range(40):                                 # a run of k quotes becomes ceil(k / 2)
        assert collapse(b"x" + b'"' * k + b"y", Q) == b"x" + b'"' * ((k + 1) // 2) + b"y"


class _Env:
    def __init__(self, mode):
        self.mode, self.gpu = mode, mode != "cpu"

    def run(self, data: bytes, start, length, status=None, quote=Q, offsets=None, out_bytes=None):
        """measure, then emit with the exclusive scan of the measured lengths (or with `offsets` /
        `out_bytes` as given).  Returns (lengths, offsets, the output bytes); the guards are checked."""
        start = np.ascontiguousarray(start, dtype=np.int64)
        length = np.ascontiguousarray(length, dtype=np.int32)
        status = None if status is None else np.ascontiguousarray(status, dtype=np.uint8)
        n, q = len(start), -1 if quote is None else quote
        C = lib()
        if self.gpu:
            import torch
            fill = np.frombuffer(b'"a""b"""', dtype=np.uint8)
            big = np.resize(fill, PAD + len(data) + PAD)
            big[PAD:PAD + len(data)] = np.frombuffer(data, dtype=np.uint8)
            dev = torch.from_numpy(big).cuda()
            d_start, d_length = torch.from_numpy(start).cuda(), torch.from_numpy(length).cuda()
            d_status = None if status is None else torch.from_numpy(status).cuda()
            sp = 0 if d_status is None else d_status.data_ptr()
            d_len = torch.full((n,), 77, dtype=torch.int32, device="cuda")
            C.text_measure_raw(dev.data_ptr() + PAD, len(data), d_start.data_ptr(), d_length.data_ptr(), sp, n, 0, q,
                               d_len.data_ptr())
            torch.cuda.synchronize()
            lens = d_len.cpu().numpy()
        else:
            buf = np.frombuffer(data, dtype=np.uint8).copy() if data else np.zeros(1, np.uint8)
            sp = 0 if status is None else status.ctypes.data
            lens = np.full(n, 77, np.int32)
            C.text_measure_raw(buf.ctypes.data, len(data), start.ctypes.data, length.ctypes.data, sp, n, -1, q,
                               lens.ctypes.data)
        if offsets is None:
            offsets = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        total = int(offsets[-1]) if out_bytes is None else out_bytes
        if self.gpu:
            d_out = torch.full((GUARD + total + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            d_off = torch.from_numpy(offsets).cuda()
            C.text_emit_raw(dev.data_ptr() + PAD, len(data), d_start.data_ptr(), d_length.data_ptr(), sp, n, 0, q,
                            d_off.data_ptr(), d_out.data_ptr() + GUARD, total)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
        else:
            out = np.full(GUARD + total + GUARD, FILL, np.uint8)
            C.text_emit_raw(buf.ctypes.data, len(data), start.ctypes.data, length.ctypes.data, sp, n, -1, q,
                            offsets.ctypes.data, out.ctypes.data + GUARD, total)
        assert (out[:GUARD] == FILL).all() and (out[GUARD + total:] == FILL).all(), "a guard byte was written"
        return lens, offsets, out[GUARD:GUARD + total].tobytes()

    def check(self, data, start, length, status=None, quote=Q):
        n = len(start)
        want = []
        for r in range(n):
            s, l = int(start[r]), int(length[r])
            live = (status is None or status[r] == 0) and s >= 0 and l >= 0 and s + l <= len(data)
            want.append(collapse(data[s:s + l], quote) if live else b"")
        lens, offsets, out = self.run(data, start, length, status, quote)
        assert lens.tolist() == [len(w) for w in want]
        assert out == b"".join(want)
        return want

    def check_values(self, values, quote=Q, lead=0):
        """Each value after `lead` bytes that belong to none (quotes: a carry from them would show)."""
        data, start = b"", []
        for v in values:
            data += b'"' * lead
            start.append(len(data))
            data += v
        return self.check(data, start, [len(v) for v in values], None, quote)


@pytest.fixture(params=[pytest.param(("cpu", 0), id="cpu"),
                        pytest.param(("gpu", 0), marks=pytest.mark.gpu, id="gpu-v0"),
                        pytest.param(("gpu", 1), marks=pytest.mark.gpu, id="gpu-v1")])
def env(request):
    mode, variant = request.param
    if mode == "cpu":
        yield _Env(mode)
        return
    request.getfixturevalue("gpu")
    default = lib().text_column_variant()
    lib().set_text_column_variant(variant)
    assert lib().text_column_variant() == variant
    yield _Env(mode)
    lib().set_text_column_variant(default)


def _letters(n, seed=0):
    return bytes(0x61 + (i * 7 + seed) % 23 for i in range(n))


def _with_quotes(n, seed=0):
    """n bytes with a doubled quote every 11 bytes, a lone one every 29 and a quote at the end."""
    v = bytearray(_letters(n, seed))
    for i in range(3, n - 1, 11):
        v[i] = v[i + 1] = Q
    for i in range(5, n, 29):
        v[i] = Q
    if n:
        v[n - 1] = Q
    return bytes(v)


# ---- cases ---------------------------------------------------------------------------------------
def test_lengths_at_every_start_phase(env):
    for lead in (0, 1, 7, 15):
        plain = [_letters(n, lead) for n in LENGTHS]
        quoted = [_with_quotes(n, lead) for n in LENGTHS]
        env.check_values(plain, lead=lead)
        want = env.check_values(quoted, lead=lead)
        assert sum(len(w) for w in want) < sum(LENGTHS)        # something was dropped
        env.check_values(quoted, quote=None, lead=lead)         # a plain copy
        env.check_values(quoted, quote=0x61, lead=lead)         # another byte as the quote


def _runs_at(edge):
    """Values with one run of k quotes that ends at, begins at or straddles byte `edge`, and the
    same values cut in the middle of the run."""
    out = []
    for k in RUNS:
        for before in sorted({0, 1, k // 2, k - 1, k}):           # quotes of the run in front of the edge
            if before > edge:
                continue
            v = bytearray(_letters(edge + 40, k))
            v[edge - before:edge - before + k] = b'"' * k
            out.append(bytes(v))
            out.append(bytes(v[:edge - before + (k + 1) // 2]))   # the run is cut by the end of the value
    return out


def test_quote_runs_across_vector_and_step_edges(env):
    values = _runs_at(VEC) + _runs_at(STEP) + _runs_at(2 * STEP)
    env.check_values(values)
    env.check_values(values, lead=5)
    # two runs in one vector, runs in neighbouring vectors, a run through two whole vectors
    more = [b'ab""cd"""e""""fg"', b'"' * 5 + b"x" + b'"' * 11 + b'"' * 3 + b"y", b"x" * 9 + b'"' * 39 + b"z",
            b"x" * 15 + b'"' * 34 + b"z" * 3, b"x" * 250 + b'"' * 23 + b"z"]
    env.check_values(more)
    env.check_values(more, lead=3)


def test_values_of_quotes_only(env):
    values = [b'"' * k for k in (16, 32, 33, 256, 257, 1, 2, 3, 15, 17, 255, 512, 513, 768)]
    want = env.check_values(values)
    assert [len(w) for w in want[:5]] == [8, 16, 17, 128, 129]
    env.check_values(values, lead=9)
    # the parity carried through vectors that are all quotes: an odd run in front of them
    env.check_values([b"ab" + b'"' * k + b"c" for k in (14, 15, 30, 31, 46, 47, 270, 271, 526, 527)])
    env.check_values([b"a" * 13 + b'"' * k + b"c" for k in (3, 19, 20, 35, 36, 259, 260)], lead=2)


def test_row_counts(env):
    rng = np.random.default_rng(4)
    for n in COUNTS:
        values = [_with_quotes(int(k), n) for k in rng.integers(0, 40, n)]
        if n >= 3:
            values[n // 2] = _with_quotes(700, 1)
        env.check_values(values)


def _random_values(n, seed):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b'"a,', dtype=np.uint8)
    lens = np.minimum(rng.geometric(0.03, n) - 1, 1200)                # skewed: most are short
    lens[rng.integers(0, n, 20)] = rng.integers(900, 1201, 20)
    lens[0], lens[1] = 1200, 0
    out = []
    for k in lens:
        p = [(.6, .3, .1), (.2, .6, .2), (.9, .05, .05)][int(rng.integers(0, 3))]
        out.append(alphabet[rng.choice(3, int(k), p=p)].tobytes())
    return out


def test_random_values_and_determinism(env):
    values = _random_values(2000, 21)
    assert max(len(v) for v in values) == 1200 and min(len(v) for v in values) == 0
    want = env.check_values(values, lead=1)
    assert sum(len(w) for w in want) < sum(len(v) for v in values)
    env.check_values(values, quote=None, lead=1)                       # quote = -1 is a plain copy
    data = b"".join(values)
    start = np.concatenate([[0], np.cumsum([len(v) for v in values])[:-1]])
    a = env.run(data, start, [len(v) for v in values])
    b = env.run(data, start, [len(v) for v in values])
    assert a[2] == b[2] and a[0].tolist() == b[0].tolist()             # two runs give identical bytes


def test_values_that_are_not_live(env):
    vals = [b'a""b', b"zzzz", b"zzzz", b"zzzz", b"zzzz", b'c""d', b"zzzz", _with_quotes(300), b"zzzz"]
    data = b"".join(vals)
    start = np.concatenate([[0], np.cumsum([len(v) for v in vals])[:-1]]).astype(np.int64)
    length = np.array([len(v) for v in vals], dtype=np.int32)
    status = np.zeros(len(vals), np.uint8)
    status[1], status[2] = 1, 2
    start[3] = -1
    length[4] = -1
    start[8] = len(data) - 3                            # start + length = data_bytes + 1
    want = env.check(data, start, length, status)
    assert [len(w) for w in want] == [3, 0, 0, 0, 0, 3, 4, len(collapse(vals[7], Q)), 0]
    start[1], length[2] = 2 ** 62, 2 ** 31 - 1          # far outside, without a status array
    want = env.check(data, start, length, None)
    assert [len(w) for w in want[:5]] == [3, 0, 0, 0, 0]
    start[8] = len(data) - 4                            # the value that ends with the data is live
    assert env.check(data, start, length, None)[8] == b"zzzz"


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
    ([0, 3, 8, 12, 500], 600),                          # too small for values 0 and 3
    ([-5, 3, 5, 40, 50], 45),                           # before the buffer, and cut by its end
    ([700, 800, 900, 1000, 1100], 600),                 # past out_bytes altogether
    ([9, 4, 4, 0, 0], 600),                             # decreasing: empty windows
    ([-2 ** 63, -2 ** 62, 0, 0, 2 ** 63 - 1], 600),     # as far out as int64 goes
    ([0, 8, 13, 17, 17 + 300], 17 + 129),               # value 3 is cut by its window and by the buffer
    ([-301, 7, 12, 16, 16 + 530], 600),                 # the long value first, 301 bytes before the buffer
], ids=["small", "straddle", "past", "decreasing", "extreme", "short-buffer", "negative-long"])
def test_emit_with_inconsistent_offsets(env, offsets, out_bytes):
    vals = [b"abcdefgh", b'ij""kl', b"mnop", _with_quotes(530, 3)]
    if offsets[0] == -301:
        vals[0], vals[3] = vals[3], vals[0]
    data = b"".join(vals)
    start = np.concatenate([[0], np.cumsum([len(v) for v in vals])[:-1]])
    want = [collapse(v, Q) for v in vals]
    before = lib().text_column_launches()
    lens, _, out = env.run(data, start, [len(v) for v in vals], None, Q, offsets=offsets, out_bytes=out_bytes)
    assert lens.tolist() == [len(w) for w in want]
    assert out == _windowed(want, offsets, out_bytes)   # no error, and nothing outside the windows
    assert lib().text_column_launches() == before + (2 if env.gpu else 0)


def test_argument_errors_and_empty_calls(env):
    C = lib()
    before = C.text_column_launches()
    for quote in (256, -2, 1 << 40):
        with pytest.raises(C.StoreError) as e:
            env.run(b'a""b', [0], [4], None, quote)
        assert e.value.args[0] == 6                     # the store's invalid-argument code
    one = np.zeros(2, np.int64)
    p = one.ctypes.data                                 # any non-null address: a rejected call touches nothing
    device = 0 if env.gpu else -1
    for args in ((p, 4, 0, p, 0, 1, device, Q, p), (p, 4, p, 0, 0, 1, device, Q, p), (0, 4, p, p, 0, 1, device, Q, p),
                 (p, 4, p, p, 0, 1, device, Q, 0)):
        with pytest.raises(C.StoreError) as e:
            C.text_measure_raw(*args)
        assert e.value.args[0] == 6
    for args in ((p, 4, 0, p, 0, 1, device, Q, p, p, 8), (p, 4, p, 0, 0, 1, device, Q, p, p, 8),
                 (p, 4, p, p, 0, 1, device, Q, 0, p, 8), (p, 4, p, p, 0, 1, device, Q, p, 0, 8),
                 (0, 4, p, p, 0, 1, device, Q, p, p, 8)):
        with pytest.raises(C.StoreError) as e:
            C.text_emit_raw(*args)
        assert e.value.args[0] == 6
    assert C.text_column_launches() == before           # nothing was launched
    C.text_measure_raw(0, 0, 0, 0, 0, 0, device, Q, 0)  # n = 0: null arrays are fine and nothing is launched
    C.text_emit_raw(0, 0, 0, 0, 0, 0, device, Q, 0, 0, 0)
    lens, offsets, out = env.run(b"", [], [])
    assert lens.size == 0 and offsets.tolist() == [0] and out == b"" and C.text_column_launches() == before
    env.check_values([b'a""b'])
    assert C.text_column_launches() == before + (2 if env.gpu else 0)
