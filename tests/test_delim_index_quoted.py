"""delim_index_raw with a quote byte: a delimiter is a cut only when the number of quote bytes
before it in the range (plus the initial state) is even.  The yardstick is that rule in numpy on
the same virtual bytes, compared for exact equality.  The harness is that of test_delim_index.py:
a 64-page arena of 4 KiB pages behind a scrambled page table; the host loop runs over a numpy arena
and the kernels over a device tensor, for both load variants, both count variants and tiles of
1 KiB (smaller than a page) and 8 KiB, plus both count variants at the default tile."""
import functools

import numpy as np
import pytest

from alluxio_amd.ops.native import lib

PAGE = 4096
NPAGES = 64
F_LEN = 39 * PAGE + 1000                       # the file ends inside its last page
TILE_SHIFTS = (10, 13)
D, Q = 0x0A, ord('"')


def _page_table():
    for seed in range(100):
        perm = np.random.default_rng(seed).permutation(NPAGES).astype(np.int64)
        if not (np.abs(np.diff(perm)) == 1).any():
            return perm
    raise AssertionError("no scrambled page table found")


PERM = _page_table()


def _arena_of(virt):
    """The arena image that shows `virt` (NPAGES pages) through PERM."""
    arena = np.empty_like(virt)
    arena.reshape(NPAGES, PAGE)[PERM] = virt.reshape(NPAGES, PAGE)
    return arena


def rule(x, d, q, in_quote=0):
    """The cut positions of the bytes x: the rule itself, independent of the code under test."""
    qm = x == q
    before = np.cumsum(qm) - qm
    return (np.flatnonzero((x == d) & ((before + in_quote) % 2 == 0)) + 1).astype(np.uint64)


def _text(n, d, q, seed, d_in=40, q_in=20, quotes=None):
    """n random bytes: about one in d_in equals d and one in q_in equals q (quotes=k: exactly k
    quote bytes at random places instead)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, n, dtype=np.uint8)
    other = next(b for b in (0x41, 0x42, 0x43) if b not in (d, q))
    x[(x == d) | (x == q)] = other                # only the planted ones
    x[rng.random(n) < 1.0 / d_in] = d
    if quotes is None:
        x[rng.random(n) < 1.0 / q_in] = q
    elif n:
        x[rng.choice(n, size=quotes, replace=False)] = q
    return x


def _surrounded(vstart, content, fill):
    """A virtual image that is `fill` everywhere except `content` at vstart."""
    virt = np.full(NPAGES * PAGE, fill, dtype=np.uint8)
    virt[vstart:vstart + len(content)] = content
    return virt


class _Env:
    def __init__(self, mode, tile_shift=0, default_shift=None):
        self.mode, self.gpu, self.tile_shift = mode, mode != "cpu", tile_shift
        self.default_shift = lib().delim_index_tile_shift() if default_shift is None else default_shift

    def cuts(self, virt, vstart, nbytes, d=D, pages=PERM, arena=None, **kw):
        arena = _arena_of(virt) if arena is None else arena
        if self.gpu:
            import torch
            dev = torch.from_numpy(arena).cuda()
            got = lib().delim_index_raw(dev.data_ptr(), pages.tolist(), PAGE, 0, vstart, nbytes, d, **kw)
            torch.cuda.synchronize()
        else:
            got = lib().delim_index_raw(arena.ctypes.data, pages.tolist(), PAGE, -1, vstart, nbytes, d, **kw)
        assert got.dtype == np.uint64 and got.ndim == 1
        return got

    def check(self, virt, vstart, nbytes, d=D, q=Q, in_quote=0):
        want = rule(virt[vstart:vstart + nbytes], d, q, in_quote)
        got = self.cuts(virt, vstart, nbytes, d, quote=q, in_quote=bool(in_quote))
        assert np.array_equal(got, want), (vstart, nbytes, in_quote, got.size, want.size)
        return got


def _gpu_modes():
    modes = [(v, c, ts) for v in (0, 1) for c in (0, 1) for ts in TILE_SHIFTS]
    modes += [(1, c, 0) for c in (0, 1)]               # tile 0: the default tile, whatever it is
    return [pytest.param(("gpu", v, c, ts), marks=pytest.mark.gpu, id=f"gpu-v{v}-c{c}-t{ts}") for v, c, ts in modes]


@pytest.fixture(params=[pytest.param(("cpu", 0, 0, 0), id="cpu")] + _gpu_modes())
def env(request):
    mode, variant, count_variant, ts = request.param
    if mode == "cpu":
        yield _Env(mode)
        return
    request.getfixturevalue("gpu")
    default = (lib().delim_index_variant(), lib().delim_index_tile_shift())
    default_count = lib().delim_quote_variant()
    lib().set_delim_index_variant(variant, ts)
    lib().set_delim_quote_variant(count_variant)
    assert lib().delim_index_tile_shift() == (ts or default[1]) and lib().delim_quote_variant() == count_variant
    yield _Env(mode, ts or default[1], default[1])
    lib().set_delim_index_variant(*default)
    lib().set_delim_quote_variant(default_count)


def _tile_edges(env, a0):
    """Addresses at which a new tile starts, for the tested tile sizes and the default one."""
    return sorted({a0 + (1 << ts) for ts in TILE_SHIFTS + (env.default_shift,)})


def test_the_rule_on_a_small_example():
    x = np.frombuffer(b'a,"b\nc""d\n"\ne\n', dtype=np.uint8)
    assert rule(x, D, Q).tolist() == [12, 14]
    assert rule(x, D, Q, 1).tolist() == [5, 10]
    assert not (np.abs(np.diff(PERM)) == 1).any()
    assert F_LEN % PAGE != 0 and min(TILE_SHIFTS) < 12 < max(TILE_SHIFTS)


@pytest.mark.parametrize("density", ["1in20", "1in200", "one"])
@pytest.mark.parametrize("in_quote", [0, 1])
def test_random_text(env, density, in_quote):
    kw = {"1in20": dict(q_in=20), "1in200": dict(q_in=200), "one": dict(quotes=1)}[density]
    text = _text(F_LEN, D, Q, 1, **kw)
    assert (text == Q).sum() == 1 if density == "one" else (text == Q).sum() > F_LEN // 400
    for fill in (D, Q):                               # the page's remaining bytes and every other page
        virt = _surrounded(0, text, fill)
        got = env.check(virt, 0, F_LEN, in_quote=in_quote)
        assert 0 < got.size < (text == D).sum() and int(got[-1]) <= F_LEN
    kw = dict(quote=Q, in_quote=bool(in_quote))
    assert np.array_equal(got, env.cuts(virt, 0, F_LEN, **kw))                       # two runs, one array
    assert np.array_equal(env.cuts(virt, 0, F_LEN, add=7 << 40, **kw), got + np.uint64(7 << 40))


@pytest.mark.parametrize("fill", [Q, D], ids=["among-quotes", "among-delimiters"])
def test_start_phases_and_short_ranges(env, fill):
    """Nothing outside the range may count or toggle."""
    for ph in range(16):
        for n in (0, 1, 15, 16, 17, 4095, 4096, 4097):
            vstart = 5 * PAGE - 32 + ph
            virt = _surrounded(vstart, _text(n, D, Q, 100 * ph + n % 97, d_in=6, q_in=9), fill)
            env.check(virt, vstart, n, in_quote=(ph + n) & 1)


V0, N0 = 3 * PAGE + 16 * 5 + 3, 50 * PAGE + 77        # the range of the edge tests
A0 = V0 & ~15                                         # tiles count from the range's first aligned vector


def _edges(env):
    """Addresses e such that bytes e - 1 and e lie on two sides of: a 16-byte vector edge, the 1 KiB
    edge between lane groups of a step, the 4 KiB step edge, each tile edge, a page edge."""
    e = [A0 + 16 * 7, A0 + 1024, A0 + 2 * 1024, A0 + 4096, A0 + 2 * 4096, 5 * PAGE, 17 * PAGE] + _tile_edges(env, A0)
    assert all(V0 + 64 < x < V0 + N0 - 64 for x in e)
    return sorted(set(e))


def _plain(seed=3):
    content = _text(N0, D, Q, seed, d_in=10 ** 9, q_in=10 ** 9)
    assert not ((content == D) | (content == Q)).any()
    return content


FIELD = np.frombuffer(b'\n"\nab\ncd\n"\n', dtype=np.uint8)   # delimiters before, after and directly inside both quotes
F_OPEN, F_CLOSE = 1, len(FIELD) - 2


def test_quoted_field_at_edges(env):
    content = _plain()
    spots = []
    for e in _edges(env):
        # the opening quote is the last byte before the edge / the first after it; so is the closing one
        spots += [e - 1 - F_OPEN, e - F_OPEN, e - 1 - F_CLOSE, e - F_CLOSE]
    spots += [V0 - F_OPEN, V0 + N0 - 1 - F_CLOSE]     # the quotes are the first / the last byte of the range
    for fill in (Q, D):
        for s in spots:
            virt = _surrounded(V0, content, fill)
            lo, hi = max(s, V0), min(s + len(FIELD), V0 + N0)
            virt[lo:hi] = FIELD[lo - s:hi - s]
            got = env.check(virt, V0, N0)
            assert got.size == (2 if s >= V0 and s + len(FIELD) <= V0 + N0 else 1), s
    virt = _surrounded(V0, content, Q)                # all of them in one image: the fields are apart
    for s in spots[:-2:4]:
        virt[s:s + len(FIELD)] = FIELD
    assert env.check(virt, V0, N0).size == 2 * len(spots[:-2:4])


def test_doubled_quote_at_edges(env):
    """A quoted field with "" inside whose two bytes fall on either side of the edge."""
    content = _plain(4)
    field = np.frombuffer(b'\n"\nab\n""\ncd\n"\n', dtype=np.uint8)
    first = 6                                          # offset of the first byte of ""
    assert field[first] == Q and field[first + 1] == Q
    spots = [e - 1 - first for e in _edges(env)] + [V0 - 1 - first, V0 + N0 - 1 - first]
    for fill in (Q, D):
        for s in spots:
            virt = _surrounded(V0, content, fill)
            lo, hi = max(s, V0), min(s + len(field), V0 + N0)
            virt[lo:hi] = field[lo - s:hi - s]
            for in_quote in (0, 1):
                env.check(virt, V0, N0, in_quote=in_quote)


def test_quoted_field_spanning_whole_tiles(env):
    """Tiles that hold delimiters and no quote, inside a quoted field: their delimiters are all
    inside, which a tile can only report through its odd-parity count."""
    span = 3 << max(TILE_SHIFTS + (env.default_shift,))
    vstart, n = PAGE + 7, span + 5 * PAGE
    text = _text(n, D, Q, 9, d_in=30, q_in=10 ** 9)
    assert not (text == Q).any()
    text[PAGE + 100] = Q
    text[PAGE + 200 + span] = Q
    virt = _surrounded(vstart, text, Q)
    got = env.check(virt, vstart, n)
    assert 0 < got.size < (text == D).sum() - span // 60
    inside = env.check(virt, vstart, n, in_quote=1)     # the complement
    assert got.size + inside.size == (text == D).sum()


def test_every_byte_a_quote(env):
    virt = np.full(NPAGES * PAGE, Q, dtype=np.uint8)
    for vstart, n in ((7 * PAGE, 3 * PAGE), (7 * PAGE + 5, 3 * PAGE + 1), (7 * PAGE + 3, 9001), (PAGE, 1)):
        for in_quote in (0, 1):
            assert env.check(virt, vstart, n, in_quote=in_quote).size == 0


def test_every_byte_a_delimiter_after_one_quote(env):
    n = 3 * PAGE
    for vstart in (7 * PAGE, 7 * PAGE + 5):
        virt = np.full(NPAGES * PAGE, D, dtype=np.uint8)
        before = lib().delim_index_launches()
        got = env.check(virt, vstart, n)
        assert np.array_equal(got, np.arange(1, n + 1, dtype=np.uint64))
        assert lib().delim_index_launches() == before + (3 if env.gpu else 0)
        virt[vstart] = Q
        before = lib().delim_index_launches()
        assert env.check(virt, vstart, n).size == 0
        assert lib().delim_index_launches() == before + (2 if env.gpu else 0)    # nothing to emit
        assert np.array_equal(env.check(virt, vstart, n, in_quote=1), np.arange(2, n + 1, dtype=np.uint64))


@pytest.mark.parametrize("q", [0x00, 0xFF])
def test_quote_values_0_and_255(env, q):
    vstart, n = 2 * PAGE + 11, 9 * PAGE + 123
    for d in (D, 0xFF - q):                             # and the other extreme as the delimiter
        virt = _surrounded(vstart, _text(n, d, q, 6 + q, q_in=50), q)
        got = env.check(virt, vstart, n, d=d, q=q)
        assert got.size > 100
        env.check(virt, vstart, n - 4000, d=d, q=q, in_quote=1)   # ends inside a tile; the rest is not loaded


@functools.lru_cache(maxsize=None)
def _carry_case():
    """The 4 MiB range of the carry test of test_delim_index.py over a page table that repeats the
    arena.  The arena image holds an odd number of quotes, so each repetition starts in the
    opposite state, and none near its two ends, so with in_quote = 1 one quoted field spans the
    boundary between the scan rounds (tile 4096 of 1 KiB: the start of repetition 16)."""
    reps = 17
    base = _text(NPAGES * PAGE, D, Q, 8, d_in=100, q_in=150)
    base[:300][base[:300] == Q] = 0x41
    base[-300:][base[-300:] == Q] = 0x41
    base[[50, 150, 250, -250, -150, -50]] = D
    if (base == Q).sum() % 2 == 0:
        base[1000] = Q if base[1000] != Q else 0x41
    assert (base == Q).sum() % 2 == 1
    virt = np.tile(base, reps)
    vstart, n = 5, (4 << 20) + 3000
    want = {s: rule(virt[vstart:vstart + n], D, Q, s) for s in (0, 1)}
    edge = (4 << 20) - vstart                           # offset in the range of the round boundary
    for k in (-250, -150, -50, 50, 150, 250):           # inside the field for in_quote = 1, outside for 0
        assert edge + k + 1 in want[0] and edge + k + 1 not in want[1]
    assert want[0].size > 10000 and want[1].size > 10000
    for w in want.values():
        w.setflags(write=False)
    return base, _arena_of(base), np.tile(PERM, reps), vstart, n, want


@pytest.mark.parametrize("in_quote", [0, 1])
def test_scan_carries_parity_and_count_across_rounds(env, in_quote):
    base, arena, pages, vstart, n, want = _carry_case()
    if env.tile_shift == 10:
        assert ((vstart & 15) + n + 1023) >> 10 > 4096
    got = env.cuts(None, vstart, n, pages=pages, arena=arena, quote=Q, in_quote=bool(in_quote))
    assert np.array_equal(got, want[in_quote])


def test_quote_absent_is_the_existing_call(env):
    text = _text(F_LEN, D, Q, 1)
    virt = _surrounded(0, text, D)
    plain = env.cuts(virt, 0, F_LEN)
    assert np.array_equal(plain, (np.flatnonzero(virt[:F_LEN] == D) + 1).astype(np.uint64))
    assert np.array_equal(env.cuts(virt, 0, F_LEN, quote=-1), plain)
    assert np.array_equal(env.cuts(virt, 0, F_LEN, quote=-1, in_quote=False), plain)
    assert env.cuts(virt, 0, F_LEN, quote=Q).size < plain.size


@pytest.mark.parametrize("case", ["quote_is_the_delimiter", "two_bytes", "negative"])
def test_rejected_quotes(env, case):
    virt = _surrounded(0, _text(F_LEN, D, Q, 1), D)
    q = {"quote_is_the_delimiter": D, "two_bytes": 256, "negative": -2}[case]
    before = lib().delim_index_launches()
    with pytest.raises(lib().StoreError) as e:
        env.cuts(virt, 0, F_LEN, quote=q)
    assert e.value.args[0] == 6                         # the store's invalid-argument code
    assert lib().delim_index_launches() == before       # nothing was launched


@pytest.mark.gpu
def test_quoted_kernels_launch_on_the_device(gpu):
    import torch
    virt = _surrounded(0, _text(F_LEN, D, Q, 1), D)
    dev = torch.from_numpy(_arena_of(virt)).cuda()
    before = lib().delim_index_launches()
    got, times = lib().delim_index_raw(dev.data_ptr(), PERM.tolist(), PAGE, 0, 0, F_LEN, D, times=True, quote=Q)
    torch.cuda.synchronize()
    assert lib().delim_index_launches() == before + 3   # count, scan, emit
    assert got.size > 0 and np.array_equal(got, rule(virt[:F_LEN], D, Q))
    assert len(times) == 3 and all(t >= 0 for t in times)
