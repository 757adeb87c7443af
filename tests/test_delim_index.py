"""delim_index_raw: the cut positions of one delimiter byte in a virtual byte range behind a
scrambled page table (a 64-page arena of 4 KiB pages), compared with numpy on the same virtual
bytes.  The same cases run over a numpy arena (the host memchr loop) and over a device tensor
(count, scan and emit kernels: both load variants, tiles of 1 KiB - smaller than a page - and of
8 KiB)."""
import numpy as np
import pytest

from alluxio_amd.ops.native import lib

PAGE = 4096
NPAGES = 64
F_LEN = 39 * PAGE + 1000                       # the file ends inside its last page
TILE_SHIFTS = (10, 13)


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


def _text(n, d, seed, one_in=40):
    """n random bytes of which about one in `one_in` equals d."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, n, dtype=np.uint8)
    x[x == d] ^= 0x55                           # no accidental delimiter ...
    x[rng.random(n) < 1.0 / one_in] = d         # ... only the planted ones
    return x


def _surrounded(vstart, content, d):
    """A virtual image that is the delimiter everywhere except `content` at vstart."""
    virt = np.full(NPAGES * PAGE, d, dtype=np.uint8)
    virt[vstart:vstart + len(content)] = content
    return virt


class _Env:
    def __init__(self, mode, variant=0, tile_shift=0):
        self.mode, self.gpu, self.tile_shift = mode, mode != "cpu", tile_shift

    def cuts(self, virt, vstart, nbytes, d, pages=PERM, arena=None, **kw):
        arena = _arena_of(virt) if arena is None else arena
        if self.gpu:
            import torch
            dev = torch.from_numpy(arena).cuda()
            got = lib().delim_index_raw(dev.data_ptr(), pages.tolist(), PAGE, 0, vstart, nbytes, d, **kw)
            torch.cuda.synchronize()
        else:
            got = lib().delim_index_raw(arena.ctypes.data, pages.tolist(), PAGE, -1, vstart, nbytes, d, **kw)
        cuts = got[0] if kw.get("times") else got
        assert cuts.dtype == np.uint64 and cuts.ndim == 1
        return got

    def check(self, virt, vstart, nbytes, d):
        want = (np.flatnonzero(virt[vstart:vstart + nbytes] == d) + 1).astype(np.uint64)
        got = self.cuts(virt, vstart, nbytes, d)
        assert np.array_equal(got, want), (vstart, nbytes, got.size, want.size)
        return got


def _gpu_modes():
    return [pytest.param(("gpu", v, ts), marks=pytest.mark.gpu, id=f"gpu-v{v}-t{ts}")
            for v in (0, 1) for ts in TILE_SHIFTS]


@pytest.fixture(params=[pytest.param(("cpu", 0, 0), id="cpu")] + _gpu_modes())
def env(request):
    mode, variant, ts = request.param
    if mode == "cpu":
        yield _Env(mode)
        return
    request.getfixturevalue("gpu")
    default = (lib().delim_index_variant(), lib().delim_index_tile_shift())
    lib().set_delim_index_variant(variant, ts)
    assert lib().delim_index_tile_shift() == ts
    yield _Env(mode, variant, ts)
    lib().set_delim_index_variant(*default)


def test_page_table_is_scrambled():
    assert not (np.abs(np.diff(PERM)) == 1).any()
    assert F_LEN % PAGE != 0 and min(TILE_SHIFTS) < 12 < max(TILE_SHIFTS)


def test_file_ending_inside_its_last_page(env):
    d = 0x0A
    virt = _surrounded(0, _text(F_LEN, d, 1), d)      # the page's remaining bytes and every other page: delimiters
    got = env.check(virt, 0, F_LEN, d)
    assert 0.5 * F_LEN / 40 < got.size < 2 * F_LEN / 40 and int(got[-1]) <= F_LEN
    assert np.array_equal(got, env.cuts(virt, 0, F_LEN, d))              # two runs, one array
    assert np.array_equal(env.cuts(virt, 0, F_LEN, d, add=7 << 40), got + np.uint64(7 << 40))


def test_start_phases_and_short_ranges(env):
    d = 0x0A
    for ph in range(16):
        for n in (0, 1, 15, 16, 17, 4095, 4096, 4097):
            vstart = 5 * PAGE - 32 + ph
            virt = _surrounded(vstart, _text(n, d, 100 * ph + n % 97, one_in=8), d)
            env.check(virt, vstart, n, d)


def test_delimiters_at_edges(env):
    d = ord(",")
    vstart, n = 3 * PAGE + 16 * 5 + 3, 50 * PAGE + 77
    a0 = vstart & ~15                                   # tiles count from the range's first aligned vector
    spots = [vstart, vstart + n - 1, 5 * PAGE - 1, 5 * PAGE]
    for ts in TILE_SHIFTS + (lib().delim_index_tile_shift(),):
        spots += [a0 + (1 << ts) - 1, a0 + (1 << ts)]
    assert all(vstart <= s < vstart + n for s in spots)
    content = _text(n, d, 3, one_in=10 ** 9)
    assert not (content == d).any()
    virt = _surrounded(vstart, content, d)
    for s in spots:
        virt[s] = d
    got = env.check(virt, vstart, n, d)
    assert got.size == len(set(spots)) and int(got[0]) == 1 and int(got[-1]) == n
    for s in spots:                                     # each one alone
        one = _surrounded(vstart, content, d)
        one[s] = d
        assert env.check(one, vstart, n, d).tolist() == [s - vstart + 1]


def test_no_delimiter(env):
    d = 0x0A
    vstart, n = PAGE + 9, 3 * PAGE + 5
    virt = _surrounded(vstart, _text(n, d, 4, one_in=10 ** 9), d)
    got = env.check(virt, vstart, n, d)
    assert got.size == 0


def test_every_byte_a_delimiter(env):
    d = 0x0A
    n = 3 * PAGE
    virt = np.full(NPAGES * PAGE, d, dtype=np.uint8)
    for vstart in (7 * PAGE, 7 * PAGE + 5):
        got = env.check(virt, vstart, n, d)
        assert np.array_equal(got, np.arange(1, n + 1, dtype=np.uint64))


@pytest.mark.parametrize("d", [0x00, 0xFF])
def test_delimiter_values_0_and_255(env, d):
    vstart, n = 2 * PAGE + 11, 9 * PAGE + 123
    virt = _surrounded(vstart, _text(n, d, 6 + d), d)
    got = env.check(virt, vstart, n, d)
    assert got.size > 100
    other = 0xFF - d                                    # bytes of the other extreme are no matches
    virt2 = virt.copy()
    virt2[vstart:vstart + n][virt2[vstart:vstart + n] != d] = other
    env.check(virt2, vstart, n, d)


def test_scan_carries_across_rounds(env):
    """More tiles than one round of the scan (4096) at the 1 KiB tile: a 4 MiB range whose page
    table shows the 64-page arena again and again."""
    d = 0x0A
    reps = 17
    base = _text(NPAGES * PAGE, d, 8, one_in=100)
    virt = np.tile(base, reps)
    pages = np.tile(PERM, reps)
    vstart, n = 5, (4 << 20) + 3000
    if env.tile_shift == 10:
        assert ((vstart & 15) + n + 1023) >> 10 > 4096
    want = (np.flatnonzero(virt[vstart:vstart + n] == d) + 1).astype(np.uint64)
    got = env.cuts(virt, vstart, n, d, pages=pages, arena=_arena_of(base))
    assert want.size > 30000 and np.array_equal(got, want)


@pytest.mark.parametrize("case", ["past_the_table", "start_past_the_table", "negative_page", "two_bytes"])
def test_rejected_arguments(env, case):
    d = 0x0A
    virt = _surrounded(0, _text(F_LEN, d, 1), d)
    pages, vstart, n = PERM.copy(), 0, F_LEN
    if case == "past_the_table":
        vstart, n = 60 * PAGE, 4 * PAGE + 1
    elif case == "start_past_the_table":
        vstart, n = NPAGES * PAGE + 1, 0
    elif case == "negative_page":
        pages[50] = -1                                  # outside the range: still refused
    elif case == "two_bytes":
        d = 0x0A0A
    before = lib().delim_index_launches()
    with pytest.raises(lib().StoreError) as e:
        env.cuts(virt, vstart, n, d, pages=pages)
    assert e.value.args[0] == 6                         # the store's invalid-argument code
    assert lib().delim_index_launches() == before       # nothing was launched


@pytest.mark.gpu
def test_kernels_launch_on_the_device(gpu):
    d = 0x0A
    virt = _surrounded(0, _text(F_LEN, d, 1), d)
    before = lib().delim_index_launches()
    env = _Env("gpu")
    got, times = env.cuts(virt, 0, F_LEN, d, times=True)
    assert lib().delim_index_launches() == before + 3   # count, scan, emit
    assert got.size > 0 and len(times) == 3 and all(t >= 0 for t in times)
    before = lib().delim_index_launches()
    assert env.cuts(_surrounded(0, _text(F_LEN, d, 1, one_in=10 ** 9), d), 0, F_LEN, d).size == 0
    assert lib().delim_index_launches() == before + 2   # no delimiter: nothing to emit
