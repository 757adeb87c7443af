"""batched_copy (K1/K2), the ring reader (K1') and the page gather (K9), byte for byte.

The rule, the same for all three: the destination starts as FILL bytes (0xA5) and every source byte
is some other value, so a byte that was written differs from one that was not.  The expected
destination is worked out in numpy from the semantics documented in kernels.h, starting from the
same fill, and the WHOLE buffer is compared: the guard bytes in front and behind, the gaps between
rows and slots, the bytes after a short page or a short read, the slots that must stay untouched.
Sources sit inside larger buffers whose other bytes are neither the data nor the fill, so a read
outside a range changes a byte.  No tolerances; slots, lengths and counters are compared exactly.

Ids: `cpu` runs the entry points' host paths (memmove, the host loop of RingReadSession with
device = -1, a PageCache with use_device = False) and so checks the numpy models against a second
implementation; on a machine with a device its buffers are pinned host memory, which batched_copy
then moves with the kernel.  The `gpu-*` ids run the kernels, one id per selectable variant; every
fixture puts back the variant it found, and the last test of the file checks that.

Which id launches which instantiation:
  batched_copy_kernel<UNROLL, LP, SP>, test_copy_*[gpu-vN]: v0 and v7 <8,0,0> (7 through the
      default: branch), v1 <8,0,1>, v2 <8,1,0>, v3 <8,1,1>, v4 <4,0,0>, v5 <4,0,1>, v8 <16,0,0>,
      v9 <16,0,1>
  seq_read_kernel<POW2, UNROLL, SP, LP>, test_ring_*[gpu-vN-case]: bit 0 of N is SP, bit 2 is LP and
      bit 1 makes UNROLL 16.  Depth and buf / 16 are powers of two in pow2, pow2_buf16,
      multiple_of_buf, shorter_than_a_vector, many_streams and the_limit: <true,...>, v0..v7 being
      its eight instantiations.  not_pow2 and short_file (depth 37) take <false,8,SP,LP>: v0/v2,
      v1/v3, v4/v6, v5/v7.  v-1 chooses by itself: v0 at these sizes, v4 in
      test_ring_picks_nontemporal_loads_by_itself
  page_lookup_gather_small_kernel<PW, UNR, SP, LP>, test_wave_gather[gpu-wN-ps]: w0 <4,4,0,0>,
      w1 <8,2,0,0>, w2 <4,4,1,0>, w3 <8,4,0,0>, w4 <4,4,0,1>, w5 <4,4,1,1>
  page_lookup_gather_kernel<LP>, test_chunk_gather*[gpu-cN]: c0 <0>, c1 and c-1 (pages up to
      512 KiB) <1>; the probe loops of both kernels in test_probe_chain_longer_than_a_window"""
import contextlib
import functools

import numpy as np
import pytest

from alluxio_amd.ops.native import lib

FILL = 0xA5
GUARD = 64            # fill bytes in front of and behind every destination
PAD = 4112            # other bytes in front of and behind a source: a multiple of 16, of no page size
INVALID = 6           # the store's invalid-argument code


def _noise(n, seed):
    """n bytes, none of them FILL."""
    a = np.random.default_rng(seed).integers(0, 255, n, dtype=np.uint8)
    a[a >= FILL] += 1
    return a


def _same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError((what, f"{bad.size} bytes differ, the first at {i}", got[i:i + 8].tolist(),
                              want[i:i + 8].tolist()))


# ---- harness -------------------------------------------------------------------------------------
class _Env:
    def __init__(self, mode):
        self.mode, self.gpu = mode, mode != "cpu"
        self.device = self.gpu or lib().device_count() > 0

    def buf(self, arr):
        """(handle, address) of a copy of `arr` that the path under test can address."""
        arr = np.ascontiguousarray(arr)
        if self.device:
            import torch
            t = torch.from_numpy(arr.copy())
            t = t.cuda() if self.gpu else t.pin_memory()
            ptr = t.data_ptr()
        else:
            raw = np.empty(arr.nbytes + 64, dtype=np.uint8)
            o = -raw.ctypes.data % 64
            t = raw[o:o + arr.nbytes].view(arr.dtype)
            t[:] = arr
            ptr = t.ctypes.data
        assert ptr % 16 == 0
        return t, ptr

    def sync(self):
        if self.device:
            import torch
            torch.cuda.synchronize()

    def host(self, handle):
        self.sync()
        return handle if isinstance(handle, np.ndarray) else handle.cpu().numpy()

    def stream(self):
        if not self.gpu:
            return 0
        import torch
        return int(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def _copy_setting(variant, grid_cap=0):
    v0, cap0 = lib().copy_variant()
    lib().set_copy_variant(variant, grid_cap)
    assert lib().copy_variant() == (variant, grid_cap or cap0)
    try:
        yield
    finally:
        lib().set_copy_variant(v0, cap0)             # 0 would keep the cap: put the recorded one back


@contextlib.contextmanager
def _seq_setting(variant, grid_cap=0):
    v0, cap0 = lib().seq_read_variant()
    lib().set_seq_read_variant(variant, grid_cap)
    assert lib().seq_read_variant() == (variant, grid_cap or cap0)
    try:
        yield
    finally:
        lib().set_seq_read_variant(v0, cap0)


@contextlib.contextmanager
def _pg_setting(small_max=None, wave=None, chunk=None):
    before = lib().page_gather_config()
    if small_max is not None:
        lib().set_page_gather_small_max(small_max)
    if wave is not None:
        lib().set_page_gather_wave_variant(wave)
    if chunk is not None:
        lib().set_page_gather_chunk_variant(chunk)
    now = lib().page_gather_config()
    assert now == tuple(b if x is None else x for b, x in zip(before, (small_max, wave, chunk)))
    try:
        yield
    finally:
        lib().set_page_gather_small_max(before[0])
        lib().set_page_gather_wave_variant(before[1])
        lib().set_page_gather_chunk_variant(before[2])


def _params(prefix, variants):
    return [pytest.param(("cpu", None), id="cpu")] + [
        pytest.param(("gpu", v), marks=pytest.mark.gpu, id=f"gpu-{prefix}{v}") for v in variants]


@pytest.fixture(scope="module", autouse=True)
def settings_before():
    found = (lib().copy_variant(), lib().seq_read_variant(), lib().page_gather_config())
    _SETTINGS.setdefault("before", found)
    yield


_SETTINGS = {}


# ==== 1. batched copy =============================================================================
# variant = unroll_sel * 4 + load policy * 2 + store policy; 7 is not listed: the default: branch
COPY_VARIANTS = [0, 1, 2, 3, 4, 5, 7, 8, 9]
PHASE_LENS = [0, 1, 3, 15, 16, 17, 31, 33, 255, 4101]


@pytest.fixture(params=_params("v", COPY_VARIANTS))
def cenv(request):
    mode, variant = request.param
    if mode == "cpu":
        yield _Env(mode)
        return
    request.getfixturevalue("gpu")
    with _copy_setting(variant):
        yield _Env(mode)


class _Layout:
    """Segments one after the other, source and destination each at a phase of its own; between two
    destinations lie 16 to 31 guard bytes."""

    def __init__(self):
        self.s = self.d = GUARD
        self.segs = []

    def add(self, n, sphase, dphase):
        s, d = self.s + sphase, self.d + dphase
        self.segs.append((s, d, n))
        self.s = -(-(s + n) // 16) * 16 + 16
        self.d = -(-(d + n) // 16) * 16 + 16
        return s, d

    def sizes(self):
        return self.s + GUARD, self.d + GUARD


def _copy_check(env, lay, seed):
    ssize, dsize = lay.sizes()
    src = _noise(ssize, seed)
    want = np.full(dsize, FILL, dtype=np.uint8)
    for s, d, n in lay.segs:
        want[d:d + n] = src[s:s + n]
    sh, sp = env.buf(src)
    dh, dp = env.buf(np.full(dsize, FILL, dtype=np.uint8))
    lib().batched_copy([(sp + s, dp + d, n) for s, d, n in lay.segs], 0, True)
    _same(env.host(dh), want, "destination")
    _same(env.host(sh), src, "source")


def test_copy_every_phase_pair(cenv):
    """16 x 16 phases x 10 lengths in one launch: the 16-byte, the 4-byte and the byte path of
    copy_range, each with its tail, and zero-length segments first, in between and last."""
    lay = _Layout()
    for sp in range(16):
        for dp in range(16):
            for n in (PHASE_LENS if (sp, dp) != (15, 15) else PHASE_LENS[::-1]):
                lay.add(n, sp, dp)
    assert len(lay.segs) == 2560 and lay.segs[0][2] == 0 and lay.segs[-1][2] == 0
    _copy_check(cenv, lay, 1)


def test_copy_ends_of_the_unrolled_loop(cenv):
    """n16 just below, at and above 256 * UNROLL for every UNROLL, with and without a byte tail;
    then the same lengths and n4 around 256 on the 4-byte path."""
    lens = [16 * (256 * u + d) + t for u in (4, 8, 16) for d in (-1, 0, 1) for t in (0, 5)]
    lay = _Layout()
    for n in lens:
        lay.add(n, 0, 0)
    for n in lens + [4 * 255, 4 * 256, 4 * 257, 4 * 256 + 3]:
        lay.add(n, 4, 12)
    _copy_check(cenv, lay, 2)


def _chunk_edges():
    c = int(lib().COPY_CHUNK)
    lay = _Layout()
    for sp, dp in ((0, 0), (4, 4), (1, 2)):             # the phase holds for every chunk of a segment
        for n in (c - 1, c, c + 1, 2 * c + 17, 3 * c + 5):
            lay.add(n, sp, dp)
    return lay


def test_copy_chunk_edges(cenv):
    _copy_check(cenv, _chunk_edges(), 3)


def test_copy_grid_stride(cenv):
    """Three workgroups for 33 chunks: each takes several, from different segments."""
    with _copy_setting(lib().copy_variant()[0], 3):
        _copy_check(cenv, _chunk_edges(), 4)
        lay = _Layout()
        for i in range(40):
            lay.add((i * 37) % 200, i % 16, (5 * i) % 16)
        _copy_check(cenv, lay, 5)


def test_copy_more_segments_than_one_launch(cenv):
    rng = np.random.default_rng(6)
    lay = _Layout()
    for n, sp, dp in zip(rng.integers(1, 41, 9000), rng.integers(0, 16, 9000), rng.integers(0, 16, 9000)):
        lay.add(int(n), int(sp), int(dp))
    assert len(lay.segs) > 8192                            # SegRing::kSegs
    _copy_check(cenv, lay, 6)


def test_copy_second_call_reads_what_the_first_wrote(cenv):
    env = cenv
    lens = [4101, 65536 + 7, 300000, 17, 1 << 20, 33]
    first, second = _Layout(), _Layout()
    for i, n in enumerate(lens):
        first.add(n, (3 * i) % 16, (7 * i + 1) % 16)
    second.d = first.d                                   # the copies of the copies lie behind the copies
    for i, (_, d, n) in enumerate(first.segs):
        second.segs.append((d, second.d + (5 * i + 2) % 16, n))
        second.d = -(-(second.segs[-1][1] + n) // 16) * 16 + 16
    ssize, dsize = first.sizes()[0], second.d + GUARD
    src = _noise(ssize, 7)
    want = np.full(dsize, FILL, dtype=np.uint8)
    for (s, d, n), (_, d2, _) in zip(first.segs, second.segs):
        want[d:d + n] = src[s:s + n]
        want[d2:d2 + n] = src[s:s + n]
    sh, sp = env.buf(src)
    dh, dp = env.buf(np.full(dsize, FILL, dtype=np.uint8))
    lib().batched_copy([(sp + s, dp + d, n) for s, d, n in first.segs], 0, False)
    lib().batched_copy([(dp + s, dp + d, n) for s, d, n in second.segs], 0, False)
    _same(env.host(dh), want, "destination")             # host() synchronizes once


# ==== 2. ring read ================================================================================
# bit 0: nontemporal stores, bit 1: unroll 16 (POW2 shapes), bit 2: nontemporal loads; -1: auto
SEQ_VARIANTS = [-1, 0, 1, 2, 3, 4, 5, 6, 7]
GAP = 32              # stream_stride - depth * buf
#                       page  file_len  buf  depth streams
RING_CASES = {
    "pow2":            (256, 10_007, 256, 8, 3),         # POW2 = true, a 7-byte tail
    "pow2_buf16":      (64, 1_000, 16, 4, 5),            # vpr = 1, shift 0, an 8-byte tail
    "not_pow2":        (256, 10_007, 48, 5, 7),          # the division path, buffers that straddle pages
    "multiple_of_buf": (4096, 8_192, 4096, 2, 2),        # the last real call is full, then EOF
    "short_file":      (256, 100, 256, 37, 3),           # cycle = 2: many passes per launch
    "shorter_than_a_vector": (64, 9, 64, 4, 2),          # only the byte tail
    "many_streams":    (256, 5_003, 32, 2, 300),         # the LDS fill loop beyond 256 threads
    "the_limit":       (64, 777, 16, 1, 8192),           # 32 KiB of LDS
}
# With grid_cap = 2 a round of the grid-stride loop takes 2 * 256 * UNROLL vectors, 4096 or 8192.  The
# two table shapes have 384 and 105 vectors, so they are also run with more streams: 8576 and
# 10500 vectors, two or three rounds, the last one ragged.
RING_CAPPED = {
    "pow2": RING_CASES["pow2"], "not_pow2": RING_CASES["not_pow2"],
    "pow2_67_streams": (256, 10_007, 256, 8, 67), "not_pow2_700_streams": (256, 10_007, 48, 5, 700),
}
RING_HOST_ONLY = {"buf_100": (256, 10_007, 100, 6, 4), "buf_24": (256, 10_007, 24, 5, 3)}


@pytest.fixture(params=_params("v", SEQ_VARIANTS))
def renv(request):
    mode, variant = request.param
    if mode == "cpu":
        yield _Env(mode)
        return
    request.getfixturevalue("gpu")
    with _seq_setting(variant):
        yield _Env(mode)


@pytest.fixture(params=["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])
def env(request):
    """Both paths at the settings as they stand."""
    if request.param == "gpu":
        request.getfixturevalue("gpu")
    return _Env(request.param)


@functools.lru_cache(maxsize=None)
def _ring_file(page, file_len):
    """(arena, page table, file bytes): the file's pages scattered over an arena about twice as
    large; the pages in between, and the rest of the file's last page, hold other bytes."""
    npg = -(-file_len // page)
    rng = np.random.default_rng(page + file_len)
    perm = rng.permutation(2 * npg + 3)[:npg].astype(np.int64)
    arena = _noise((2 * npg + 3) * page, file_len)
    data = _noise(file_len, file_len + 1)
    for v in range(npg):
        part = data[v * page:(v + 1) * page]
        arena[perm[v] * page:perm[v] * page + part.size] = part
    return arena, perm, data


def _ring_starts(file_len, buf, streams):
    """Start offsets: 0, the file's last buffer, one beyond the file (it clamps to the EOF call),
    the rest spread over the file's calls (distinct while there are calls left).  Two streams cannot
    hold all three: they take the last buffer and the one beyond, and a stream that starts at EOF
    reads call 0 next."""
    calls = -(-file_len // buf)
    last, beyond = (calls - 1) * buf, (calls + 3) * buf
    if streams == 2:
        return [last, beyond]
    starts = [((7 * s) % calls) * buf for s in range(streams)]
    starts[:3] = [0, last, beyond]
    return starts


def _ring_steps(shape):
    """At least 4; up to 12 where that lets a stream that starts at 0 pass the file's end twice."""
    file_len, buf, depth = shape[1], shape[2], shape[3]
    cycle = -(-file_len // buf) + 1
    return max(4, min(-(-2 * cycle // depth) + 1, 12))


def _ring_guard(buf):
    return GUARD + -(-buf // 64) * 64


def _ring_walk(shape, steps, data):
    """Per step: (ring, bytes, eofs, positions, last calls, total, reopens), every call of every
    step applied to one modelled ring (the ring that is yielded lives on into the next step)."""
    page, file_len, buf, depth, streams = shape
    stride, guard = depth * buf + GAP, _ring_guard(buf)
    cycle = -(-file_len // buf) + 1
    c_init = [min(o // buf, cycle - 1) for o in _ring_starts(file_len, buf, streams)]
    ring = np.full(guard + streams * stride + guard, FILL, dtype=np.uint8)
    sample = _ring_sample(streams)
    total, reopens = 0, 0
    for t in range(steps):
        nbytes = eofs = 0
        last = {}
        for s in range(streams):
            for k in range(depth):
                c = (c_init[s] + t * depth + k) % cycle
                if c == cycle - 1:                        # EOF: reopen, nothing written
                    eofs += 1
                    last[s, k] = (file_len, 0)
                    continue
                off = c * buf
                ln = min(buf, file_len - off)
                d = guard + s * stride + k * buf
                ring[d:d + ln] = data[off:off + ln]
                nbytes += ln
                last[s, k] = (off, ln)
        total += nbytes
        reopens += eofs
        pos = {s: min(((c_init[s] + (t + 1) * depth) % cycle) * buf, file_len) for s in sample}
        yield ring, nbytes, eofs, pos, {(s, k): last[s, k] for s in sample for k in range(depth)}, total, reopens


@functools.lru_cache(maxsize=None)
def _ring_model(shape, steps):
    """The walk over the shape's own file, computed once for all ids."""
    return [(step[0].copy(),) + step[1:] for step in _ring_walk(shape, steps, _ring_file(shape[0], shape[1])[2])]


def _ring_sample(streams):
    return list(range(streams)) if streams <= 300 else sorted(set(range(0, streams, 97)) | {streams - 1})


def _ring_open(env, shape, ring_ptr, arena_ptr, perm=None, **kw):
    page, file_len, buf, depth, streams = shape
    perm = _ring_file(page, file_len)[1] if perm is None else perm
    a = dict(arena_base=arena_ptr + PAD, file_pages=perm.tolist(), page_size=page, file_len=file_len,
             device=0 if env.gpu else -1, dst_base=ring_ptr + _ring_guard(buf), stream_stride=depth * buf + GAP,
             buf_bytes=buf, depth=depth, streams=streams, dst_kind=1 if env.gpu else 0,
             start_offsets=_ring_starts(file_len, buf, streams))
    a.update(kw)
    return lib().RingReadSession.remote(**a)


def _ring_buffers(env, shape, arena=None):
    page, file_len, buf, depth, streams = shape
    arena = _ring_file(page, file_len)[0] if arena is None else arena
    big = np.concatenate([_noise(PAD, 11), arena, _noise(PAD, 12)])
    size = 2 * _ring_guard(buf) + streams * (depth * buf + GAP)
    return env.buf(big), env.buf(np.full(size, FILL, dtype=np.uint8))


def _ring_check(env, shape, file=None, steps=None):
    """`file`: (arena, page table, file bytes) where the shape's own file is not meant."""
    depth, steps = shape[3], steps or _ring_steps(shape)
    want = _ring_model(shape, steps) if file is None else _ring_walk(shape, steps, file[2])
    (ah, ap), (rh, rp) = _ring_buffers(env, shape, None if file is None else file[0])
    sess = _ring_open(env, shape, rp, ap, None if file is None else file[1])
    try:
        for t, (ring, nbytes, eofs, pos, last, total, reopens) in enumerate(want):
            assert sess.step(env.stream()) == (nbytes, eofs), t
            _same(env.host(rh), ring, f"ring after step {t}")
            assert (sess.total_bytes, sess.reopens, sess.calls) == (total, reopens, (t + 1) * depth), t
            for s in pos:
                assert sess.position(s) == pos[s], (t, s)
            for (s, k), call in last.items():
                assert sess.last_call(s, k) == call, (t, s, k)
    finally:
        sess.close()
    assert reopens >= 2                                   # the file's end was passed


@pytest.mark.parametrize("case", list(RING_CASES))
def test_ring_shapes(renv, case):
    _ring_check(renv, RING_CASES[case])


@pytest.mark.parametrize("case", list(RING_CAPPED))
def test_ring_grid_stride(renv, case):
    with _seq_setting(lib().seq_read_variant()[0], 2):
        _ring_check(renv, RING_CAPPED[case])


@pytest.mark.gpu
def test_ring_picks_nontemporal_loads_by_itself(gpu):
    """Variant -1 and 128 MiB of distinct file bytes in one launch (32 streams that start at
    distinct calls x 4 reads of 1 MiB): the launcher takes the nontemporal-load kernel by itself.
    The file's 129 pages repeat the 13 pages of a small arena, so only the ring is large."""
    page = buf = 1 << 20
    shape = (page, (128 << 20) + 5, buf, 4, 32)
    arena = _noise(16 * page, 40)
    perm = np.array([(5 * v + 3) % 13 for v in range(129)], dtype=np.int64)
    data = np.concatenate([arena[p * page:(p + 1) * page] for p in perm])[:shape[1]]
    starts = _ring_starts(shape[1], buf, 32)
    assert len({min(o // buf, 129) for o in starts}) * 4 * buf >= 128 << 20
    with _seq_setting(-1):
        _ring_check(_Env("gpu"), shape, (arena, perm, data), steps=4)


@pytest.mark.parametrize("case", list(RING_HOST_ONLY))
def test_ring_cpu_only_buffer_sizes_that_are_no_multiple_of_16(case):
    _ring_check(_Env("cpu"), RING_HOST_ONLY[case])


def test_ring_model_on_a_small_example():
    shape = (64, 9, 64, 4, 2)                            # one call of 9 bytes, then EOF: cycle = 2
    steps = _ring_model(shape, 4)
    assert [s[1:3] for s in steps] == [(2 * 9 * 2, 4)] * 4 and steps[-1][5:] == (144, 16)
    ring, guard, data = steps[0][0], _ring_guard(64), _ring_file(64, 9)[2]
    assert _ring_starts(9, 64, 2) == [0, 256]            # stream 0 reads at k = 0 and 2, stream 1 at 1 and 3
    assert (ring[guard:guard + 9] == data).all() and (ring[guard + 9:guard + 128] == FILL).all()
    assert (ring[guard + 128:guard + 137] == data).all() and (ring[:guard] == FILL).all()
    s1 = guard + 4 * 64 + GAP
    assert (ring[guard + 137:s1 + 64] == FILL).all() and (ring[s1 + 64:s1 + 73] == data).all()


RING_REJECTED = ["8193_streams", "stride_too_small", "empty_file", "short_page_table", "page_size_not_pow2"]
RING_REJECTED_ON_DEVICE = ["buf_24", "stride_not_16", "ring_base_8"]     # the host loop takes these


@pytest.mark.parametrize("mode,case", [pytest.param("cpu", c, id=f"cpu-{c}") for c in RING_REJECTED] + [
    pytest.param("gpu", c, marks=pytest.mark.gpu, id=f"gpu-{c}") for c in RING_REJECTED + RING_REJECTED_ON_DEVICE])
def test_ring_rejections(request, mode, case):
    if mode == "gpu":
        request.getfixturevalue("gpu")
    env = _Env(mode)
    shape = RING_CASES["not_pow2"]
    page, file_len, buf, depth, streams = shape
    kw = {}
    if case == "8193_streams":
        shape, kw = (page, file_len, buf, depth, 2), dict(streams=8193, start_offsets=[])
    elif case == "buf_24":
        kw = dict(buf_bytes=24)
    elif case == "stride_not_16":
        kw = dict(stream_stride=depth * buf + 8)
    elif case == "ring_base_8":
        kw = dict(dst_base=8)                               # added to the ring's address below
    elif case == "stride_too_small":
        kw = dict(stream_stride=depth * buf - 16)
    elif case == "empty_file":
        kw = dict(file_len=0)
    elif case == "short_page_table":
        kw = dict(file_pages=_ring_file(page, file_len)[1].tolist()[:-1])
    else:
        kw = dict(page_size=192)
    (ah, ap), (rh, rp) = _ring_buffers(env, shape)
    if "dst_base" in kw:
        kw["dst_base"] = rp + _ring_guard(buf) + 8
    with pytest.raises(lib().StoreError) as e:
        _ring_open(env, shape, rp, ap, **kw)
    assert e.value.args[0] == INVALID
    assert (env.host(rh) == FILL).all()                  # nothing was written
    _ring_open(env, shape, rp, ap).close()               # and the same shape without the flaw is taken


# ==== 3. page gather ==============================================================================
WAVE_VARIANTS = [0, 1, 2, 3, 4, 5]        # requests per wave 4, 8, 4, 8, 4, 4
CHUNK_VARIANTS = [-1, 0, 1]
MISS = (77 << 24) | 5                     # keys from here on are never inserted


def _key(fid, idx):
    return (fid << 24) | idx


def _mixed_lens(ps, extra=()):
    lens = []
    for n in [ps, ps - 1, ps - 16, 17, 16, 15, 1, 0, *extra]:
        if 0 <= n <= ps and n not in lens:
            lens.append(n)
    return lens * 3


class _Pages:
    """A cache (device or host) of `slots` pages of `ps` bytes and what it must hold."""

    def __init__(self, env, ps, lens, slots=None, seed=0):
        self.env, self.ps, self.seed = env, ps, seed
        self.pc = lib().PageCache(0, (slots or len(lens) + 2) * ps, ps, env.gpu)
        assert self.pc.on_device == env.gpu
        self.data, self.slot, self.keys, self._rows = {}, {}, [], {}
        for j, n in enumerate(lens):
            self.put(_key(3 + j % 3, 1000 + 7 * j), n)

    def put(self, key, n, evict=False):
        """Key -> n bytes.  The slot is first filled with a whole page of other bytes, so what
        follows a short page in the arena is neither the page nor the fill."""
        self.seed += 1
        self.pc.put_bytes(key, _noise(self.ps, 10_000 + self.seed), evict)
        data = _noise(n, 20_000 + self.seed)
        assert self.pc.put_bytes(key, data, False) == []
        if key not in self.data:
            self.keys.append(key)
        self.data[key] = data
        self.slot[key] = self.pc.lookup(key)[0]
        self._rows.clear()

    def erase(self, key):
        assert self.pc.erase(key)
        del self.data[key], self.slot[key]
        self.keys.remove(key)
        self._rows.clear()

    def rows(self, stride):
        """[pages + 1, stride]: what a hit on each page leaves in its row; the last row is a miss."""
        if stride not in self._rows:
            r = np.full((len(self.keys) + 1, stride), FILL, dtype=np.uint8)
            for j, k in enumerate(self.keys):
                r[j, :self.data[k].size] = self.data[k]
            self._rows[stride] = r
        return self._rows[stride]

    def gather(self, req, stride=None, base=0):
        """Gather the keys `req` into rows of `stride` bytes that start `base` bytes behind a
        16-byte boundary, and compare everything."""
        env, stride = self.env, stride or self.ps
        n = len(req)
        index = {k: j for j, k in enumerate(self.keys)}
        which = np.array([index.get(k, len(self.keys)) for k in req])
        size = GUARD + base + n * stride + GUARD
        want = np.full(size, FILL, dtype=np.uint8)
        want[GUARD + base:GUARD + base + n * stride] = self.rows(stride)[which].reshape(-1)
        want_slot = np.array([self.slot.get(k, -1) for k in req], dtype=np.int32)
        want_len = np.array([self.data[k].size if k in self.data else 0 for k in req], dtype=np.int32)
        dh, dp = env.buf(np.full(size, FILL, dtype=np.uint8))
        kh, kp = env.buf(np.array(req, dtype=np.int64))
        sh, sp = env.buf(np.full(n, 77, dtype=np.int32))
        lh, lp = env.buf(np.full(n, 77, dtype=np.int32))
        self.pc.gather(kp, n, dp + GUARD + base, stride, sp, lp, env.stream())
        _same(env.host(sh), want_slot, "slot_out")
        _same(env.host(lh), want_len, "len_out")
        _same(env.host(dh), want, f"destination, n={n} stride={stride} base={base}")
        return want_slot


def _requests(pages, n, shift, group=8):
    """n keys: in the g-th group of eight, position (g + shift) % 8 is a miss, which puts a miss at
    every position of a wave's four (or eight) requests; the hits walk through the pages five at a
    time, so the longest page of a wave is a different request each time."""
    req = []
    for i in range(n):
        g, pos = divmod(i, group)
        if pos == (g + shift) % group:
            req.append(MISS + i)
        else:
            req.append(pages.keys[(5 * i + 3 * shift) % len(pages.keys)])
    return req


_CACHES = {}


def _pages(env, ps, extra=()):
    key = (env.mode, ps)
    if key not in _CACHES:
        _CACHES[key] = _Pages(env, ps, _mixed_lens(ps, extra), seed=ps)
    p = _CACHES[key]
    p.env = env
    return p


@pytest.fixture(params=_params("w", WAVE_VARIANTS))
def wenv(request):
    mode, variant = request.param
    if mode == "cpu":
        yield _Env(mode)
        return
    request.getfixturevalue("gpu")
    with _pg_setting(wave=variant):
        yield _Env(mode)


@pytest.fixture(params=_params("c", CHUNK_VARIANTS))
def kenv(request):
    mode, variant = request.param
    if mode == "cpu":
        yield _Env(mode)
        return
    request.getfixturevalue("gpu")
    with _pg_setting(chunk=variant):
        yield _Env(mode)


def test_page_key_hash_is_splitmix64():
    assert lib().page_key_hash(0) == 0xE220A8397B1DCDAF      # SplitMix64's first output for seed 0
    assert lib().page_key_hash(1) != lib().page_key_hash(2)


@pytest.mark.parametrize("ps", [16, 256, 4096, 16384])
def test_wave_gather(wenv, ps):
    """Partial lengths (the len & 15 tail, maxlen over mixed lengths), misses at every position of
    a wave, n % PW != 0, one wave, two waves and more than one workgroup."""
    pages = _pages(wenv, ps)
    for n in (1, 2, 3, 4, 5, 7, 8, 9):
        for shift in range(8):
            pages.gather(_requests(pages, n, shift))
    slots = pages.gather(_requests(pages, 257, 3))
    assert (slots < 0).sum() == 32 and (slots >= 0).sum() == 225


@pytest.mark.parametrize("ps", [32 << 10, 128 << 10, (128 << 10) + 4096])
def test_chunk_gather(kenv, ps):
    """Pages above small_max.  128 KiB + 4096 has two chunks, the second one short, and lengths that
    end just before, at and just behind the first chunk.  Strides of ps + 4 and ps + 1 and a base
    at +4 reach the 4-byte and the byte path of copy_range."""
    pages = _pages(kenv, ps, extra=[(128 << 10) - 1, 128 << 10, (128 << 10) + 1])
    for stride, base in ((ps, 0), (ps + 4, 0), (ps + 1, 0), (ps + 16, 4)):
        for shift in (0, 3):
            pages.gather(_requests(pages, 13, shift), stride, base)


def test_chunk_gather_of_small_pages(kenv):
    """256-byte pages: through the chunk kernel by small_max = 0, and by a destination that the wave
    kernel does not take (the launcher then leaves it by itself)."""
    pages = _pages(kenv, 256)
    layouts = ((256, 0), (256 + 4, 0), (256 + 1, 0), (256 + 16, 4))
    with _pg_setting(small_max=0):
        for stride, base in layouts:
            for n in (1, 5, 64):
                pages.gather(_requests(pages, n, 2), stride, base)
    for stride, base in layouts[1:]:
        pages.gather(_requests(pages, 9, 1), stride, base)


def _many_requests(pages, n):
    idx = np.random.default_rng(n).integers(0, len(pages.keys) + 1, n)       # the last index: a miss
    table = np.array(pages.keys + [MISS], dtype=np.int64)
    return table[idx].tolist()


def test_chunk_gather_above_its_grid_cap(env):
    """70 000 requests of 256-byte pages, above 65535 workgroups: some workgroups serve two
    requests, with the pair of barriers in between."""
    pages = _pages(env, 256)
    with _pg_setting(small_max=0):
        pages.gather(_many_requests(pages, 70_000))


def test_wave_gather_above_its_grid_cap(env):
    """140 000 requests of 64-byte pages, above 8192 workgroups x 4 waves x 4 requests."""
    assert lib().page_gather_config()[1] in (0, 2, 4, 5)
    pages = _pages(env, 64)
    pages.gather(_many_requests(pages, 140_000))


# ---- probe chains ------------------------------------------------------------------------------
CHAIN_SLOTS, CHAIN_TABLE = 128, 512       # next_pow2(4 * slots) entries
CHAIN_HOME, CHAIN_LEN = CHAIN_TABLE - 40, 100


@functools.lru_cache(maxsize=None)
def _chain_keys():
    """CHAIN_LEN + 1 keys whose home (hash & mask) lies in the eight entries from CHAIN_HOME on.  The
    first eight have one home each, in order, so key j of the chain lands j entries behind
    CHAIN_HOME; keys 63 and 64 have CHAIN_HOME as their home: the edge of the first probe window."""
    pool = [[] for _ in range(8)]
    for fid in range(1, 9):
        for page in range(4000):
            k = _key(fid, page)
            o = (lib().page_key_hash(k) & (CHAIN_TABLE - 1)) - CHAIN_HOME
            if 0 <= o < 8:
                pool[o].append(k)
    keys = [pool[o].pop() for o in range(8)]
    for j in range(8, CHAIN_LEN + 1):
        keys.append(pool[0 if j in (63, 64) else j % 8].pop())
    return keys


def _landing(keys):
    """Entry of each key after linear-probing inserts in order into an empty table."""
    taken, at = set(), {}
    for k in keys:
        i = lib().page_key_hash(k) & (CHAIN_TABLE - 1)
        while i in taken:
            i = (i + 1) & (CHAIN_TABLE - 1)
        taken.add(i)
        at[k] = i
    return at


@pytest.fixture(params=["cpu", pytest.param("gpu-wave4", marks=pytest.mark.gpu),
                        pytest.param("gpu-wave8", marks=pytest.mark.gpu), pytest.param("gpu-chunk", marks=pytest.mark.gpu)])
def penv(request):
    if request.param == "cpu":
        yield _Env("cpu")
        return
    request.getfixturevalue("gpu")
    kw = {"gpu-wave4": dict(wave=2), "gpu-wave8": dict(wave=1), "gpu-chunk": dict(small_max=0)}[request.param]
    with _pg_setting(**kw):
        yield _Env("gpu")


def test_probe_chain_longer_than_a_window(penv):
    """A chain of 100 keys that starts 40 entries before the table's end: it wraps past entry 0, its
    later keys lie more than one 64-entry window from home, and a third of it turns into
    tombstones."""
    keys, never = _chain_keys()[:CHAIN_LEN], _chain_keys()[CHAIN_LEN]
    at = _landing(keys)
    dist = {(at[k] - lib().page_key_hash(k)) & (CHAIN_TABLE - 1) for k in keys}
    assert {63, 64} <= dist and max(dist) > 90 and min(at.values()) == 0        # the window edge; the wrap
    pages = _Pages(penv, 64, [], slots=CHAIN_SLOTS, seed=500)
    assert pages.pc.table_size == CHAIN_TABLE
    for j, k in enumerate(keys):
        pages.put(k, (64, 63, 17, 48, 1)[j % 5])
    req = keys + [never, MISS]
    slots = pages.gather(req)
    assert (slots[:CHAIN_LEN] >= 0).all() and slots[CHAIN_LEN] == -1 and slots[CHAIN_LEN + 1] == -1
    erased = keys[::3]
    for k in erased:
        pages.erase(k)                                      # tombstones do not stop the probe
    slots = pages.gather(req)
    assert [s < 0 for s in slots[:CHAIN_LEN]] == [j % 3 == 0 for j in range(CHAIN_LEN)] and slots[CHAIN_LEN] == -1
    pages.put(erased[20], 33)                               # key 60 of the chain, back in
    slots = pages.gather(req + [erased[20]])
    assert slots[60] >= 0 and slots[-1] == slots[60] and (slots[:CHAIN_LEN] >= 0).sum() == CHAIN_LEN - len(erased) + 1


def test_gathered_pages_are_not_evicted(env):
    """Stamps: what the latest gathers touched (here the oldest pages of a full cache) stays; the
    put evicts the oldest pages that were not gathered."""
    pages = _Pages(env, 256, [256, 100] * 64, slots=128, seed=900)
    keys = list(pages.keys)
    hot = keys[:16]
    for _ in range(3):
        pages.gather(hot + [MISS])
    fresh = _key(9, 1)
    evicted = pages.pc.put_bytes(fresh, _noise(256, 901), True)
    assert sorted(evicted) == sorted(keys[16:18])           # slots / 64 = 2 victims
    assert pages.pc.contains(fresh) and all(pages.pc.contains(k) for k in hot)
    for k in evicted:
        del pages.data[k], pages.slot[k]
        pages.keys.remove(k)
    pages._rows.clear()
    slots = pages.gather(hot + evicted)
    assert (slots[:16] >= 0).all() and (slots[16:] == -1).all()


# ==== afterwards ==================================================================================
def test_settings_are_back_after_the_cpu_and_gpu_ids():
    _CACHES.clear()
    assert (lib().copy_variant(), lib().seq_read_variant(), lib().page_gather_config()) == _SETTINGS["before"]
