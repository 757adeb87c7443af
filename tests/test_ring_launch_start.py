"""What a ring-read launch takes from its arguments instead of from memory (the streams' shared
cursor, the first page-table entries of the launch's window), byte for byte, at the smallest shapes
at which it can go wrong.

As in test_ring_fast_path.py: the ring starts as FILL bytes and no source byte is FILL; the file's
pages are scattered through a larger arena of other bytes; the streams' strides are GAP bytes wider
than their slots and the ring has guard bytes in front and behind.  The expected ring comes from a
numpy model of the read(buf)/reopen loop written here, and the WHOLE buffer is compared after
every step, with the step's byte and EOF counts, the totals and every stream's position.  No
tolerances.  Every case runs for enough steps to pass the EOF call twice.

`cpu` ids run RingReadSession's host loop (device = -1), `gpu-vN` ids the fast kernel under variant
N (bit 0: nontemporal stores, bit 1: U = 16, bit 2: nontemporal loads, -1: the launcher's choice)
and assert through seq_read_last_launch(detail=True) what the launch took from its arguments: the
cursor where every stream starts at the same call, INLINE page entries in every session."""
import contextlib
import functools

import numpy as np
import pytest

from alluxio_amd.ops.native import lib

FILL = 0xA5
GUARD = 64            # fill bytes in front of and behind the ring
GAP = 32              # stream_stride - depth * buf
PAD = 4112            # other bytes in front of and behind the arena: a multiple of 16, of no page size
INLINE = 4            # page entries a launch carries (kSeqInlinePages)
VARIANTS = [-1, 0, 1, 4, 2, 7]

#         page   file_len                      buf  depth streams
TAIL7 = (1024, 5 * 1024 + 7, 1024, 3, 5)                 # cycle 7, a tail chunk of 7 bytes
CASES = {
    "tail7":            TAIL7,
    # the window spans 8 pages, more than INLINE: inline and loaded entries mix within one launch
    "window_8_pages":   (1024, 6 * 1024 + 40, 2048, 4, 3),
    # the window lies inside one page, then straddles two, then wraps past EOF to page 0
    "window_in_a_page": (16384, 5 * 16384 + 3 * 1024 + 5, 4096, 4, 3),
    "depth_above_cycle": (1024, 1500, 1024, 8, 3),        # cycle = 3: the MULTI loop
}
RAGGED = (2048, 20 * 1024 + 16, 1024, 16, 9)              # under grid_cap 1 and 2


def _noise(n, seed):
    """n bytes, none of them FILL."""
    a = np.random.default_rng(seed).integers(0, 255, n, dtype=np.uint8)
    a[a >= FILL] += 1
    return a


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError((what, f"{bad.size} bytes differ, the first at {i}", got[i:i + 8].tolist(),
                              want[i:i + 8].tolist()))


@functools.lru_cache(maxsize=None)
def _file(page, file_len, at_end=False):
    """(arena, page table, file bytes): the file's pages scattered over an arena about twice as
    large; the pages in between, and the rest of the file's last page, hold other bytes.
    at_end: the file's last page is the arena's last page."""
    npg = -(-file_len // page)
    rng = np.random.default_rng(3 * page + file_len)
    perm = rng.permutation(2 * npg + 3)[:npg].astype(np.int64)
    if at_end:
        last = 2 * npg + 2
        if last in perm[:-1]:
            perm[int(np.flatnonzero(perm == last)[0])] = perm[-1]
        perm[-1] = last
    assert len(set(perm.tolist())) == npg
    arena = _noise((2 * npg + 3) * page, file_len + 2)
    data = _noise(file_len, file_len + 3)
    for v in range(npg):
        part = data[v * page:(v + 1) * page]
        arena[perm[v] * page:perm[v] * page + part.size] = part
    return arena, perm, data


def _mixed_starts(file_len, buf, streams):
    """0, the file's last buffer, one beyond the file (it clamps to the EOF call), the rest spread
    over the file's calls."""
    calls = -(-file_len // buf)
    starts = [((5 * s + 1) % calls) * buf for s in range(streams)]
    starts[:3] = [0, (calls - 1) * buf, (calls + 3) * buf]
    return tuple(starts)


def _steps(shape):
    """At least 3; enough for a stream to pass the file's end twice wherever it starts."""
    file_len, buf, depth = shape[1], shape[2], shape[3]
    cycle = -(-file_len // buf) + 1
    return max(3, min(-(-3 * cycle // depth) + 1, 16))


@functools.lru_cache(maxsize=None)
def _model(shape, starts, at_end=False):
    """Per step: (ring, bytes, eofs, positions, total, reopens)."""
    page, file_len, buf, depth, streams = shape
    data = _file(page, file_len, at_end)[2]
    stride = depth * buf + GAP
    cycle = -(-file_len // buf) + 1
    c_init = [min(o // buf, cycle - 1) for o in starts]
    ring = np.full(GUARD + streams * stride + GUARD, FILL, dtype=np.uint8)
    total = reopens = 0
    out = []
    for t in range(_steps(shape)):
        nbytes = eofs = 0
        for s in range(streams):
            for k in range(depth):
                c = (c_init[s] + t * depth + k) % cycle
                if c == cycle - 1:                        # EOF: reopen, nothing written
                    eofs += 1
                    continue
                off = c * buf
                ln = min(buf, file_len - off)
                d = GUARD + s * stride + k * buf
                ring[d:d + ln] = data[off:off + ln]
                nbytes += ln
        total += nbytes
        reopens += eofs
        pos = [min(((c_init[s] + (t + 1) * depth) % cycle) * buf, file_len) for s in range(streams)]
        out.append((ring.copy(), nbytes, eofs, pos, total, reopens))
    assert min((c_init[s] + _steps(shape) * depth) // cycle - c_init[s] // cycle for s in range(streams)) >= 2
    return out


def test_model_on_a_small_example():
    shape = CASES["depth_above_cycle"]                    # calls of 1024 and 476 bytes, then EOF
    steps = _model(shape, (1024,) * 3)                    # every stream from call 1: calls 1 2 0 1 2 0 1 2
    assert steps[0][1:3] == (3 * (476 + 1500 + 1500), 3 * 3)
    ring, data = steps[0][0], _file(1024, 1500)[2]
    assert (ring[:GUARD] == FILL).all() and (ring[GUARD:GUARD + 476] == data[1024:]).all()
    assert (ring[GUARD + 476:GUARD + 2048] == FILL).all()            # the tail of slot 0, the EOF call's slot 1
    assert (ring[GUARD + 2048:GUARD + 3072] == data[:1024]).all()


class _Env:
    def __init__(self, gpu):
        self.gpu = gpu

    def buf(self, arr):
        arr = np.ascontiguousarray(arr)
        if self.gpu:
            import torch
            t = torch.from_numpy(arr.copy()).cuda()
            ptr = t.data_ptr()
        else:
            raw = np.empty(arr.nbytes + 64, dtype=np.uint8)
            o = -raw.ctypes.data % 64
            t = raw[o:o + arr.nbytes]
            t[:] = arr
            ptr = t.ctypes.data
        assert ptr % 16 == 0
        return t, ptr

    def host(self, handle):
        return handle.cpu().numpy() if self.gpu else handle     # .cpu() synchronizes

    def stream(self):
        if not self.gpu:
            return 0
        import torch
        return int(torch.cuda.current_stream().cuda_stream)


@contextlib.contextmanager
def _setting(variant, grid_cap=0):
    v0, cap0 = lib().seq_read_variant()
    lib().set_seq_read_variant(variant, grid_cap)
    try:
        yield
    finally:
        lib().set_seq_read_variant(v0, cap0)


class _Run:
    """One session over its own arena and ring, stepped and checked one step at a time."""

    def __init__(self, env, shape, starts, at_end=False):
        page, file_len, buf, depth, streams = shape
        self.env, self.shape, self.t = env, shape, 0
        self.want = _model(shape, tuple(starts), at_end)
        arena, perm, _ = _file(page, file_len, at_end)
        self.ah, ap = env.buf(np.concatenate([_noise(PAD, 11), arena, _noise(PAD, 12)]))
        self.rh, rp = env.buf(np.full(self.want[0][0].size, FILL, dtype=np.uint8))
        self.sess = lib().RingReadSession.remote(
            arena_base=ap + PAD, file_pages=perm.tolist(), page_size=page, file_len=file_len,
            device=0 if env.gpu else -1, dst_base=rp + GUARD, stream_stride=depth * buf + GAP, buf_bytes=buf,
            depth=depth, streams=streams, dst_kind=1 if env.gpu else 0, start_offsets=list(starts))

    def step(self, detail=None):
        """detail: (cursor from the arguments, inline page entries) the launch must report."""
        t, depth, streams = self.t, self.shape[3], self.shape[4]
        ring, nbytes, eofs, pos, total, reopens = self.want[t]
        assert self.sess.step(self.env.stream()) == (nbytes, eofs), t
        if detail is not None:
            got = lib().seq_read_last_launch(detail=True)
            assert len(got) == 5 and got[:3] == lib().seq_read_last_launch(), t
            assert (got[0], got[3], got[4]) == ("fast",) + detail, (t, got)
        _same(self.env.host(self.rh), ring, f"ring after step {t}")
        assert (self.sess.total_bytes, self.sess.reopens, self.sess.calls) == (total, reopens, (t + 1) * depth), t
        assert [self.sess.position(s) for s in range(streams)] == pos, t
        self.t += 1
        return self.t < len(self.want)

    def close(self):
        self.sess.close()


def _check(env, shape, starts, detail=None, at_end=False):
    run = _Run(env, shape, starts, at_end)
    try:
        while run.step(detail):
            pass
    finally:
        run.close()


def _uniform(shape, call=0):
    return (call * shape[2],) * shape[4]


@pytest.mark.parametrize("case", list(CASES))
def test_uniform_cursor_cpu(case):
    _check(_Env(False), CASES[case], _uniform(CASES[case]))


def test_other_starts_cpu():
    _check(_Env(False), TAIL7, _mixed_starts(*TAIL7[1:3], TAIL7[4]))
    _check(_Env(False), TAIL7, _uniform(TAIL7, 2))
    _check(_Env(False), RAGGED, _uniform(RAGGED))
    _check(_Env(False), TAIL7, _uniform(TAIL7), at_end=True)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=[f"v{v}" for v in VARIANTS])
@pytest.mark.parametrize("case", list(CASES))
def test_uniform_cursor_gpu(gpu, case, variant):
    """Every stream starts at call 0 (no start offsets: the default session)."""
    with _setting(variant):
        _check(_Env(True), CASES[case], _uniform(CASES[case]), (True, INLINE))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=[f"v{v}" for v in VARIANTS])
def test_differing_cursors_are_loaded_gpu(gpu, variant):
    """Starts 0, last buffer, beyond the file, ...: the cursors come from c_init[s]; the inline
    page entries are stream 0's."""
    with _setting(variant):
        _check(_Env(True), TAIL7, _mixed_starts(*TAIL7[1:3], TAIL7[4]), (False, INLINE))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=[f"v{v}" for v in VARIANTS])
@pytest.mark.parametrize("call", [2, 5, 6], ids=["call2", "last_call", "eof_call"])
def test_equal_nonzero_starts_are_uniform_gpu(gpu, call, variant):
    with _setting(variant):
        _check(_Env(True), TAIL7, _uniform(TAIL7, call), (True, INLINE))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=[f"v{v}" for v in VARIANTS])
@pytest.mark.parametrize("cap", [1, 2])
def test_ragged_rounds_under_a_grid_cap_gpu(gpu, cap, variant):
    """18 trips of 8 (9 of 16) on 4 or 8 waves: a wave's last trip is not its first."""
    with _setting(variant, cap):
        _check(_Env(True), RAGGED, _uniform(RAGGED), (True, INLINE))
        assert lib().seq_read_last_launch()[2] == cap


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [-1, 0, 2], ids=["v-1", "v0", "v2"])
def test_file_ends_with_the_arena_gpu(gpu, variant):
    """Cached loads; the file's last page is the arena's last page: every read of the launch, the
    wrap to page 0 behind the EOF call included, resolves inside the file's pages."""
    with _setting(variant):
        _check(_Env(True), TAIL7, _uniform(TAIL7), (True, INLINE), at_end=True)
        _check(_Env(True), CASES["window_in_a_page"], _uniform(CASES["window_in_a_page"]), (True, INLINE), at_end=True)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [-1, 7], ids=["v-1", "v7"])
def test_two_sessions_alternate_on_one_stream_gpu(gpu, variant):
    """One uniform, one not, of different shapes: what a session keeps between its steps (kernel,
    grid, cursor choice, page entries) does not reach the other."""
    env = _Env(True)
    with _setting(variant):
        a = _Run(env, TAIL7, _uniform(TAIL7, 2))
        b = _Run(env, CASES["window_8_pages"], _mixed_starts(*CASES["window_8_pages"][1:3], 3))
        try:
            more_a = more_b = True
            while more_a or more_b:
                more_a = more_a and a.step((True, INLINE))
                more_b = more_b and b.step((False, INLINE))
        finally:
            a.close()
            b.close()


@pytest.mark.gpu
def test_a_new_variant_replaces_a_session_s_kernel_gpu(gpu):
    """The kernel and grid a session keeps are chosen anew once the variant is set."""
    env = _Env(True)
    v0 = lib().seq_read_variant()
    run = _Run(env, RAGGED, _uniform(RAGGED))
    try:
        with _setting(0, 2):
            run.step((True, INLINE))
            assert lib().seq_read_last_launch() == ("fast", 8, 2)
            lib().set_seq_read_variant(2, 1)
            run.step((True, INLINE))
            assert lib().seq_read_last_launch() == ("fast", 16, 1)
        while run.step((True, INLINE)):
            pass
    finally:
        run.close()
    assert lib().seq_read_variant() == v0                 # the setting is back where it was
