"""The ring reader's fast kernel (seq_read_fast_kernel: buf a multiple of 1 KiB, pages of at least
1 KiB), byte for byte, at the smallest shapes at which it can go wrong.

As in test_copy_kernels.py: the ring starts as FILL bytes and no source byte is FILL; the file's
pages are scattered through a larger arena of other bytes; the streams' strides are GAP bytes wider
than their slots and the ring has guard bytes in front and behind.  The expected ring comes from a
numpy model of the read(buf)/reopen loop written here, and the WHOLE buffer is compared after
every step, with the step's byte and EOF counts, the totals, every stream's position and every
call of the step.  No tolerances.

`cpu` ids run RingReadSession's host loop (device = -1), `gpu-vN` ids the kernel under variant N
(bit 0: nontemporal stores, bit 1: U = 16, bit 2: nontemporal loads, -1: the launcher's choice) and
assert through seq_read_last_launch() which kernel ran, with what U and grid."""
import contextlib
import functools

import numpy as np
import pytest

from alluxio_amd.ops.native import lib

FILL = 0xA5
GUARD = 64            # fill bytes in front of and behind the ring
GAP = 32              # stream_stride - depth * buf
PAD = 4112            # other bytes in front of and behind the arena: a multiple of 16, of no page size
VARIANTS = [-1, 0, 1, 4, 5, 2, 7]

#         page   file_len          buf  depth streams
CASES = {
    "tail7_one_chunk_per_page":  (1024, 5 * 1024 + 7, 1024, 3, 5),     # depth no power of two, a 7-byte tail chunk
    "read_spans_two_pages":      (1024, 6 * 1024 + 40, 2048, 4, 3),    # tail: two whole vectors, then 8 bytes
    "file_multiple_of_buf":      (4096, 3 * 4096, 1024, 4, 4),         # the EOF call leaves its slot's fill untouched
    "cycle_below_depth":         (1024, 1500, 1024, 8, 3),             # cycle = 3: passes and EOFs inside one launch
    "ragged_rounds":             (2048, 20 * 1024 + 16, 1024, 16, 9),  # run under grid_cap 1 and 2 as well
    # 8 KiB trips in 16 KiB pages: some are contiguous in file and ring (one lookup for the trip),
    # some straddle a page, the pass ends inside one
    "contiguous_trips":          (16384, 5 * 16384 + 3 * 1024 + 5, 4096, 4, 3),
}
GENERAL = (256, 10_007, 48, 5, 7)


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
def _file(page, file_len):
    """(arena, page table, file bytes): the file's pages scattered over an arena about twice as
    large; the pages in between, and the rest of the file's last page, hold other bytes."""
    npg = -(-file_len // page)
    rng = np.random.default_rng(3 * page + file_len)
    perm = rng.permutation(2 * npg + 3)[:npg].astype(np.int64)
    arena = _noise((2 * npg + 3) * page, file_len + 2)
    data = _noise(file_len, file_len + 3)
    for v in range(npg):
        part = data[v * page:(v + 1) * page]
        arena[perm[v] * page:perm[v] * page + part.size] = part
    return arena, perm, data


def _starts(file_len, buf, streams):
    """0, the file's last buffer, one beyond the file (it clamps to the EOF call), the rest spread
    over the file's calls."""
    calls = -(-file_len // buf)
    starts = [((5 * s + 1) % calls) * buf for s in range(streams)]
    starts[:3] = [0, (calls - 1) * buf, (calls + 3) * buf]
    return starts


def _steps(shape):
    """At least 3; enough for a stream that starts at 0 to pass the file's end twice, so that
    launch_base % cycle wraps."""
    file_len, buf, depth = shape[1], shape[2], shape[3]
    cycle = -(-file_len // buf) + 1
    return max(3, min(-(-2 * cycle // depth) + 1, 12))


@functools.lru_cache(maxsize=None)
def _model(shape):
    """Per step: (ring, bytes, eofs, positions, last calls, total, reopens)."""
    page, file_len, buf, depth, streams = shape
    data = _file(page, file_len)[2]
    stride = depth * buf + GAP
    cycle = -(-file_len // buf) + 1
    c_init = [min(o // buf, cycle - 1) for o in _starts(file_len, buf, streams)]
    ring = np.full(GUARD + streams * stride + GUARD, FILL, dtype=np.uint8)
    total = reopens = 0
    out = []
    for t in range(_steps(shape)):
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
                d = GUARD + s * stride + k * buf
                ring[d:d + ln] = data[off:off + ln]
                nbytes += ln
                last[s, k] = (off, ln)
        total += nbytes
        reopens += eofs
        pos = [min(((c_init[s] + (t + 1) * depth) % cycle) * buf, file_len) for s in range(streams)]
        out.append((ring.copy(), nbytes, eofs, pos, last, total, reopens))
    return out


def test_model_on_a_small_example():
    shape = CASES["cycle_below_depth"]                    # calls of 1024 and 476 bytes, then EOF
    assert _starts(1500, 1024, 3) == [0, 1024, 5120]      # call indexes 0, 1 and 2 (clamped)
    steps = _model(shape)
    assert len(steps) == 3
    # 8 calls from call index 0, 1, 2 of a cycle of 3: two full passes each, then calls 0 1 / 1 2 / 2 0
    assert steps[0][1:3] == ((2 * 1500 + 1500) + (2 * 1500 + 476) + (2 * 1500 + 1024), 2 + 3 + 3)
    ring, data = steps[0][0], _file(1024, 1500)[2]
    assert (ring[:GUARD] == FILL).all() and (ring[GUARD:GUARD + 1024] == data[:1024]).all()
    assert (ring[GUARD + 1024:GUARD + 1500] == data[1024:]).all()
    assert (ring[GUARD + 1500:GUARD + 2048] == FILL).all()


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


def _open(env, shape, ring_ptr, arena_ptr):
    page, file_len, buf, depth, streams = shape
    return lib().RingReadSession.remote(
        arena_base=arena_ptr + PAD, file_pages=_file(page, file_len)[1].tolist(), page_size=page,
        file_len=file_len, device=0 if env.gpu else -1, dst_base=ring_ptr + GUARD,
        stream_stride=depth * buf + GAP, buf_bytes=buf, depth=depth, streams=streams,
        dst_kind=1 if env.gpu else 0, start_offsets=_starts(file_len, buf, streams))


def _check(env, shape, launch=None):
    """`launch`: (path, U, grid) that seq_read_last_launch() must report after every step."""
    page, file_len, buf, depth, streams = shape
    want = _model(shape)
    ah, ap = env.buf(np.concatenate([_noise(PAD, 11), _file(page, file_len)[0], _noise(PAD, 12)]))
    rh, rp = env.buf(np.full(want[0][0].size, FILL, dtype=np.uint8))
    sess = _open(env, shape, rp, ap)
    try:
        for t, (ring, nbytes, eofs, pos, last, total, reopens) in enumerate(want):
            assert sess.step(env.stream()) == (nbytes, eofs), t
            if launch is not None:
                assert lib().seq_read_last_launch() == launch, t
            _same(env.host(rh), ring, f"ring after step {t}")
            assert (sess.total_bytes, sess.reopens, sess.calls) == (total, reopens, (t + 1) * depth), t
            assert [sess.position(s) for s in range(streams)] == pos, t
            for (s, k), call in last.items():
                assert sess.last_call(s, k) == call, (t, s, k)
    finally:
        sess.close()
    assert reopens >= 2                                   # the file's end was passed


def _fast_launch(shape, variant, grid_cap):
    """What the launcher must report: U from bit 1, and a grid of ceil(trips / 4 waves) workgroups,
    capped (every shape here is far below a device's resident workgroups)."""
    buf, depth, streams = shape[2:]
    unroll = 16 if variant >= 0 and variant & 2 else 8
    trips = -(-(streams * depth * (buf // 1024)) // unroll)
    return ("fast", unroll, min(-(-trips // 4), grid_cap))


@pytest.mark.parametrize("case", list(CASES))
def test_fast_shapes_cpu(case):
    _check(_Env(False), CASES[case])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=[f"v{v}" for v in VARIANTS])
@pytest.mark.parametrize("case", list(CASES))
def test_fast_shapes_gpu(gpu, case, variant):
    with _setting(variant):
        cap = lib().seq_read_variant()[1]
        _check(_Env(True), CASES[case], _fast_launch(CASES[case], variant, cap))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS, ids=[f"v{v}" for v in VARIANTS])
@pytest.mark.parametrize("cap", [1, 2])
def test_persistent_loop_ragged_rounds_gpu(gpu, cap, variant):
    """144 chunks = 18 trips of 8 (9 of 16) on 4 or 8 waves: several rounds, the last one ragged."""
    shape = CASES["ragged_rounds"]
    with _setting(variant, cap):
        launch = _fast_launch(shape, variant, cap)
        assert launch[2] == cap
        _check(_Env(True), shape, launch)


def test_general_shape_cpu():
    _check(_Env(False), GENERAL)


@pytest.mark.gpu
def test_general_shape_takes_the_general_kernel(gpu):
    with _setting(-1):
        _check(_Env(True), GENERAL)
        path, unroll, grid = lib().seq_read_last_launch()
        assert (path, unroll) == ("general", 8) and grid >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("nontemporal", [False, True], ids=["plain", "nt"])
@pytest.mark.parametrize("nbytes,grid", [(16, 0), (8192 * 5 + 48, 0), (8192 * 11 + 8176, 2)])
def test_store_fill_writes_its_range_and_nothing_else(gpu, nbytes, grid, nontemporal):
    """The store-only roof kernel of tools/store_roof.py: whole 8 KiB trips, a rest of single
    vectors, a grid that strides; the guards in front and behind stay."""
    env = _Env(True)
    h, p = env.buf(np.full(GUARD + nbytes + GUARD, FILL, dtype=np.uint8))
    used = lib().store_fill(p + GUARD, nbytes, 0x01020304, nontemporal, grid, env.stream())
    assert 1 <= used <= (grid or used)
    want = np.full(GUARD + nbytes + GUARD, FILL, dtype=np.uint8)
    want[GUARD:GUARD + nbytes] = np.tile(np.array([4, 3, 2, 1], dtype=np.uint8), nbytes // 4)
    _same(env.host(h), want, "filled buffer")
    with pytest.raises(Exception):
        lib().store_fill(p + GUARD, 24, 0, nontemporal, grid, env.stream())     # not a multiple of 16
