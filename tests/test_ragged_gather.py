"""RaggedGatherSession through its raw-arena constructor: a 64-page arena behind a scrambled page
table, every record compared byte for byte with numpy slices of the same (virtual) bytes.  The
same cases run over a numpy arena (host loop) and over a device tensor (plan + copy kernels,
both inner-loop variants)."""
import numpy as np
import pytest

from alluxio_amd.ops.native import lib

PAGE = 4096
NPAGES = 64
GUARD = 64
F1_PAGES = 40
F1_LEN = (F1_PAGES - 1) * PAGE + 1000          # the first file ends inside its last page
F2_BASE = F1_PAGES * PAGE                      # the second file starts on a fresh virtual page
F2_LEN = (NPAGES - F1_PAGES) * PAGE            # ... and ends with the last byte of the page table
LENS = [0, 1, 3, 15, 16, 17, 31, 33, 4095, 4096, 4097, 3 * 4096 + 5]


def _page_table():
    for seed in range(100):
        perm = np.random.default_rng(seed).permutation(NPAGES).astype(np.int64)
        if not (np.abs(np.diff(perm)) == 1).any():
            return perm
    raise AssertionError("no scrambled page table found")


PERM = _page_table()
VIRT = np.random.default_rng(5).integers(0, 256, NPAGES * PAGE, dtype=np.uint8)   # bytes by virtual address
ARENA = np.empty_like(VIRT)
for _v in range(NPAGES):
    ARENA[PERM[_v] * PAGE:(PERM[_v] + 1) * PAGE] = VIRT[_v * PAGE:(_v + 1) * PAGE]


def _records():
    """(starts, lengths, named groups of record numbers)."""
    recs, groups = [], {}

    def add(name, start, length):
        groups.setdefault(name, []).append(len(recs))
        recs.append((start, length))

    for i, n in enumerate(LENS):                       # every length at every source phase, near a page end
        for ph in range(16):
            add("lens", 2 * PAGE - 64 + 16 * i + ph, n)
    for a in range(1, 16):                             # straddle a page boundary by a bytes before, b after
        for b in range(1, 16):
            add("straddle", 5 * PAGE - a, a + b)
    add("page_end", 7 * PAGE - 100, 100)
    add("four_pages", 9 * PAGE + 4090, 3 * PAGE + 5)
    add("eof", F1_LEN - 777, 777)                      # ends at the first file's last byte
    add("eof", F2_BASE, 5000)                          # the second file's first bytes
    add("eof", F2_BASE + F2_LEN - 4099, 4099)          # ends at the last byte of the page table
    for ph in range(16):
        add("r33", 12 * PAGE - 40 + ph, 33)
    for k in range(17):
        add("tiny", 20000 + 21 * k, k)
    for k in range(6):
        add("zero", 30000 + 7 * k, 0)
    add("long", 3 * PAGE + 7, 2500)
    starts = np.array([s for s, _ in recs], dtype=np.uint64)
    lens = np.array([n for _, n in recs], dtype=np.uint32)
    for s, n in recs:
        assert s + n <= F1_LEN or (s >= F2_BASE and s + n <= F2_BASE + F2_LEN)
    return starts, lens, groups


STARTS, RLENS, GROUPS = _records()
N = len(STARTS)
_ENV = {}


class _Env:
    def __init__(self, mode):
        self.mode = mode
        self.gpu = mode != "cpu"
        if self.gpu:
            import torch
            self.torch = torch
            self.arena = torch.from_numpy(ARENA).cuda()
            base, dev = self.arena.data_ptr(), 0
        else:
            self.arena = ARENA.copy()
            base, dev = self.arena.ctypes.data, -1
        self.sess = lib().RaggedGatherSession.raw(base, PERM.tolist(), PAGE, dev, STARTS, RLENS)

    def alloc(self, n, dtype, fill):
        if self.gpu:
            t = {np.uint8: self.torch.uint8, np.uint64: self.torch.int64, np.uint32: self.torch.int32}[dtype]
            x = self.torch.full((n,), fill, dtype=t, device="cuda")
            return x, x.data_ptr()
        x = np.full(n, fill, dtype=dtype)
        return x, x.ctypes.data

    def host(self, x, dtype):
        if self.gpu:
            self.torch.cuda.synchronize()
            return x.cpu().numpy().view(dtype)
        return x

    def gather(self, idx, dst, cap, off, ln, **kw):
        stream = int(self.torch.cuda.current_stream().cuda_stream) if self.gpu else 0
        return self.sess.gather(np.asarray(idx, dtype=np.int64), dst, cap, off, ln, dst_kind=1 if self.gpu else 0,
                                stream=stream, **kw)


@pytest.fixture(params=["cpu", pytest.param("gpu", marks=pytest.mark.gpu),
                        pytest.param("gpu_funnel", marks=pytest.mark.gpu)])
def env(request):
    mode = request.param
    if mode != "cpu":
        request.getfixturevalue("gpu")
        lib().set_ragged_gather_variant(1 if mode == "gpu_funnel" else 0)
    if mode not in _ENV:
        _ENV[mode] = _Env(mode)
    yield _ENV[mode]
    if mode != "cpu":
        lib().set_ragged_gather_variant(0)


def _expect(idx, layout, align=16, max_len=0, stride=0, pad=0):
    idx = np.asarray(idx, dtype=np.int64)
    lens = RLENS[idx].astype(np.int64)
    if layout == "packed":
        adv = (lens + align - 1) // align * align
        off = np.concatenate([[0], np.cumsum(adv)]).astype(np.uint64)
        data = np.zeros(int(off[-1]), dtype=np.uint8)
    else:
        lens = np.minimum(lens, max_len)
        off = (np.arange(len(idx) + 1) * stride).astype(np.uint64)
        data = np.full(len(idx) * stride, pad, dtype=np.uint8)
    for r, i in enumerate(idx):
        s, o, n = int(STARTS[i]), int(off[r]), int(lens[r])
        data[o:o + n] = VIRT[s:s + n]
    return data, off, lens.astype(np.uint32)


def _run(env, idx, layout="packed", align=16, max_len=0, stride=0, pad=0):
    want, woff, wlen = _expect(idx, layout, align, max_len, stride, pad)
    nb = len(idx)
    cap = len(want)
    buf, bptr = env.alloc(GUARD + cap + GUARD, np.uint8, 0xA5)
    off, optr = env.alloc(nb + 1, np.uint64, 0)
    ln, lptr = env.alloc(max(nb, 1), np.uint32, 0)
    total, data_bytes = env.gather(idx, bptr + GUARD, cap, optr, lptr, layout=layout, align=align,
                                   row_stride=stride, max_len=max_len, pad_value=pad)
    got = env.host(buf, np.uint8)
    assert (got[:GUARD] == 0xA5).all() and (got[GUARD + cap:] == 0xA5).all(), "guard bytes overwritten"
    goff, glen = env.host(off, np.uint64), env.host(ln, np.uint32)[:nb]
    assert np.array_equal(goff, woff) and np.array_equal(glen, wlen)
    assert total == cap and int(goff[-1]) == cap and data_bytes == int(wlen.sum())
    bad = np.nonzero(got[GUARD:GUARD + cap] != want)[0]
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:4]}"
    return woff


def test_page_table_is_scrambled():
    assert not (np.abs(np.diff(PERM)) == 1).any()
    assert F1_LEN % PAGE != 0 and F2_BASE % PAGE == 0 and F2_BASE > F1_LEN


def test_record_lengths_and_source_phases(env):
    idx = GROUPS["lens"]
    assert {int(STARTS[i]) % 16 for i in idx} == set(range(16))
    assert sorted({int(RLENS[i]) for i in idx}) == LENS
    _run(env, idx)
    _run(env, idx, align=1)


def test_page_edges_long_records_and_end_of_file(env):
    idx = GROUPS["straddle"] + GROUPS["page_end"] + GROUPS["four_pages"] + GROUPS["eof"]
    i4 = GROUPS["four_pages"][0]
    assert (int(STARTS[i4]) + int(RLENS[i4]) - 1) // PAGE - int(STARTS[i4]) // PAGE == 3
    ie = GROUPS["page_end"][0]
    assert (int(STARTS[ie]) + int(RLENS[ie])) % PAGE == 0
    ends = [int(STARTS[i]) + int(RLENS[i]) for i in GROUPS["eof"]]
    assert F1_LEN in ends and F2_BASE + F2_LEN in ends
    _run(env, idx, align=1)
    _run(env, idx, align=16)


def test_all_phase_pairs(env):
    idx = [i for i in GROUPS["r33"] for _ in range(16)]     # 16 rows per source phase
    off = _run(env, idx, align=1)
    pairs = {(int(STARTS[i]) % 16, int(o) % 16) for i, o in zip(idx, off[:-1])}
    assert len(pairs) == 256


@pytest.mark.parametrize("align", [1, 2, 16, 256])
def test_packed_alignments(env, align):
    idx = GROUPS["lens"][::5] + GROUPS["straddle"][::17] + GROUPS["long"] + GROUPS["zero"][:2]
    off = _run(env, idx, align=align)
    assert all(int(o) % align == 0 for o in off)


def test_padded_with_truncation(env):
    idx = GROUPS["lens"][::3] + GROUPS["four_pages"] + GROUPS["zero"][:1] + GROUPS["long"]
    assert max(int(RLENS[i]) for i in idx) > 1000
    _run(env, idx, layout="padded", max_len=1000, stride=1000, pad=0x7F)


def test_padded_without_truncation(env):
    idx = GROUPS["lens"][::3] + GROUPS["four_pages"] + GROUPS["eof"]
    longest = max(int(RLENS[i]) for i in idx)
    _run(env, idx, layout="padded", max_len=longest, stride=longest, pad=0x11)


def test_batch_sizes(env):
    _run(env, GROUPS["four_pages"])                               # B = 1
    rng = np.random.default_rng(9)
    _run(env, rng.integers(0, N, 257))                            # B = 257, any record
    tiny = np.array(GROUPS["tiny"])
    assert int(RLENS[tiny].max()) <= 16
    _run(env, tiny[rng.integers(0, len(tiny), 5000)], align=1)    # the plan's scan carries across rounds
    _run(env, tiny[rng.integers(0, len(tiny), 5000)], align=16)
    _run(env, GROUPS["zero"] * 3)                                 # only zero-length records
    _run(env, GROUPS["zero"] * 3, layout="padded", max_len=8, stride=8, pad=3)
    _run(env, [N - 1, N - 1, 40, 40, 7, 3, 3, 0])                 # repeated and descending


def test_empty_batch(env):
    _run(env, [])


@pytest.mark.parametrize("case", ["index_n", "index_neg", "too_many", "align_3", "capacity_short"])
def test_rejected_arguments(env, case):
    idx = list(GROUPS["lens"][:40])
    kw = dict(layout="packed", align=16)
    want, _, _ = _expect(idx, "packed", 16)
    cap = len(want)
    if case == "index_n":
        idx[7] = N
    elif case == "index_neg":
        idx[7] = -1
    elif case == "too_many":
        idx = [GROUPS["zero"][0]] * (lib().RaggedGatherSession.max_batch + 1)
    elif case == "align_3":
        kw["align"] = 3
    elif case == "capacity_short":
        cap -= 1
    buf, bptr = env.alloc(GUARD + len(want) + GUARD, np.uint8, 0xA5)
    off, optr = env.alloc(len(idx) + 1, np.uint64, 0)
    ln, lptr = env.alloc(len(idx), np.uint32, 0)
    before = env.sess.gathers
    with pytest.raises(lib().StoreError):
        env.gather(idx, bptr + GUARD, cap, optr, lptr, **kw)
    assert env.sess.gathers == before                             # nothing was launched
    assert (env.host(buf, np.uint8) == 0xA5).all()
    assert not env.host(off, np.uint64).any()
