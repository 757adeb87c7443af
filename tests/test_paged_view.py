"""The three store entry points that read a cached file through a page table (RingReadSession,
RaggedGatherSession, delim_index_store) on one native store of host arenas: they refuse the same
block lists with the same codes, leave no read lock behind, and see the same bytes.  Runs without
a GPU: the store has no device dir, so every consumer takes its host loop."""
import numpy as np
import pytest

from alluxio_amd.ops.native import lib

PAGE = 4096
DIR_PAGES = 16
INVALID_ARGUMENT, INVALID_STATE = 6, 4
ENTRIES = ["ring", "ragged", "delim"]
D = 0x0A

# blocks of the store: id -> (tier, medium, bytes)
A0, A1, A_HALF, B0, F0 = 10, 11, 12, 20, 30
BLOCKS = {A0: (0, "DRAM", 2 * PAGE), A1: (0, "DRAM", PAGE + 100), A_HALF: (0, "DRAM", PAGE + PAGE // 2),
          B0: (0, "DRAM2", PAGE), F0: (1, "SSD", PAGE)}


def _text(n, seed):
    t = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    t[t == D] = 0x20
    t[np.random.default_rng(seed + 1).integers(0, n, max(1, n // 50))] = D
    return t


def _put(s, bid, tier, medium, data):
    s.create_block(1, bid, tier=tier, medium=medium, initial=data.nbytes)
    s.write(1, bid, 0, data.ctypes.data, data.nbytes, 0)
    s.commit_block(1, bid)


@pytest.fixture
def store(tmp_path):
    """Two host memory dirs of 4 KiB pages and one file dir.  Fillers come first and A1 is written
    before A0, so the pages of the file (A0, A1) neither start the arena nor ascend."""
    C = lib()
    specs, keep = [], []
    for medium in ("DRAM", "DRAM2"):
        arena = np.zeros(DIR_PAGES * PAGE, dtype=np.uint8)
        keep.append(arena)
        d = C.DirSpec()
        d.tier, d.tier_alias, d.medium, d.kind = 0, "MEM", medium, C.DirKind.HOST
        d.base, d.capacity, d.page_size = arena.ctypes.data, arena.nbytes, PAGE
        specs.append(d)
    f = C.DirSpec()
    f.tier, f.tier_alias, f.medium, f.kind = 1, "SSD", "SSD", C.DirKind.FILE
    f.path, f.capacity = str(tmp_path / "ssd"), 1 << 20
    specs.append(f)
    s = C.BlockStore(specs, annotator=0, alloc_policy=0, device=0)
    s._keep = keep
    s.data = {bid: _text(n, bid) for bid, (_, _, n) in BLOCKS.items()}
    for k in range(5):                                  # pages 0..4 of the first dir
        _put(s, 100 + k, 0, "DRAM", np.zeros(PAGE, dtype=np.uint8))
    s.remove_block(1, 101)
    s.remove_block(1, 103)
    for bid in (A1, A0, A_HALF, B0, F0):
        _put(s, bid, *BLOCKS[bid][:2], s.data[bid])
    return s


def _len(bid):
    return BLOCKS[bid][2]


def _call(s, entry, ids, lens):
    """Opens (and closes) the entry point over one file; returns what it read: the bytes of the
    file as the consumer sees them, or the cuts."""
    C = lib()
    n = max(1, sum(lens))
    if entry == "ring":
        ring = np.zeros(n, dtype=np.uint8)
        r = C.RingReadSession(s, 7, ids, lens, ring.ctypes.data, n, n, 1, 1, 0)
        try:
            got, eofs = r.step()
            assert (got, eofs) == (n, 0) and r.last_call(0, 0) == (0, n)
        finally:
            r.close()
        return ring
    if entry == "ragged":
        offs = np.array([0, 1, PAGE - 1, PAGE + 7, n], dtype=np.uint64)
        g = C.RaggedGatherSession(s, 7, [(ids, lens)], [offs])
        try:
            dst = np.zeros(n, dtype=np.uint8)
            out_off, out_len = np.zeros(offs.size, dtype=np.uint64), np.zeros(offs.size - 1, dtype=np.uint32)
            total, data = g.gather(np.arange(offs.size - 1), dst.ctypes.data, dst.nbytes, out_off.ctypes.data,
                                   out_len.ctypes.data, align=1, dst_kind=0)
            assert (total, data) == (n, n) and np.array_equal(out_off, offs)
        finally:
            g.close()
        return dst
    return C.delim_index_store(s, 7, ids, lens, D)


def _assert_unlocked(s, ids):
    for bid in set(ids):
        lk = s.lock_block(8, bid, True, 0)              # -1: somebody still holds a lock
        assert lk > 0, f"block {bid} is still locked"
        s.unlock(lk)


REFUSALS = {
    "sizes_differ": ([A0, A1], [2 * PAGE], INVALID_ARGUMENT),
    "file_tier": ([A0, F0], [2 * PAGE, PAGE], INVALID_ARGUMENT),
    "two_dirs": ([A0, B0], [2 * PAGE, PAGE], INVALID_ARGUMENT),
    "first_block_ends_mid_page": ([A_HALF, A1], [PAGE + PAGE // 2, PAGE + 100], INVALID_ARGUMENT),
    "length_past_the_block": ([A0, A1], [2 * PAGE, 3 * PAGE], INVALID_STATE),
}


@pytest.mark.parametrize("case", list(REFUSALS))
@pytest.mark.parametrize("entry", ENTRIES)
def test_refusal_and_lock_release(store, entry, case):
    ids, lens, code = REFUSALS[case]
    before = lib().delim_index_launches()
    with pytest.raises(lib().StoreError) as e:
        _call(store, entry, ids, lens)
    assert e.value.args[0] == code, e.value.args
    if entry == "delim":
        assert lib().delim_index_launches() == before
    _assert_unlocked(store, ids)


@pytest.mark.parametrize("entry", ENTRIES)
def test_success_sees_the_file_and_releases_its_locks(store, entry):
    ids, lens = [A0, A1], [_len(A0), _len(A1)]
    pages = [p for bid in ids for p in store.block_pages(bid)[0]]
    assert len(pages) == 4 and pages != sorted(pages) and min(pages) > 0, pages
    assert _len(A1) % PAGE != 0
    want = np.concatenate([store.data[A0], store.data[A1]])
    got = _call(store, entry, ids, lens)
    if entry == "delim":
        cuts = (np.flatnonzero(want == D) + 1).astype(np.uint64)
        assert cuts.size > 10 and np.array_equal(got, cuts)
    else:
        assert np.array_equal(got, want)
    _assert_unlocked(store, ids)
