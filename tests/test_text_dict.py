"""text_dict_*_raw and TextDictionary: first-occurrence codes of text values against a dictionary that
persists across calls.  The yardstick everywhere is the Python loop

    codes = [d.setdefault(v, len(d)) for v in values]        # d persists across calls

over the live values in row order, compared exactly, together with the dictionary's entries in code
order (``list(d)``).

Ids: `cpu` runs the host loops (device=-1); `gpu-v0` (one lane per value) and `gpu-v1` (sixteen
lanes per value) run the kernels.  In the raw tests the data is a slice in the middle of a larger
tensor of plausible bytes, at an odd phase, so a read outside a value changes a result instead of
going unseen, and the slot, first and code outputs sit between guard elements that are filled
before the calls and checked after them."""
import numpy as np
import pytest
import torch

from alluxio_amd.models import RaggedBatch, TextDictionary
from alluxio_amd.ops.native import lib

PAD = 4099          # bytes before the slice: an odd phase
GUARD = 5           # int32 elements on either side of slot_of, first, first_len and codes
MARK = 0x5A5A5A5A   # the outputs and their guards before the call
ECAP, BCAP = 8192, 1 << 20                                      # entry storage of the raw driver: fixed

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 513, 4099]
COUNTS = [0, 1, 15, 16, 17, 255, 256, 257, 4096]


def yardstick(d: dict, values, live=None):
    return [d.setdefault(v, len(d)) if live is None or live[r] else -1 for r, v in enumerate(values)]


class _Env:
    def __init__(self, mode):
        self.gpu = mode != "cpu"
        self.device = torch.device("cuda", 0) if self.gpu else torch.device("cpu")
        self.devno = 0 if self.gpu else -1

    def sync(self):
        if self.gpu:
            torch.cuda.synchronize()

    def batch(self, values) -> RaggedBatch:
        """A packed batch of the values on the device, its data at an odd phase inside a larger tensor."""
        lens = np.array([len(v) for v in values], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        data = b"".join(values)
        big = np.resize(np.frombuffer(b"abc\0a", dtype=np.uint8), PAD + len(data) + PAD)
        big[PAD:PAD + len(data)] = np.frombuffer(data, dtype=np.uint8)
        flat = torch.from_numpy(big).to(self.device)[PAD:PAD + len(data)]
        return RaggedBatch(flat, torch.from_numpy(offs).to(self.device), torch.from_numpy(lens).to(self.device))

    def dictionary(self, capacity=1024) -> TextDictionary:
        return TextDictionary(self.device, capacity=capacity)


class _Raw:
    """The passes of one encode or lookup through the raw functions, with the state in tensors of
    this object, guards around every per-row output and the data at an odd phase."""

    def __init__(self, env, capacity=1024):
        self.env, dev = env, env.device
        self.table = torch.full((capacity,), -1, dtype=torch.int64, device=dev)
        self.ent_hash = torch.zeros(ECAP, dtype=torch.int64, device=dev)
        self.ent_off = torch.zeros(ECAP + 1, dtype=torch.int64, device=dev)
        self.ent_data = torch.full((BCAP,), 0xEE, dtype=torch.uint8, device=dev)
        self.D = self.nbytes = 0

    def grow(self, capacity):
        self.table = torch.full((capacity,), -1, dtype=torch.int64, device=self.env.device)
        lib().text_dict_rehash_raw(self.ent_hash.data_ptr(), self.D, self.table.data_ptr(), capacity, self.env.devno)

    def _guarded(self, n):
        return torch.full((GUARD + n + GUARD,), MARK, dtype=torch.int32, device=self.env.device)

    def _inner(self, t, n):
        self.env.sync()
        h = t.cpu().numpy()
        assert (h[:GUARD] == MARK).all() and (h[GUARD + n:] == MARK).all(), "a guard element was written"
        return h[GUARD:GUARD + n]

    def run(self, data: bytes, start, length, status=None, insert=True):
        """Returns (codes, first) as lists; the dictionary grows when insert is set."""
        C, env, dev, no = lib(), self.env, self.env.device, self.env.devno
        n = len(start)
        big = np.resize(np.frombuffer(b"abc\0a", dtype=np.uint8), PAD + len(data) + PAD)
        big[PAD:PAD + len(data)] = np.frombuffer(data, dtype=np.uint8)
        d_data = torch.from_numpy(big).to(dev)
        d_start = torch.from_numpy(np.ascontiguousarray(start, dtype=np.int64)).to(dev)
        d_len = torch.from_numpy(np.ascontiguousarray(length, dtype=np.int32)).to(dev)
        d_status = None if status is None else torch.from_numpy(np.ascontiguousarray(status, dtype=np.uint8)).to(dev)
        sp = 0 if d_status is None else d_status.data_ptr()
        slot_of, first, first_len, codes = (self._guarded(n) for _ in range(4))
        g = 4 * GUARD
        hashes = torch.zeros(n, dtype=torch.int64, device=dev)
        cap, table = self.table.numel(), self.table.data_ptr()
        C.text_dict_probe_raw(d_data.data_ptr() + PAD, len(data), d_start.data_ptr(), d_len.data_ptr(), sp, n, no,
                              self.ent_data.data_ptr(), self.nbytes, self.ent_off.data_ptr(), self.D, table, cap, insert,
                              slot_of.data_ptr() + g, hashes.data_ptr())
        rank_ptr, h_first = 0, [0] * n
        if insert:
            C.text_dict_first_raw(table, cap, slot_of.data_ptr() + g, d_len.data_ptr(), n, no, first.data_ptr() + g,
                                  first_len.data_ptr() + g)
            h_first = self._inner(first, n).tolist()
            h_flen = self._inner(first_len, n)
            rank = torch.from_numpy(np.cumsum(h_first, dtype=np.int64)).to(dev)
            byte_off = torch.from_numpy(np.concatenate([[0], np.cumsum(h_flen, dtype=np.int64)])).to(dev)
            rank_ptr = rank.data_ptr()
        C.text_dict_codes_raw(table, cap, slot_of.data_ptr() + g, rank_ptr, n, self.D, no, codes.data_ptr() + g)
        if insert and n:
            new, nb = int(sum(h_first)), int(h_flen.sum())
            assert self.D + new <= ECAP and self.nbytes + nb <= BCAP
            C.text_dict_commit_raw(table, cap, slot_of.data_ptr() + g, hashes.data_ptr(), first.data_ptr() + g,
                                   rank.data_ptr(), byte_off.data_ptr(), n, self.D, self.ent_hash.data_ptr(),
                                   self.ent_off.data_ptr(), ECAP, self.nbytes, no)
            C.text_emit_raw(d_data.data_ptr() + PAD, len(data), d_start.data_ptr(), d_len.data_ptr(), sp, n, no, -1,
                            byte_off.data_ptr(), self.ent_data.data_ptr() + self.nbytes, nb)
            self.D, self.nbytes = self.D + new, self.nbytes + nb
        out = self._inner(codes, n).tolist()
        self._inner(slot_of, n)
        return out, h_first

    def encode(self, values, insert=True):
        data = b"".join(values)
        start = np.concatenate([[0], np.cumsum([len(v) for v in values])[:-1]]) if values else []
        return self.run(data, start, [len(v) for v in values], None, insert)

    def entries(self):
        self.env.sync()
        cuts = self.ent_off[:self.D + 1].cpu().tolist()
        text = self.ent_data[:self.nbytes].cpu().numpy().tobytes()
        return [text[cuts[c]:cuts[c + 1]] for c in range(self.D)]

    def check(self, ref: dict, values):
        """One encode of the values against the yardstick dictionary `ref`, which it updates."""
        before = len(ref)
        want = yardstick(ref, values)
        seen, want_first = set(range(before)), []
        for c in want:
            want_first.append(0 if c in seen else 1)
            seen.add(c)
        codes, first = self.encode(values)
        assert codes == want
        assert first == want_first
        assert self.entries() == list(ref)


@pytest.fixture(params=[pytest.param(("cpu", 0), id="cpu"),
                        pytest.param(("gpu", 0), marks=pytest.mark.gpu, id="gpu-v0"),
                        pytest.param(("gpu", 1), marks=pytest.mark.gpu, id="gpu-v1")])
def env(request):
    mode, variant = request.param
    if mode == "cpu":
        yield _Env(mode)
        return
    request.getfixturevalue("gpu")
    default = lib().text_dict_variant()
    lib().set_text_dict_variant(variant)
    assert lib().text_dict_variant() == variant
    yield _Env(mode)
    lib().set_text_dict_variant(default)


def _letters(n, seed=0):
    return bytes(0x61 + (i * 7 + seed) % 23 for i in range(n))


def _flip(v: bytes, i: int) -> bytes:
    return v[:i] + bytes([v[i] ^ 0x20]) + v[i + 1:]


# ---- cases ---------------------------------------------------------------------------------------
def test_lengths_and_values_that_differ_in_one_byte(env):
    values = []
    for n in LENGTHS:
        v = _letters(n, n)
        values.append(v)
        for i in (n - 1, 15, 16, 255, 256):             # the last byte, and either side of a vector and a step edge
            if 0 <= i < n:
                values.append(_flip(v, i))
    assert len(set(values)) > 3 * len(LENGTHS)
    rng = np.random.default_rng(2)
    rows = values + [values[i] for i in rng.permutation(len(values))]    # every value a second time
    raw, ref = _Raw(env), {}
    raw.check(ref, rows)
    assert len(ref) == len(set(values))
    raw.grow(4096)                                      # a larger table, filled from the stored hashes
    raw.check(ref, rows[::-1])                          # nothing new: every code is a committed one
    assert len(ref) == len(set(values))


def test_prefix_chains_and_zero_padding(env):
    chain = [b"a" * k for k in list(range(0, 41)) + [255, 256, 257, 258]]
    traps = [b"", b"\0", b"\0\0", b"a", b"a\0", b"a\0\0", b"\0a", b"a" * 8, b"a" * 8 + b"\0", b"a" * 16 + b"\0",
             b"\0" * 7, b"\0" * 8, b"\0" * 9, b"\0" * 16, b"\0" * 17]
    assert len(set(traps)) == len(traps)
    raw, ref = _Raw(env), {}
    raw.check(ref, traps + chain + traps[::-1] + chain[::-1])
    assert len(ref) == len(set(traps + chain))


@pytest.mark.parametrize("mix", ["one", "two", "distinct"])
def test_row_counts(env, mix):
    for n in COUNTS:
        if mix == "one":                                # the most contention on one slot
            values = [b"the same value"] * n
        elif mix == "two":
            values = [(b"left", b"right, and longer than sixteen bytes")[r & 1] for r in range(n)]
        else:
            values = [b"v%d" % (r * 7919 % 100003) for r in range(n)]
        raw, ref = _Raw(env, capacity=max(2, 1 << (2 * n).bit_length())), {}
        raw.check(ref, values)
        assert len(ref) == {"one": min(n, 1), "two": min(n, 2), "distinct": n}[mix]


@pytest.mark.parametrize("bits", [0, 2])
def test_forced_collisions(env, bits):
    C = lib()
    assert C.text_dict_hash_bits() == 64
    distinct = [b"key-%d" % i + b"x" * (i % 40) for i in range(300)]
    rng = np.random.default_rng(bits)
    rows = distinct + [distinct[i] for i in rng.integers(0, 300, 400)]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    C.set_text_dict_hash_bits(bits)
    try:
        assert C.text_dict_hash_bits() == bits
        raw, ref = _Raw(env, capacity=2048), {}
        raw.check(ref, rows)                            # every value walks one chain (four with two bits)
        raw.grow(4096)
        raw.check(ref, rows[:100] + [b"new-%d" % i for i in range(20)])
        assert len(ref) == 320
        codes, _ = raw.encode(distinct + [b"unknown"], insert=False)
        assert codes == [ref[v] for v in distinct] + [-1]
    finally:
        C.set_text_dict_hash_bits(64)
    assert C.text_dict_hash_bits() == 64


def test_three_batches_into_a_small_dictionary(env):
    d, ref = env.dictionary(capacity=8), {}
    assert d.capacity == 8 and d.size == 0 and d.tolist() == []
    caps = [d.capacity]
    for b in range(3):
        distinct = [b"item %d" % i + b"." * (i % 19) for i in range(25 * b, 25 * b + 50)]    # half overlap the batch before
        rng = np.random.default_rng(b)
        rows = [distinct[i] for i in rng.integers(0, 50, 10)] + distinct
        size, old = d.size, set(ref)
        want = yardstick(ref, rows)
        codes = d.encode(env.batch(rows)).cpu().tolist()
        assert codes == want
        assert d.size == len(ref) == size + (50 if b == 0 else 25)
        assert min(c for c, v in zip(codes, rows) if v not in old) == size                   # new ones continue from size
        caps.append(d.capacity)
        assert d.capacity >= 2 * d.size
    assert caps == [8, 128, 256, 512]                   # two rehashes of a dictionary that holds entries
    entries = d.tolist()
    assert entries == list(ref)
    vals = d.values
    assert vals.offsets.cpu().tolist()[-1] == sum(len(v) for v in ref) and vals.lengths.cpu().tolist() == [len(v) for v in ref]
    again = d.encode(env.batch(list(ref))).cpu().tolist()                                    # old values keep their codes
    assert again == list(range(len(ref))) and all(entries[c] == v for c, v in zip(again, ref))


def test_lookup_adds_nothing(env):
    d = env.dictionary(capacity=64)
    known = [b"red", b"green", b"", b"blue" * 70]
    assert d.encode(env.batch(known + known)).cpu().tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    env.sync()
    table, size, cap = d._table.cpu().numpy().tobytes(), d.size, d.capacity
    rows = [b"blue" * 70, b"blue" * 69, b"yellow", b"", b"red", b"re", b"redd", b"green"]
    assert d.lookup(env.batch(rows)).cpu().tolist() == [3, -1, -1, 2, 0, -1, -1, 1]
    assert d.lookup(env.batch(rows), status=[0, 0, 0, 1, 2, 0, 0, 0]).cpu().tolist() == [3, -1, -1, -1, -1, -1, -1, 1]
    assert d.lookup(env.batch([])).cpu().tolist() == []
    env.sync()
    assert d._table.cpu().numpy().tobytes() == table and d.size == size and d.capacity == cap and d.tolist() == known
    big = [b"w%d" % i for i in range(5000)]             # more rows than the table has slots: still nothing added
    assert d.lookup(env.batch(big)).cpu().tolist() == [-1] * 5000 and d.capacity == cap
    raw, ref = _Raw(env), {}                            # the raw lookup, with its guards
    raw.check(ref, known)
    codes, first = raw.encode(rows, insert=False)
    assert codes == [3, -1, -1, 2, 0, -1, -1, 1] and raw.D == 4 and raw.entries() == known


def test_from_values_round_trip(env):
    vocab = [b"", b"a", b"a\0", b"b" * 300, b"label-7", b"\xff\xfe"]
    d = TextDictionary.from_values(vocab, env.device)
    assert d.size == len(vocab) and d.tolist() == vocab
    assert d.lookup(env.batch(vocab[::-1] + [b"nope"])).cpu().tolist() == [5, 4, 3, 2, 1, 0, -1]
    saved = d.tolist()
    e = TextDictionary.from_values(saved, env.device)
    assert e.tolist() == saved and e.encode(env.batch([b"new", b"a"])).cpu().tolist() == [6, 1]
    with pytest.raises(ValueError):
        TextDictionary.from_values([b"x", b"x"], env.device)
    assert TextDictionary.from_values([], env.device).tolist() == []


def test_values_that_are_not_live(env):
    vals = [b"keep", b"zzzz", b"zzzz", b"zzzz", b"zzzz", b"keep", b"zzzz", b"other", b"zzzz"]
    data = b"".join(vals)
    start = np.concatenate([[0], np.cumsum([len(v) for v in vals])[:-1]]).astype(np.int64)
    length = np.array([len(v) for v in vals], dtype=np.int32)
    status = np.zeros(len(vals), np.uint8)
    status[1], status[2] = 1, 2
    start[3] = -1
    length[4] = -1
    start[8] = len(data) - 3                            # start + length = data_bytes + 1: outside the data
    raw = _Raw(env)
    codes, first = raw.run(data, start, length, status)
    assert codes == [0, -1, -1, -1, -1, 0, 1, 2, -1] and first == [1, 0, 0, 0, 0, 0, 1, 1, 0]
    assert raw.entries() == [b"keep", b"zzzz", b"other"]
    start[1], length[2] = 2 ** 62, 2 ** 31 - 1          # far outside, without a status array
    codes, _ = raw.run(data, start, length, None)
    assert codes == [0, -1, -1, -1, -1, 0, 1, 2, -1] and raw.D == 3
    start[8] = len(data) - 4                            # the value that ends with the data is live
    assert raw.run(data, start, length, None)[0][8] == 1
    d = env.dictionary()                                # and through the class
    got = d.encode(env.batch([b"a", b"b", b"a", b""]), status=[0, 3, 0, 0]).cpu().tolist()
    assert got == [0, -1, 0, 1] and d.tolist() == [b"a", b""]


def _mixed_values(n, seed):
    rng = np.random.default_rng(seed)
    pool = [b"k%d" % i + b"-" * int(k) for i, k in enumerate(rng.integers(0, 30, 400))]
    pool += [_letters(int(k), i) for i, k in enumerate(rng.integers(200, 700, 30))]
    return [pool[i] for i in rng.integers(0, len(pool), n)]


def test_two_runs_and_all_variants_agree(env):
    rows = _mixed_values(3000, 8)
    ref = {}
    want = yardstick(ref, rows)
    a, b = env.dictionary(capacity=16), env.dictionary(capacity=4096)     # the capacity does not show
    ca, cb = a.encode(env.batch(rows)), b.encode(env.batch(rows))
    assert ca.cpu().tolist() == cb.cpu().tolist() == want
    assert a.tolist() == b.tolist() == list(ref)
    va, vb = a.values, b.values
    assert torch.equal(va.data, vb.data) and torch.equal(va.offsets, vb.offsets)
    host = TextDictionary("cpu")                        # the host loops give the same
    cpu = _Env("cpu")
    assert host.encode(cpu.batch(rows)).tolist() == want and host.tolist() == a.tolist()
    if env.gpu:                                         # and so does the other kernel variant
        C = lib()
        mine = C.text_dict_variant()
        C.set_text_dict_variant(1 - mine)
        try:
            o = env.dictionary()
            assert o.encode(env.batch(rows)).cpu().tolist() == want and o.tolist() == a.tolist()
            assert o.lookup(env.batch(rows[:500])).cpu().tolist() == want[:500]
        finally:
            C.set_text_dict_variant(mine)
        assert a.lookup(env.batch(rows[:500])).cpu().tolist() == want[:500]      # entries of one variant, probe of the other


def test_argument_errors_and_empty_calls(env):
    C, no = lib(), env.devno
    before = C.text_dict_launches()
    p = np.zeros(64, np.int64).ctypes.data              # any non-null address: a rejected call touches nothing

    def probe(data=p, nbytes=4, start=p, length=p, n=1, D=0, table=p, cap=8, insert=True, slot_of=p, hashes=p):
        C.text_dict_probe_raw(data, nbytes, start, length, 0, n, no, p, 0, p, D, table, cap, insert, slot_of, hashes)

    bad = [dict(cap=1), dict(n=5, cap=8), dict(n=2, D=3, cap=8), dict(D=5, cap=8, insert=False),   # undersized tables
           dict(cap=12), dict(cap=0), dict(cap=1 << 32),                                            # not a power of two / too large
           dict(n=(1 << 30) + 1, cap=1 << 31), dict(D=1 << 31, cap=1 << 31, insert=False),          # counts out of range
           dict(data=0), dict(start=0), dict(length=0), dict(table=0), dict(slot_of=0), dict(hashes=0)]
    for kw in bad:
        with pytest.raises(C.StoreError) as e:
            probe(**kw)
        assert e.value.args[0] == 6, kw                 # the store's invalid-argument code
    others = [lambda: C.text_dict_first_raw(p, 12, p, p, 1, no, p, p), lambda: C.text_dict_first_raw(0, 8, p, p, 1, no, p, p),
              lambda: C.text_dict_first_raw(p, 8, p, p, 1, no, 0, p), lambda: C.text_dict_first_raw(p, 8, p, p, 1, no, p, 0),
              lambda: C.text_dict_codes_raw(p, 8, 0, 0, 1, 0, no, p), lambda: C.text_dict_codes_raw(p, 8, p, 0, 1, 0, no, 0),
              lambda: C.text_dict_codes_raw(p, 7, p, 0, 1, 0, no, p),
              lambda: C.text_dict_commit_raw(p, 8, p, p, p, 0, p, 1, 0, p, p, 4, 0, no),
              lambda: C.text_dict_commit_raw(p, 8, p, p, p, p, p, 1, 0, 0, p, 4, 0, no),
              lambda: C.text_dict_commit_raw(p, 9, p, p, p, p, p, 1, 0, p, p, 4, 0, no),
              lambda: C.text_dict_rehash_raw(p, 5, p, 8, no), lambda: C.text_dict_rehash_raw(0, 2, p, 8, no),
              lambda: C.text_dict_rehash_raw(p, 2, p, 6, no),
              lambda: C.text_emit_raw(p, 4, p, p, 0, 1, no, 256, p, p, 8)]                           # the append pass: its quote
    for call in others:
        with pytest.raises(C.StoreError) as e:
            call()
        assert e.value.args[0] == 6
    for bits in (-1, 65):
        with pytest.raises(C.StoreError):
            C.set_text_dict_hash_bits(bits)
    assert C.text_dict_hash_bits() == 64
    d = env.dictionary(capacity=8)                      # the wrapper sizes the table itself
    with pytest.raises(ValueError):
        d.encode(RaggedBatch(torch.zeros(4, dtype=torch.float32), [0], [4]))
    assert C.text_dict_launches() == before             # nothing was launched
    probe(data=0, nbytes=0, start=0, length=0, n=0, table=0, cap=1, slot_of=0, hashes=0)    # n = 0: null arrays are fine
    C.text_dict_first_raw(0, 1, 0, 0, 0, no, 0, 0)
    C.text_dict_codes_raw(0, 1, 0, 0, 0, 0, no, 0)
    C.text_dict_commit_raw(0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, no)
    C.text_dict_rehash_raw(0, 0, 0, 1, no)
    assert d.encode(env.batch([])).cpu().tolist() == [] and d.lookup(env.batch([])).cpu().tolist() == []
    raw = _Raw(env)
    assert raw.encode([]) == ([], []) and raw.D == 0
    assert C.text_dict_launches() == before and d.size == 0
    assert d.encode(env.batch([b"x", b"y", b"x"])).cpu().tolist() == [0, 1, 0]
    # probe, first, codes, commit (the append is a text-column launch)
    assert C.text_dict_launches() == before + (4 if env.gpu else 0)
    assert d.lookup(env.batch([b"y"])).cpu().tolist() == [1]
    assert C.text_dict_launches() == before + (6 if env.gpu else 0)
