"""Training-input integration: HBM-cached datasets gathered straight into GPU batches.

The reference serves ML input pipelines through its POSIX (FUSE) and Hadoop clients — a trainer
opens files and issues small reads, one syscall / RPC per record.  On MI355X the dataset's blocks
sit in the worker's HBM arena, so a whole batch of records (random indices, spanning block
boundaries) is planned on the host and moved by ONE page-gather kernel launch into a
``[batch, record_bytes]`` device tensor, on a side stream, double-buffered so the next batch is in
flight while the model consumes the current one:

* worker in this process  -> ``BlockStore.read_batch`` (native planner + gather kernel);
* worker in another process on this node -> HIP IPC mapping of its arena (held for the loader's
  lifetime) + the batched copy kernel on this GPU (over xGMI when the worker owns another GPU);
* anything else -> the regular client stream per record (host path).

``FixedRecordDataset`` is the map-style view (``torch.utils.data.Dataset``) for code that wants
per-sample access; ``DeviceBatchLoader`` is the fast path.

Variable-length records (tokenised documents, encoded images) are an ``IndexedRecordDataset``:
per-file offset arrays (or the ``<path>.idx`` sidecar, or one record per file).  The loader then
yields ``RaggedBatch(data, offsets, lengths)``, packed or padded.  When one in-process worker holds
every block in one memory dir, a batch is one ``RaggedGatherSession.gather``: the page table and
the record index live on the device, a plan launch sizes the rows and a copy launch moves them, and
the host does nothing per record or page.  Other sources take the general path above.
"""
from __future__ import annotations

import numpy as np

from ..utils import ids
from ..utils.tracing import traced


class _FileLayout:
    """Path, length and block layout of one file; the BlockInfo list is materialised on first use
    (a 1 M-file listing must not pay for 1 M sub-message wrappers it may never touch)."""

    __slots__ = ("info", "path", "length", "block_size", "_blocks")

    def __init__(self, status):
        i = status.info
        self.info = i
        self.path = i.path
        self.length = i.length
        self.block_size = i.blockSizeBytes
        self._blocks = None

    @property
    def blocks(self):
        if self._blocks is None:
            self._blocks = [fbi.blockInfo for fbi in self.info.fileBlockInfos]
        return self._blocks

    @property
    def block_ids(self):
        return self.info.blockIds


class _LazyLayouts:
    """``files`` of a columnar listing: the _FileLayout of entry i is parsed on first access."""

    def __init__(self, cols, keep):
        self._cols, self._keep = cols, keep
        self._cache: dict = {}

    def __len__(self) -> int:
        return len(self._keep)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        lay = self._cache.get(i)
        if lay is None:
            lay = self._cache[i] = _FileLayout(self._cols.status(int(self._keep[i])))
        return lay

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]


class FixedRecordDataset:
    """Records of ``record_bytes`` laid end to end across one or more files."""

    def __init__(self, fs, paths, record_bytes: int, dtype="uint8", shape=None, device=None):
        import torch
        self.fs = fs
        self.record_bytes = record_bytes
        self.dtype = getattr(torch, str(dtype)) if isinstance(dtype, str) else dtype
        self.shape = tuple(shape) if shape else None
        self.device = device
        self.files = [_FileLayout(fs.get_status(p)) for p in ([paths] if isinstance(paths, str) else paths)]
        self.counts = [f.length // record_bytes for f in self.files]
        self.starts = np.cumsum([0] + self.counts)

    def __len__(self):
        return int(self.starts[-1])

    def locate(self, idx: int) -> tuple[int, int]:
        """(file index, byte offset) of record ``idx``."""
        if idx < 0:
            idx += len(self)
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        f = int(np.searchsorted(self.starts, idx, side="right") - 1)
        return f, (idx - int(self.starts[f])) * self.record_bytes

    def _view(self, raw):
        t = raw.view(self.dtype)
        return t.view(self.shape) if self.shape else t

    def __getitem__(self, idx):
        import torch
        f, off = self.locate(idx)
        out = torch.empty(self.record_bytes, dtype=torch.uint8, device=self.device)
        with self.fs.open_file(self.files[f].path) as s:
            s.pread(off, out)
        return self._view(out)


class FileListDataset(FixedRecordDataset):
    """One record per file of a directory (BASELINE config 4: ImageNet-shaped 128 KB files), with
    the metadata of every file from ONE ``listStatus`` (batched metadata: no per-file getStatus;
    the FileInfos carry their block ids and locations).  Files longer than ``record_bytes`` are
    truncated, shorter ones zero-padded (``lengths`` keeps the true sizes)."""

    def __init__(self, fs, directory: str, record_bytes: int | None = None, dtype="uint8", shape=None,
                 device=None):
        import torch
        self.fs = fs
        self.dtype = getattr(torch, str(dtype)) if isinstance(dtype, str) else dtype
        self.shape = tuple(shape) if shape else None
        self.device = device
        cols = fs.list_status_columns(directory) if hasattr(fs, "list_status_columns") else None
        if cols is None:
            sts = sorted((s for s in fs.list_status(directory) if not s.is_folder), key=lambda s: s.path)
            self.paths = [s.path for s in sts]
            self.lengths = np.array([s.length for s in sts], dtype=np.uint64)
            self.files = [_FileLayout(s) for s in sts]
            nblocks = np.array([len(f.block_ids) for f in self.files], dtype=np.int64)
            bsizes = np.array([f.block_size for f in self.files], dtype=np.int64)
            self.block_ids = np.array([f.block_ids[0] if len(f.block_ids) else -1 for f in self.files], dtype=np.int64)
        else:
            # columnar listing: no per-file Python objects until a file's layout is needed
            keep = np.nonzero(cols.folder == 0)[0]
            paths = [cols.paths[i] for i in keep]
            if any(paths[k] > paths[k + 1] for k in range(len(paths) - 1)):
                order = sorted(range(len(paths)), key=paths.__getitem__)
                keep, paths = keep[order], [paths[k] for k in order]
            self.paths = paths
            self.lengths = cols.lengths[keep].astype(np.uint64)
            self.files = _LazyLayouts(cols, keep)
            nblocks, bsizes = cols.nblocks[keep], cols.block_sizes[keep]
            self.block_ids = cols.first_blocks[keep].astype(np.int64)
        n = len(self.paths)
        self.record_bytes = int(record_bytes or (self.lengths.max() if n else 0))
        self.counts = [1] * n
        self.starts = np.arange(n + 1)
        # single-block records: the gather plan is a vector op over these arrays
        self.single_block = bool(np.all(nblocks == 1)) and bool(np.all(bsizes >= self.record_bytes))
        self.read_lengths = np.minimum(self.lengths, np.uint64(self.record_bytes))

    def locate(self, idx: int) -> tuple[int, int]:
        if idx < 0:
            idx += len(self)
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        return idx, 0


INDEX_MAGIC = b"AMDXIDX1"


def _check_offsets(offsets, what: str) -> np.ndarray:
    off = np.asarray(offsets)
    if off.ndim != 1 or off.size < 1:
        raise ValueError(f"{what}: a record index is a 1-D array of n+1 offsets")
    if off.dtype.kind not in "iu":
        raise ValueError(f"{what}: offsets must be integers")
    if off.dtype.kind == "u" and off.size and int(off.max()) > np.iinfo(np.int64).max:
        raise ValueError(f"{what}: offset out of range")
    off = off.astype(np.int64)
    if int(off[0]) < 0 or (off.size > 1 and bool((np.diff(off) < 0).any())):
        raise ValueError(f"{what}: record offsets must be non-negative and must not decrease")
    return off


def write_index(fs, path: str, offsets, **kw) -> str:
    """Write the sidecar ``<path>.idx`` of a record file: ``AMDXIDX1``, a uint64 ``n`` and the
    ``n+1`` uint64 record offsets, little-endian.  Returns the sidecar's path."""
    off = _check_offsets(offsets, path)
    body = INDEX_MAGIC + np.array([off.size - 1], dtype="<u8").tobytes() + off.astype("<u8").tobytes()
    fs.write_file(path + ".idx", body, **kw)
    return path + ".idx"


def read_index(fs, path: str) -> np.ndarray:
    """The int64 offsets stored in ``<path>.idx`` (see :func:`write_index`)."""
    raw = fs.read_file(path + ".idx")
    if len(raw) < 16 or raw[:8] != INDEX_MAGIC:
        raise ValueError(f"{path}.idx: not a record index (bad magic)")
    n = int(np.frombuffer(raw, dtype="<u8", count=1, offset=8)[0])
    if len(raw) < 16 + 8 * (n + 1):
        raise ValueError(f"{path}.idx: truncated ({len(raw)} bytes for {n} records)")
    return _check_offsets(np.frombuffer(raw, dtype="<u8", count=n + 1, offset=16), path + ".idx")


def _delimiter_byte(delimiter) -> int:
    d = delimiter.encode() if isinstance(delimiter, str) else bytes(delimiter)
    if len(d) != 1:
        raise ValueError(f"the delimiter must be exactly one byte, got {len(d)}")
    return d[0]


def _quote_byte(quote, delim: int):
    """None, or the one byte of ``quote``; it may not equal the delimiter."""
    if quote is None:
        return None
    q = quote.encode() if isinstance(quote, str) else bytes(quote)
    if len(q) != 1:
        raise ValueError(f"the quote must be exactly one byte, got {len(q)}")
    if q[0] == delim:
        raise ValueError("the quote must differ from the delimiter")
    return q[0]


def _store_cuts(fs, lay: _FileLayout, delim: int, quote=None):
    """Cut positions of one file from the worker's own memory (``delim_index_store``: kernels for
    an HBM dir, the host loop for a DRAM dir), or None when the loader's rule sends the file to
    the stream path: a block not held by one in-process worker, or a layout the native call
    refuses (file tier, several dirs)."""
    from ..ops.native import lib
    ctx = getattr(fs, "ctx", None)
    if ctx is None or not hasattr(ctx, "in_process_worker"):
        return None
    holders = None
    for b in lay.blocks:
        here = {id(w): w for w in (ctx.in_process_worker(loc.workerAddress) for loc in b.locations) if w is not None}
        holders = here if holders is None else {k: w for k, w in holders.items() if k in here}
        if not holders:
            return None
    w = next(iter(holders.values()))
    ids_ = [int(b) for b in lay.block_ids]
    lens = [min(lay.block_size, lay.length - k * lay.block_size) for k in range(len(ids_))]
    try:
        if quote is None:
            return lib().delim_index_store(w.native, ids.create_session_id(), ids_, lens, delim)
        return lib().delim_index_store(w.native, ids.create_session_id(), ids_, lens, delim, quote=quote)
    except lib().StoreError as e:
        if len(e.args) >= 1 and e.args[0] in (1, 6):     # block gone or a layout the call does not take
            return None
        from ..ops.native import translate
        raise translate(e) from None


def _stream_cuts(fs, path: str, delim: int, chunk_bytes: int, quote=None) -> np.ndarray:
    """The same cut positions from the client stream, ``chunk_bytes`` at a time.  With a quote the
    state "inside quotes" (the parity of the quote bytes so far) travels from chunk to chunk."""
    parts, pos, state = [], 0, 0
    buf = np.empty(max(1, int(chunk_bytes)), dtype=np.uint8)
    with fs.open_file(path) as f:
        while True:
            n = f.readinto(buf)
            if n <= 0:
                break
            hit = buf[:n] == delim
            if quote is not None:
                # the state after each byte, relative to the chunk's start; a delimiter is no quote,
                # so at a delimiter it is also the state before it
                inside = np.logical_xor.accumulate(buf[:n] == quote)
                hit &= inside if state else ~inside     # an even number of quote bytes before it
                state ^= int(inside[-1])
            parts.append(np.flatnonzero(hit).astype(np.uint64) + np.uint64(pos + 1))
            pos += n
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)


def build_delimited_index(fs, path: str, delimiter=b"\n", quote=None, write: bool = False, device_plan="auto",
                          chunk_bytes: int = 8 << 20, **write_kw) -> np.ndarray:
    """The record index of a delimited text file (JSONL, CSV, one document per line): int64 offsets
    ``[0, every cut ..., file length]`` where a cut is the byte after a delimiter, so records keep
    their trailing delimiter (``bytes.splitlines(keepends=True)`` for ``\\n``), a last line without
    one is a record and an empty file gives ``[0]``.

    ``quote`` (one byte, not the delimiter; ``'"'`` for CSV) makes the index quote-aware: every
    quote byte toggles the state "inside quotes", the file starts outside, and a delimiter is a cut
    only when the number of quote bytes before it is even.  A doubled quote ``""`` toggles twice,
    so this is the record structure of every well-formed RFC 4180 file, line breaks inside quoted
    fields included.  It is not the ``csv`` module's lenient reading of a stray quote in the
    middle of an unquoted field: there the two disagree.  A file that ends inside quotes is no
    error; its tail is the last record.

    When one in-process worker holds every block in one memory dir the delimiters are found where
    the bytes are (count, scan and emit kernels through the page table for an HBM dir, a memchr
    loop for a DRAM dir); otherwise, or with ``device_plan=False``, the file is read through the
    client stream ``chunk_bytes`` at a time.  All paths return the same array.  ``write=True`` also
    stores it as the ``<path>.idx`` sidecar (``write_kw`` goes to :func:`write_index`)."""
    delim = _delimiter_byte(delimiter)
    quote = _quote_byte(quote, delim)
    if device_plan not in ("auto", False):
        raise ValueError("device_plan must be 'auto' or False")
    lay = _FileLayout(fs.get_status(path))
    cuts = None
    if device_plan == "auto" and lay.length and len(lay.block_ids):
        cuts = _store_cuts(fs, lay, delim, quote)
    if cuts is None:
        cuts = _stream_cuts(fs, path, delim, chunk_bytes, quote) if lay.length else np.zeros(0, dtype=np.uint64)
    off = np.empty(cuts.size + 2, dtype=np.int64)
    off[0] = 0
    off[1:-1] = cuts
    off[-1] = lay.length
    if lay.length == 0 or (cuts.size and int(cuts[-1]) == lay.length):
        off = off[:-1]
    if write:
        write_index(fs, path, off, **write_kw)
    return off


class RaggedBatch(tuple):
    """``(data, offsets, lengths)`` of a batch of variable-length records.  Packed: ``data`` is
    1-D and record r is ``data[offsets[r]:offsets[r] + lengths[r]]``; padded: ``data`` is
    ``[B, max_len]`` and ``offsets[r] = r * max_len``.  Offsets and lengths count elements."""

    __slots__ = ()

    def __new__(cls, data, offsets, lengths):
        return tuple.__new__(cls, (data, offsets, lengths))

    data = property(lambda self: self[0])
    offsets = property(lambda self: self[1])
    lengths = property(lambda self: self[2])


class IndexedRecordDataset:
    """Variable-length records laid end to end in one or more files.  ``index`` holds, per file,
    the ``n+1`` monotone byte offsets of its records (``None``: read the sidecar ``<path>.idx``)."""

    ragged = True

    def __init__(self, fs, paths, index=None, dtype="uint8", device=None):
        paths = [paths] if isinstance(paths, str) else list(paths)
        if index is None:
            index = [read_index(fs, p) for p in paths]
        elif len(paths) == 1 and not isinstance(index, (list, tuple)):
            index = [index]
        if len(index) != len(paths):
            raise ValueError("one offset array per file is required")
        files = [_FileLayout(fs.get_status(p)) for p in paths]
        self.paths = paths
        self._init(fs, files, [_check_offsets(o, p) for o, p in zip(index, paths)],
                   np.array([f.length for f in files], dtype=np.int64), dtype, device)

    def _init(self, fs, files, offsets, file_lengths, dtype, device, file_blocks=None):
        import torch
        self.fs = fs
        self.dtype = getattr(torch, str(dtype)) if isinstance(dtype, str) else dtype
        self.itemsize = torch.empty(0, dtype=self.dtype).element_size()
        self.device = device
        self.files = files
        self.offsets = offsets
        self._file_blocks = file_blocks
        for k, off in enumerate(offsets):
            if int(off[-1]) > int(file_lengths[k]):
                raise ValueError(f"file {k}: record offsets run past the end of the file "
                                 f"({int(off[-1])} > {int(file_lengths[k])})")
        self.counts = [len(o) - 1 for o in offsets]
        self.starts = np.cumsum([0] + self.counts)
        n = int(self.starts[-1])
        self.record_offsets = np.concatenate([o[:-1] for o in offsets]) if n else np.zeros(0, np.int64)
        self.lengths = np.concatenate([np.diff(o) for o in offsets]) if n else np.zeros(0, np.int64)
        if n and int(self.lengths.max()) >= 2 ** 32 - 256:
            raise ValueError("records of 4 GiB or more are not supported")
        if self.itemsize > 1 and bool((self.lengths % self.itemsize).any()):
            raise ValueError(f"every record length must be a multiple of the item size ({self.itemsize})")
        self.max_bytes = int(self.lengths.max()) if n else 0

    @classmethod
    def from_files(cls, fs, directory: str, dtype="uint8", device=None):
        """One record per file of ``directory`` at its true length, from one columnar listing."""
        self = cls.__new__(cls)
        cols = fs.list_status_columns(directory) if hasattr(fs, "list_status_columns") else None
        file_blocks = None
        if cols is None:
            sts = sorted((s for s in fs.list_status(directory) if not s.is_folder), key=lambda s: s.path)
            self.paths = [s.path for s in sts]
            lengths = np.array([s.length for s in sts], dtype=np.int64)
            files = [_FileLayout(s) for s in sts]
        else:
            keep = np.nonzero(cols.folder == 0)[0]
            paths = [cols.paths[i] for i in keep]
            if any(paths[k] > paths[k + 1] for k in range(len(paths) - 1)):
                order = sorted(range(len(paths)), key=paths.__getitem__)
                keep, paths = keep[order], [paths[k] for k in order]
            self.paths = paths
            lengths = cols.lengths[keep].astype(np.int64)
            files = _LazyLayouts(cols, keep)
            if bool(np.all(cols.nblocks[keep] <= 1)):
                # single-block files: the session's block list comes from the columns alone
                first = cols.first_blocks[keep].astype(np.int64)
                file_blocks = [([int(b)], [int(n)]) if n else ([], []) for b, n in zip(first, lengths)]
        self._init(fs, files, [np.array([0, n], dtype=np.int64) for n in lengths], lengths, dtype, device,
                   file_blocks)
        return self

    @classmethod
    def from_delimited(cls, fs, paths, delimiter=b"\n", dtype="uint8", device=None, write_index: bool = False,
                       quote=None):
        """One record per line (or per ``delimiter``-terminated piece) of one or more text files:
        the index of each file comes from :func:`build_delimited_index`, and ``write_index=True``
        also stores it as the file's ``.idx`` sidecar.  ``quote='"'`` keeps a CSV row with line
        breaks inside quoted fields in one record (see :func:`build_delimited_index`)."""
        paths = [paths] if isinstance(paths, str) else list(paths)
        index = [build_delimited_index(fs, p, delimiter, quote=quote, write=write_index) for p in paths]
        return cls(fs, paths, index=index, dtype=dtype, device=device)

    def __len__(self):
        return int(self.starts[-1])

    def locate(self, idx: int) -> tuple[int, int]:
        """(file index, byte offset) of record ``idx``."""
        if idx < 0:
            idx += len(self)
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        f = int(np.searchsorted(self.starts, idx, side="right") - 1)
        return f, int(self.record_offsets[idx])

    def file_blocks(self):
        """[(block ids, block lengths)] per file, the form a gather session takes."""
        if self._file_blocks is None:
            out = []
            for f in self.files:
                ids_ = [int(b) for b in f.block_ids]
                out.append((ids_, [min(f.block_size, f.length - k * f.block_size) for k in range(len(ids_))]))
            self._file_blocks = out
        return self._file_blocks

    def __getitem__(self, idx):
        import torch
        if idx < 0:
            idx += len(self)
        f, off = self.locate(idx)
        out = torch.empty(int(self.lengths[idx]), dtype=torch.uint8, device=self.device)
        if out.numel():
            with self.fs.open_file(self.files[f].path) as s:
                s.pread(off, out)
        return out.view(self.dtype)


class DeviceBatchLoader:
    """Iterates ``[batch, *shape]`` device tensors of records gathered by one kernel per batch.

    Over an :class:`IndexedRecordDataset` it yields :class:`RaggedBatch` instead: ``layout`` is
    ``"packed"`` (row starts rounded up to ``align`` bytes, a power of two up to 256; gaps are
    zero) or ``"padded"`` (``[B, max_len]`` elements, longer records truncated, the rest filled
    with the byte ``pad_value``; ``max_len`` defaults to the longest record).  With
    ``device_plan="auto"`` a batch is one ``RaggedGatherSession.gather`` when every block is held
    by one in-process worker in one memory dir; ``device_plan=False`` keeps the general path."""

    def __init__(self, dataset: FixedRecordDataset, batch_size: int, shuffle: bool = False, seed: int = 0,
                 drop_last: bool = False, device=None, prefetch: int = 2, layout: str = "packed", align: int = 16,
                 max_len: int | None = None, pad_value: int = 0, device_plan="auto"):
        import torch
        self.ds = dataset
        self.ragged = bool(getattr(dataset, "ragged", False))
        if self.ragged:
            if layout not in ("packed", "padded"):
                raise ValueError("layout must be 'packed' or 'padded'")
            if align < 1 or align > 256 or align & (align - 1):
                raise ValueError("align must be a power of two from 1 to 256")
            if not 0 <= pad_value <= 255:
                raise ValueError("pad_value is one byte")
            if device_plan not in ("auto", False):
                raise ValueError("device_plan must be 'auto' or False")
            self.layout = layout
            self.align = max(align, dataset.itemsize)      # rows start on whole elements
            self.max_bytes = dataset.max_bytes if max_len is None else int(max_len) * dataset.itemsize
            self.pad_value = pad_value
        self.device_plan = device_plan
        self._gather = False          # RaggedGatherSession once opened; None: general path
        self._gather_worker = None
        self.batch_size = batch_size
        self.shuffle = shuffle
        self.seed = seed
        self.drop_last = drop_last
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu"))
        self.prefetch = max(1, prefetch)
        self.epoch = 0
        self._sources = None
        self.session = ids.create_session_id()
        self.stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None

    # ---- sources ------------------------------------------------------------------------------
    def _open_sources(self):
        """Per block: ('local', worker) | ('ipc', DeviceBlockHandle, base) | ('stream', None)."""
        if self._sources is not None:
            return self._sources
        ctx = self.ds.fs.ctx
        src = {}
        self._locks = []
        for f in self.ds.files:
            for b in f.blocks:
                chosen = ("stream", None)
                for loc in b.locations:
                    w = ctx.in_process_worker(loc.workerAddress)
                    if w is not None:
                        self._locks.append((w, w.lock_block(self.session, b.blockId)))
                        chosen = ("local", w)
                        break
                # same-node holder: map its arena (HBM via HIP IPC, DRAM via shared memory) and
                # gather with the copy kernel (host memcpy without a GPU)
                from ..ops.native import has_gpu
                if chosen[0] == "stream" and (self.device.type == "cuda" or not has_gpu()):
                    for loc in b.locations:
                        if not ctx.is_local(loc.workerAddress):
                            continue
                        try:
                            from ..client.context import worker_address_str
                            from ..parallel.ipc import map_handle
                            from ..proto import pb
                            stub = ctx.worker_stub(worker_address_str(loc.workerAddress))
                            h = stub.OpenDeviceBlock(pb.block.OpenDeviceBlockRequest(block_id=b.blockId,
                                                                                     session_id=self.session))
                            try:
                                base = map_handle(h, self.device.index or 0)
                            except Exception:
                                stub.UnlockDeviceBlock(pb.block.UnlockDeviceBlockRequest(
                                    block_id=b.blockId, lock_id=h.lock_id, session_id=self.session))
                                raise
                            self._locks.append((stub, h))
                            chosen = ("ipc", (h, base))
                            break
                        except Exception:  # noqa: BLE001 - fall back to the stream path
                            continue
                src[b.blockId] = chosen
        self._sources = src
        return src

    def close(self):
        from ..proto import pb
        if self._gather:
            self._gather.close()
        self._gather = False
        self._gather_worker = None
        for holder, lk in getattr(self, "_locks", []):
            try:
                if isinstance(lk, int):
                    holder.unlock(lk)
                else:
                    holder.UnlockDeviceBlock(pb.block.UnlockDeviceBlockRequest(
                        block_id=lk.block_id, lock_id=lk.lock_id, session_id=self.session))
            except Exception:  # noqa: BLE001
                pass
        self._locks = []
        self._sources = None
        self._one_worker = False

    # ---- planning -----------------------------------------------------------------------------
    def _pieces(self, rec_idx: int, nbytes: int | None = None):
        """[(block info, offset in block, length, offset in record)] for one record (its first
        ``nbytes`` bytes; default: the dataset's fixed record size)."""
        f, off = self.ds.locate(rec_idx)
        lay = self.ds.files[f]
        out, done, n = [], 0, self.ds.record_bytes if nbytes is None else nbytes
        while done < n:
            bi = (off + done) // lay.block_size
            boff = (off + done) - bi * lay.block_size
            take = min(n - done, lay.block_size - boff)
            out.append((lay.blocks[bi], boff, take, done))
            done += take
        return out

    def _single_worker(self):
        """The in-process worker holding every block of a single-block-record dataset (then the
        batch plan is pure array arithmetic + one ``read_batch_arrays``), else None."""
        if not getattr(self.ds, "single_block", False):
            return None
        if getattr(self, "_one_worker", False) is not False:
            return self._one_worker
        srcs = self._open_sources()
        ws = {id(o): o for how, o in srcs.values() if how == "local"}
        self._one_worker = next(iter(ws.values())) if len(ws) == 1 and \
            all(how == "local" for how, _ in srcs.values()) else None
        return self._one_worker

    @traced("DeviceBatchLoader.fill")
    def _fill(self, out, indices):
        """Gather records ``indices`` into rows of ``out`` (uint8 [B, record_bytes])."""
        w = self._single_worker()
        if w is not None:
            ix = np.asarray(indices, dtype=np.int64)
            lens = self.ds.read_lengths[ix]
            if (lens < self.ds.record_bytes).any():
                out.zero_()                # pad short files
            dsts = np.uint64(out.data_ptr()) + np.arange(len(ix), dtype=np.uint64) * np.uint64(self.ds.record_bytes)
            stream = int(self.stream.cuda_stream) if self.stream is not None else 0
            w.native.read_batch_arrays(self.ds.block_ids[ix], np.zeros(len(ix), dtype=np.uint64), lens, dsts,
                                       1 if out.is_cuda else 0, stream, not out.is_cuda)
            w._count_read(int(lens.sum()), 1 if out.is_cuda else 0)
            return
        row = self.ds.record_bytes
        self._gather_rows(out.view(-1), indices, [r * row for r in range(len(indices))], None)

    def _gather_rows(self, flat, indices, row_offs, lens):
        """The general path: record ``indices[r]`` (its first ``lens[r]`` bytes; None: the fixed
        record size) lands at byte ``row_offs[r]`` of the 1-D uint8 tensor ``flat``, planned per
        record and per block on the host."""
        srcs = self._open_sources()
        kind = 1 if flat.is_cuda else 0
        by_worker: dict[int, tuple] = {}
        ipc_segs = []
        slow = []
        base_ptr = flat.data_ptr()
        for r, idx in enumerate(indices):
            nbytes = None if lens is None else int(lens[r])
            for bi, boff, n, roff in self._pieces(int(idx), nbytes):
                how, obj = srcs[bi.blockId]
                dst = base_ptr + int(row_offs[r]) + roff
                if how == "local":
                    by_worker.setdefault(id(obj), (obj, []))[1].append((bi.blockId, boff, n, dst, kind))
                elif how == "ipc":
                    h, base = obj
                    from ..parallel.ipc import page_segments
                    ipc_segs.extend(page_segments(base, list(h.pages), h.page_size, boff, n, dst))
                else:
                    slow.append((r, int(idx)))
        stream = int(self.stream.cuda_stream) if self.stream is not None else 0
        for w, reqs in by_worker.values():
            w.read_batch(reqs, stream, sync=not flat.is_cuda)
        if ipc_segs:
            from ..ops.native import lib
            lib().batched_copy(ipc_segs, stream, True)
        for r, idx in sorted(set(slow)):
            f, off = self.ds.locate(idx)
            n = self.ds.record_bytes if lens is None else int(lens[r])
            with self.ds.fs.open_file(self.ds.files[f].path) as s:
                s.pread(off, flat[int(row_offs[r]):int(row_offs[r]) + n])

    # ---- variable-length records ---------------------------------------------------------------
    def _gather_session(self):
        """The RaggedGatherSession of this loader, or None when the general path serves it
        (``device_plan=False``, blocks held elsewhere, in several dirs or in a file tier, or
        batches that live in the other kind of memory than the arena)."""
        if self._gather is not False:
            return self._gather
        self._gather = None
        if self.device_plan is False or len(self.ds) == 0:
            return None
        srcs = self._open_sources()
        ws = {id(o): o for how, o in srcs.values() if how == "local"}
        if len(ws) != 1 or not all(how == "local" for how, _ in srcs.values()):
            return None
        from ..ops.native import lib
        w = next(iter(ws.values()))
        try:
            g = lib().RaggedGatherSession(w.native, self.session, self.ds.file_blocks(),
                                          [np.ascontiguousarray(o, dtype=np.uint64) for o in self.ds.offsets])
        except lib().StoreError as e:
            if len(e.args) >= 1 and e.args[0] == 6:     # invalid argument: a layout the session does not take
                return None
            raise
        if g.arena_on_device != (self.device.type == "cuda"):
            g.close()
            return None
        self._gather, self._gather_worker = g, w
        return g

    @traced("DeviceBatchLoader.fill_ragged")
    def _fill_ragged(self, indices) -> RaggedBatch:
        import torch
        ix = np.ascontiguousarray(indices, dtype=np.int64)
        nb, item = len(ix), self.ds.itemsize
        lens = self.ds.lengths[ix]
        padded = self.layout == "padded"
        if padded:
            lens = np.minimum(lens, self.max_bytes)
            data = torch.empty((nb, self.max_bytes), dtype=torch.uint8, device=self.device)
        else:
            adv = (lens + (self.align - 1)) & ~np.int64(self.align - 1)
            data = torch.empty(int(adv.sum()), dtype=torch.uint8, device=self.device)
        g = self._gather_session()
        if g is not None:
            off = torch.empty(nb + 1, dtype=torch.int64, device=self.device)
            ln32 = torch.empty(nb, dtype=torch.int32, device=self.device)
            kind = 1 if data.is_cuda else 0
            stream = int(self.stream.cuda_stream) if self.stream is not None else 0
            from ..ops.native import native_errors
            with native_errors():
                _, nbytes = g.gather(ix, data.data_ptr(), data.numel(), off.data_ptr(), ln32.data_ptr(), self.layout,
                                     self.align, self.max_bytes, self.max_bytes, self.pad_value, kind, stream)
            self._gather_worker._count_read(int(nbytes), kind)
            ln = ln32.to(torch.int64)
        else:
            if padded:
                offs = np.arange(nb + 1, dtype=np.int64) * self.max_bytes
                data.fill_(self.pad_value)
            else:
                offs = np.concatenate([[0], np.cumsum(adv)]).astype(np.int64)
                data.zero_()
            self._gather_rows(data.view(-1), ix, offs, lens)
            off = torch.from_numpy(offs).to(self.device)
            ln = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int64)).to(self.device)
        if item > 1:
            off, ln = off // item, ln // item
        return RaggedBatch(data.view(self.ds.dtype), off, ln)

    def gather(self, indices) -> RaggedBatch:
        """The records ``indices`` of an :class:`IndexedRecordDataset` as one :class:`RaggedBatch`, now:
        what iteration yields for that batch, for callers that choose the records themselves.  The
        work runs on the loader's stream and torch's current stream waits for it."""
        import torch
        if not self.ragged:
            raise TypeError("gather takes a loader over an IndexedRecordDataset")
        ix = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        if len(ix) and (int(ix.min()) < 0 or int(ix.max()) >= len(self.ds)):
            raise IndexError("a record index outside the dataset")
        if self.stream is None:
            return self._fill_ragged(ix)
        with torch.cuda.stream(self.stream):
            batch = self._fill_ragged(ix)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(ev)
        for t in batch:
            t.record_stream(cur)
        return batch

    # ---- iteration ----------------------------------------------------------------------------
    def __len__(self):
        n = len(self.ds)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        import torch
        n = len(self.ds)
        order = np.random.default_rng(self.seed + self.epoch).permutation(n) if self.shuffle else np.arange(n)
        self.epoch += 1
        batches = [order[i:i + self.batch_size] for i in range(0, n, self.batch_size)]
        if self.drop_last and batches and len(batches[-1]) < self.batch_size:
            batches.pop()
        pending = []

        def launch(ix):
            if self.ragged:
                if self.stream is None:
                    return self._fill_ragged(ix), None
                with torch.cuda.stream(self.stream):
                    batch = self._fill_ragged(ix)
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
                return batch, ev
            buf = torch.empty((len(ix), self.ds.record_bytes), dtype=torch.uint8, device=self.device)
            if self.stream is not None:
                with torch.cuda.stream(self.stream):
                    self._fill(buf, ix)
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
            else:
                self._fill(buf, ix)
                ev = None
            return buf, ev

        it = iter(batches)
        for ix in it:
            pending.append(launch(ix))
            if len(pending) >= self.prefetch:
                break
        while pending:
            buf, ev = pending.pop(0)
            nxt = next(it, None)
            if nxt is not None:
                pending.append(launch(nxt))
            if self.ragged:
                if ev is not None:
                    cur = torch.cuda.current_stream(self.device)
                    cur.wait_event(ev)
                    for t in buf:
                        t.record_stream(cur)
                yield buf
                continue
            if ev is not None:
                torch.cuda.current_stream(self.device).wait_event(ev)
                buf.record_stream(torch.cuda.current_stream(self.device))
            t = buf.view(self.ds.dtype)
            yield t.view((buf.shape[0],) + self.ds.shape) if self.ds.shape else t

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
