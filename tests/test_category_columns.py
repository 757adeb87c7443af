"""Category columns through parse_fields and read_delimited_columns: a CSV from csv.writer whose label
field holds separators, doubled quotes and line breaks, read back as int32 codes.  The yardstick is

    codes = [d.setdefault(v, len(d)) for v in values]

over what csv.reader yields for the field, in row order, with -1 (``None`` in ``tolist()``) exactly
where the text column of the same call has ``None``.  `cpu` runs on a DRAM-tier mini cluster (the
host loops), `cuda` on the HBM tier (the kernels); one cluster and one file per device serve all
the tests of this file."""
import csv
import io

import numpy as np
import pytest
import torch

from alluxio_amd.minicluster import LocalAlluxioCluster
from alluxio_amd.models import (FieldColumns, RaggedBatch, TextDictionary, build_delimited_index, parse_fields,
                                read_delimited_columns)

NROWS = 3000
PIECES = ["red", "green", "blue", "a,b", 'say "hi"', "two\nlines", '"', '""', ",", "x" * 40, "Red", "re", "r", "0"]
PATH = "/cat/table.csv"


def _labels():
    rng = np.random.default_rng(31)
    pool = ["".join(PIECES[i] for i in rng.integers(0, len(PIECES), int(rng.integers(1, 4)))) for _ in range(90)]
    return ["" if r % 17 == 5 else pool[int(rng.integers(0, min(len(pool), 5 + r // 20)))] for r in range(NROWS)]


class _World:
    def __init__(self, device, cluster):
        self.device, self.fs = device, cluster.client()
        labels = _labels()
        buf = io.StringIO()
        csv.writer(buf, lineterminator="\n").writerows([r, lab, f"t{r % 7}"] for r, lab in enumerate(labels))
        self.blob = buf.getvalue().encode()
        assert b'""' in self.blob and b',"' in self.blob
        self.fs.write_file(PATH, self.blob, write_type="MUST_CACHE")
        self.index = np.ascontiguousarray(build_delimited_index(self.fs, PATH, b"\n", quote='"')).astype(np.int64)
        assert len(self.index) == NROWS + 1
        # what csv.reader yields for the fields, and the yardstick over them
        read = list(csv.reader(io.StringIO(self.blob.decode(), newline="")))
        assert len(read) == NROWS and [r[1] for r in read] == labels
        self.values = [r[1].encode() or None for r in read]
        self.tags = [r[2].encode() for r in read]
        self.ref = {}
        self.codes = [None if v is None else self.ref.setdefault(v, len(self.ref)) for v in self.values]
        assert len(self.ref) > 50 and None in self.codes

    def batch(self, lo=0, hi=NROWS) -> RaggedBatch:
        """Rows lo..hi of the file as one packed batch on the device."""
        data = torch.from_numpy(np.frombuffer(self.blob, dtype=np.uint8).copy()).to(self.device)
        cut = torch.from_numpy(self.index[lo:hi + 1].copy()).to(self.device)
        return RaggedBatch(data, cut[:-1], cut[1:] - cut[:-1])


@pytest.fixture(scope="module", params=[pytest.param("cpu", id="cpu"),
                                        pytest.param("cuda", marks=pytest.mark.gpu, id="cuda")])
def world(request):
    device = request.param
    if device == "cuda" and not torch.cuda.is_available():
        pytest.fail("gpu-marked test ran without a visible HIP device")
    conf = {"alluxio.worker.tieredstore.level0.dirs.path": "dram" if device == "cpu" else "hbm:0",
            "alluxio.worker.hbm.page.size": "64KB", "alluxio.user.block.size.bytes.default": "256KB"}
    with LocalAlluxioCluster(num_workers=1, conf=conf) as c:
        w = _World(device, c)
        yield w
        w.fs.close()


def _minus(codes):
    return [-1 if c is None else c for c in codes]


def test_codes_are_those_of_the_loop_over_csv_reader(world):
    got = parse_fields(world.batch(), {"label": (1, "category"), "text": (1, "text"), "id": (0, "int64")}, quote='"')
    label, text = got["label"], got["text"]
    assert label.values.dtype == torch.int32 and label.values.device.type == world.device
    assert isinstance(label.dictionary, TextDictionary) and text.dictionary is None
    texts = text.tolist()
    assert texts == world.values                        # the text column is what csv.reader yields
    assert label.tolist() == world.codes                # None exactly where the text column has None
    assert label.values.cpu().tolist() == _minus(world.codes)
    assert torch.equal(label.status, text.status)
    assert label.dictionary.tolist() == list(world.ref) and label.dictionary.size == len(world.ref)
    entries = label.dictionary.tolist()                 # decoding the codes gives the text column back
    assert [None if c is None else entries[c] for c in label.tolist()] == texts
    assert "category" in repr(label) and label.start is None and label.data is None


def test_a_dictionary_is_shared_across_calls_and_columns(world):
    d = TextDictionary(world.device, capacity=8)
    first = parse_fields(world.batch(0, 1000), {"label": (1, "dict")}, quote='"', dictionaries={"label": d})
    assert first["label"].dictionary is d
    rest = parse_fields(world.batch(1000, NROWS), [(0, "int64"), (1, "category")], quote='"', dictionaries={1: d})
    assert rest[1].dictionary is d
    assert first["label"].tolist() + rest[1].tolist() == world.codes and d.tolist() == list(world.ref)
    both = FieldColumns.concat([parse_fields(world.batch(0, 1000), [(0, "int64"), (1, "category")], quote='"',
                                             dictionaries={1: d}), rest])
    assert both[1].dictionary is d and both[1].tolist() == world.codes and both.rows == NROWS
    # two category columns of one call, one of them into the shared dictionary: tags come after the labels
    got = parse_fields(world.batch(), {"tag": (2, "category"), "label": (1, "category")}, quote='"',
                       dictionaries={"tag": d})
    ref = dict(world.ref)
    assert got["tag"].tolist() == [ref.setdefault(v, len(ref)) for v in world.tags]
    assert got["label"].dictionary is not d and got["label"].tolist() == world.codes
    # a frozen vocabulary: lookup of the text column adds nothing
    size = d.size
    text = parse_fields(world.batch(0, 200), [(1, "text")], quote='"')[0]
    assert d.lookup(text).cpu().tolist() == _minus(world.codes[:200]) and d.size == size
    with pytest.raises(ValueError, match="not a category"):
        parse_fields(world.batch(0, 10), {"id": (0, "int64")}, dictionaries={"id": d})
    with pytest.raises(KeyError):
        parse_fields(world.batch(0, 10), {"label": (1, "category")}, dictionaries={"lable": d})
    with pytest.raises(TypeError):
        parse_fields(world.batch(0, 10), {"label": (1, "category")}, dictionaries={"label": {}})


def test_codes_are_file_global_over_many_batches(world):
    mine = TextDictionary(world.device, capacity=8)
    small = read_delimited_columns(world.fs, PATH, {"label": (1, "category"), "id": (0, "int64")}, quote='"',
                                   batch_size=64, device=world.device, dictionaries={"label": mine})
    assert small.rows == NROWS and small["label"].dictionary is mine      # the caller's dictionary comes back
    assert small["label"].tolist() == world.codes and mine.tolist() == list(world.ref)
    assert small["id"].values.cpu().tolist() == list(range(NROWS))
    large = read_delimited_columns(world.fs, PATH, [(1, "category")], quote='"', batch_size=65536, device=world.device)
    assert large[0].dictionary is not mine and large[0].dictionary.tolist() == mine.tolist()
    assert torch.equal(large[0].values, small["label"].values) and torch.equal(large[0].status, small["label"].status)
    # a second file-wide read into the same dictionary: nothing new, the same codes
    again = read_delimited_columns(world.fs, PATH, [(1, "category")], quote='"', batch_size=500, device=world.device,
                                   dictionaries={0: mine})
    assert again[0].tolist() == world.codes and mine.size == len(world.ref)
    none = read_delimited_columns(world.fs, PATH, [(1, "category")], quote='"', skip_rows=10 ** 6, device=world.device)
    assert none.rows == 0 and none[0].values.dtype == torch.int32 and none[0].dictionary.size == 0


def test_concat_needs_one_dictionary(world):
    spec = {"label": (1, "category")}
    a = parse_fields(world.batch(0, 100), spec, quote='"')
    b = parse_fields(world.batch(100, 200), spec, quote='"')
    with pytest.raises(ValueError, match="different dictionaries"):
        FieldColumns.concat([a, b])
    c = parse_fields(world.batch(100, 200), spec, quote='"', dictionaries={"label": a["label"].dictionary})
    assert FieldColumns.concat([a, c])["label"].tolist() == world.codes[:200]


def test_more_than_32_columns(world):
    rows = [[f"c{j}-{(r * (j + 1)) % (3 + j)}" if (r + j) % 9 else "" for j in range(40)] for r in range(300)]
    buf = io.StringIO()
    csv.writer(buf, lineterminator="\n").writerows(rows)
    blob = buf.getvalue().encode()
    cuts = np.array([0] + [i + 1 for i, ch in enumerate(blob) if ch == 0x0A], dtype=np.int64)
    data = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(world.device)
    cut = torch.from_numpy(cuts).to(world.device)
    batch = RaggedBatch(data, cut[:-1], cut[1:] - cut[:-1])
    kinds = ["category" if j % 3 == 0 else ("text" if j % 3 == 1 else "span") for j in range(40)]
    shared = TextDictionary(world.device)
    got = parse_fields(batch, [(j, kinds[j]) for j in range(40)], quote='"', dictionaries={0: shared, 39: shared})
    assert len(got) == 40
    ref0 = {}
    for j in range(40):
        column = [r[j].encode() or None for r in rows]
        if kinds[j] == "text":
            assert got[j].tolist() == column
        elif kinds[j] == "category":
            ref = ref0 if j in (0, 39) else {}          # columns 0 and 39 share a dictionary, in that order
            assert got[j].tolist() == [None if v is None else ref.setdefault(v, len(ref)) for v in column], j
            assert got[j].dictionary.tolist() == list(ref) or j == 0
    assert got[0].dictionary is shared and got[39].dictionary is shared and shared.tolist() == list(ref0)
