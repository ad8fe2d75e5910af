"""CPU-only checks of HyperDepth forest evaluation: the forest file round trip, the loader's rejections, the C ABI's
exports and argument validation before any HIP call, and the numpy restatement against the reference's output
(tests/golden/hyperdepth.npz, written by make_golden_hyperdepth.py)."""
import ctypes
import os
import struct

import numpy as np
import pytest

from connecting_the_dots_amd import _lib
from connecting_the_dots_amd import hyperdepth as hd
from tests import hyperdepth_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hyperdepth.npz")


def golden_cases():
    z = np.load(GOLDEN)
    for ci, name in enumerate(z["names"]):
        k = "c%d_" % ci
        bins, row_from, row_to, n_forests = (int(x) for x in z[k + "params"])
        forests = [R.forest_from_arrays({key: z["%sf%d_%s" % (k, fi, key)] for key in
                                         ("tree_len", "kind", "split", "leaf", "cls", "cnt")})
                   for fi in range(n_forests)]
        yield dict(name=str(name), ims=z[k + "ims"], bins=bins, row_from=row_from, row_to=row_to, forests=forests,
                   rows=z[k + "rows"], expected=z[k + "expected"])


def normalised_rows(c):
    H = c["ims"].shape[1]
    r0 = 0 if c["row_from"] < 0 else c["row_from"]
    r1 = H if (c["row_to"] < 0 or c["row_to"] > H) else c["row_to"]
    return r0, r1


def same_bits(a, b):
    """bit-identical, except that any NaN matches any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int32), b[~nb].view(np.int32))


@pytest.mark.parametrize("case", list(golden_cases()), ids=lambda c: c["name"])
def test_restatement_matches_reference_fixture(case):
    r0, r1 = normalised_rows(case)
    out = R.eval_rows([case["forests"][i] for i in case["rows"]], 0, case["ims"], case["bins"], r0, r1)
    assert same_bits(out[:, r0:r1], case["expected"])
    assert np.isnan(out[:, :r0]).all() and np.isnan(out[:, r1:]).all()


def test_fixture_covers_the_cases():
    names = [c["name"] for c in golden_cases()]
    assert names == ["clamp_offsets", "shapes", "zero_rules", "ties", "subrange", "realistic"]
    cases = {c["name"]: c for c in golden_cases()}
    assert np.isnan(cases["zero_rules"]["expected"][..., 1]).any()          # an all-zero leaf set
    thr = np.concatenate([R.forest_to_arrays(f)["split"][:, 0] for f in cases["clamp_offsets"]["forests"]])
    thr = thr.view(np.float32)
    assert np.isnan(thr).any() and (thr == np.inf).any() and (thr == -np.inf).any()
    real = cases["realistic"]["forests"][0]
    assert len(real.trees) == 6
    lens = [len(nd.classes) for t in real.trees for nd in t if isinstance(nd, hd.Leaf)]
    assert 100 <= min(lens) and max(lens) <= 300 and len(lens) == 6 * 256


def test_save_after_load_is_byte_identical(tmp_path):
    for c in golden_cases():
        for f in c["forests"]:
            p, q = tmp_path / "a.bin", tmp_path / "b.bin"
            hd.save_forest(f, p)
            hd.save_forest(hd.load_forest(p), q)
            assert p.read_bytes() == q.read_bytes()


def test_nan_threshold_bits_survive(tmp_path):
    C = 4
    lf = hd.Leaf(C, C, np.array([1], np.int32), np.array([2], np.int32), 2)
    payload = np.array([0x7fc01234], np.int32).view(np.float32)[0]
    s = hd.Split(payload, 0, 0, 1, 2, 3, 4, 1, 2)
    p = tmp_path / "f.bin"
    hd.save_forest(hd.Forest([[s, lf, lf]]), p)
    raw = p.read_bytes()
    assert raw[8:12] == struct.pack("<i", 1) and raw[12:16] == struct.pack("<I", 0x7fc01234)
    back = hd.load_forest(p)
    assert np.asarray(back.trees[0][0].threshold).view(np.int32) == 0x7fc01234


def _leaf(C, cls=(0,), cnt=(1,)):
    return hd.Leaf(C, C, np.array(cls, np.int32), np.array(cnt, np.int32), int(sum(cnt)))


def _write(path, forest):
    hd.save_forest(forest, path)
    return path


def test_loader_rejections(tmp_path):
    p = tmp_path / "f.bin"
    ok = hd.Forest([[hd.Split(np.float32(0), 0, 0, 1, 2, 3, 4, 1, 2), _leaf(8), _leaf(8, (3,), (2,))]])
    hd.load_forest(_write(p, ok))
    raw = p.read_bytes()
    with pytest.raises(hd.ForestFormatError, match="unknown node type"):
        p.write_bytes(raw[:8] + struct.pack("<i", 2) + raw[12:])
        hd.load_forest(p)
    with pytest.raises(hd.ForestFormatError, match="truncated"):
        p.write_bytes(raw[:-3])
        hd.load_forest(p)
    with pytest.raises(hd.ForestFormatError, match="trailing"):
        p.write_bytes(raw + b"\0")
        hd.load_forest(p)
    with pytest.raises(hd.ForestFormatError, match="without trees"):
        p.write_bytes(struct.pack("<Q", 0))
        hd.load_forest(p)
    with pytest.raises(hd.ForestFormatError, match="class counts"):          # unequal n_counts in one forest
        hd.load_forest(_write(p, hd.Forest([[hd.Split(np.float32(0), 0, 0, 1, 2, 3, 4, 1, 2), _leaf(8), _leaf(9)]])))
    with pytest.raises(hd.ForestFormatError, match="classes per leaf"):      # C == 0
        hd.load_forest(_write(p, hd.Forest([[hd.Leaf(0, 0, np.zeros(0, np.int32), np.zeros(0, np.int32), 0)]])))
    with pytest.raises(hd.ForestFormatError, match="classes per leaf"):      # C == 1: defined there, unsupported here
        hd.load_forest(_write(p, hd.Forest([[_leaf(1)]])))
    with pytest.raises(hd.ForestFormatError, match="negative"):
        hd.load_forest(_write(p, hd.Forest([[_leaf(8, (1, 2), (3, -1))]])))
    with pytest.raises(hd.ForestFormatError, match="2\\^20"):
        hd.load_forest(_write(p, hd.Forest([[hd.Split(np.float32(0), 0, 0, 1, 2, -(1 << 20) - 1, 4, 1, 2), _leaf(8),
                                             _leaf(8)]])))
    hd.load_forest(_write(p, hd.Forest([[hd.Split(np.float32(0), 0, 0, 1 << 20, 2, -(1 << 20), 4, 1, 2), _leaf(8),
                                         _leaf(8)]])))
    with pytest.raises(hd.ForestFormatError, match="overflow|2\\^31"):
        big = _leaf(8, (1,), (1 << 30,))
        hd.load_forest(_write(p, hd.Forest([[big], [big]])))


def test_rows_must_agree_on_the_class_count():
    a, b = hd.Forest([[_leaf(8)]]), hd.Forest([[_leaf(10)]])
    with pytest.raises(hd.ForestFormatError, match="disagree"):
        hd.HyperDepthForests([a, b], 0, "cuda:0")


def test_flatten_layout():
    C = 8
    f = hd.Forest([[hd.Split(np.float32(1.5), 7, 9, 1, 2, 3, 4, 1, 2), _leaf(C, (1, 5), (2, 3)), _leaf(C, (0,), (4,))],
                   [_leaf(C, (7,), (1,))]])
    fl = hd.flatten(f)
    assert fl["nodes"].tolist() == [[int(np.float32(1.5).view(np.int32)), 1, 3, 2, 4, ~0, ~1, 0]]
    assert fl["roots"].tolist() == [0, ~2]
    assert fl["lens"].tolist() == [2, 1, 1] and fl["sums"].tolist() == [5, 4, 1]
    assert fl["entries"].tolist() == [[1, 2], [5, 3], [0, 4], [7, 1]]
    assert fl["max_depth"] == 1


# ------------------------------------------------------------------------------------------------------------------
# C ABI
# ------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_bound():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "ctd_hyperdepth_eval_f32")
    assert "ctd_hyperdepth_eval_f32" in _lib.SIGNATURES
    assert _lib.lib().ctd_version() == 5
    assert ctypes.sizeof(_lib.HdTables) == 88


class _Buf:
    """a host buffer standing in for device pointers: validation must reject before it is ever dereferenced"""

    def __init__(self, n):
        self.raw = ctypes.create_string_buffer(n + 512)
        self.ptr = (ctypes.addressof(self.raw) + 255) // 256 * 256


def test_validation_needs_no_gpu():
    L = _lib.lib()
    buf = _Buf(4096)
    p = buf.ptr

    def tables(**kw):
        d = dict(nodes=p, roots=p, leaf_off=p, leaf_sum=p, entries=p, n_nodes=1, n_leaves=2, n_entries=3, row0=0,
                 n_rows=8, n_trees=6, n_classes=6400, max_depth=8, reserved=0)
        d.update(kw)
        return _lib.HdTables(**d)

    def call(tab=None, ims=p, N=1, H=8, W=16, row_from=0, row_to=8, bins=10, out=p):
        return L.ctd_hyperdepth_eval_f32(ctypes.byref(tab if tab is not None else tables()), ims, N, H, W, row_from,
                                         row_to, bins, out, -1, None)

    assert L.ctd_hyperdepth_eval_f32(None, p, 1, 8, 16, 0, 8, 10, p, -1, None) == 1
    assert call(N=-1) == 1
    assert call(H=0) == 1 and call(W=0) == 1 and call(H=1 << 24, row_to=1) == 1
    assert call(row_from=-1) == 1 and call(row_from=5, row_to=4) == 1 and call(row_to=9) == 1
    assert call(tab=tables(row0=1)) == 1                           # rows [0, 8) requested, tables hold [1, 9)
    assert call(tab=tables(n_rows=7)) == 1
    assert call(tab=tables(n_trees=0)) == 1 and call(tab=tables(n_trees=17)) == 1
    assert call(tab=tables(n_classes=1)) == 1
    assert call(bins=0) == 1
    assert call(tab=tables(n_nodes=-1)) == 1 and call(tab=tables(n_entries=-1)) == 1
    assert call(tab=tables(max_depth=-1)) == 1
    assert call(ims=None) == 1 and call(out=None) == 1
    assert call(tab=tables(roots=None)) == 1 and call(tab=tables(leaf_off=None)) == 1
    assert call(tab=tables(nodes=None)) == 1 and call(tab=tables(entries=None)) == 1
    assert call(tab=tables(nodes=p + 8)) == 1                      # nodes are read as 16-byte pairs
    assert call(tab=tables(entries=p + 4)) == 1
    assert call(tab=tables(n_classes=16384 - 6 * 256 + 1)) == 3    # the LDS histogram does not fit 64 KiB
    assert call(N=0) == 0                                          # nothing to do: no HIP call
    assert call(N=0, row_from=3, row_to=3, tab=tables(row0=100, n_rows=0)) == 0   # an empty range needs no forest
    assert call(N=0, tab=tables(nodes=None, n_nodes=0, entries=None, n_entries=0)) == 0


def test_python_surface_checks():
    with pytest.raises(Exception, match="ims.shape != disps.shape"):
        hd.eval_forest(np.zeros((1, 4, 5), np.uint8), np.zeros((1, 4, 6), np.float32))
    with pytest.raises(ValueError):
        hd.eval_forest(np.zeros((1, 4, 5), np.float32), np.zeros((1, 4, 5), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        hd.HyperDepthForests.from_prefix("nowhere", [3, 5])
