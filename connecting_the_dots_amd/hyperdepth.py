"""HyperDepth random-forest disparity evaluation and training on the device.

The reference's `hyperdepth/` module (the random-forest baseline the paper compares against) trains one forest per
image row and evaluates it on the CPU: hyperdepth.h:253-287 `eval`, through rf/forest.h `inferencemt`.  Here:

    load_forest(path) / save_forest(forest, path)         the reference's binary forest file (rf/serialization.h)
    HyperDepthForests.from_prefix(prefix, rows, device)   packs the forests of a row range into device tables, once
    forests.eval(ims, n_disp_bins, row_from, row_to)      -> [N, H, W, 3] f32 (disp, prob, |disp - disp2|), one launch
    eval_forest(ims, disps, ...)                          drop-in for hyperdepth.pyx `eval_forest` (numpy in and out)
    HyperDepthForests.train(ims, disps, TrainParams(), ...)  trains the forests of a row range on the device
    forests.to_forests()                                  -> the host Forest list (file pre-order), for save_forest
    train_forest(params, ims, disps, ...)                 drop-in for hyperdepth.pyx `train_forest` (numpy in, files out)

The kernel is ctd_hyperdepth_eval_f32 (include/ctd_hip.h states the semantics and the table layout); its output is
bit-identical to the reference's.  Differences from the reference, all on inputs it leaves undefined or that this
port does not support:
  - rows outside [row_from, row_to) are NaN (the reference returns them uninitialised, np.empty);
  - the loader raises on: an unknown node type, a forest without trees, leaves of one forest with different class
    counts, fewer than 2 classes, negative counts, split offsets beyond 2^20, per-pixel count sums that could overflow
    an int32, a truncated file or trailing bytes; `from_prefix` raises when the rows' class counts disagree;
  - training draws its randomness from a counter-based generator keyed by a seed (the reference seeds std::mt19937
    from std::random_device), and scores a split with an exact int64 entropy cost; include/ctd_hip.h
    (ctd_hyperdepth_train_f32) states the whole contract, tests/hyperdepth_train_ref.py restates it in numpy.
    Trained forests therefore differ from the reference's run by run, as its own runs differ from each other;
    tests/test_hyperdepth_train_gpu.py compares their held-out quality with recorded reference runs.
There is no CPU path: a missing library or GPU is an error.
"""
import ctypes
import struct
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

PATCH_HALF = 16            # RawSample::at: the reference's 32 x 32 patch is centred on the pixel (hyperdepth.h:190)
MAX_OFFSET = 1 << 20       # |h|, |w| beyond this are rejected (the reference's int arithmetic could overflow)
MAX_TREES = 16             # kernel limit (ctd_hyperdepth_eval_f32)
MAX_TRAIN_DEPTH = 24       # ctd_hyperdepth_train_f32 limits
MAX_TEST_SAMPLES = 8192
INT32_MAX = (1 << 31) - 1
_I4 = np.dtype("<i4")


@dataclass
class Split:
    """SplitFunctionPixelDifference (rf/splitfcn.h): left iff v(h0, w0) - v(h1, w1) < threshold.  `threshold` keeps
    the file's f32 bits (NaN payloads included); `left` / `right` index the tree's node list."""
    threshold: np.float32
    c0: int
    c1: int
    h0: int
    h1: int
    w0: int
    w1: int
    left: int = -1
    right: int = -1


@dataclass
class Leaf:
    """HyperdepthLeafFunction (hyperdepth.h:51-160) as a class-sorted sparse list: counts[classes[i]] = counts_[i],
    every other of the n_counts dense counts is zero.  n_classes and sum_counts are kept for the file only."""
    n_classes: int
    n_counts: int
    classes: np.ndarray     # int32, strictly increasing
    counts: np.ndarray      # int32, non-zero
    sum_counts: int


@dataclass
class Forest:
    """trees[t] is tree t's node list in the file's pre-order; node 0 is the root."""
    trees: list


class ForestFormatError(ValueError):
    pass


# ------------------------------------------------------------------------------------------------------------------
# file format
# ------------------------------------------------------------------------------------------------------------------
def _parse(buf, path):
    pos = 0
    size = len(buf)

    def take(n):
        nonlocal pos
        if pos + n > size:
            raise ForestFormatError("%s: truncated at byte %d" % (path, pos))
        p = pos
        pos += n
        return p

    (n_trees,) = struct.unpack_from("<Q", buf, take(8))
    if n_trees == 0:
        raise ForestFormatError("%s: a forest without trees (the reference reduces fcns[0])" % path)
    if n_trees > (size - 8) // 4:
        raise ForestFormatError("%s: %d trees do not fit the file" % (path, n_trees))
    trees = []
    for _ in range(n_trees):
        nodes = []
        # explicit stack of (parent index, side); the root has no parent
        stack = [(-1, None)]
        while stack:
            parent, side = stack.pop()
            (typ,) = struct.unpack_from("<i", buf, take(4))
            idx = len(nodes)
            if parent >= 0:
                setattr(nodes[parent], side, idx)
            if typ == 1:
                p = take(28)
                thr = np.frombuffer(buf, "<f4", 1, p)[0]
                c0, c1, h0, h1, w0, w1 = struct.unpack_from("<6i", buf, p + 4)
                nodes.append(Split(thr, c0, c1, h0, h1, w0, w1))
                stack.append((idx, "right"))    # pre-order: the left subtree is read first
                stack.append((idx, "left"))
            elif typ == 0:
                n_classes, n_counts = struct.unpack_from("<2i", buf, take(8))
                if n_counts < 0:
                    raise ForestFormatError("%s: negative class count %d" % (path, n_counts))
                p = take(4 * n_counts)
                dense = np.frombuffer(buf, _I4, n_counts, p)
                (sum_counts,) = struct.unpack_from("<i", buf, take(4))
                cls = np.nonzero(dense)[0].astype(np.int32)
                nodes.append(Leaf(n_classes, n_counts, cls, dense[cls].astype(np.int32), sum_counts))
            else:
                raise ForestFormatError("%s: unknown node type %d at byte %d" % (path, typ, pos - 4))
        trees.append(nodes)
    if pos != size:
        raise ForestFormatError("%s: %d trailing bytes after the forest" % (path, size - pos))
    return Forest(trees)


def validate(forest, what="forest"):
    """The checks of load_forest on a Forest built in memory; returns the class count C."""
    C = None
    total = 0
    for nodes in forest.trees:
        best = 0
        for nd in nodes:
            if isinstance(nd, Split):
                if max(abs(nd.h0), abs(nd.h1), abs(nd.w0), abs(nd.w1)) > MAX_OFFSET:
                    raise ForestFormatError("%s: split offset beyond 2^20 (%d, %d, %d, %d)" %
                                            (what, nd.h0, nd.h1, nd.w0, nd.w1))
                continue
            if C is None:
                C = nd.n_counts
            elif nd.n_counts != C:
                raise ForestFormatError("%s: leaves with %d and %d class counts (the reference's Reduce indexes past "
                                        "the shorter one)" % (what, C, nd.n_counts))
            if len(nd.counts) and int(nd.counts.min()) < 0:
                raise ForestFormatError("%s: negative leaf count" % what)
            s = int(nd.counts.astype(np.int64).sum())
            best = max(best, s)
        total += best
    if not forest.trees:
        raise ForestFormatError("%s: a forest without trees" % what)
    if C is None or C < 2:
        raise ForestFormatError("%s: %s classes per leaf (at least 2 are supported; 0 is undefined in the reference, "
                                "1 gives it pos2 = -1)" % (what, C))
    if total > INT32_MAX:
        raise ForestFormatError("%s: the summed leaf counts of one pixel can exceed 2^31 - 1 (int overflow in the "
                                "reference)" % what)
    return C


def load_forest(path):
    """Reads one forest file written by the reference's BinarySerializationOut (or save_forest)."""
    with open(path, "rb") as f:
        buf = f.read()
    forest = _parse(buf, path)
    validate(forest, path)
    return forest


def forest_bytes(forest):
    """The file image of `forest`: rf/serialization.h BinarySerializationOut, pre-order, dense leaf counts."""
    out = [struct.pack("<Q", len(forest.trees))]
    for nodes in forest.trees:
        stack = [0]
        while stack:
            nd = nodes[stack.pop()]
            if isinstance(nd, Split):
                out.append(struct.pack("<i", 1))
                out.append(np.asarray(nd.threshold, "<f4").tobytes())
                out.append(struct.pack("<6i", nd.c0, nd.c1, nd.h0, nd.h1, nd.w0, nd.w1))
                stack.append(nd.right)
                stack.append(nd.left)
            else:
                dense = np.zeros(nd.n_counts, _I4)
                dense[np.asarray(nd.classes, np.int64)] = nd.counts
                out.append(struct.pack("<3i", 0, nd.n_classes, nd.n_counts))
                out.append(dense.tobytes())
                out.append(struct.pack("<i", nd.sum_counts))
    return b"".join(out)


def save_forest(forest, path):
    """Writes `forest` in the reference's format; save_forest(load_forest(p), q) reproduces p byte for byte.
    Nothing is validated here, so that malformed files can be written on purpose."""
    with open(path, "wb") as f:
        f.write(forest_bytes(forest))


# ------------------------------------------------------------------------------------------------------------------
# device tables (layout: ctd_hd_tables of include/ctd_hip.h)
# ------------------------------------------------------------------------------------------------------------------
HdTables = _lib.HdTables


def flatten(forest):
    """One forest as flat arrays with forest-local indices: nodes [n, 8] int32 (threshold bits, h0, w0, h1, w1, left,
    right, 0), roots [T] int32, leaf lengths / sums, entries [E, 2] int32 (class, count), the longest path in splits.
    A child or root value v >= 0 is a node, v < 0 is leaf ~v."""
    nodes, roots, lens, sums, ents = [], [], [], [], []
    max_depth = 0
    for tree in forest.trees:
        nmap, lmap = {}, {}
        for i, nd in enumerate(tree):
            if isinstance(nd, Split):
                nmap[i] = len(nodes) + len(nmap)
            else:
                lmap[i] = len(lens) + len(lmap)
        ref = lambda i: nmap[i] if i in nmap else ~lmap[i]          # noqa: E731
        depth = {0: 0}
        for i, nd in enumerate(tree):                               # pre-order: a parent precedes its children
            if isinstance(nd, Split):
                thr = int(np.asarray(nd.threshold, "<f4").view("<i4"))
                nodes.append((thr, nd.h0, nd.w0, nd.h1, nd.w1, ref(nd.left), ref(nd.right), 0))
                depth[nd.left] = depth[nd.right] = depth[i] + 1
            else:
                lens.append(len(nd.classes))
                sums.append(int(nd.counts.astype(np.int64).sum()))
                ents.append(np.stack([np.asarray(nd.classes, np.int32), np.asarray(nd.counts, np.int32)], 1))
                max_depth = max(max_depth, depth[i])
        roots.append(ref(0))
    return dict(nodes=np.asarray(nodes, np.int32).reshape(-1, 8), roots=np.asarray(roots, np.int32),
                lens=np.asarray(lens, np.int64), sums=np.asarray(sums, np.int32),
                entries=np.concatenate(ents).reshape(-1, 2).astype(np.int32), max_depth=max_depth)


def _shift(v, node_base, leaf_base):
    return np.where(v >= 0, v + node_base, v - leaf_base).astype(np.int32)


class HyperDepthForests:
    """The forests of rows [row0, row0 + n_rows), packed once into device tables (ctd_hd_tables).  Rows with fewer
    trees than the most are padded with an empty leaf, which adds nothing to any sum.  Reusable across calls."""

    def __init__(self, forests, row0, device=None):
        forests = list(forests)
        if not forests:
            raise ValueError("no forests")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("HyperDepthForests lives on a GPU device, got %s" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        Cs = {validate(f, "row %d" % (row0 + i)) for i, f in enumerate(forests)}
        if len(Cs) != 1:
            raise ForestFormatError("rows disagree on the class count (%s): not supported" % sorted(Cs))
        T = max(len(f.trees) for f in forests)
        if T > MAX_TREES:
            raise ForestFormatError("%d trees per forest; the kernel supports at most %d" % (T, MAX_TREES))
        flat_cache = {}
        nodes, roots, lens, sums, ents = [], [], [np.zeros(1, np.int64)], [np.zeros(1, np.int32)], []
        n_nodes, n_leaves, max_depth = 0, 1, 0            # leaf 0 is the empty padding leaf
        for f in forests:
            fl = flat_cache.get(id(f))
            if fl is None:
                fl = flat_cache[id(f)] = flatten(f)
            nd = fl["nodes"].copy()
            nd[:, 5] = _shift(nd[:, 5], n_nodes, n_leaves)
            nd[:, 6] = _shift(nd[:, 6], n_nodes, n_leaves)
            r = np.full(T, ~0, np.int32)
            r[:len(fl["roots"])] = _shift(fl["roots"], n_nodes, n_leaves)
            nodes.append(nd)
            roots.append(r)
            lens.append(fl["lens"])
            sums.append(fl["sums"])
            ents.append(fl["entries"])
            n_nodes += len(nd)
            n_leaves += len(fl["lens"])
            max_depth = max(max_depth, fl["max_depth"])
        lens = np.concatenate(lens)
        off = np.zeros(len(lens) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        host = dict(nodes=np.concatenate(nodes).reshape(-1, 8), roots=np.stack(roots), leaf_off=off,
                    leaf_sum=np.concatenate(sums), entries=np.concatenate(ents).reshape(-1, 2))
        self.device = dev
        self.row0, self.n_rows, self.n_trees, self.n_classes, self.max_depth = row0, len(forests), T, Cs.pop(), max_depth
        self.tensors = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in host.items()}
        t = self.tensors
        ptr = lambda x: x.data_ptr() if x.numel() else None     # noqa: E731
        self._tables = HdTables(ptr(t["nodes"]), t["roots"].data_ptr(), t["leaf_off"].data_ptr(),
                                t["leaf_sum"].data_ptr(), ptr(t["entries"]), len(host["nodes"]), len(lens),
                                len(host["entries"]), row0, self.n_rows, T, self.n_classes, max_depth, 0)

    @classmethod
    def from_prefix(cls, prefix, rows, device=None):
        """Loads `<prefix><row>.bin` for every row of `rows` (a contiguous ascending range of rows)."""
        rows = [int(r) for r in rows]
        if not rows or rows != list(range(rows[0], rows[0] + len(rows))):
            raise ValueError("rows must be a non-empty contiguous ascending range")
        return cls([load_forest("%s%d.bin" % (prefix, r)) for r in rows], rows[0], device)

    @property
    def entry_bytes(self):
        return self.tensors["entries"].numel() * 4

    def eval(self, ims, n_disp_bins=10, row_from=-1, row_to=-1, out=None):
        """ims: uint8 [N, H, W] on the tables' device -> [N, H, W, 3] f32 (disp, prob, |disp - disp2|), launched on
        the current stream.  row_from / row_to as the reference: < 0 -> 0, < 0 or > H -> H.  Every row of the range
        needs a forest here; rows outside it are NaN."""
        if not (isinstance(ims, torch.Tensor) and ims.dtype == torch.uint8 and ims.dim() == 3):
            raise ValueError("ims must be a uint8 tensor [N, H, W]")
        if ims.device != self.device:
            raise RuntimeError("ims is on %s, the forests on %s" % (ims.device, self.device))
        ims = ims.contiguous()
        N, H, W = ims.shape
        row_from = 0 if row_from < 0 else row_from
        row_to = H if (row_to > H or row_to < 0) else row_to
        row_from = min(row_from, row_to)                 # an empty range evaluates nothing, as the reference's loop
        if row_from < row_to and (row_from < self.row0 or row_to > self.row0 + self.n_rows):
            raise ValueError("rows [%d, %d) requested, forests loaded for [%d, %d)" %
                             (row_from, row_to, self.row0, self.row0 + self.n_rows))
        if out is None:
            out = torch.empty((N, H, W, 3), dtype=torch.float32, device=self.device)
        elif not (out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (N, H, W, 3)
                  and out.device == self.device):
            raise ValueError("out must be a contiguous f32 tensor [N, H, W, 3] on %s" % self.device)
        st = _lib.lib().ctd_hyperdepth_eval_f32(ctypes.byref(self._tables), ims.data_ptr(), N, H, W,
                                                row_from, row_to, int(n_disp_bins), out.data_ptr(), self.device.index,
                                                torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(st, "hyperdepth eval")
        return out


def eval_forest(ims, disps, n_disp_bins=10, depth_switch=0, n_threads=18, forest_prefix="forest", row_from=-1,
                row_to=-1):
    """Drop-in for the reference's hyperdepth.pyx `eval_forest`: numpy uint8 [N, H, W] in, f32 [N, H, W, 3] out.
    `disps` is only shape-checked (as there); depth_switch and n_threads are accepted and ignored.  Runs on the
    current GPU; rows outside [row_from, row_to) are NaN."""
    ims = np.ascontiguousarray(ims)
    if ims.dtype != np.uint8 or ims.ndim != 3:
        raise ValueError("ims must be uint8 [N, H, W]")
    disps = np.asarray(disps)
    if disps.ndim != 3:
        raise ValueError("disps must be [N, H, W]")
    n, h, w = ims.shape
    if n != disps.shape[0] or h != disps.shape[1] or w != disps.shape[2]:
        raise Exception("ims.shape != disps.shape")
    r0 = 0 if row_from < 0 else row_from
    r1 = h if (row_to > h or row_to < 0) else row_to
    dev = torch.device("cuda", torch.cuda.current_device())
    if r0 >= r1:
        return np.full((n, h, w, 3), np.nan, np.float32)
    forests = HyperDepthForests.from_prefix(forest_prefix, range(r0, r1), dev)
    out = forests.eval(torch.from_numpy(ims).to(dev), n_disp_bins, r0, r1)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------
# training (ctd_hyperdepth_train_f32 of include/ctd_hip.h)
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class TrainParams:
    """hyperdepth.pyx `TrainParams`: the same names and defaults.  print_node_info is accepted and ignored."""
    n_trees: int = 6
    max_tree_depth: int = 8
    n_test_split_functions: int = 50
    n_test_thresholds: int = 10
    n_test_samples: int = 4096
    min_samples_to_split: int = 16
    min_samples_for_leaf: int = 8
    print_node_info: int = 100

    def __str__(self):
        return ("n_trees=%d, max_tree_depth=%d, n_test_split_functions=%d, n_test_thresholds=%d, n_test_samples=%d, "
                "min_samples_to_split=%d, min_samples_for_leaf=%d" %
                (self.n_trees, self.max_tree_depth, self.n_test_split_functions, self.n_test_thresholds,
                 self.n_test_samples, self.min_samples_to_split, self.min_samples_for_leaf))


def x_log_x_table(n):
    """The contract's cost table X[0..n]: int64(rint(x * log(x) * 2^32)), X[0] = X[1] = 0, in float64 on the host."""
    x = np.arange(n + 1, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = x * np.log(x) * 2.0 ** 32
    v[:2] = 0
    return np.rint(v).astype(np.int64)


def check_train_args(params, N, H, W, n_disp_bins, row_from, row_to):
    """The restrictions of ctd_hyperdepth_train_f32, as ValueError; returns the row range."""
    p = params
    lim = [("n_trees", p.n_trees, 1, MAX_TREES), ("max_tree_depth", p.max_tree_depth, 0, MAX_TRAIN_DEPTH),
           ("n_test_split_functions", p.n_test_split_functions, 0, (1 << 20) - 1),
           ("n_test_thresholds", p.n_test_thresholds, 0, (1 << 16) - 1),
           ("n_test_samples", p.n_test_samples, 1, MAX_TEST_SAMPLES),
           ("min_samples_to_split", p.min_samples_to_split, 0, INT32_MAX),
           ("min_samples_for_leaf", p.min_samples_for_leaf, 1, INT32_MAX)]
    for name, v, lo, hi in lim:
        if not (isinstance(v, (int, np.integer)) and lo <= v <= hi):
            raise ValueError("%s = %r: must be an integer in [%d, %d]" % (name, v, lo, hi))
    if not (isinstance(n_disp_bins, (int, np.integer)) and n_disp_bins >= 1):
        raise ValueError("n_disp_bins must be >= 1")
    if W * n_disp_bins > INT32_MAX:
        raise ValueError("W * n_disp_bins must be below 2^31")
    if min(N, H, W) < 1 or H >= 1 << 24 or W >= 1 << 24 or N * H * W > INT32_MAX:
        raise ValueError("ims [N, H, W] must be non-empty, H, W < 2^24 and N * H * W < 2^31")
    r0 = 0 if row_from < 0 else row_from
    r1 = H if (row_to > H or row_to < 0) else row_to
    if r0 >= r1:
        raise ValueError("empty row range [%d, %d)" % (r0, r1))
    return r0, r1


def _train(cls, ims, disps, params, n_disp_bins=10, depth_switch=0, row_from=-1, row_to=-1, seed=0, device=None):
    """HyperDepthForests.train: see there."""
    if not (isinstance(ims, torch.Tensor) and ims.dtype == torch.uint8 and ims.dim() == 3):
        raise ValueError("ims must be a uint8 tensor [N, H, W]")
    if not (isinstance(disps, torch.Tensor) and disps.dtype == torch.float32 and disps.shape == ims.shape):
        raise ValueError("disps must be a float32 tensor of the shape of ims")
    dev = ims.device if device is None else torch.device(device)
    if dev.type != "cuda" or ims.device != dev or disps.device != dev:
        raise RuntimeError("ims and disps must live on one GPU device")
    N, H, W = ims.shape
    r0, r1 = check_train_args(params, N, H, W, n_disp_bins, row_from, row_to)
    R, T, D = r1 - r0, params.n_trees, params.max_tree_depth
    ims, disps = ims.contiguous(), disps.contiguous()
    L = _lib.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    counts_d = torch.empty(R, dtype=torch.int64, device=dev)
    _lib.check(L.ctd_hyperdepth_train_count_f32(disps.data_ptr(), N, H, W, r0, r1, int(n_disp_bins),
                                                 counts_d.data_ptr(), dev.index, stream), "hyperdepth train count")
    counts = counts_d.cpu().numpy()
    splits = sum(T * min((1 << D) - 1, max(int(n) - 1, 0)) for n in counts)
    cap_nodes, cap_leaves, cap_entries = splits, splits + R * T, T * int(counts.sum())
    p = _lib.HdTrainParams(T, D, params.n_test_split_functions, params.n_test_thresholds, params.n_test_samples,
                           params.min_samples_to_split, params.min_samples_for_leaf, int(depth_switch),
                           int(n_disp_bins), 0, int(seed) & ((1 << 64) - 1))
    counts_h = np.ascontiguousarray(counts, np.int64)
    ws_bytes = L.ctd_hyperdepth_train_workspace_bytes(ctypes.byref(p), R, counts_h.ctypes.data, cap_leaves)
    if ws_bytes == 0:
        raise ValueError("hyperdepth train: arguments refused")
    t = {"nodes": torch.empty((max(cap_nodes, 1), 8), dtype=torch.int32, device=dev),
         "roots": torch.empty((R, T), dtype=torch.int32, device=dev),
         "leaf_off": torch.empty(cap_leaves + 1, dtype=torch.int64, device=dev),
         "leaf_sum": torch.empty(cap_leaves, dtype=torch.int32, device=dev),
         "entries": torch.empty((max(cap_entries, 1), 2), dtype=torch.int32, device=dev)}
    used = torch.zeros(5, dtype=torch.int64, device=dev)
    X = torch.from_numpy(x_log_x_table(params.n_test_samples)).to(dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = _lib.HdTrainOut(t["nodes"].data_ptr(), t["roots"].data_ptr(), t["leaf_off"].data_ptr(),
                          t["leaf_sum"].data_ptr(), t["entries"].data_ptr(), used.data_ptr(), cap_nodes, cap_leaves,
                          cap_entries)
    _lib.check(L.ctd_hyperdepth_train_f32(ctypes.byref(p), X.data_ptr(), X.numel(), ims.data_ptr(), disps.data_ptr(),
                                          N, H, W, r0, r1, counts_h.ctypes.data, ws.data_ptr(), ws_bytes,
                                          ctypes.byref(out), dev.index, stream), "hyperdepth train")
    n_nodes, n_leaves, n_entries, max_depth, err = (int(v) for v in used.cpu())
    if err:
        raise RuntimeError("hyperdepth train: output capacity exceeded (a bound of include/ctd_hip.h failed)")
    t["nodes"], t["leaf_off"] = t["nodes"][:n_nodes], t["leaf_off"][:n_leaves + 1]
    t["leaf_sum"], t["entries"] = t["leaf_sum"][:n_leaves], t["entries"][:n_entries]
    return cls._from_tables(t, r0, T, W * int(n_disp_bins), max_depth, dev)


def _from_tables(cls, tensors, row0, n_trees, n_classes, max_depth, device):
    """A HyperDepthForests over device tables already in the ctd_hd_tables layout (a training call's output)."""
    self = cls.__new__(cls)
    self.device = device
    self.row0, self.n_rows, self.n_trees = row0, tensors["roots"].shape[0], n_trees
    self.n_classes, self.max_depth = n_classes, max_depth
    self.tensors = tensors
    ptr = lambda x: x.data_ptr() if x.numel() else None     # noqa: E731
    self._tables = HdTables(ptr(tensors["nodes"]), tensors["roots"].data_ptr(), tensors["leaf_off"].data_ptr(),
                            ptr(tensors["leaf_sum"]), ptr(tensors["entries"]), tensors["nodes"].shape[0],
                            tensors["leaf_sum"].shape[0], tensors["entries"].shape[0], row0, self.n_rows, n_trees,
                            n_classes, max_depth, 0)
    return self


def _to_forests(self):
    """The host Forest of every row, trees in the file's pre-order, leaves with the header n_classes_ = -1 and
    n_counts = the class count: what the reference's trainer writes (save_forest gives its file)."""
    h = {k: v.cpu().numpy() for k, v in self.tensors.items()}
    nodes, off, sums, ents = h["nodes"], h["leaf_off"], h["leaf_sum"], h["entries"]
    forests = []
    for r in range(self.n_rows):
        trees = []
        for t in range(self.n_trees):
            lst = []

            def emit(v):
                me = len(lst)
                if v < 0:
                    leaf = ~int(v)
                    e = ents[off[leaf]:off[leaf + 1]]
                    lst.append(Leaf(-1, self.n_classes, e[:, 0].astype(np.int32), e[:, 1].astype(np.int32),
                                    int(sums[leaf])))
                    return me
                nd = nodes[v]
                s = Split(np.int32(nd[0]).view(np.float32), 0, 0, int(nd[1]), int(nd[3]), int(nd[2]), int(nd[4]))
                lst.append(s)
                s.left = emit(nd[5])
                s.right = emit(nd[6])
                return me

            emit(h["roots"][r, t])
            trees.append(lst)
        forests.append(Forest(trees))
    return forests


HyperDepthForests.train = classmethod(_train)
HyperDepthForests.train.__func__.__doc__ = """Trains the forests of rows [row_from, row_to) (the reference's clamping)
    from uint8 ims and f32 disps [N, H, W] on one GPU, on the current stream, and returns them as device tables ready
    for `.eval`.  params: TrainParams; the result is an exact function of the inputs and `seed` (include/ctd_hip.h,
    ctd_hyperdepth_train_f32).  Raises ValueError on the contract's restrictions, before any launch."""
HyperDepthForests._from_tables = classmethod(_from_tables)
HyperDepthForests.to_forests = _to_forests


def train_forest(params, ims, disps, n_disp_bins=10, depth_switch=0, n_threads=18, forest_prefix="forest",
                 row_from=-1, row_to=-1, seed=0):
    """Drop-in for the reference's hyperdepth.pyx `train_forest`: numpy uint8 ims and f32 disps [N, H, W] in,
    `<forest_prefix><row>.bin` out for every trained row.  n_threads is accepted and ignored; `seed` keys the
    generator.  Runs on the current GPU."""
    ims = np.ascontiguousarray(ims)
    disps = np.ascontiguousarray(disps)
    if ims.dtype != np.uint8 or ims.ndim != 3 or disps.dtype != np.float32 or disps.ndim != 3:
        raise ValueError("ims must be uint8 [N, H, W] and disps float32 [N, H, W]")
    if ims.shape != disps.shape:
        raise Exception("ims.shape != disps.shape")
    dev = torch.device("cuda", torch.cuda.current_device())
    forests = HyperDepthForests.train(torch.from_numpy(ims).to(dev), torch.from_numpy(disps).to(dev), params,
                                      n_disp_bins, depth_switch, row_from, row_to, seed, dev)
    for r, f in enumerate(forests.to_forests()):
        save_forest(f, "%s%d.bin" % (forest_prefix, forests.row0 + r))
    return forests
