"""Generate tests/golden/hyperdepth.npz by running the reference's HyperDepth `eval_forest` (build machine only).

    python tests/golden/make_golden_hyperdepth.py <reference checkout>

The reference's hyperdepth/hyperdepth.pyx is cythonized as C++ into a temporary directory and compiled there with
g++ -O3 -std=c++11 -fopenmp against the checkout's hyperdepth/ headers; nothing of it is copied.  The forests are
written with this project's save_forest (the reference's trainer seeds itself from std::random_device and has no
reproducible output), the reference's eval_forest reads them back and evaluates.  The fixture stores the inputs
(images, the forests in the sparse encoding of tests/hyperdepth_ref.py, parameters) and the rows
[row_from, row_to) of the reference's output: the rows outside are uninitialised there (np.empty).
It also records the reference module's wall time on this machine's CPU for the realistic case (key
`ref_seconds_realistic`), which tools/time_hyperdepth.py reports beside the GPU numbers.
"""
import glob
import os
import subprocess
import sys
import sysconfig
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hyperdepth.npz")

from connecting_the_dots_amd.hyperdepth import Forest, Leaf, Split, save_forest  # noqa: E402
from tests import hyperdepth_ref as R  # noqa: E402


def build_reference(ref):
    src = os.path.join(ref, "hyperdepth", "hyperdepth.pyx")
    tmp = tempfile.mkdtemp(prefix="ctd_hyperdepth_ref_")
    cpp = os.path.join(tmp, "hyperdepth.cpp")
    subprocess.check_call(["cython", "--cplus", "-3", src, "-o", cpp])
    so = os.path.join(tmp, "hyperdepth" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call(["g++", "-O3", "-std=c++11", "-fopenmp", "-shared", "-fPIC",
                           "-I" + os.path.join(ref, "hyperdepth"), "-I" + sysconfig.get_paths()["include"],
                           "-I" + np.get_include(), cpp, "-o", so])
    sys.path.insert(0, tmp)
    import hyperdepth
    return hyperdepth


def leaf(C, pairs):
    cls = np.asarray([c for c, _ in pairs], np.int32)
    cnt = np.asarray([n for _, n in pairs], np.int32)
    o = np.argsort(cls)
    return Leaf(C, C, cls[o], cnt[o], int(cnt.sum()))


def split(thr, h0, w0, h1, w1, c0=0, c1=0):
    return Split(np.float32(thr), c0, c1, h0, h1, w0, w1)


def tree(spec):
    """nested tuples -> pre-order node list: (split, left, right) or a Leaf"""
    nodes = []

    def add(s):
        i = len(nodes)
        if isinstance(s, Leaf):
            nodes.append(s)
        else:
            nodes.append(s[0])
            nodes[i].left = add(s[1])
            nodes[i].right = add(s[2])
        return i

    add(spec)
    return nodes


def cases():
    rs = np.random.RandomState(1234)
    out = []

    # 1. H < 32 (both clamps), offsets outside 0..31 (negative ones too), non-zero c0 / c1, NaN and +-inf thresholds
    H, W, bins = 20, 40, 4
    C = W * bins
    fs = []
    for _ in range(3):
        trees = [R.random_tree(rs, 4, C, 6, off_lo=-40, off_hi=72, thr_scale=40.0) for _ in range(3)]
        for nodes in trees:
            for nd in nodes:
                if isinstance(nd, Split):
                    nd.c0, nd.c1 = int(rs.randint(-5, 6)), int(rs.randint(-5, 6))
                    u = rs.rand()
                    if u < 0.1:
                        nd.threshold = np.float32(np.nan)
                    elif u < 0.2:
                        nd.threshold = np.float32(np.inf)
                    elif u < 0.3:
                        nd.threshold = np.float32(-np.inf)
        fs.append(Forest(trees))
    out.append(dict(name="clamp_offsets", ims=rs.randint(0, 256, (2, H, W)).astype(np.uint8), bins=bins,
                    row_from=-1, row_to=-1, forests=fs, rows=[i % 3 for i in range(H)]))

    # 2. a root that is a leaf, trees of unequal depth, single-class leaves, bins 10
    H, W, bins = 24, 30, 10
    C = W * bins
    fs = []
    for _ in range(2):
        trees = [tree(leaf(C, [(int(c), int(rs.randint(1, 5))) for c in rs.choice(C, 4, replace=False)]))]
        trees.append(R.random_tree(rs, 6, C, 3, min_depth=1, one_class=0.5))
        trees.append(R.random_tree(rs, 3, C, 1, one_class=1.0))
        fs.append(Forest(trees))
    out.append(dict(name="shapes", ims=rs.randint(0, 256, (2, H, W)).astype(np.uint8), bins=bins, row_from=-1,
                    row_to=-1, forests=fs, rows=[i % 2 for i in range(H)]))

    # 3. zero rules: all-zero leaf sets (prob NaN), one non-zero class at 0 and elsewhere
    H, W, bins = 12, 33, 4
    C = W * bins
    z = leaf(C, [])
    t0 = tree((split(0, 16, 16, 16, 20), leaf(C, [(0, 3)]), z))
    t1 = tree((split(0, 16, 16, 12, 16), z, (split(10, 16, 16, 16, 8), leaf(C, [(7, 2)]), z)))
    t2 = tree((split(-5, 16, 14, 16, 18), z, leaf(C, [(0, 1), (C - 1, 1)])))
    fs = [Forest([t0, t1]), Forest([t1, t2]), Forest([t0, t2, t1]), Forest([tree(z), tree(z)])]
    out.append(dict(name="zero_rules", ims=rs.randint(0, 256, (3, H, W)).astype(np.uint8), bins=bins, row_from=-1,
                    row_to=-1, forests=fs, rows=[i % 4 for i in range(H)]))

    # 4. exact ties of S across trees, for pos and pos2 (few classes, counts in 1..3)
    H, W, bins = 16, 48, 4
    C = W * bins
    fs = []
    for _ in range(3):
        trees = []
        for _ in range(4):
            nodes = R.random_tree(rs, 3, C, 4)
            for nd in nodes:
                if isinstance(nd, Leaf):
                    cls = np.sort(rs.choice(np.arange(0, C, 37), min(4, len(range(0, C, 37))), replace=False))
                    nd.classes, nd.counts = cls.astype(np.int32), rs.randint(1, 4, len(cls)).astype(np.int32)
                    nd.sum_counts = int(nd.counts.sum())
            trees.append(nodes)
        fs.append(Forest(trees))
    hand = Forest([tree(leaf(C, [(5, 3), (9, 2)])), tree(leaf(C, [(9, 1), (2, 3)])), tree(leaf(C, [(11, 1), (12, 1)]))])
    fs.append(hand)                                  # S[2] = S[5] = S[9] = 3: pos 2, pos2 5
    out.append(dict(name="ties", ims=rs.randint(0, 256, (2, H, W)).astype(np.uint8), bins=bins, row_from=-1,
                    row_to=-1, forests=fs, rows=[i % 4 for i in range(H)]))

    # 5. a row_from / row_to sub-range
    H, W, bins = 40, 50, 10
    C = W * bins
    fs = [R.random_forest(rs, 4, 5, C, 20) for _ in range(2)]
    out.append(dict(name="subrange", ims=rs.randint(0, 256, (2, H, W)).astype(np.uint8), bins=bins, row_from=5,
                    row_to=17, forests=fs, rows=[i % 2 for i in range(H)]))

    # 6. realistic lists: 6 trees, depth 8, leaf lists of 100 .. 300 classes out of C = 960 (one forest, three rows)
    H, W, bins = 36, 96, 10
    C = W * bins
    fs = [R.random_forest(rs, 6, 8, C, 200)]
    out.append(dict(name="realistic", ims=rs.randint(0, 256, (2, H, W)).astype(np.uint8), bins=bins, row_from=14,
                    row_to=17, forests=fs, rows=[0] * H))
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    hdm = build_reference(os.path.abspath(sys.argv[1]))
    store = {}
    names = []
    for ci, c in enumerate(cases()):
        tmp = tempfile.mkdtemp(prefix="ctd_hd_case_")
        prefix = os.path.join(tmp, "forest")
        H = c["ims"].shape[1]
        for r in range(H):
            save_forest(c["forests"][c["rows"][r]], "%s%d.bin" % (prefix, r))
        disps = np.zeros(c["ims"].shape, np.float32)
        t0 = time.time()
        res = hdm.eval_forest(c["ims"], disps, n_disp_bins=c["bins"], depth_switch=0, n_threads=4,
                              forest_prefix=prefix, row_from=c["row_from"], row_to=c["row_to"])
        secs = time.time() - t0
        r0 = 0 if c["row_from"] < 0 else c["row_from"]
        r1 = H if (c["row_to"] < 0 or c["row_to"] > H) else c["row_to"]
        k = "c%d_" % ci
        names.append(c["name"])
        store[k + "ims"] = c["ims"]
        store[k + "params"] = np.asarray([c["bins"], c["row_from"], c["row_to"], len(c["forests"])], np.int64)
        store[k + "rows"] = np.asarray(c["rows"], np.int32)
        store[k + "expected"] = np.asarray(res)[:, r0:r1]
        for fi, f in enumerate(c["forests"]):
            for key, arr in R.forest_to_arrays(f).items():
                store["%sf%d_%s" % (k, fi, key)] = arr
        if c["name"] == "realistic":
            store["ref_seconds_realistic"] = np.asarray([secs, c["ims"].shape[0] * (r1 - r0) * c["ims"].shape[2]])
        for p in glob.glob(prefix + "*.bin"):
            os.remove(p)
        os.rmdir(tmp)
        ex = store[k + "expected"]
        print("%-14s N %d H %d W %d rows [%d, %d)  nan prob %d  %.3f s" %
              (c["name"], *c["ims"].shape, r0, r1, int(np.isnan(ex[..., 1]).sum()), secs))
    store["names"] = np.asarray(names)
    np.savez_compressed(OUT, **store)
    print("wrote %s  %.1f KB" % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
