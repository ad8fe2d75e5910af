"""A numpy restatement of the reference's HyperDepth forest evaluation (hyperdepth.h:253-287), plus the fixture's
sparse forest encoding and a seeded random-forest generator.  Shared by the HyperDepth tests, the fixture generator
and tools/time_hyperdepth.py.

The restatement follows the semantics stated with ctd_hyperdepth_eval_f32 in include/ctd_hip.h, in numpy: the walk
per tree vectorised over a row's pixels, the leaf sums as an exact float64 bincount per distinct leaf tuple, pos / pos2
by np.argmax (first index of the maximum), the outputs in f32 in the reference's operation order.
test_hyperdepth_host.py pins it to the reference through the fixture.
"""
import numpy as np

from connecting_the_dots_amd.hyperdepth import Forest, Leaf, Split, flatten, validate


def _walk(fl, ims, row):
    """leaf index (forest-local) per [N, W] pixel and tree -> [N * W, T]"""
    N, H, W = ims.shape
    nodes = fl["nodes"]
    cols = np.tile(np.arange(W), N)
    imgs = np.repeat(np.arange(N), W)
    out = np.empty((N * W, len(fl["roots"])), np.int64)
    for t, root in enumerate(fl["roots"]):
        v = np.full(N * W, root, np.int64)
        act = v >= 0
        while act.any():
            nd = nodes[v[act]]
            c, n = cols[act], imgs[act]
            r0 = np.clip(row + nd[:, 1].astype(np.int64) - 16, 0, H - 1)
            c0 = np.clip(c + nd[:, 2].astype(np.int64) - 16, 0, W - 1)
            r1 = np.clip(row + nd[:, 3].astype(np.int64) - 16, 0, H - 1)
            c1 = np.clip(c + nd[:, 4].astype(np.int64) - 16, 0, W - 1)
            d = ims[n, r0, c0].astype(np.float32) - ims[n, r1, c1].astype(np.float32)
            thr = nd[:, 0].astype(np.int32).view(np.float32)
            with np.errstate(invalid="ignore"):
                v[act] = np.where(d < thr, nd[:, 5], nd[:, 6])
            act = v >= 0
        out[:, t] = ~v
    return out


def _reduce(fl, C, leaves, chunk=256):
    """pos, pos2, S[pos], sum(S) per row of leaves [P, T]"""
    off = np.zeros(len(fl["lens"]) + 1, np.int64)
    np.cumsum(fl["lens"], out=off[1:])
    cls, cnt = fl["entries"][:, 0].astype(np.int64), fl["entries"][:, 1].astype(np.float64)
    uniq, inv = np.unique(leaves, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    U = len(uniq)
    pos, pos2, spos = np.empty(U, np.int64), np.empty(U, np.int64), np.empty(U, np.int64)
    tot = fl["sums"].astype(np.int64)[uniq].sum(1)
    for u0 in range(0, U, chunk):
        lv = uniq[u0:u0 + chunk]
        k = len(lv)
        starts, lens = off[lv].reshape(-1), fl["lens"][lv].reshape(-1)
        owner = np.repeat(np.repeat(np.arange(k), lv.shape[1]), lens)
        excl = np.repeat(np.cumsum(lens) - lens, lens)
        idx = np.repeat(starts, lens) + np.arange(int(lens.sum())) - excl
        S = np.bincount(owner * C + cls[idx], weights=cnt[idx], minlength=k * C).reshape(k, C)
        p = S.argmax(1)
        spos[u0:u0 + k] = S[np.arange(k), p].astype(np.int64)
        S[np.arange(k), p] = -1
        pos[u0:u0 + k], pos2[u0:u0 + k] = p, S.argmax(1)
    return pos[inv], pos2[inv], spos[inv], tot[inv]


def eval_rows(forests, row0, ims, n_disp_bins, row_from, row_to):
    """forests[r - row0] is the Forest of row r.  ims uint8 [N, H, W] -> f32 [N, H, W, 3]; rows outside
    [row_from, row_to) are NaN (row_from / row_to already normalised)."""
    N, H, W = ims.shape
    out = np.full((N, H, W, 3), np.nan, np.float32)
    flat = {}
    for row in range(row_from, row_to):
        f = forests[row - row0]
        fl = flat.get(id(f))
        if fl is None:
            fl = flat[id(f)] = flatten(f)
        out[:, row] = eval_row_flat(fl, validate(f), ims, row, n_disp_bins)
    return out


def eval_row_flat(fl, C, ims, row, n_disp_bins):
    """one row from a flattened forest (hyperdepth.flatten's dict) -> f32 [N, W, 3]"""
    N, H, W = ims.shape
    cols = np.tile(np.arange(W), N).astype(np.float32)
    nb = np.float32(n_disp_bins)
    pos, pos2, spos, tot = _reduce(fl, C, _walk(fl, ims, row))
    d = cols - pos.astype(np.float32) / nb
    d2 = cols - pos2.astype(np.float32) / nb
    with np.errstate(invalid="ignore", divide="ignore"):
        prob = spos.astype(np.float32) / tot.astype(np.int32).astype(np.float32)
    return np.stack([d, prob, np.abs(d - d2)], 1).reshape(N, W, 3)


# ------------------------------------------------------------------------------------------------------------------
# sparse encoding of forests (the fixture stores forests this way; save_forest rebuilds the reference's files)
# ------------------------------------------------------------------------------------------------------------------
def forest_to_arrays(forest):
    tree_len, kind, split, leaf, cls, cnt = [], [], [], [], [], []
    for nodes in forest.trees:
        order, stack = [], [0]
        while stack:
            i = stack.pop()
            order.append(i)
            if isinstance(nodes[i], Split):
                stack += [nodes[i].right, nodes[i].left]
        tree_len.append(len(order))
        for i in order:
            nd = nodes[i]
            if isinstance(nd, Split):
                kind.append(1)
                split.append([int(np.asarray(nd.threshold, "<f4").view("<i4")), nd.c0, nd.c1, nd.h0, nd.h1, nd.w0,
                              nd.w1])
            else:
                kind.append(0)
                leaf.append([nd.n_classes, nd.n_counts, nd.sum_counts, len(nd.classes)])
                cls.append(np.asarray(nd.classes, np.int32))
                cnt.append(np.asarray(nd.counts, np.int32))
    return dict(tree_len=np.asarray(tree_len, np.int64), kind=np.asarray(kind, np.int8),
                split=np.asarray(split, np.int32).reshape(-1, 7), leaf=np.asarray(leaf, np.int32).reshape(-1, 4),
                cls=np.concatenate(cls).astype(np.int32), cnt=np.concatenate(cnt).astype(np.int32))


def forest_from_arrays(d):
    trees, k, s, lf, e = [], 0, 0, 0, 0
    for n in d["tree_len"]:
        nodes, stack = [], [(-1, None)]
        for _ in range(int(n)):
            parent, side = stack.pop()
            if parent >= 0:
                setattr(nodes[parent], side, len(nodes))
            if d["kind"][k] == 1:
                row = d["split"][s]
                s += 1
                stack += [(len(nodes), "right"), (len(nodes), "left")]
                nodes.append(Split(np.int32(row[0]).view(np.float32), *[int(x) for x in row[1:]]))
            else:
                nc, ncount, sc, ln = [int(x) for x in d["leaf"][lf]]
                lf += 1
                nodes.append(Leaf(nc, ncount, d["cls"][e:e + ln].copy(), d["cnt"][e:e + ln].copy(), sc))
                e += ln
            k += 1
        trees.append(nodes)
    return Forest(trees)


# ------------------------------------------------------------------------------------------------------------------
# seeded random forests
# ------------------------------------------------------------------------------------------------------------------
def random_tree(rng, depth, C, mean_len, off_lo=0, off_hi=32, thr_scale=64.0, min_depth=None, one_class=0.0):
    """Pre-order node list.  Leaves at depth `depth` (or between min_depth and depth when given) carry sorted
    distinct classes, ~mean_len of them (uniform in [mean_len / 2, 3 mean_len / 2]), counts in 1..20."""
    nodes = []

    def grow(dep):
        idx = len(nodes)
        stop = dep >= depth or (min_depth is not None and dep >= min_depth and rng.rand() < 0.4)
        if stop:
            if rng.rand() < one_class:
                L = 1
            else:
                L = int(rng.randint(max(1, mean_len // 2), max(2, mean_len * 3 // 2 + 1)))
            L = min(L, C)
            cls = np.sort(rng.choice(C, L, replace=False)).astype(np.int32)
            cnt = rng.randint(1, 21, L).astype(np.int32)
            nodes.append(Leaf(C, C, cls, cnt, int(cnt.sum())))
            return idx
        h0, h1, w0, w1 = (int(x) for x in rng.randint(off_lo, off_hi, 4))
        thr = np.float32(np.round(rng.randn() * thr_scale))
        nodes.append(Split(thr, int(rng.randint(0, 3)), int(rng.randint(0, 3)), h0, h1, w0, w1))
        nodes[idx].left = grow(dep + 1)
        nodes[idx].right = grow(dep + 1)
        return idx

    grow(0)
    return nodes


def random_forest(rng, n_trees, depth, C, mean_len, **kw):
    return Forest([random_tree(rng, depth, C, mean_len, **kw) for _ in range(n_trees)])
