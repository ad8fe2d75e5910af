"""CPU-only: pins tests/dispfilter_ref.py (the yardstick of the disparity post-filter kernels) against a plain scalar
flood fill, a scalar sort-based median and hand-written cases, checks the usefulness claim on the reference alone, and
the C ABI's argument checks, which run before any HIP call."""
import numpy as np
import pytest

from tests import dispfilter_ref as dr
from tests import workloads

NAN = np.float32(np.nan)


# ---- scalar restatements ----------------------------------------------------------------------------------------------
def flood_fill(disp, valid, max_diff, connectivity):
    H, W = disp.shape
    live = [[bool(np.isfinite(disp[y, x])) and (valid is None or bool(valid[y, x])) for x in range(W)] for y in range(H)]
    steps = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    label = np.full((H, W), -1, np.int32)
    size = np.zeros((H, W), np.int32)
    for y0 in range(H):
        for x0 in range(W):
            if not live[y0][x0] or label[y0, x0] >= 0:
                continue
            label[y0, x0] = y0 * W + x0                          # raster order: the first pixel met is the smallest index
            stack, members = [(y0, x0)], [(y0, x0)]
            while stack:
                y, x = stack.pop()
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and live[yy][xx] and label[yy, xx] < 0 and \
                            abs(np.float32(disp[y, x] - disp[yy, xx])) <= np.float32(max_diff):
                        label[yy, xx] = y0 * W + x0
                        stack.append((yy, xx))
                        members.append((yy, xx))
            for y, x in members:
                size[y, x] = len(members)
    return label, size


def scalar_median(disp, valid, window, fill_min):
    H, W = disp.shape
    r = window // 2
    out = np.full((H, W), NAN, np.float32)
    ok = np.zeros((H, W), np.uint8)

    def live(y, x):
        return bool(np.isfinite(disp[y, x])) and (valid is None or bool(valid[y, x]))
    for y in range(H):
        for x in range(W):
            vals = [disp[yy, xx] for yy in range(y - r, y + r + 1) for xx in range(x - r, x + r + 1)
                    if 0 <= yy < H and 0 <= xx < W and live(yy, xx)]
            m = len(vals)
            if live(y, x) or (fill_min > 0 and m >= fill_min):
                out[y, x] = sorted(vals)[(m - 1) // 2]           # (sorted is stable: ties keep window raster order)
                ok[y, x] = 1
    return out, ok


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.nan_to_num(a, nan=0.0).view(np.uint32 if a.dtype == np.float32 else a.dtype),
                       np.nan_to_num(b, nan=0.0).view(np.uint32 if b.dtype == np.float32 else b.dtype))


def random_map(rs, H, W, kind):
    if kind == "few":
        d = rs.randint(0, 3, (H, W)).astype(np.float32)
    elif kind == "int":
        d = rs.randint(0, 12, (H, W)).astype(np.float32)
    else:
        d = (rs.rand(H, W) * 6).astype(np.float32)
    d[rs.rand(H, W) < 0.08] = NAN
    d[rs.rand(H, W) < 0.02] = np.float32(np.inf)
    valid = (rs.rand(H, W) < 0.85).astype(np.uint8) * rs.randint(1, 8, (H, W)).astype(np.uint8)
    return d, valid


# ---- the restatement against the scalar code --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["few", "int", "real"])
def test_components_equal_a_scalar_flood_fill(kind):
    rs = np.random.RandomState(len(kind))
    for H, W in ((1, 1), (1, 9), (7, 1), (6, 11), (13, 17)):
        d, valid = random_map(rs, H, W, kind)
        for v in (None, valid):
            for max_diff in (0.0, 0.5, 1.0, np.inf):
                for conn in (4, 8):
                    want = flood_fill(d, v, max_diff, conn)
                    got = dr.components(d, v, max_diff, conn)
                    assert same(got[0], want[0]) and same(got[1], want[1]), (kind, H, W, max_diff, conn)
                    keep, size = dr.speckle(d, v, max_diff, 3, conn)
                    assert same(size, want[1]) and np.array_equal(keep, (want[1] > 3).astype(np.uint8))


@pytest.mark.parametrize("window", [3, 5, 7])
def test_median_equals_a_scalar_sort(window):
    rs = np.random.RandomState(window)
    for H, W in ((1, 1), (2, 9), (9, 2), (8, 13)):
        for kind in ("few", "real"):
            d, valid = random_map(rs, H, W, kind)
            d[rs.rand(H, W) < 0.1] = np.float32(-0.0)            # signed zeros among the zeros of "few"
            for v in (None, valid):
                for fill_min in (0, 1, (window * window + 1) // 2):
                    want = scalar_median(d, v, window, fill_min)
                    got = dr.median(d, v, window, fill_min)
                    assert same(got[0], want[0]) and same(got[1], want[1]), (window, H, W, kind, fill_min)


def test_partition_against_scipy_where_it_imports():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import coo_matrix
    rs = np.random.RandomState(4)
    d, valid = random_map(rs, 40, 53, "int")
    for conn in (4, 8):
        live = dr.live_mask(d, valid)
        a, b = dr.edges(d, live, 1.0, conn)
        n = d.size
        _, lab = csgraph.connected_components(coo_matrix((np.ones(len(a)), (a, b)), shape=(n, n)), directed=False)
        label, _ = dr.components(d, valid, 1.0, conn)
        lv = live.ravel()
        pairs = set(zip(lab[lv].tolist(), label.ravel()[lv].tolist()))
        assert len(pairs) == len(set(lab[lv].tolist())) == len(set(label.ravel()[lv].tolist()))   # a bijection


# ---- hand-written cases -----------------------------------------------------------------------------------------------
def test_a_chain_is_one_component_although_its_ends_differ_by_three():
    d = np.array([[0, 1, 2, 3]], np.float32)
    label, size = dr.components(d, None, 1.0, 4)
    assert label.tolist() == [[0, 0, 0, 0]] and size.tolist() == [[4, 4, 4, 4]]
    label, size = dr.components(d, None, 0.5, 4)
    assert label.tolist() == [[0, 1, 2, 3]] and size.tolist() == [[1, 1, 1, 1]]


def test_u_shape_takes_the_minimum_index_of_the_other_arm():
    """the arms of the U meet in the last row only: a single raster pass gives the right arm the label 2 first"""
    live = np.array([[1, 0, 1],
                     [1, 0, 1],
                     [1, 1, 1]], bool)
    d = np.where(live, np.float32(5), NAN)
    label, size = dr.components(d)
    assert label.tolist() == [[0, -1, 0], [0, -1, 0], [0, 0, 0]]
    assert size.tolist() == [[7, 0, 7], [7, 0, 7], [7, 7, 7]]
    label, _ = dr.components(d, live)                           # the same through the mask
    assert label[0, 2] == 0
    d[2, 1] = 9                                                  # cut the bottom: two arms
    label, size = dr.components(d)
    assert label.tolist() == [[0, -1, 2], [0, -1, 2], [0, 7, 2]] and size[2].tolist() == [3, 1, 3]


def test_a_diagonal_touch_joins_under_connectivity_8_only():
    d = np.array([[1, NAN], [NAN, 1]], np.float32)
    assert dr.components(d, None, 1.0, 4)[0].tolist() == [[0, -1], [-1, 3]]
    assert dr.components(d, None, 1.0, 8)[0].tolist() == [[0, -1], [-1, 0]]
    d = np.array([[NAN, 1], [1, NAN]], np.float32)               # the other diagonal
    assert dr.components(d, None, 1.0, 4)[1].tolist() == [[0, 1], [1, 0]]
    assert dr.components(d, None, 1.0, 8)[0].tolist() == [[-1, 1], [1, -1]]
    board = (np.indices((4, 6)).sum(0) % 2 == 0)
    d = np.where(board, np.float32(0), NAN)
    assert int(dr.components(d, None, 0.0, 4)[1].max()) == 1
    assert set(dr.components(d, None, 0.0, 8)[1][board].tolist()) == {12}


def test_nan_inf_and_masked_pixels_are_not_live_and_do_not_bridge():
    d = np.array([[1, NAN, 1, np.inf, 1, 1, 1]], np.float32)
    valid = np.array([[1, 1, 1, 1, 1, 0, 2]], np.uint8)
    label, size = dr.components(d, valid, np.inf, 8)
    assert label.tolist() == [[0, -1, 2, -1, 4, -1, 6]] and size.tolist() == [[1, 0, 1, 0, 1, 0, 1]]
    keep, _ = dr.speckle(d, valid, np.inf, 0, 4)
    assert keep.tolist() == [[1, 0, 1, 0, 1, 0, 1]]              # max_size 0 keeps every live pixel
    assert int(dr.speckle(d, valid, np.inf, 1, 4)[0].sum()) == 0
    frames = np.stack([np.zeros((2, 2), np.float32)] * 2)        # nothing crosses frames
    label, size = dr.components(frames)
    assert label.tolist() == [[[0, 0], [0, 0]]] * 2 and int(size.max()) == 4


def test_median_even_count_corners_and_fill():
    d = np.array([[4, 1], [3, 2]], np.float32)
    out, ok = dr.median(d, None, 3, 0)                           # every window is the whole image: m = 4, the lower median
    assert out.tolist() == [[2, 2], [2, 2]] and ok.tolist() == [[1, 1], [1, 1]]
    d = np.arange(25, dtype=np.float32).reshape(5, 5)
    out, _ = dr.median(d, None, 3, 0)
    assert out[0, 0] == 1 and out[0, 4] == 4 and out[4, 4] == 19  # corners: 4 of {0,1,5,6}, {3,4,8,9}, {18,19,23,24}
    assert out[0, 2] == 3 and out[2, 2] == 12                     # an edge (m = 6: rank 2 of 1,2,3,6,7,8) and the centre
    assert dr.median(d, None, 7, 0)[0][2, 2] == 12               # 7 x 7 clipped to the image: all 25
    hole = d.copy()
    hole[2, 2] = NAN
    valid = np.ones((5, 5), np.uint8)
    valid[0, 0] = 0
    out, ok = dr.median(hole, valid, 3, 0)
    assert np.isnan(out[2, 2]) and ok[2, 2] == 0 and np.isnan(out[0, 0]) and ok[0, 0] == 0
    assert out[1, 1] == 6                                        # live: 1,2,5,6,7,10,11 -> rank 3
    out, ok = dr.median(hole, valid, 3, 8)                       # the hole has 8 live neighbours, the corner 3
    assert out[2, 2] == 11 and ok[2, 2] == 1 and np.isnan(out[0, 0])
    out, ok = dr.median(hole, valid, 3, 3)
    assert out[0, 0] == 5 and ok[0, 0] == 1                      # 1, 5, 6
    out, ok = dr.median(hole, valid, 3, 9)
    assert np.isnan(out[2, 2]) and ok.sum() == 23
    z = np.array([[0.0, -0.0, 0.0]], np.float32)                 # signed zeros compare equal: raster order decides
    assert np.signbit(dr.median(z, None, 3, 0)[0]).tolist() == [[False, True, True]]


def test_disparity_filter_is_the_composition():
    rs = np.random.RandomState(9)
    d, valid = random_map(rs, 12, 19, "few")
    for v in (None, valid):
        keep, _ = dr.speckle(d, v, 0.0, 2, 4)
        want = dr.median(d, keep, 5, 3)
        got = dr.disparity_filter(d, v, 0.0, 2, 4, 5, 3)
        assert same(got[0], want[0]) and same(got[1], want[1])
        out, k = dr.disparity_filter(d, v, 0.0, 2, 4, 0)
        assert same(k, keep) and np.array_equal(np.isnan(out), keep == 0) and np.array_equal(out[keep != 0], d[keep != 0])


def test_adversarial_masks_are_single_components():
    for H, W in ((9, 11), (33, 70), (432, 512)):
        for mask in (dr.serpentine(H, W), dr.spiral(H, W)):
            d = np.where(mask, np.float32(3), NAN)
            label, size = dr.components(d, None, 0.0, 4)
            assert set(label[mask].tolist()) == {0} and set(size[mask].tolist()) == {int(mask.sum())}
            assert int(mask.sum()) > H * W // 2 - H - W


# ---- usefulness, on the reference alone -------------------------------------------------------------------------------
def numpy_sad_argmin(ir, pat, D, bs):
    """plain argmin of a block SAD volume, zero padded: cost[d, y, x] = sum over the block of |ir[y, x] - pat[y, x - d]|"""
    H, W = ir.shape
    r = bs // 2
    cost = np.empty((D, H, W), np.float32)
    for d in range(D):
        shifted = np.zeros_like(pat)
        shifted[:, d:] = pat[:, :W - d]
        ad = np.pad(np.abs(ir - shifted), r)
        c = np.cumsum(np.cumsum(ad.astype(np.float64), 0), 1)
        c = np.pad(c, ((1, 0), (1, 0)))
        cost[d] = c[bs:, bs:] - c[:-bs, bs:] - c[bs:, :-bs] + c[:-bs, :-bs]
    return cost.argmin(0)


def test_speckle_removal_removes_gross_errors():
    """synth_ir at 96 x 160, D 48, seed 2025, plus N(0, 0.15^2) noise, block-5 SAD (here a numpy volume; the GPU test
    uses the project's), plain argmin, max_diff 1, max_size 20, connectivity 4, counted columns >= D + block.  Gross
    error share among kept pixels <= one third of the plain share, and >= 98 % of the non-gross pixels kept."""
    H, W, D, bs = 96, 160, 48, 5
    rs = np.random.RandomState(2025)
    pat = workloads.syn_dot_pattern(H, W)
    ir, disp = workloads.synth_ir(pat, rs, D)
    ir = (ir + rs.normal(0, 0.15, ir.shape)).astype(np.float32)
    idx = numpy_sad_argmin(ir, pat.astype(np.float32), D, bs)
    plain, kept_share, kept_good = usefulness(idx, disp, D, bs)
    assert 3.0 * kept_share <= plain and kept_good >= 0.98


def usefulness(idx, disp, D, bs):
    H, W = idx.shape
    cols = np.zeros((H, W), bool)
    cols[:, D + bs:] = True
    gross = np.abs(idx - disp) > 1
    keep, _ = dr.speckle(idx.astype(np.float32), None, 1.0, 20, 4)
    kept = (keep != 0) & cols
    plain = gross[cols].mean()
    kept_share = gross[kept].mean()
    kept_good = (kept & ~gross).sum() / max((cols & ~gross).sum(), 1)
    print("gross errors: %.4f of the counted pixels, %.4f of the kept ones (%.1f x fewer); %.4f of the non-gross kept" % (
        plain, kept_share, plain / max(kept_share, 1e-9), kept_good))
    return plain, kept_share, kept_good


# ---- the C ABI's argument checks need no GPU --------------------------------------------------------------------------
def test_argument_errors_come_before_any_hip_call():
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    INVALID = 1
    p = 256                                                      # any non-NULL address: rejected calls never touch it

    def comp(disp=p, valid=None, max_diff=1.0, conn=4, label=p, size=p, N=1, H=8, W=8, ws=p, nws=1 << 20):
        return L.ctd_disp_components_f32(disp, valid, max_diff, conn, label, size, N, H, W, ws, nws, -1, None)
    for bad in (dict(max_diff=-1.0), dict(max_diff=float("nan")), dict(conn=6), dict(H=0), dict(W=-1), dict(N=-1),
                dict(H=1 << 16, W=1 << 15), dict(N=3, H=1 << 15, W=1 << 15), dict(disp=None), dict(label=None),
                dict(size=None)):
        assert comp(**bad) == INVALID, bad
    assert comp(N=0) == 0 and comp(N=0, ws=None, nws=0) == 0
    assert comp(ws=None) == 2 and comp(nws=8) == 2 and comp(ws=p + 4) == 2    # CTD_ERR_WORKSPACE
    assert L.ctd_disp_components_workspace_bytes(2, 5, 7) >= 3 * 4 * 70
    assert L.ctd_disp_components_workspace_bytes(1, 0, 7) == 0
    assert L.ctd_disp_components_workspace_bytes(1, 1 << 16, 1 << 15) == 0
    spk = lambda max_diff=1.0, max_size=20, conn=4, keep=p, N=1: L.ctd_disp_speckle_f32(
        p, None, max_diff, max_size, conn, keep, None, N, 8, 8, p, 1 << 20, -1, None)
    assert spk(max_size=-1) == INVALID and spk(conn=5) == INVALID and spk(max_diff=-0.5) == INVALID
    assert spk(keep=None) == INVALID and spk(N=0) == 0
    med = lambda window=3, fill_min=0, out=3 * p, vout=2 * p, N=1, H=8: L.ctd_disp_median_f32(
        p, None, window, fill_min, out, vout, N, H, 8, -1, None)
    for bad in (dict(window=4), dict(window=1), dict(window=9), dict(fill_min=-1), dict(out=None), dict(vout=None),
                dict(H=0), dict(N=-2)):
        assert med(**bad) == INVALID, bad
    assert L.ctd_disp_median_f32(p, None, 3, 0, p, 2 * p, 1, 8, 8, -1, None) == INVALID       # out is disp
    assert med(N=0) == 0 and med(H=1 << 30) == INVALID


def test_python_surface_and_cpu_tensors():
    import torch
    from connecting_the_dots_amd import torchext as te
    x = torch.zeros(4, 5)
    for name in ("disp_components", "disp_speckle", "disp_median", "disparity_filter"):
        assert hasattr(te, name), name
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            getattr(te, name)(x)
