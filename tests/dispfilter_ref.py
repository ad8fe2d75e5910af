"""Numpy restatement of the disparity post-filter rules of include/ctd_hip.h (ctd_disp_components_f32,
ctd_disp_speckle_f32, ctd_disp_median_f32 and torchext.disparity_filter).  It is the only yardstick of the kernels
(tests/test_disp_filter_gpu.py); tests/test_disp_filter_host.py pins it against a scalar flood fill, a scalar
sort-based median and hand-written cases.

    live(p)     = valid[p] != 0 (valid None: everywhere) and isfinite(disp[p])
    linked(p,q) = live(p) and live(q) and |disp[p] - disp[q]| <= max_diff in f32, q one of the 4 (8) neighbours of p
    label       = the smallest in-frame index h * W + w of the component, -1 where not live;  size = its pixel count, 0
    keep        = live and size > max_size
    median      = rank (m - 1) // 2 of the m live values of the clipped window in stable ascending order (ties in window
                  raster order), where p is live or fill_min > 0 and m >= fill_min; NaN and valid_out 0 elsewhere

The labelling is vectorised union-find: every round hangs the larger of two linked roots under the smaller
(np.minimum.at) and compresses all paths by pointer jumping, so the number of trees at least halves per round and a
root is always the minimum of its set.
"""
import numpy as np

# the neighbours that come before a pixel in raster order, as (dy, dx): left, up | up-left, up-right
BACKWARD = {4: ((0, -1), (-1, 0)), 8: ((0, -1), (-1, 0), (-1, -1), (-1, 1))}


def live_mask(disp, valid=None):
    disp = np.asarray(disp)
    assert disp.dtype == np.float32
    live = np.isfinite(disp)
    if valid is not None:
        live &= np.asarray(valid) != 0
    return live


def edges(disp, live, max_diff, connectivity):
    """linked pairs of one frame [H,W] as two arrays of linear indices (a later in raster order than b)"""
    if connectivity not in BACKWARD:
        raise ValueError("connectivity must be 4 or 8")
    if not max_diff >= 0:
        raise ValueError("max_diff must be >= 0")
    H, W = disp.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    md = np.float32(max_diff)
    A, B = [], []
    for dy, dx in BACKWARD[connectivity]:
        ys, yq = slice(-dy, H), slice(0, H + dy)                     # dy is 0 or -1
        xs, xq = slice(max(-dx, 0), W + min(-dx, 0)), slice(max(dx, 0), W + min(dx, 0))
        p, q = disp[ys, xs], disp[yq, xq]
        with np.errstate(over="ignore", invalid="ignore"):
            ok = live[ys, xs] & live[yq, xq] & (np.abs(p - q) <= md)
        A.append(idx[ys, xs][ok])
        B.append(idx[yq, xq][ok])
    return np.concatenate(A), np.concatenate(B)


def _roots(n, a, b):
    parent = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        differ = ra != rb
        if not differ.any():
            return parent
        a, b, ra, rb = a[differ], b[differ], ra[differ], rb[differ]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp


def components(disp, valid=None, max_diff=1.0, connectivity=4):
    """disp [N,H,W] | [H,W] f32 -> (label int32, size int32)"""
    disp = np.asarray(disp)
    if disp.ndim == 2:
        label, size = components(disp[None], None if valid is None else np.asarray(valid)[None], max_diff, connectivity)
        return label[0], size[0]
    live = live_mask(disp, valid)
    N, H, W = disp.shape
    label = np.full((N, H * W), -1, np.int32)
    size = np.zeros((N, H * W), np.int32)
    for f in range(N):
        a, b = edges(disp[f], live[f], max_diff, connectivity)
        root = _roots(H * W, a, b)
        lv = live[f].ravel()
        counts = np.bincount(root[lv], minlength=H * W)
        label[f, lv] = root[lv]
        size[f, lv] = counts[root[lv]]
    return label.reshape(N, H, W), size.reshape(N, H, W)


def speckle(disp, valid=None, max_diff=1.0, max_size=20, connectivity=4):
    """-> (keep uint8, size int32)"""
    if max_size < 0:
        raise ValueError("max_size must be >= 0")
    _, size = components(disp, valid, max_diff, connectivity)
    return (live_mask(disp, valid) & (size > max_size)).astype(np.uint8), size


def median(disp, valid=None, window=3, fill_min=0):
    """-> (out f32 with NaN where valid_out is 0, valid_out uint8)"""
    if window not in (3, 5, 7):
        raise ValueError("window must be 3, 5 or 7")
    if fill_min < 0:
        raise ValueError("fill_min must be >= 0")
    disp = np.asarray(disp)
    if disp.ndim == 2:
        out, ok = median(disp[None], None if valid is None else np.asarray(valid)[None], window, fill_min)
        return out[0], ok[0]
    live = live_mask(disp, valid)
    N, H, W = disp.shape
    r = window // 2
    padded = np.full((N, H + 2 * r, W + 2 * r), np.nan, np.float32)  # outside the image and dead pixels: NaN, sorted last
    padded[:, r:r + H, r:r + W] = np.where(live, disp, np.float32(np.nan))
    taps = np.stack([padded[:, ky:ky + H, kx:kx + W] for ky in range(window) for kx in range(window)])   # raster order
    m = (~np.isnan(taps)).sum(0)
    ordered = np.sort(taps, axis=0, kind="stable")
    pick = np.take_along_axis(ordered, np.maximum(m - 1, 0)[None] // 2, 0)[0]
    ok = live | ((fill_min > 0) & (m >= fill_min))
    return np.where(ok, pick, np.float32(np.nan)).astype(np.float32), ok.astype(np.uint8)


def disparity_filter(disp, valid=None, max_diff=1.0, max_size=20, connectivity=4, window=3, fill_min=0):
    """-> (disp_out f32, valid_out uint8): speckle, then the median on valid & keep; window 0 skips the median"""
    disp = np.asarray(disp)
    keep, _ = speckle(disp, valid, max_diff, max_size, connectivity)
    if window == 0:
        return np.where(keep != 0, disp, np.float32(np.nan)).astype(np.float32), keep
    both = keep if valid is None else ((np.asarray(valid) != 0) & (keep != 0)).astype(np.uint8)
    return median(disp, both, window, fill_min)


# ---- shapes the tests and the timing tool share -----------------------------------------------------------------------
def serpentine(H, W):
    """live mask of a one-pixel-wide path that covers the frame as one 4-connected component: every even row in full,
    joined alternately at the right and the left end"""
    m = np.zeros((H, W), bool)
    m[0::2] = True
    odd = np.arange(1, H, 2)
    m[odd[0::2], W - 1] = True
    m[odd[1::2], 0] = True
    return m


def spiral(H, W):
    """live mask of a one-pixel-wide rectangular spiral from the corner inwards, its arms one pixel apart: one
    4-connected component (a walk that turns right whenever the pixel ahead, or the one after it, is taken)"""
    m = np.zeros((H, W), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True

    def can_step():
        y1, x1, y2, x2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if not (0 <= y1 < H and 0 <= x1 < W) or m[y1, x1]:
            return False
        return not (0 <= y2 < H and 0 <= x2 < W and m[y2, x2])

    turns = 0
    while turns < 2:
        if can_step():
            y, x, turns = y + dy, x + dx, 0
            m[y, x] = True
        else:
            dy, dx, turns = dx, -dy, turns + 1
    return m
