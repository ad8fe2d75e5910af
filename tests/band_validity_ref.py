"""Plain numpy restatement of the definition of include/ctd_hip_band_validity.h (a module, not a test): the band match
(idx, best) of a volume V [N,D,H,W] under per-pixel ranges [lo, hi] [N,H,W] together with the pattern-side match idx_r,
the uniqueness gap and the flag byte *over what the bands hold*.  It loops over d only, in the style of validity_ref.py.
`naive` is the same definition as a loop over every element, for the host test.

Costs are negated first (exact in floating point), so "best" is the maximum for both families; `best` itself is taken
from V as it is.  Pixel (f,h,w) holds d when max(lo, 0) <= d <= min(hi, D-1)."""
import numpy as np

IN_PATTERN, LR_OK, UNIQUE = 1, 2, 4


def _clip(lo, hi, D):
    return np.maximum(np.asarray(lo, np.int64), 0), np.minimum(np.asarray(hi, np.int64), D - 1)


def band_validity_ref(vol, lo, hi, maximise, lr_tol=1, min_gap=0.0):
    """(idx int64, best f32, flags u8, idx_r int64, gap f32), each [N,H,W]"""
    V = np.asarray(vol, np.float32)
    Vm = V if maximise else -V
    N, D, H, W = V.shape
    lo, hi = _clip(lo, hi, D)
    assert lo.shape == (N, H, W) and hi.shape == (N, H, W)
    ninf = np.float32(-np.inf)
    # pixel side: the first index of the best held score
    idx = np.full((N, H, W), -1, np.int64)
    top = np.full((N, H, W), ninf, np.float32)
    for d in range(D):
        held = (lo <= d) & (d <= hi)
        take = held & ((idx < 0) | (Vm[:, d] > top))                # strict: the first index keeps a tie
        idx[take] = d
        top[take] = Vm[:, d][take]
    some = idx >= 0
    d0 = np.where(some, idx, 0)
    best = np.take_along_axis(V, d0[:, None], 1)[:, 0].copy()
    best[~some] = np.nan
    # pattern side: column x takes d from pixel x + d, if that pixel holds d
    idx_r = np.full((N, H, W), -1, np.int64)
    rtop = np.full((N, H, W), ninf, np.float32)
    for d in range(min(D, W)):
        held = ((lo <= d) & (d <= hi))[:, :, d:]
        y = Vm[:, d, :, d:]                                         # y[..., x] = V[d][x + d]
        ir, rt = idx_r[:, :, :W - d], rtop[:, :, :W - d]
        upd = held & ((ir < 0) | (y > rt))
        ir[upd] = d
        rt[upd] = y[upd]
    # the gap over held, non-adjacent disparities
    s1 = np.take_along_axis(Vm, d0[:, None], 1)[:, 0]
    s2 = np.full((N, H, W), ninf, np.float32)
    for d in range(D):
        far = some & (lo <= d) & (d <= hi) & (np.abs(d - d0) >= 2)
        s2 = np.where(far, np.maximum(s2, Vm[:, d]), s2)
    with np.errstate(invalid="ignore"):
        gap = (s1 - s2).astype(np.float32)                          # one f32 subtraction; +inf where s2 = -inf
    gap[~some] = np.nan
    # flags
    x = np.arange(W)[None, None, :] - idx
    in_pattern = some & (x >= 0)
    back = np.take_along_axis(idx_r, np.where(in_pattern, x, 0), 2)
    assert bool((back[in_pattern] >= 0).all())                      # the pixel's own candidate landed there
    lr_ok = in_pattern & (np.abs(back - idx) <= int(lr_tol))
    with np.errstate(invalid="ignore"):
        unique = some & (gap > np.float32(min_gap))
    flags = (in_pattern * IN_PATTERN + lr_ok * LR_OK + unique * UNIQUE).astype(np.uint8)
    return idx, best, flags, idx_r, gap


def naive(vol, lo, hi, maximise, lr_tol=1, min_gap=0.0):
    """the definition of include/ctd_hip_band_validity.h element by element"""
    V = np.asarray(vol, np.float32)
    N, D, H, W = V.shape
    lo, hi = _clip(lo, hi, D)
    better = (lambda a, b: a > b) if maximise else (lambda a, b: a < b)
    idx = np.full((N, H, W), -1, np.int64)
    best = np.full((N, H, W), np.nan, np.float32)
    idx_r = np.full((N, H, W), -1, np.int64)
    gap = np.full((N, H, W), np.nan, np.float32)
    flags = np.zeros((N, H, W), np.uint8)

    def holds(f, h, w, d):
        return lo[f, h, w] <= d <= hi[f, h, w]

    for f in range(N):
        for h in range(H):
            for w in range(W):
                for d in range(D):
                    if holds(f, h, w, d) and (idx[f, h, w] < 0 or better(V[f, d, h, w], V[f, idx[f, h, w], h, w])):
                        idx[f, h, w] = d
                if idx[f, h, w] >= 0:
                    best[f, h, w] = V[f, idx[f, h, w], h, w]
            for x in range(W):
                for d in range(min(D, W - x)):
                    if holds(f, h, x + d, d) and (idx_r[f, h, x] < 0 or
                                                  better(V[f, d, h, x + d], V[f, idx_r[f, h, x], h, x + idx_r[f, h, x]])):
                        idx_r[f, h, x] = d
    for f in range(N):
        for h in range(H):
            for w in range(W):
                d0 = int(idx[f, h, w])
                if d0 < 0:
                    continue
                s2 = None
                for d in range(D):
                    if holds(f, h, w, d) and abs(d - d0) >= 2 and (s2 is None or better(V[f, d, h, w], s2)):
                        s2 = V[f, d, h, w]
                s1 = V[f, d0, h, w]
                if s2 is None:
                    g = np.float32(np.inf)
                else:
                    g = np.float32(s1 - s2) if maximise else np.float32(s2 - s1)
                gap[f, h, w] = g
                fl = 0
                if w - d0 >= 0:
                    fl |= IN_PATTERN
                    assert idx_r[f, h, w - d0] >= 0
                    if abs(int(idx_r[f, h, w - d0]) - d0) <= lr_tol:
                        fl |= LR_OK
                if g > np.float32(min_gap):
                    fl |= UNIQUE
                flags[f, h, w] = fl
    return idx, best, flags, idx_r, gap
