"""Numpy f32 restatement of band-limited semi-global matching (include/ext/ctd_hip_band_sgm.h): the band rule, the band
volume gathered from an exact volume, and the aggregation -- one direction at a time, vectorised over everything but
the path axis, in the association and summation order of tests/sgm_ref.py.  It is the yardstick of the band SGM
kernels (tests/test_band_sgm_gpu.py); tests/test_band_sgm_host.py pins it against sgm_ref on the +inf-masked full
volume and against a scalar triple loop.

    lo' = max(lo, 0), hi'' = min(hi, D-1, lo' + slots - 1); p holds d when lo' <= d <= hi'', slot k = d - lo', n(p) held
    C = Vb (maximise=True: -Vb).  A direction is a step (dy, dx); q = (y - dy, x - dx).
    q outside the image or n(q) = 0:  L(p,d) = C(p,d)
    otherwise:  m = min L(q,k) over held k
                t = min(L(q,d), m + P2, L(q,d-1) + P1, L(q,d+1) + P1), an L(q,.) term only where q holds it
                L(p,d) = C(p,d) + (t - m)
    S = ((L0 + L1) + L2) + ...;  idx = lo' + first argmin slot of S;  best = S there;  empty band: idx -1, best NaN
"""
import numpy as np

from tests.sgm_ref import directions

_INF = np.float32(np.inf)
_NAN = np.float32(np.nan)


def band_rule(lo, hi, D, slots):
    """lo, hi int arrays -> (lo' int64, clamped to D: a pixel with lo' >= D holds nothing; n int64)"""
    l = np.clip(np.asarray(lo).astype(np.int64), 0, D)
    u = np.minimum(np.clip(np.asarray(hi).astype(np.int64), -1, D - 1), l + slots - 1)
    return l, np.maximum(u - l + 1, 0)


def band_gather(vol, lo, hi, slots):
    """vol [N,D,H,W] f32, lo / hi [N,H,W] -> Vb [N,slots,H,W]: vol at lo' + k in the held slots, NaN elsewhere"""
    vol = np.asarray(vol)
    N, D, H, W = vol.shape
    l, n = band_rule(lo, hi, D, slots)
    vb = np.full((N, slots, H, W), _NAN, np.float32)
    for k in range(slots):
        v = np.take_along_axis(vol, np.clip(l + k, 0, D - 1)[:, None], 1)[:, 0]
        vb[:, k] = np.where(k < n, v, _NAN)
    return vb


def band_expand(vb, lo, hi, D, fill):
    """the inverse of band_gather: [N,D,H,W] with `fill` outside the bands"""
    N, slots, H, W = vb.shape
    l, n = band_rule(lo, hi, D, slots)
    out = np.full((N, D, H, W), np.float32(fill), np.float32)
    f, y, x = np.indices((N, H, W))
    for k in range(slots):
        held = k < n
        out[f[held], (l + k)[held], y[held], x[held]] = vb[:, k][held]
    return out


def _step(Cp, lp, n_p, Lq, lq, nq, p1, p2):
    """Cp, Lq [slots, n] f32 (anything in unheld slots); lp, n_p, lq, nq [n] -> L(p, .) [slots, n], NaN where unheld"""
    slots = Cp.shape[0]
    k = np.arange(slots)[:, None]
    Lm = np.where(k < nq, Lq, _INF)
    m = Lm.min(axis=0)

    def at(kq):                                          # L(q, .) at q's slot kq; +inf where q does not hold it
        return np.where((kq >= 0) & (kq < nq), np.take_along_axis(Lm, np.clip(kq, 0, slots - 1), 0), _INF)

    kq = k + (lp - lq)
    with np.errstate(invalid="ignore"):                  # (inf - inf where n(q) = 0: replaced below)
        t = np.minimum(at(kq), m + p2)
        t = np.minimum(t, at(kq - 1) + p1)
        t = np.minimum(t, at(kq + 1) + p1)
        L = Cp + (t - m)
    L = np.where(nq == 0, Cp, L)
    return np.where(k < n_p, L, _NAN).astype(np.float32)


def path_cost(C, l, n, dy, dx, p1, p2):
    """L of one direction; C [slots,H,W] f32 in cost sign, l / n [H,W]"""
    assert C.dtype == np.float32 and C.ndim == 3
    p1, p2 = np.float32(p1), np.float32(p2)
    slots, H, W = C.shape
    L = np.where(np.arange(slots)[:, None, None] < n, C, _NAN).astype(np.float32)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for x in xs:
            if 0 <= x - dx < W:
                L[:, :, x] = _step(C[:, :, x], l[:, x], n[:, x], L[:, :, x - dx], l[:, x - dx], n[:, x - dx], p1, p2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    x = np.arange(W)
    ok = (x - dx >= 0) & (x - dx < W)                    # predecessor column inside the image
    xq = x[ok] - dx
    for y in ys:
        if not 0 <= y - dy < H:
            continue
        L[:, y, ok] = _step(C[:, y, ok], l[y, ok], n[y, ok], L[:, y - dy, xq], l[y - dy, xq], n[y - dy, xq], p1, p2)
    return L


def aggregate(C, l, n, p1, p2, paths):
    """S [slots,H,W] of a band cost volume, in the fixed summation order; NaN in the unheld slots"""
    S = None
    for dy, dx in directions(paths):
        L = path_cost(C, l, n, dy, dx, p1, p2)
        S = L if S is None else S + L
    return S


def band_sgm_ref(vb, lo, hi, D, p1, p2, paths=8, maximise=False):
    """vb [N,slots,H,W] f32, lo / hi [N,H,W] -> (S_b f32 like vb, idx int64, best f32); S_b and best in cost sign"""
    vb = np.asarray(vb)
    assert vb.dtype == np.float32 and vb.ndim == 4
    slots = vb.shape[1]
    l, n = band_rule(lo, hi, D, slots)
    S = np.stack([aggregate(-v if maximise else v, l[f], n[f], p1, p2, paths) for f, v in enumerate(vb)])
    held = np.arange(slots)[None, :, None, None] < n[:, None]
    k = np.where(held, S, _INF).argmin(axis=1)           # (first slot on ties)
    idx = np.where(n > 0, l + k, -1).astype(np.int64)
    best = np.where(n > 0, np.take_along_axis(S, k[:, None], 1)[:, 0], _NAN).astype(np.float32)
    return S, idx, best
