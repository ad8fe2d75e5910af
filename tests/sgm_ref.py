"""Numpy f32 restatement of the semi-global aggregation rule of include/ctd_hip.h (ctd_sgm_aggregate_f32): one
direction at a time, vectorised over everything but the path axis, in the stated association and summation order.
It is the only yardstick of the SGM kernels (tests/test_sgm_gpu.py); tests/test_sgm_host.py pins it against a scalar
triple loop.

    C[d,y,x]: lower is better (maximise=True: C = -vol).  A direction is a step (dy, dx); q = (y - dy, x - dx).
    q outside the image:  L(p,d) = C(p,d)
    otherwise:            m = min_k L(q,k)
                          t = min(L(q,d), m + P2, L(q,d-1) + P1 [d >= 1], L(q,d+1) + P1 [d + 1 < D])
                          L(p,d) = C(p,d) + (t - m)
    S = ((L0 + L1) + L2) + ... over DIRECTIONS[:paths];  idx = first argmin_d S;  best = S[idx]
"""
import numpy as np

# -> <- down down-right down-left up up-right up-left, as (dy, dx)
DIRECTIONS = ((0, 1), (0, -1), (1, 0), (1, 1), (1, -1), (-1, 0), (-1, 1), (-1, -1))
NAMES = ("right", "left", "down", "down_right", "down_left", "up", "up_right", "up_left")


def directions(paths):
    if paths not in (4, 8):
        raise ValueError("paths must be 4 or 8")
    return (DIRECTIONS[0], DIRECTIONS[1], DIRECTIONS[2], DIRECTIONS[5]) if paths == 4 else DIRECTIONS


def _step(Cp, Lq, p1, p2):
    """Cp, Lq [D, n] f32 -> L(p, .) [D, n]"""
    m = Lq.min(axis=0)
    t = np.minimum(Lq, m + p2)
    t[1:] = np.minimum(t[1:], Lq[:-1] + p1)
    t[:-1] = np.minimum(t[:-1], Lq[1:] + p1)
    return Cp + (t - m)


def path_cost(C, dy, dx, p1, p2):
    """L of one direction; C [D,H,W] f32"""
    assert C.dtype == np.float32 and C.ndim == 3
    p1, p2 = np.float32(p1), np.float32(p2)
    D, H, W = C.shape
    L = C.copy()
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for x in xs:
            if 0 <= x - dx < W:
                L[:, :, x] = _step(C[:, :, x], L[:, :, x - dx], p1, p2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    x = np.arange(W)
    ok = (x - dx >= 0) & (x - dx < W)                    # predecessor column inside the image
    for y in ys:
        if not 0 <= y - dy < H:
            continue
        L[:, y, ok] = _step(C[:, y, ok], L[:, y - dy, x[ok] - dx], p1, p2)
    return L


def aggregate(C, p1, p2, paths):
    """S [D,H,W] of a cost volume C [D,H,W] f32, in the fixed summation order"""
    S = None
    for dy, dx in directions(paths):
        L = path_cost(C, dy, dx, p1, p2)
        S = L if S is None else S + L
    return S


def sgm_ref(vol, p1, p2, paths=8, maximise=False):
    """vol [N,D,H,W] | [D,H,W] f32 -> (S f32 like vol, idx int64, best f32); S and best in cost sign"""
    vol = np.asarray(vol)
    assert vol.dtype == np.float32
    if vol.ndim == 3:
        S, idx, best = sgm_ref(vol[None], p1, p2, paths, maximise)
        return S[0], idx[0], best[0]
    S = np.stack([aggregate(-v if maximise else v, p1, p2, paths) for v in vol])
    idx = S.argmin(axis=1).astype(np.int64)              # (first index on ties)
    best = np.take_along_axis(S, idx[:, None], 1)[:, 0]
    return S, idx, best
