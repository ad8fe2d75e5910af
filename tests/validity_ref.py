"""Plain numpy restatement of the match-validity rule of include/ctd_hip.h (a module, not a test): the pattern-side
match idx_r, the uniqueness gap and the flag byte of a volume V [N,D,H,W] and an index tensor idx [N,H,W].  It loops
over d only.  `naive` is the same rule as a loop over every element, for the host test.

Costs are negated first (exact in floating point), so "best" is the maximum for both families: the first index of the
maximum of -V is the first index of the minimum of V, and (-s1) - (-s2) is the same f32 subtraction as s2 - s1."""
import numpy as np

IN_PATTERN, LR_OK, UNIQUE = 1, 2, 4


def pattern_side(vol, maximise):
    """idx_r [N,H,W] int64 and the diagonal's best score (in the maximising domain)"""
    V = np.asarray(vol, np.float32)
    V = V if maximise else -V
    N, D, H, W = V.shape
    best = np.full((N, H, W), -np.inf, np.float32)
    idx_r = np.zeros((N, H, W), np.int64)
    for d in range(min(D, W)):                      # column x takes d while x + d < W
        y = V[:, d, :, d:]                          # y[..., x] = V[d][x + d]
        b = best[:, :, :W - d]
        upd = y > b                                 # strict: the first index keeps a tie
        idx_r[:, :, :W - d][upd] = d
        b[upd] = y[upd]
    return idx_r, best


def gap_of(vol, idx, maximise):
    """gap [N,H,W] f32 and (s1, s2) in the maximising domain (s2 = -inf where no non-adjacent disparity exists)"""
    V = np.asarray(vol, np.float32)
    V = V if maximise else -V
    N, D, H, W = V.shape
    idx = np.asarray(idx, np.int64)
    in_range = (idx >= 0) & (idx < D)
    d0 = np.where(in_range, idx, 0)
    s1 = np.take_along_axis(V, d0[:, None], 1)[:, 0]
    s2 = np.full((N, H, W), -np.inf, np.float32)
    for d in range(D):
        far = np.abs(d - d0) >= 2
        s2 = np.where(far, np.maximum(s2, V[:, d]), s2)
    with np.errstate(invalid="ignore"):
        gap = (s1 - s2).astype(np.float32)          # one f32 subtraction; +inf where s2 = -inf
    gap[~in_range] = np.nan
    return gap, s1, s2


def validity_ref(vol, idx, maximise, lr_tol=1, min_gap=0.0):
    """(flags u8, idx_r int64, gap f32), each [N,H,W]"""
    V = np.asarray(vol, np.float32)
    N, D, H, W = V.shape
    idx = np.asarray(idx, np.int64)
    idx_r, _ = pattern_side(V, maximise)
    gap, _, _ = gap_of(V, idx, maximise)
    in_range = (idx >= 0) & (idx < D)
    x = np.arange(W)[None, None, :] - idx
    in_pattern = in_range & (x >= 0)
    xs = np.where(in_pattern, x, 0)
    back = np.take_along_axis(idx_r, xs, 2)
    lr_ok = in_pattern & (np.abs(back - idx) <= int(lr_tol))
    with np.errstate(invalid="ignore"):
        unique = in_range & (gap > np.float32(min_gap))
    flags = (in_pattern * IN_PATTERN + lr_ok * LR_OK + unique * UNIQUE).astype(np.uint8)
    return flags, idx_r, gap


def naive(vol, idx, maximise, lr_tol=1, min_gap=0.0):
    """the rule of include/ctd_hip.h element by element"""
    V = np.asarray(vol, np.float32)
    N, D, H, W = V.shape
    better = (lambda a, b: a > b) if maximise else (lambda a, b: a < b)
    idx_r = np.zeros((N, H, W), np.int64)
    gap = np.zeros((N, H, W), np.float32)
    flags = np.zeros((N, H, W), np.uint8)
    for f in range(N):
        for h in range(H):
            for x in range(W):
                bi = 0
                for d in range(1, min(D, W - x)):
                    if better(V[f, d, h, x + d], V[f, bi, h, x + bi]):
                        bi = d
                idx_r[f, h, x] = bi
    for f in range(N):
        for h in range(H):
            for w in range(W):
                d0 = int(idx[f, h, w])
                if not 0 <= d0 < D:
                    gap[f, h, w] = np.nan
                    continue
                s2 = None
                for d in range(D):
                    if abs(d - d0) >= 2 and (s2 is None or better(V[f, d, h, w], s2)):
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
                    if abs(int(idx_r[f, h, w - d0]) - d0) <= lr_tol:
                        fl |= LR_OK
                if g > np.float32(min_gap):
                    fl |= UNIQUE
                flags[f, h, w] = fl
    return flags, idx_r, gap


# ---------------------------------------------------------------------------------------------------------------------
# which pixels / pattern columns the fast path must, and must not, settle by exact re-scoring -- from the reference
# volume alone.  The fast scores f obey |f - x| <= e(x) = 1e-5 |x| + 1e-6 of the reference-order scores x.
# ---------------------------------------------------------------------------------------------------------------------
def _e(x):
    return 1e-5 * np.abs(np.asarray(x, np.float64)) + 1e-6


def expected_lists(vol, idx, maximise, min_gap=0.0):
    """dict of bool [N,H,W] masks.
    col_must: the diagonal's best score is attained twice or more (an exact tie: the two fast scores then lie within
      both bounds of each other, so no margin can prove the winner);  col_never: the best beats every other entry of the
      diagonal by more than 4 x both bounds (the fast scores are then farther apart than 2 x both bounds).
    pix_must: a non-adjacent disparity exists and gap == min_gap exactly (the fast gap then lies within both bounds of
      min_gap);  pix_never: no non-adjacent disparity, idx out of range, or |gap - min_gap| > 4 x both bounds."""
    V = np.asarray(vol, np.float32)
    Vm = V if maximise else -V
    N, D, H, W = V.shape
    idx_r, best = pattern_side(V, maximise)
    count = np.zeros((N, H, W), np.int64)
    second = np.full((N, H, W), -np.inf, np.float32)
    for d in range(min(D, W)):
        y = Vm[:, d, :, d:]
        b = best[:, :, :W - d]
        count[:, :, :W - d] += y == b
        other = idx_r[:, :, :W - d] != d
        s = second[:, :, :W - d]
        s[...] = np.where(other, np.maximum(s, y), s)
    col_must = count >= 2
    with np.errstate(invalid="ignore"):
        far = best.astype(np.float64) - second.astype(np.float64) > 4 * (_e(best) + _e(np.where(np.isfinite(second), second, 0)))
    col_never = ~np.isfinite(second) | far
    gap, s1, s2 = gap_of(V, idx, maximise)
    has = np.isfinite(s2) & ~np.isnan(gap)
    with np.errstate(invalid="ignore"):
        delta = s1.astype(np.float64) - s2.astype(np.float64)
        pix_must = has & (gap == np.float32(min_gap)) & (delta == float(np.float32(min_gap)))
        pix_never = ~has | (np.abs(delta - float(np.float32(min_gap))) > 4 * (_e(s1) + _e(np.where(has, s2, 0))) + 1e-6)
    return {"col_must": col_must, "col_never": col_never & ~col_must, "pix_must": pix_must, "pix_never": pix_never & ~pix_must}
