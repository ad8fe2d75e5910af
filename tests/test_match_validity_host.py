"""CPU checks of the match-validity rule (include/ctd_hip.h) as tests/validity_ref.py states it: against an
element-by-element evaluation on small volumes (planted ties, D = 1, 2, 3, W < D, indices out of range), and the
properties that pin the rule on the committed reference volumes.  The last test needs the library (no GPU): the new
entry points validate their arguments before any HIP call."""
import numpy as np
import pytest

from tests import validity_ref as vr
from tests.util import golden


def random_case(seed, N, D, H, W, ties):
    rs = np.random.RandomState(seed)
    # few distinct values: exact ties on the pixel side and along the diagonals, everywhere
    vol = (rs.randint(0, 4, size=(N, D, H, W)) * 0.25 if ties else rs.randn(N, D, H, W)).astype(np.float32)
    idx = rs.randint(-2, D + 2, size=(N, H, W)).astype(np.int64)
    return vol, idx


@pytest.mark.parametrize("maximise", [True, False])
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", [(2, 1, 3, 7), (1, 2, 4, 6), (2, 3, 3, 5), (1, 9, 2, 4), (2, 6, 5, 11), (1, 12, 3, 12)])
def test_numpy_rule_equals_the_naive_loop(shape, ties, maximise):
    N, D, H, W = shape
    vol, idx = random_case(D * 100 + W + ties, N, D, H, W, ties)
    for lr_tol, min_gap in ((0, 0.0), (1, 0.25), (2, 0.5)):
        got = vr.validity_ref(vol, idx, maximise, lr_tol, min_gap)
        want = vr.naive(vol, idx, maximise, lr_tol, min_gap)
        assert np.array_equal(got[0], want[0])
        assert np.array_equal(got[1], want[1])
        assert np.array_equal(got[2], want[2], equal_nan=True)


def test_planted_ties_take_the_first_index():
    """a diagonal whose best value sits at d = 1 and d = 3, and a pixel whose runner-up equals its best"""
    N, D, H, W = 1, 5, 1, 8
    vol = np.zeros((N, D, H, W), np.float32)
    x = 2
    vol[0, 1, 0, x + 1] = 0.75
    vol[0, 3, 0, x + 3] = 0.75
    idx = np.full((N, H, W), 1, np.int64)
    vol[0, 1, 0, 6] = 0.5
    vol[0, 4, 0, 6] = 0.5                               # |4 - 1| >= 2: s2 == s1
    flags, idx_r, gap = vr.validity_ref(vol, idx, True, 0, 0.0)
    assert idx_r[0, 0, x] == 1
    assert gap[0, 0, 6] == 0.0 and not flags[0, 0, 6] & vr.UNIQUE
    # minimising: all-equal costs tie everywhere, the first index is 0
    flags, idx_r, gap = vr.validity_ref(np.ones((1, 4, 2, 6), np.float32), np.zeros((1, 2, 6), np.int64), False)
    assert not idx_r.any() and not gap.any() and not (flags & vr.UNIQUE).any()
    assert ((flags & vr.LR_OK) != 0).all()


def test_small_disparity_ranges():
    """D = 1, 2: no non-adjacent disparity, gap = +inf and UNIQUE holds; D = 3: only d0 = 0 and 2 have one"""
    for D in (1, 2):
        vol, _ = random_case(D, 1, D, 2, 5, False)
        idx = np.zeros((1, 2, 5), np.int64)
        flags, idx_r, gap = vr.validity_ref(vol, idx, True, 1, 10.0)
        assert np.isposinf(gap).all() and ((flags & vr.UNIQUE) != 0).all()
    vol, _ = random_case(3, 1, 3, 2, 5, False)
    gap = vr.validity_ref(vol, np.ones((1, 2, 5), np.int64), True)[2]
    assert np.isposinf(gap).all()
    gap = vr.validity_ref(vol, np.zeros((1, 2, 5), np.int64), True)[2]
    assert np.array_equal(gap, vol[:, 0] - vol[:, 2])
    # out of range: NaN gap, no flag
    flags, _, gap = vr.validity_ref(vol, np.full((1, 2, 5), 3, np.int64), True)
    assert np.isnan(gap).all() and not flags.any()


def golden_volumes():
    g = golden("xcorrvol_small")
    for k in (0, 2, 3, 10):                              # the f32 cases
        yield "ncc%d" % k, g["vol_%d" % k][None], g["argmax_%d" % k][None], True
    c = golden("costvol")
    for t in range(4):
        yield "cost%d" % t, c["vol_%d" % t][None], c["argmin_%d" % t][None], False


@pytest.mark.parametrize("case", list(golden_volumes()), ids=lambda c: c[0])
def test_properties_on_the_committed_reference_volumes(case):
    _, vol, idx, maximise = case
    N, D, H, W = vol.shape
    Vm = vol if maximise else -vol
    flags, idx_r, gap = vr.validity_ref(vol, idx, maximise, 1, 0.0)
    # first index on ties: nothing earlier on the diagonal reaches the winner, nothing at all beats it
    for x in range(W):
        n = min(D, W - x)
        diag = np.stack([Vm[:, d, :, x + d] for d in range(n)], 1)          # [N, n, H]
        win = np.take_along_axis(diag, idx_r[:, None, :, x], 1)[:, 0]
        assert (diag <= win[:, None]).all()
        earlier = np.arange(n)[None, :, None] < idx_r[:, None, :, x]
        assert not (earlier & (diag == win[:, None])).any()
    assert (idx_r + np.arange(W) < W).all() and (idx_r >= 0).all() and (idx_r < D).all()
    # IN_PATTERN against w - idx
    assert np.array_equal((flags & vr.IN_PATTERN) != 0, np.arange(W)[None, None] - idx >= 0)
    # the committed idx is the volume's argbest: the gap to any other disparity is never negative
    assert (gap >= 0).all()
    # lr_tol monotone, min_gap monotone; the other bits do not move
    prev = None
    for tol in (0, 1, 2, 5, D):
        f = vr.validity_ref(vol, idx, maximise, tol, 0.0)[0]
        if prev is not None:
            assert ((prev & vr.LR_OK) <= (f & vr.LR_OK)).all()
            assert np.array_equal(prev & ~np.uint8(vr.LR_OK), f & ~np.uint8(vr.LR_OK))
        prev = f
    assert np.array_equal((prev & vr.LR_OK) != 0, (prev & vr.IN_PATTERN) != 0)   # tolerance D: every in-pattern match
    prev = None
    for mg in (0.0, 0.01, 0.1, 1.0, 1e9):
        f = vr.validity_ref(vol, idx, maximise, 1, mg)[0]
        if prev is not None:
            assert ((prev & vr.UNIQUE) >= (f & vr.UNIQUE)).all()
            assert np.array_equal(prev & ~np.uint8(vr.UNIQUE), f & ~np.uint8(vr.UNIQUE))
        prev = f
    assert np.array_equal((prev & vr.UNIQUE) != 0, np.isposinf(gap))


def test_expected_lists_are_disjoint_and_see_ties():
    vol, idx = random_case(5, 2, 6, 4, 9, True)
    e = vr.expected_lists(vol, np.clip(idx, 0, 5), True, 0.0)
    assert e["col_must"].any() and e["pix_must"].any()
    assert not (e["col_must"] & e["col_never"]).any() and not (e["pix_must"] & e["pix_never"]).any()


def test_entry_points_validate_before_any_hip_call():
    from connecting_the_dots_amd import _lib, torchext
    import torch
    L = _lib.lib()
    assert L.ctd_match_validity_f32(None, 1, None, None, None, None, 1, 8, 8, 8, -1, 0.0, -1, None) == 1      # lr_tol < 0
    assert L.ctd_match_validity_f32(None, 1, None, None, None, None, 1, 8, 8, 8, 1, float("nan"), -1, None) == 1
    assert L.ctd_match_validity_f32(None, 1, None, None, None, None, 1, 8, 8, 8, 1, 0.0, -1, None) == 1       # NULL
    assert L.ctd_match_validity_f32(None, 1, None, None, None, None, 0, 8, 8, 8, 1, 0.0, -1, None) == 0       # no frames
    assert L.ctd_xcorrvol_validity_workspace_bytes(16, 1, 432, 512, 128, 9, 1) > 4 * 16 * 128 * 432 * 512
    assert L.ctd_xcorrvol_validity_workspace_bytes(2, 2, 32, 64, 16, 9, 1) == 0          # fast: one channel only
    assert L.ctd_xcorrvol_validity_workspace_bytes(2, 2, 32, 64, 16, 9, 0) > 0
    assert L.ctd_costvol_validity_workspace_bytes(2, 32, 64, 16, 11, 3, 1, 0) == 0       # fast: blocks 3/5/7/9
    assert L.ctd_costvol_validity_workspace_bytes(2, 32, 64, 16, 11, 3, 0, 0) > 0
    assert L.ctd_xcorrvol_validity_f32(None, None, 0, None, None, None, None, 1, 2, 8, 8, 4, 9, 1, 1, 0.0, None, 0, -1,
                                       None) == 1                                        # NULL pointers
    assert L.ctd_costvol_validity_f32(None, None, 0, None, None, None, None, 1, 8, 8, 4, 9, 7, 0.5, 0, 1, 0.0, None, 0,
                                      -1, None) == 1                                     # bad type
    for name in ("match_validity", "xcorrvol_validity", "costvol_validity"):
        assert hasattr(torchext, name)
    with pytest.raises(RuntimeError):
        torchext.match_validity(torch.zeros(1, 4, 3, 5), torch.zeros(1, 3, 5, dtype=torch.int64), True)   # CPU tensors
