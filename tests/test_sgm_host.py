"""CPU checks of the semi-global aggregation rule (include/ctd_hip.h) as tests/sgm_ref.py states it: against an
independent scalar triple-loop restatement on tiny shapes (every direction alone, 4 and 8 paths, D = 1, 2, 3, 7,
H = 1 and W = 1), one case computed by hand, and -- through the library, no GPU needed -- the workspace query, the
argument validation that precedes any HIP call, and the Python surface."""
import numpy as np
import pytest

from tests import sgm_ref as sr

F = np.float32


def naive_path(C, dy, dx, p1, p2):
    """L of one direction, one scalar at a time"""
    D, H, W = C.shape
    p1, p2 = F(p1), F(p2)
    L = np.zeros_like(C)
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
    xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
    for y in ys:
        for x in xs:
            qy, qx = y - dy, x - dx
            if not (0 <= qy < H and 0 <= qx < W):
                for d in range(D):
                    L[d, y, x] = C[d, y, x]
                continue
            m = L[0, qy, qx]
            for k in range(1, D):
                m = min(m, L[k, qy, qx])
            for d in range(D):
                t = min(L[d, qy, qx], F(m + p2))
                if d >= 1:
                    t = min(t, F(L[d - 1, qy, qx] + p1))
                if d + 1 < D:
                    t = min(t, F(L[d + 1, qy, qx] + p1))
                L[d, y, x] = F(C[d, y, x] + F(t - m))
    return L


def naive_aggregate(C, p1, p2, paths):
    S = None
    for dy, dx in sr.directions(paths):
        L = naive_path(C, dy, dx, p1, p2)
        S = L if S is None else (S + L).astype(F)
    return S


SHAPES = [(1, 1, 1), (1, 3, 4), (2, 1, 5), (2, 4, 1), (3, 3, 3), (3, 1, 1), (7, 4, 6), (7, 5, 3), (2, 6, 7)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pen", [(0.0, 0.0), (0.3, 0.3), (0.02, 0.16), (0.1, 50.0)])
def test_reference_equals_the_scalar_restatement(shape, pen):
    D, H, W = shape
    rs = np.random.RandomState(D * 100 + H * 10 + W)
    C = rs.rand(D, H, W).astype(F)
    for name, (dy, dx) in zip(sr.NAMES, sr.DIRECTIONS):
        got, want = sr.path_cost(C, dy, dx, *pen), naive_path(C, dy, dx, *pen)
        assert got.dtype == F and np.array_equal(got, want), name
    for paths in (4, 8):
        assert np.array_equal(sr.aggregate(C, pen[0], pen[1], paths), naive_aggregate(C, pen[0], pen[1], paths))


def test_planted_ties_and_maximise():
    """few distinct values: ties everywhere; the first index wins; maximise negates the input exactly"""
    rs = np.random.RandomState(1)
    vol = (rs.randint(0, 4, size=(2, 5, 4, 6)) * 0.25).astype(F)
    S, idx, best = sr.sgm_ref(vol, 0.25, 0.5, 8, False)
    for f in range(2):
        assert np.array_equal(S[f], naive_aggregate(vol[f], 0.25, 0.5, 8))
    for (f, y, x), i in np.ndenumerate(idx):
        col = S[f, :, y, x]
        assert col[i] == col.min() and not (col[:i] == col.min()).any() and best[f, y, x] == col[i]
    Sm, im, bm = sr.sgm_ref(-vol, 0.25, 0.5, 8, True)
    assert np.array_equal(Sm, S) and np.array_equal(im, idx) and np.array_equal(bm, best)
    s3 = sr.sgm_ref(vol[0], 0.25, 0.5, 4)
    s4 = sr.sgm_ref(vol[:1], 0.25, 0.5, 4)
    assert s3[0].shape == (5, 4, 6) and all(np.array_equal(a, b[0]) for a, b in zip(s3, s4))
    with pytest.raises(ValueError):
        sr.sgm_ref(vol, 0.1, 0.2, 5)


def test_one_case_by_hand():
    """D = 3, one row of three pixels, direction right, P1 = 1, P2 = 4 (all values exact in f32).
    x = 0: no predecessor, L = C = (5, 1, 7).
    x = 1: m = 1.  t(0) = min(5, 1 + 4, L(1) + 1 = 2) = 2;  t(1) = min(1, 5, 5 + 1, 7 + 1) = 1;
           t(2) = min(7, 5, L(1) + 1 = 2) = 2.  L = C + (t - m) = (2 + 1, 9 + 0, 0 + 1) = (3, 9, 1).
    x = 2: m = 1.  t(0) = min(3, 5, 9 + 1) = 3;  t(1) = min(9, 5, 3 + 1, 1 + 1) = 2;  t(2) = min(1, 5, 9 + 1) = 1.
           L = (4 + 2, 4 + 1, 4 + 0) = (6, 5, 4)."""
    C = np.array([[[5, 2, 4]], [[1, 9, 4]], [[7, 0, 4]]], F)          # [D=3, H=1, W=3]
    L = sr.path_cost(C, 0, 1, 1.0, 4.0)
    assert np.array_equal(L[:, 0, 0], [5, 1, 7])
    assert np.array_equal(L[:, 0, 1], [3, 9, 1])
    assert np.array_equal(L[:, 0, 2], [6, 5, 4])
    # one row: the vertical and diagonal directions have no predecessor anywhere
    for dy, dx in sr.DIRECTIONS[2:]:
        assert np.array_equal(sr.path_cost(C, dy, dx, 1.0, 4.0), C)
    # left: x = 2 starts; x = 1: m = 4, t = (4, 4, 4) -> L = C; x = 0: L(q) = (2, 9, 0), m = 0,
    #   t(0) = min(2, 4, 9 + 1) = 2, t(1) = min(9, 4, 2 + 1, 0 + 1) = 1, t(2) = 0 -> L = (7, 2, 7)
    Ll = sr.path_cost(C, 0, -1, 1.0, 4.0)
    assert np.array_equal(Ll[:, 0, 1], [2, 9, 0]) and np.array_equal(Ll[:, 0, 0], [7, 2, 7])
    S, idx, best = sr.sgm_ref(C, 1.0, 4.0, 4)
    assert np.array_equal(S, ((L + Ll) + C) + C)
    # S = (22, 5, 28) at x = 0, (9, 36, 1) at x = 1, (18, 17, 16) at x = 2
    assert np.array_equal(idx[0], [1, 2, 2]) and np.array_equal(best[0], [5, 1, 16])


def test_entry_points_validate_before_any_hip_call():
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    V = 16 * 128 * 432 * 512
    assert L.ctd_version() == 5
    assert L.ctd_sgm_workspace_bytes(16, 128, 432, 512, 8, 0) == 4 * V
    assert L.ctd_sgm_workspace_bytes(16, 128, 432, 512, 4, 0) == 4 * V
    assert L.ctd_sgm_workspace_bytes(16, 128, 432, 512, 8, 1) == 0        # S_out holds the volume
    assert L.ctd_sgm_workspace_bytes(1, 1, 1, 1, 4, 0) == 4
    assert L.ctd_sgm_workspace_bytes(16, 128, 432, 512, 6, 0) == 0        # paths
    assert L.ctd_sgm_workspace_bytes(0, 128, 432, 512, 8, 0) == 0
    assert L.ctd_sgm_workspace_bytes(16, 257, 43, 51, 8, 0) == 0          # D > 256: unsupported
    assert L.ctd_sgm_workspace_bytes(64, 128, 432, 1024, 8, 0) == 0       # >= 2^31 elements

    def call(p1=0.02, p2=0.16, paths=8, frames=1, D=8, H=8, W=8):
        return L.ctd_sgm_aggregate_f32(None, 0, p1, p2, paths, None, None, None, frames, D, H, W, None, 0, -1, None)

    INVALID, UNSUPPORTED = 1, 3
    assert call() == INVALID                                              # NULL pointers
    for bad in (dict(paths=5), dict(paths=0), dict(p1=-0.1), dict(p1=0.2, p2=0.1), dict(p1=float("nan")),
                dict(p2=float("nan")), dict(p2=float("inf")), dict(p1=float("inf"), p2=float("inf")), dict(frames=0),
                dict(D=0), dict(H=0), dict(W=-1), dict(frames=64, D=128, H=432, W=1024)):
        assert call(**bad) == INVALID, bad
    # with pointers that are never dereferenced: validation, then support, then the workspace, all before any HIP call
    import ctypes
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def call_p(D=8, **k):
        a = dict(p1=0.02, p2=0.16, paths=8)
        a.update(k)
        return L.ctd_sgm_aggregate_f32(p, 0, a["p1"], a["p2"], a["paths"], None, p, p, 1, D, 8, 8, None, 0, -1, None)

    assert call_p(paths=7) == INVALID and call_p(p1=0.5) == INVALID
    assert call_p(D=257) == UNSUPPORTED
    assert call_p() == 2                                                  # CTD_ERR_WORKSPACE: S_out and workspace NULL


def test_python_surface():
    import torch
    from connecting_the_dots_amd import torchext
    for name in ("sgm_aggregate", "costvol_sgm", "xcorrvol_sgm"):
        assert callable(getattr(torchext, name))
    with pytest.raises(RuntimeError):
        torchext.sgm_aggregate(torch.zeros(1, 4, 3, 5), 0.02, 0.16)                      # CPU tensor
    with pytest.raises(RuntimeError):
        torchext.costvol_sgm(torch.zeros(3, 5), torch.zeros(3, 5), 4, 3, "sad", 0.5, 0.02, 0.16)
    with pytest.raises(RuntimeError):
        torchext.xcorrvol_sgm(torch.zeros(1, 1, 3, 5), torch.zeros(1, 3, 5), 4, 3, 0.02, 0.16)
