"""CPU checks of band-limited semi-global matching (include/ext/ctd_hip_band_sgm.h) as tests/band_sgm_ref.py states it:
against tests/sgm_ref.py on the full volume with +inf outside each pixel's band (the rule's justification: bit-equal
where no band is empty), against an independent scalar triple loop where bands are empty or truncated, the full band
against sgm_ref outright; and -- through the library, no GPU needed -- the header's prototypes against bandsgm's
table, every rejection in the stated order, and that the pinned interface lists did not move."""
import ctypes
import glob
import os

import numpy as np
import pytest

from tests import band_sgm_ref as br
from tests import sgm_ref as sr
from tests.abi_headers import parse_header

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "ctd_hip_band_sgm.h")
PENS = [(0.0, 0.0), (0.3, 0.3), (0.02, 0.16), (0.1, 50.0)]


def random_bands(rs, shape, D, max_width, empty=0.0):
    """lo / hi int32 with widths 1 .. max_width inside [0, D-1]; a share `empty` of the pixels holds nothing"""
    width = rs.randint(1, min(max_width, D) + 1, size=shape)
    lo = np.array([rs.randint(0, D - w + 1) for w in width.ravel()]).reshape(shape)
    hi = lo + width - 1
    gone = rs.rand(*shape) < empty
    lo, hi = np.where(gone, lo + 3, lo), np.where(gone, lo - 1, hi)
    return lo.astype(np.int32), hi.astype(np.int32)


def masked(vol, lo, hi):
    """the full volume with +inf outside [lo, hi]"""
    d = np.arange(vol.shape[1])[None, :, None, None]
    return np.where((d >= lo[:, None]) & (d <= hi[:, None]), vol, F(np.inf)).astype(F)


def naive_band_path(C, l, n, dy, dx, p1, p2):
    """L of one direction over a band volume C [slots,H,W] (cost sign), one scalar at a time; NaN where unheld"""
    slots, H, W = C.shape
    p1, p2 = F(p1), F(p2)
    L = np.full_like(C, np.nan)
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
    xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
    for y in ys:
        for x in xs:
            qy, qx = y - dy, x - dx
            if not (0 <= qy < H and 0 <= qx < W) or n[qy, qx] == 0:
                for k in range(n[y, x]):
                    L[k, y, x] = C[k, y, x]
                continue
            nq = n[qy, qx]
            m = L[0, qy, qx]
            for k in range(1, nq):
                m = min(m, L[k, qy, qx])
            for k in range(n[y, x]):
                kq = l[y, x] + k - l[qy, qx]                 # the slot of q that holds the same disparity
                t = F(m + p2)
                if 0 <= kq < nq:
                    t = min(L[kq, qy, qx], t)
                if 0 <= kq - 1 < nq:
                    t = min(t, F(L[kq - 1, qy, qx] + p1))
                if 0 <= kq + 1 < nq:
                    t = min(t, F(L[kq + 1, qy, qx] + p1))
                L[k, y, x] = F(C[k, y, x] + F(t - m))
    return L


def naive_band_sgm(vb, lo, hi, D, p1, p2, paths, maximise=False):
    slots = vb.shape[1]
    l, n = br.band_rule(lo, hi, D, slots)
    S = []
    for f, v in enumerate(vb):
        acc = None
        for dy, dx in sr.directions(paths):
            L = naive_band_path(-v if maximise else v, l[f], n[f], dy, dx, p1, p2)
            acc = L if acc is None else (acc + L).astype(F)
        S.append(acc)
    S = np.stack(S)
    idx = np.full(lo.shape, -1, np.int64)
    best = np.full(lo.shape, np.nan, F)
    for (f, y, x), cnt in np.ndenumerate(n):
        for k in range(cnt):
            if idx[f, y, x] < 0 or S[f, k, y, x] < best[f, y, x]:
                idx[f, y, x], best[f, y, x] = l[f, y, x] + k, S[f, k, y, x]
    return S, idx, best


def same(a, b):
    """bit-equal, NaN masks included"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isnan(a), F(0), a).view(np.int32),
                                                                       np.where(np.isnan(b), F(0), b).view(np.int32))


def check_against_masked(vol, lo, hi, slots, pen, paths):
    N, D, H, W = vol.shape
    vb = br.band_gather(vol, lo, hi, slots)
    Sb, idx, best = br.band_sgm_ref(vb, lo, hi, D, pen[0], pen[1], paths)
    Sm, im, bm = sr.sgm_ref(masked(vol, lo, hi), pen[0], pen[1], paths)
    assert not np.isnan(Sm).any()
    assert same(br.band_expand(Sb, lo, hi, D, np.inf), Sm)             # bit-equal in band, +inf outside
    assert np.array_equal(idx, im) and same(best, bm)


MASKED_SHAPES = [(1, 1, 1), (1, 3, 4), (2, 1, 5), (2, 4, 1), (3, 3, 3), (5, 1, 1), (7, 4, 6), (12, 5, 7), (40, 3, 5),
                 (23, 6, 1), (31, 1, 9)]


@pytest.mark.parametrize("shape", MASKED_SHAPES)
@pytest.mark.parametrize("pen", PENS)
def test_band_rule_is_sgm_on_the_inf_masked_volume(shape, pen):
    """random bands of width 1 .. 5, no empty pixel, D = 1 .. 40, ragged H and W including 1, 4 and 8 paths"""
    D, H, W = shape
    rs = np.random.RandomState(D * 100 + H * 10 + W)
    vol = rs.rand(2, D, H, W).astype(F)
    lo, hi = random_bands(rs, (2, H, W), D, 5)
    for paths in (4, 8):
        check_against_masked(vol, lo, hi, 5, pen, paths)


@pytest.mark.parametrize("pen", [(0.0, 0.0), (0.25, 0.5)])
def test_tie_volumes_against_the_masked_volume(pen):
    rs = np.random.RandomState(3)
    vol = (rs.randint(0, 4, size=(2, 12, 5, 6)) * 0.25).astype(F)
    lo, hi = random_bands(rs, (2, 5, 6), 12, 5)
    for paths in (4, 8):
        check_against_masked(vol, lo, hi, 5, pen, paths)
    S, idx, best = br.band_sgm_ref(br.band_gather(vol, lo, hi, 5), lo, hi, 12, pen[0], pen[1], 8)
    for (f, y, x), i in np.ndenumerate(idx):                            # the first slot wins
        col = S[f, :hi[f, y, x] - lo[f, y, x] + 1, y, x]
        k = i - lo[f, y, x]
        assert col[k] == col.min() and not (col[:k] == col.min()).any() and best[f, y, x] == col[k]


@pytest.mark.parametrize("shape", [(1, 1, 1), (6, 3, 4), (9, 1, 6), (9, 5, 1), (12, 4, 5)])
@pytest.mark.parametrize("pen", PENS)
def test_reference_equals_the_scalar_restatement_with_empty_and_truncated_bands(shape, pen):
    """the restart at an empty predecessor, bands out of range, and bands wider than `slots`"""
    D, H, W = shape
    rs = np.random.RandomState(D * 100 + H * 10 + W + 7)
    vol = rs.rand(2, D, H, W).astype(F)
    lo, hi = random_bands(rs, (2, H, W), D, 6, empty=0.3)
    lo.flat[0], hi.flat[0] = -5, D + 5                                  # out of range both ways: clipped
    if lo.size > 2:
        lo.flat[1], hi.flat[1] = D, D + 3                               # beyond D: empty
        lo.flat[2], hi.flat[2] = -9, -1                                 # below 0: empty
    for slots in (1, 3, 6):
        vb = br.band_gather(vol, lo, hi, slots)
        l, n = br.band_rule(lo, hi, D, slots)
        assert n.max() <= slots and (n[lo > hi] == 0).all()
        assert np.array_equal(np.isnan(vb), np.arange(slots)[None, :, None, None] >= n[:, None])
        for maximise in (False, True):
            for paths in (4, 8):
                got = br.band_sgm_ref(vb, lo, hi, D, pen[0], pen[1], paths, maximise)
                want = naive_band_sgm(vb, lo, hi, D, pen[0], pen[1], paths, maximise)
                assert all(same(a, b) for a, b in zip(got, want)), (slots, maximise, paths)
                assert ((got[1] == -1) == (n == 0)).all() and (np.isnan(got[2]) == (n == 0)).all()


def test_truncation_keeps_the_first_slots():
    rs = np.random.RandomState(5)
    vol = rs.rand(1, 10, 3, 4).astype(F)
    lo = np.full((1, 3, 4), 2, np.int32)
    hi = np.full((1, 3, 4), 8, np.int32)
    vb = br.band_gather(vol, lo, hi, 3)
    assert np.array_equal(vb, vol[:, 2:5])
    cut = br.band_sgm_ref(vb, lo, hi, 10, 0.1, 0.4, 8)
    narrow = br.band_sgm_ref(vb, lo, lo + 2, 10, 0.1, 0.4, 8)
    assert all(same(a, b) for a, b in zip(cut, narrow))


@pytest.mark.parametrize("shape", [(1, 2, 3), (5, 4, 6), (8, 1, 7), (7, 6, 1)])
def test_full_band_equals_sgm_ref(shape):
    D, H, W = shape
    rs = np.random.RandomState(D + H + W)
    vol = rs.rand(2, D, H, W).astype(F)
    lo = np.zeros((2, H, W), np.int32)
    hi = np.full((2, H, W), D - 1, np.int32)
    vb = br.band_gather(vol, lo, hi, D)
    assert np.array_equal(vb, vol)
    for paths in (4, 8):
        for maximise in (False, True):
            got = br.band_sgm_ref(vb, lo, hi, D, 0.02, 0.16, paths, maximise)
            want = sr.sgm_ref(vol, 0.02, 0.16, paths, maximise)
            assert all(same(a, b) for a, b in zip(got, want))


# ---------------------------------------------------------------------------------------------------------------------
# the header, the table and the library
# ---------------------------------------------------------------------------------------------------------------------

C_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "size_t": ctypes.c_size_t}


def test_header_matches_the_module_table_and_the_library():
    from connecting_the_dots_amd import _lib, bandsgm
    functions, structs = parse_header(HEADER)
    assert not structs and list(functions) == list(bandsgm.TABLE)       # the header's order
    bound = bandsgm.lib()
    assert bound is _lib.lib()
    for name, (ret, params) in functions.items():
        res, args = bandsgm.TABLE[name]
        assert res is C_SCALARS[ret], name
        assert len(args) == len(params), name
        for i, (ctype, declared) in enumerate(zip(args, params)):
            assert (ctype is ctypes.c_void_p) if declared.endswith("*") else (ctype is C_SCALARS[declared]), (name, i)
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype == res, name
    text = open(HEADER).read()
    import re
    assert re.findall(r'#\s*include\s*[<"]([^>"]+)[>"]', text) == ["../ctd_hip.h"]


def test_the_pinned_interface_did_not_move():
    from connecting_the_dots_amd import _lib, bandsgm, torchext
    from connecting_the_dots_amd import build
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert headers == sorted(_lib.TABLES) and len(headers) == 14
    assert "ext/ctd_hip_band_sgm.h" not in _lib.TABLES and bandsgm.TABLE not in _lib.TABLES.values()
    assert not any(name in table for table in _lib.TABLES.values() for name in bandsgm.TABLE)
    assert len(torchext.functions.__all__) == 65
    assert not any(n in torchext.functions.__all__ for n in ("band_sgm_aggregate", "costvol_band_sgm", "band_width"))
    assert HEADER in build._headers()                                   # a stale header rebuilds


INVALID, WORKSPACE, UNSUPPORTED = 1, 2, 3


def test_entry_points_validate_before_any_hip_call():
    from connecting_the_dots_amd import bandsgm
    L = bandsgm.lib()
    buf = ctypes.create_string_buffer(1024)
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    nan, inf = float("nan"), float("inf")

    # the workspace query
    assert L.ctd_band_sgm_workspace_bytes(16, 5, 432, 512, 128, 8, 0) == 4 * 16 * 5 * 432 * 512
    assert L.ctd_band_sgm_workspace_bytes(1, 1, 1, 1, 1, 4, 0) == 4
    assert L.ctd_band_sgm_workspace_bytes(16, 5, 432, 512, 128, 8, 1) == 0    # S_b holds the volume
    for bad in ((16, 0, 432, 512, 128, 8), (16, 65, 432, 512, 128, 8), (16, 5, 432, 512, 128, 6), (0, 5, 432, 512, 128, 8),
                (-1, 5, 432, 512, 128, 8), (16, 5, 0, 512, 128, 8), (16, 5, 432, 0, 128, 8), (16, 5, 432, 512, 0, 8),
                (1024, 64, 432, 512, 128, 8)):
        assert L.ctd_band_sgm_workspace_bytes(*bad, 0) == 0, bad

    # ctd_band_sgm_aggregate_f32
    def agg(vol=p, lo=p, hi=p, p1=0.02, p2=0.16, paths=8, S=None, idx=p, best=p, frames=1, slots=5, H=8, W=8, D=16, ws=None,
            nws=0):
        return L.ctd_band_sgm_aggregate_f32(vol, lo, hi, 0, p1, p2, paths, S, idx, best, frames, slots, H, W, D, ws, nws,
                                            -1, None)

    for bad in (dict(slots=0), dict(slots=-3), dict(paths=5), dict(paths=0), dict(p1=-0.1), dict(p1=0.2, p2=0.1),
                dict(p1=nan), dict(p2=nan), dict(p2=inf), dict(p1=inf, p2=inf), dict(frames=-1), dict(D=0), dict(H=0),
                dict(W=-1), dict(H=65536, W=65536, D=1)):
        assert agg(**bad) == INVALID, bad
        assert agg(frames=0, **{k: v for k, v in bad.items() if k != "frames"}) == INVALID or "frames" in bad, bad
    assert agg(frames=0, vol=None, lo=None, hi=None, idx=None, best=None) == 0          # nothing to do
    for name in ("vol", "lo", "hi", "idx", "best"):
        assert agg(**{name: None}) == INVALID, name
        assert agg(slots=65, **{name: None}) == INVALID, name                           # NULLs before support
    assert agg(slots=65, paths=3) == INVALID                                            # scalars before support
    assert agg(slots=65) == UNSUPPORTED
    assert agg(frames=1 << 14, H=512, W=512, slots=1) == UNSUPPORTED                    # frames * H * W >= 2^31
    assert agg(frames=1 << 9, H=512, W=512, slots=64) == UNSUPPORTED                    # frames * slots * H * W >= 2^31
    assert agg(slots=65, ws=None) == UNSUPPORTED                                        # support before the workspace
    assert agg() == WORKSPACE                                                           # S_b and workspace NULL
    assert agg(ws=p, nws=4 * 5 * 64 - 1) == WORKSPACE                                   # short
    assert agg(ws=p + 4, nws=1 << 20) == WORKSPACE                                      # misaligned

    # the band volume calls
    def ncc(in0=p, in1=p, stride=0, lo=p, hi=p, vb=p, frames=1, slots=5, H=8, W=8, D=16, bs=5, flags=0, ws=p, nws=0):
        return L.ctd_xcorrvol_band_volume_f32(in0, in1, stride, lo, hi, vb, frames, slots, H, W, D, bs, flags, ws, nws, -1,
                                              None)

    def cost(im=p, pat=p, stride=0, lo=p, hi=p, vb=p, frames=1, slots=5, H=8, W=8, D=16, bs=5, type=1):
        return L.ctd_costvol_band_volume_f32(im, pat, stride, lo, hi, vb, frames, slots, H, W, D, bs, type, 0.1, -1, None)

    shared = (dict(slots=0), dict(bs=4), dict(bs=0), dict(bs=-1), dict(stride=7), dict(D=0), dict(H=0), dict(W=0),
              dict(frames=-1), dict(H=65536, W=65536, D=1))
    for bad in shared + (dict(flags=1), dict(flags=0x200)):
        assert ncc(**bad) == INVALID, bad
    for bad in shared + (dict(type=-1), dict(type=4)):
        assert cost(**bad) == INVALID, bad
    assert ncc(frames=0, in0=None, in1=None, lo=None, hi=None, vb=None, ws=None) == 0
    assert cost(frames=0, im=None, pat=None, lo=None, hi=None, vb=None) == 0
    assert ncc(frames=0, slots=0) == INVALID and cost(frames=0, type=9) == INVALID      # still checked
    for name in ("in0", "in1", "lo", "hi", "vb"):
        assert ncc(slots=65, **{name: None}) == INVALID, name
    for name in ("im", "pat", "lo", "hi", "vb"):
        assert cost(slots=65, **{name: None}) == INVALID, name
    assert ncc(slots=65, ws=None) == UNSUPPORTED and cost(slots=65) == UNSUPPORTED
    assert ncc(frames=1 << 14, H=512, W=512, slots=1, stride=512 * 512) == UNSUPPORTED
    assert cost(frames=1 << 9, H=512, W=512, slots=64) == UNSUPPORTED
    assert ncc(ws=None) == WORKSPACE and ncc(nws=16) == WORKSPACE and ncc(ws=p + 16, nws=1 << 30) == WORKSPACE
    assert ncc(flags=0x100, ws=None) == WORKSPACE                                       # CTD_PATTERN_PREPARED is a legal flag


def test_python_surface():
    import torch
    from connecting_the_dots_amd import bandsgm
    for name in ("band_width", "xcorrvol_band_volume", "costvol_band_volume", "band_sgm_aggregate", "xcorrvol_band_sgm",
                 "costvol_band_sgm", "band_volume_expand"):
        assert callable(getattr(bandsgm, name)), name
    lo = torch.tensor([[[0, 3, 9, -4]]], dtype=torch.int32)
    hi = torch.tensor([[[2, 2, 20, 1]]], dtype=torch.int32)
    assert bandsgm.band_width(lo, hi, 12) == 3 and bandsgm.band_width(lo, hi, 5) == 3
    assert bandsgm.band_width(lo[..., 1:2], hi[..., 1:2], 12) == 0
    with pytest.raises(RuntimeError):
        bandsgm.band_width(lo.long(), hi, 12)
    # band_volume_expand is torch only: against the numpy restatement, on the CPU
    rs = np.random.RandomState(0)
    vol = rs.rand(2, 9, 3, 4).astype(F)
    blo, bhi = random_bands(rs, (2, 3, 4), 9, 6, empty=0.3)
    vb = br.band_gather(vol, blo, bhi, 4)
    got = bandsgm.band_volume_expand(torch.from_numpy(vb), torch.from_numpy(blo), torch.from_numpy(bhi), 9, float("inf"))
    assert same(got.numpy(), br.band_expand(vb, blo, bhi, 9, np.inf))
    got3 = bandsgm.band_volume_expand(torch.from_numpy(vb[0]), torch.from_numpy(blo[0]), torch.from_numpy(bhi[0]), 9, -1.0)
    assert same(got3.numpy(), br.band_expand(vb[:1], blo[:1], bhi[:1], 9, -1.0)[0])
    z = torch.zeros(3, 5)
    i = torch.zeros(3, 5, dtype=torch.int32)
    with pytest.raises(RuntimeError):
        bandsgm.band_sgm_aggregate(torch.zeros(1, 4, 3, 5), i[None], i[None], 8, 0.02, 0.16)          # CPU tensors
    with pytest.raises(RuntimeError):
        bandsgm.costvol_band_volume(z, z, i, i, 4, 3, "sad", 0.5)
    with pytest.raises(RuntimeError):
        bandsgm.xcorrvol_band_sgm(z[None, None], z[None], i[None], i[None], 4, 3, 0.02, 0.16)
