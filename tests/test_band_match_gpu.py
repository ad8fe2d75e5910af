"""GPU parity of band-limited matching (torchext.xcorrvol_argmax_band / costvol_argmin_band): idx and best equal, bit for
bit, the restatement tests/band_ref.py applied to the reference-order volume of the same inputs (xcorrvol / costvol
algo="exact", themselves pinned to the reference goldens).  Every call is made twice and must return identical bits.

Shapes (H, W, D, bs): a single ragged tile; several tiles; a ragged block-9 case; D > W (every band reaches the
replicated left border); D = 1; three tile columns with a ragged last one at block 7; block 11 (the run-time block-size
path).  Each with 1 and 3 frames and with a shared and a per-frame pattern.  Band kinds: (a) the full range, (b) width 1,
(c) random ranges reaching outside [0, D-1] (empty, clipped at either end, wholly outside), (d) `disparity_band` of a
noisy prior with NaNs and a per-pixel radius, (e) exact ties (a constant pattern, a pattern of period 4 along the row)."""
import numpy as np
import pytest
import torch

from tests import workloads
from tests.band_ref import band_ref

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 4, 3), (16, 40, 8, 5), (24, 33, 16, 9), (12, 20, 32, 9), (9, 9, 1, 9), (33, 70, 64, 7), (10, 18, 8, 11)]
ALL_TYPES = ["mse", "sad", "census_mse", "census_sad"]
ALL_TYPE_SHAPES = [(16, 40, 8, 5), (24, 33, 16, 9)]


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scene(N, H, W, D, per_frame, seed):
    """frames [N,H,W] of workloads.synth_ir on a dot pattern, the pattern(s) [H,W] | [N,H,W], the true disparity"""
    rs = np.random.RandomState(seed)
    pat = workloads.syn_dot_pattern(H, W, seed)
    pats = np.stack([np.roll(pat, i, 1) for i in range(N)]) if per_frame else pat
    out = [workloads.synth_ir(pats[i] if per_frame else pat, rs, D, (8, 16)) for i in range(N)]
    return np.stack([o[0] for o in out]), pats, np.stack([o[1] for o in out])


def bands(te, N, H, W, D, gt, seed):
    """name -> (lo, hi) int32 CPU tensors [N,H,W] of the band kinds (a) .. (d)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    out["full"] = (torch.zeros(N, H, W, dtype=torch.int32), torch.full((N, H, W), D - 1, dtype=torch.int32))
    d = torch.randint(0, D, (N, H, W), generator=g, dtype=torch.int32)
    out["width1"] = (d, d.clone())
    # random ends in [-3, D+2]; an eighth each forced empty (lo > hi), to start left of 0, to end right of D-1, to lie
    # wholly left / wholly right of the range, to be the whole int32 range and to be the emptiest int32 range
    lo = torch.randint(-3, D + 3, (N, H, W), generator=g, dtype=torch.int32)
    hi = torch.randint(-3, D + 3, (N, H, W), generator=g, dtype=torch.int32)
    kind = torch.randint(0, 8, (N, H, W), generator=g)
    lo2, hi2 = torch.minimum(lo, hi), torch.maximum(lo, hi)
    lo = torch.where(kind == 0, hi2 + 1, lo2)                           # empty
    hi = torch.where(kind == 0, lo2, hi2)
    lo = torch.where(kind == 1, torch.full_like(lo, -3), lo)            # clipped at the left end
    hi = torch.where(kind == 2, torch.full_like(hi, D + 2), hi)         # clipped at the right end
    lo, hi = torch.where(kind == 3, torch.full_like(lo, -3), lo), torch.where(kind == 3, torch.full_like(hi, -1), hi)
    lo, hi = torch.where(kind == 4, torch.full_like(lo, D), lo), torch.where(kind == 4, torch.full_like(hi, D + 2), hi)
    big = 2 ** 31 - 1                                                   # any int32 is legal
    lo, hi = torch.where(kind == 5, torch.full_like(lo, -big - 1), lo), torch.where(kind == 5, torch.full_like(hi, big), hi)
    lo, hi = torch.where(kind == 6, torch.full_like(lo, big), lo), torch.where(kind == 6, torch.full_like(hi, -big - 1), hi)
    out["random"] = (lo.contiguous(), hi.contiguous())
    prior = torch.from_numpy(gt).float() + 1.5 * torch.randn(N, H, W, generator=g)
    prior[torch.rand(N, H, W, generator=g) < 0.1] = float("nan")
    radius = 4.0 * torch.rand(N, H, W, generator=g)
    radius[torch.rand(N, H, W, generator=g) < 0.05] = -1.0
    out["prior"] = te.disparity_band(prior, radius, D)
    return out


def assert_band(out, ref, what):
    idx, best = out[0].cpu(), out[1].cpu()
    ridx, rbest = ref
    assert idx.dtype == torch.int64 and best.dtype == torch.float32 and idx.shape == ridx.shape
    bad = int((idx != ridx).sum())
    assert bad == 0, "%s: %d of %d indices differ" % (what, bad, idx.numel())
    assert torch.equal(torch.isnan(best), idx < 0), what
    a = torch.where(idx < 0, torch.zeros_like(best), best).view(torch.int32)
    b = torch.where(ridx < 0, torch.zeros_like(rbest), rbest).view(torch.int32)
    bad = int((a != b).sum())
    assert bad == 0, "%s: %d of %d best values differ in their bits" % (what, bad, a.numel())


def same_bits(x, y):
    return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(x, y))


def check_kinds(te, call, vol, maximise, N, H, W, D, gt, seed, what):
    """kinds (a) .. (d) through `call(lo, hi)`, each twice; returns the full-range result"""
    full = None
    for name, (lo, hi) in bands(te, N, H, W, D, gt, seed).items():
        lo_d, hi_d = lo.cuda(), hi.cuda()
        out = call(lo_d, hi_d)
        assert_band(out, band_ref(vol, lo, hi, maximise), "%s %s" % (what, name))
        assert same_bits(out, call(lo_d, hi_d)), "%s %s: two runs differ" % (what, name)
        if name == "full":
            full = out
            assert int((out[0] < 0).sum()) == 0
        if name == "width1":
            assert torch.equal(out[0].cpu(), lo.to(torch.int64))
            assert torch.equal(out[1].cpu(), vol.cpu().gather(1, lo.to(torch.int64).unsqueeze(1)).squeeze(1))
        if name == "random":
            n_empty = int((out[0] < 0).sum())
            assert 0 < n_empty < out[0].numel(), "the random bands must mix empty and non-empty ranges"
    return full


# ---------------------------------------------------------------------------------------------------------------------
# 1. NCC
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_ncc_band_equals_band_ref(te, shape, N, per_frame):
    H, W, D, bs = shape
    fr, pat, gt = scene(N, H, W, D, per_frame, H * W + D + bs)
    in0 = dev(fr[:, None])
    in1 = dev(pat[:, None]) if per_frame else dev(pat[None])
    vol = te.xcorrvol_batch(in0, in1, D, bs, algo="exact")
    full = check_kinds(te, lambda lo, hi: te.xcorrvol_argmax_band(in0, in1, lo, hi, D, bs), vol, True, N, H, W, D, gt,
                       H + W + N, "ncc %s N %d per_frame %s" % (shape, N, per_frame))
    assert torch.equal(full[0], vol.argmax(1))
    if bs <= 9:           # (the fused exact matcher has kernels for blocks 3/5/7/9 only; block 11 has the volume's argmax)
        assert torch.equal(full[0], te.xcorrvol_argmax(in0, in1, D, bs, algo="exact")[0])


def tie_patterns(H, W, seed):
    rs = np.random.RandomState(seed)
    return {"zero": np.zeros((H, W), np.float32), "constant": np.full((H, W), 0.375, np.float32),
            "period4": np.tile(rs.rand(H, 4).astype(np.float32), (1, (W + 3) // 4))[:, :W]}


def tie_bands(N, H, W, D, seed):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randint(-2, D, (N, H, W), generator=g, dtype=torch.int32)
    hi = lo + torch.randint(-1, D + 1, (N, H, W), generator=g, dtype=torch.int32)
    return lo.contiguous(), hi.contiguous()


@pytest.mark.parametrize("shape", SHAPES)
def test_ncc_band_ties_take_the_first_index(te, shape):
    H, W, D, bs = shape
    N = 2
    fr = np.stack([workloads.uniform_frame(H * W + i, H, W)[0] for i in range(N)])
    in0 = dev(fr[:, None])
    lo, hi = tie_bands(N, H, W, D, H + D)
    lo_c, hi_c = lo.clamp(min=0).to(torch.int64), hi.clamp(max=D - 1).to(torch.int64)
    for name, pat in tie_patterns(H, W, bs).items():
        in1 = dev(pat[None])
        vol = te.xcorrvol_batch(in0, in1, D, bs, algo="exact")
        out = te.xcorrvol_argmax_band(in0, in1, lo.cuda(), hi.cuda(), D, bs)
        assert_band(out, band_ref(vol, lo, hi, True), "ncc ties %s %s" % (name, shape))
        assert same_bits(out, te.xcorrvol_argmax_band(in0, in1, lo.cuda(), hi.cuda(), D, bs))
        idx = out[0].cpu()
        if name == "zero":
            # every score is 0.0: the first index of the band.  (A non-zero constant is not flat in the reference's f32
            # window mean -- the sum of bs^2 quotients can miss it by an ulp -- so its scores are rounding noise; it is
            # checked against band_ref only.)
            assert bool((vol == 0).all())
            assert torch.equal(idx, torch.where(lo_c <= hi_c, lo_c, torch.full_like(lo_c, -1)))
        elif D > 4:
            v = vol.cpu()
            assert int((v[:, :-4] == v[:, 4:]).sum()) > 0              # the period gives exact ties at d, d + 4


# ---------------------------------------------------------------------------------------------------------------------
# 2. costs
# ---------------------------------------------------------------------------------------------------------------------
def cost_cases():
    for shape in SHAPES:
        for ty in (ALL_TYPES if shape in ALL_TYPE_SHAPES else ["sad", "census_sad"]):
            yield shape, ty


@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("shape,ty", list(cost_cases()))
def test_cost_band_equals_band_ref(te, shape, ty, N, per_frame):
    H, W, D, bs = shape
    fr, pat, gt = scene(N, H, W, D, per_frame, H * W + D + bs + 1)
    im, p = dev(fr), dev(pat)
    vol = te.costvol(im, p, D, bs, ty, 0.5, algo="exact")
    full = check_kinds(te, lambda lo, hi: te.costvol_argmin_band(im, p, lo, hi, D, bs, ty, 0.5), vol, False, N, H, W, D,
                       gt, H + W + N + 1, "%s %s N %d per_frame %s" % (ty, shape, N, per_frame))
    assert torch.equal(full[0], te.costvol_argmin(im, p, D, bs, ty, 0.5)[0])
    assert torch.equal(full[0], vol.argmin(1))


@pytest.mark.parametrize("ty", ["sad", "census_sad"])
@pytest.mark.parametrize("shape", SHAPES)
def test_cost_band_ties_take_the_first_index(te, shape, ty):
    H, W, D, bs = shape
    N = 2
    im = dev(np.stack([workloads.uniform_frame(H * W + 7 + i, H, W)[0] for i in range(N)]))
    lo, hi = tie_bands(N, H, W, D, H + D + 1)
    lo_c, hi_c = lo.clamp(min=0).to(torch.int64), hi.clamp(max=D - 1).to(torch.int64)
    for name, pat in tie_patterns(H, W, bs + 1).items():
        p = dev(pat)
        vol = te.costvol(im, p, D, bs, ty, 0.5, algo="exact")
        out = te.costvol_argmin_band(im, p, lo.cuda(), hi.cuda(), D, bs, ty, 0.5)
        assert_band(out, band_ref(vol, lo, hi, False), "%s ties %s %s" % (ty, name, shape))
        assert same_bits(out, te.costvol_argmin_band(im, p, lo.cuda(), hi.cuda(), D, bs, ty, 0.5))
        idx = out[0].cpu()
        if name != "period4":
            assert bool((vol == vol[:, :1]).all())                     # every cost of a pixel is equal
            assert torch.equal(idx, torch.where(lo_c <= hi_c, lo_c, torch.full_like(lo_c, -1)))
        elif D > 4:
            v = vol.cpu()
            assert int((v[:, :-4] == v[:, 4:]).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. the prepared pattern, the sub-pixel keyword, squeezed inputs, errors
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_frame", [False, True])
def test_prepared_handle_is_shared_with_the_subpixel_op(te, per_frame):
    N, H, W, D, bs = 3, 24, 33, 16, 9
    fr, pat, gt = scene(N, H, W, D, per_frame, 99)
    in0 = dev(fr[:, None])
    in1 = dev(pat[:, None]) if per_frame else dev(pat[None])
    lo, hi = (t.cuda() for t in bands(te, N, H, W, D, gt, 5)["prior"])
    plain = te.xcorrvol_argmax_band(in0, in1, lo, hi, D, bs)
    some_idx = torch.from_numpy(gt).cuda().clamp(0, D - 1)
    sub_plain = te.xcorrvol_subpixel(in0, in1, some_idx, D, bs)
    # the sub-pixel op fills the planes, the band call reuses them, the sub-pixel op reuses them again
    h = te.prepare_pattern(in1, N, D, bs)
    assert same_bits(te.xcorrvol_subpixel(in0, in1, some_idx, D, bs, prepared=h), sub_plain)
    assert len(h.subpixel) == 1
    for _ in range(2):
        assert same_bits(te.xcorrvol_argmax_band(in0, in1, lo, hi, D, bs, prepared=h), plain)
    assert same_bits(te.xcorrvol_subpixel(in0, in1, some_idx, D, bs, prepared=h), sub_plain)
    assert len(h.subpixel) == 1
    # the other way round: the band call fills them
    h2 = te.prepare_pattern(in1, N, D, bs)
    assert same_bits(te.xcorrvol_argmax_band(in0, in1, lo, hi, D, bs, prepared=h2), plain)
    assert same_bits(te.xcorrvol_subpixel(in0, in1, some_idx, D, bs, prepared=h2), sub_plain)
    assert same_bits(te.xcorrvol_argmax_band(in0, in1, lo, hi, D, bs, prepared=h2), plain)
    assert len(h2.subpixel) == 1
    with pytest.raises(RuntimeError):
        te.xcorrvol_argmax_band(in0, in1.clone(), lo, hi, D, bs, prepared=h)       # another pattern tensor


def test_subpixel_keyword_appends_the_refinement(te):
    N, H, W, D, bs = 2, 16, 40, 8, 5
    fr, pat, gt = scene(N, H, W, D, False, 123)
    in0, in1 = dev(fr[:, None]), dev(pat[None])
    lo, hi = (t.cuda() for t in bands(te, N, H, W, D, gt, 6)["prior"])
    out = te.xcorrvol_argmax_band(in0, in1, lo, hi, D, bs, subpixel="parabola")
    assert len(out) == 4 and same_bits(out[:2], te.xcorrvol_argmax_band(in0, in1, lo, hi, D, bs))
    assert int((out[0] < 0).sum()) > 0
    assert same_bits(out[2:], te.xcorrvol_subpixel(in0, in1, out[0], D, bs, "parabola"))
    assert bool(torch.isnan(out[2][out[0] < 0]).all()) and int(out[3][out[0] < 0].sum()) == 0
    im, p = dev(fr), dev(pat)
    out = te.costvol_argmin_band(im, p, lo, hi, D, bs, "sad", 0.5, subpixel="equiangular")
    assert len(out) == 4 and same_bits(out[:2], te.costvol_argmin_band(im, p, lo, hi, D, bs, "sad", 0.5))
    assert same_bits(out[2:], te.costvol_subpixel(im, p, out[0], D, bs, "sad", 0.5, "equiangular"))
    with pytest.raises(RuntimeError):
        te.xcorrvol_argmax_band(in0, in1, lo, hi, D, bs, subpixel="cubic")


def test_squeezed_inputs(te):
    H, W, D, bs = 16, 40, 8, 5
    fr, pat, gt = scene(1, H, W, D, False, 31)
    lo, hi = bands(te, 1, H, W, D, gt, 7)["random"]
    in0, in1 = dev(fr), dev(pat[None])                                  # [1,H,W] frame, lo / hi [H,W]
    idx, best = te.xcorrvol_argmax_band(in0, in1, lo[0].cuda(), hi[0].cuda(), D, bs)
    assert idx.shape == (H, W) and best.shape == (H, W)
    vol = te.xcorrvol_batch(in0[None], in1, D, bs, algo="exact")
    assert_band((idx[None], best[None]), band_ref(vol, lo, hi, True), "squeezed ncc")
    idx, best = te.costvol_argmin_band(dev(fr[0]), dev(pat), lo[0].cuda(), hi[0].cuda(), D, bs, "sad", 0.5)
    assert idx.shape == (H, W)
    vol = te.costvol(dev(fr), dev(pat), D, bs, "sad", 0.5, algo="exact")
    assert_band((idx[None], best[None]), band_ref(vol, lo, hi, False), "squeezed sad")


def test_wrapper_errors(te):
    N, H, W, D, bs = 1, 16, 40, 8, 5
    fr, pat, _ = scene(N, H, W, D, False, 8)
    in0, in1 = dev(fr[:, None]), dev(pat[None])
    lo = torch.zeros(N, H, W, dtype=torch.int32, device="cuda")
    hi = torch.full((N, H, W), D - 1, dtype=torch.int32, device="cuda")
    calls = [lambda lo, hi: te.xcorrvol_argmax_band(in0, in1, lo, hi, D, bs),
             lambda lo, hi: te.costvol_argmin_band(dev(fr), dev(pat), lo, hi, D, bs, "sad")]
    for call in calls:
        assert len(call(lo, hi)) == 2
        for bad in ((lo.float(), hi), (lo, hi.long()), (lo[:, :8], hi), (lo, hi[:, :, :8]), (lo.cpu(), hi), (lo, hi.cpu()),
                    (lo.transpose(1, 2), hi.transpose(1, 2)), (lo[0], hi[0])):
            with pytest.raises(RuntimeError):
                call(*bad)
    with pytest.raises(RuntimeError):
        te.xcorrvol_argmax_band(in0, in1, lo, hi, D, 4)                 # even block
    with pytest.raises(RuntimeError):
        te.xcorrvol_argmax_band(in0.double(), in1.double(), lo, hi, D, bs)
    with pytest.raises(RuntimeError):
        te.costvol_argmin_band(dev(fr), dev(pat), lo, hi, D, bs, "nope")
    with pytest.raises(RuntimeError):
        te.costvol_argmin_band(dev(fr), dev(pat), lo, hi, D, 6, "sad")
