"""GPU parity of the sub-pixel refinement (torchext.xcorrvol_subpixel / costvol_subpixel and the `subpixel` keyword of
the matchers): the refined disparity and the refined flag equal, bit for bit, a torch-CPU float32 restatement of the
rule in include/ctd_hip.h applied to the entries of the reference-order volume (xcorrvol / costvol algo="exact", itself
pinned to the reference goldens) gathered at idx - 1, idx, idx + 1.  Also: the edge cases of the rule, and the accuracy
gain on the Kinect pattern shifted by a known fraction of a pixel."""
import numpy as np
import pytest
import torch

from tests import workloads
from tests.subpixel_ref import fit_reference
from tests.util import golden

pytestmark = pytest.mark.gpu

TYPES = ["mse", "sad", "census_mse", "census_sad"]
MODES = ["parabola", "equiangular"]


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_bits(disp, refined, ref, what=""):
    rd, rr = ref
    disp, refined = disp.cpu(), refined.cpu()
    assert disp.dtype == torch.float32 and refined.dtype == torch.uint8
    assert disp.shape == rd.shape and refined.shape == rr.shape
    assert torch.equal(torch.isnan(disp), torch.isnan(rd)), what
    a = torch.where(torch.isnan(disp), torch.zeros_like(disp), disp).view(torch.int32)
    b = torch.where(torch.isnan(rd), torch.zeros_like(rd), rd).view(torch.int32)
    bad = int((a != b).sum())
    assert bad == 0, "%s: %d of %d disparities differ" % (what, bad, a.numel())
    assert torch.equal(refined, rr), what


def frames_for(kind, N, H, W, D, seed):
    rs = np.random.RandomState(seed)
    if kind == "uniform":
        return np.stack([workloads.uniform_frame(seed + i, H, W)[0] for i in range(N)]), rs.rand(H, W).astype(np.float32)
    pat = workloads.syn_dot_pattern(H, W, seed)
    return np.stack([workloads.synth_ir(pat, rs, D, (8, 16))[0] for _ in range(N)]), pat


# ---------------------------------------------------------------------------------------------------------------------
# 1. NCC, standalone op
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "dots"])
@pytest.mark.parametrize("bs", [3, 5, 7, 9, 11])
@pytest.mark.parametrize("shape", [(5, 37, 16, 2, True), (23, 130, 128, 1, False), (17, 61, 1, 1, False),
                                   (9, 50, 2, 2, False), (12, 66, 16, 3, False)])
def test_ncc_standalone_equals_rule_on_exact_volume(te, shape, bs, kind):
    """ragged W, H < block, D = 1 / 2 / 16 / 128, shared and per-frame patterns; the argmax and random indices"""
    H, W, D, N, per_frame = shape
    fr, pat = frames_for(kind, N, H, W, D, H * W + bs)
    in0 = dev(fr[:, None])
    if per_frame:
        in1 = dev(np.stack([np.roll(pat, i, 1) for i in range(N)])[:, None])
    else:
        in1 = dev(pat[None])
    vol = te.xcorrvol_batch(in0, in1, D, bs, algo="exact")
    gen = torch.Generator().manual_seed(H * W * D + bs)
    idxs = {"argmax": vol.argmax(1), "random": torch.randint(0, D, (N, H, W), generator=gen).cuda()}
    for name, idx in idxs.items():
        for mode in MODES:
            disp, refined = te.xcorrvol_subpixel(in0, in1, idx, D, bs, mode)
            assert_bits(disp, refined, fit_reference(vol, idx, True, mode), "%s %s bs %d %s" % (name, mode, bs, shape))
    if D >= 3 and kind == "dots":
        assert int(te.xcorrvol_subpixel(in0, in1, idxs["argmax"], D, bs)[1].sum()) > 0


def test_ncc_standalone_squeezed_frame(te):
    fr, pat = frames_for("dots", 1, 20, 40, 12, 7)
    in0, in1 = dev(fr), dev(pat[None])                 # [1,H,W] frame, idx [H,W]
    vol = te.xcorrvol_batch(in0[None], in1, 12, 5, algo="exact")
    idx = vol[0].argmax(0)
    disp, refined = te.xcorrvol_subpixel(in0, in1, idx, 12, 5)
    assert disp.shape == (20, 40)
    assert_bits(disp[None], refined[None], fit_reference(vol, idx[None], True, "parabola"))


# ---------------------------------------------------------------------------------------------------------------------
# 2. through the NCC matchers
# ---------------------------------------------------------------------------------------------------------------------
def _lcn_inputs(te, N, H, W, D, seed):
    rs = np.random.RandomState(seed)
    pat = workloads.syn_dot_pattern(H, W, seed)
    raw = dev(np.stack([workloads.synth_ir(pat, rs, D, (16, 32))[0] for _ in range(N)])[:, None])
    pat_lcn = te.lcn(dev(pat[None, None]), 5, 0.05)[0][0].contiguous()
    return raw, pat_lcn


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,bs", [(128, 9), (126, 9), (128, 7)])    # ranked fast path; unranked; block 7
def test_xcorrvol_argmax_subpixel(te, mode, W, bs):
    N, H, D = 2, 40, 64
    raw, pat_lcn = _lcn_inputs(te, N, H, W, D, W + bs)
    x = te.lcn(raw, 5, 0.05)[0]
    vol = te.xcorrvol_batch(x, pat_lcn, D, bs, algo="exact")
    plain = te.xcorrvol_argmax(x, pat_lcn, D, bs)
    out = te.xcorrvol_argmax(x, pat_lcn, D, bs, subpixel=mode)
    assert len(out) == 4 and torch.equal(out[0], plain[0]) and torch.equal(out[1], plain[1])
    assert_bits(out[2], out[3], fit_reference(vol, out[0], True, mode), "xcorrvol_argmax")
    out = te.xcorrvol_argmax(x, pat_lcn, D, bs, return_volume=True, subpixel=mode)
    assert len(out) == 5 and out[2].shape == (N, D, H, W) and torch.equal(out[0], plain[0])
    assert_bits(out[3], out[4], fit_reference(vol, out[0], True, mode), "xcorrvol_argmax + volume")
    # a prepared pattern keeps the planes of this op: the second call reuses them
    h = te.prepare_pattern(pat_lcn, N, D, bs)
    for _ in range(2):
        out = te.xcorrvol_argmax(x, pat_lcn, D, bs, prepared=h, subpixel=mode)
        assert torch.equal(out[0], plain[0])
        assert_bits(out[2], out[3], fit_reference(vol, out[0], True, mode), "xcorrvol_argmax prepared")
    assert len(h.subpixel) == 1


def test_xcorrvol_argmax_subpixel_default_is_unchanged(te):
    raw, pat_lcn = _lcn_inputs(te, 1, 24, 64, 32, 5)
    x = te.lcn(raw, 5, 0.05)[0]
    assert len(te.xcorrvol_argmax(x, pat_lcn, 32, 9)) == 2
    assert len(te.xcorrvol_argmax(x, pat_lcn, 32, 9, subpixel=None)) == 2
    assert len(te.lcn_xcorrvol_argmax(raw, pat_lcn, 32, 9, subpixel=None)) == 4


@pytest.mark.parametrize("lcn_algo", ["exact", "fast"])
@pytest.mark.parametrize("W", [128, 122])                           # fused kernel; W % 4 != 0 takes the fallback
@pytest.mark.parametrize("mode", MODES)
def test_lcn_xcorrvol_argmax_subpixel_refines_against_its_lcn(te, lcn_algo, W, mode):
    N, H, D = 2, 36, 48
    raw, pat_lcn = _lcn_inputs(te, N, H, W, D, W)
    out = te.lcn_xcorrvol_argmax(raw, pat_lcn, D, 9, lcn_algo=lcn_algo, subpixel=mode)
    assert len(out) == 6
    y, idx = out[0], out[2]
    vol = te.xcorrvol_batch(y, pat_lcn, D, 9, algo="exact")
    assert_bits(out[4], out[5], fit_reference(vol, idx, True, mode), "lcn_xcorrvol_argmax %s" % lcn_algo)
    h = te.prepare_pattern(pat_lcn, N, D, 9)
    out = te.lcn_xcorrvol_argmax(raw, pat_lcn, D, 9, lcn_algo=lcn_algo, subpixel=mode, prepared=h, return_volume=True)
    assert len(out) == 7
    assert_bits(out[5], out[6], fit_reference(vol, out[2], True, mode), "lcn_xcorrvol_argmax prepared")


# ---------------------------------------------------------------------------------------------------------------------
# 3. costs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", [3, 5, 7, 9])
@pytest.mark.parametrize("ty", TYPES)
def test_costs_equal_rule_on_exact_volume(te, ty, bs):
    N, H, W, D = 2, 21, 75, 24
    rs = np.random.RandomState(bs * 7 + len(ty))
    pat = rs.randn(H, W).astype(np.float32)
    im = np.stack([np.roll(pat, 5 + 3 * i, 1) + 0.2 * rs.randn(H, W).astype(np.float32) for i in range(N)])
    for per_frame in (False, True):
        p = dev(np.stack([pat] * N) if per_frame else pat)
        vol = te.costvol(dev(im), p, D, bs, ty, 0.5, algo="exact")
        gen = torch.Generator().manual_seed(bs + D)
        for idx in (vol.argmin(1), torch.randint(0, D, (N, H, W), generator=gen).cuda()):
            for mode in MODES:
                disp, refined = te.costvol_subpixel(dev(im), p, idx, D, bs, ty, 0.5, mode)
                assert_bits(disp, refined, fit_reference(vol, idx, False, mode), "%s bs %d %s" % (ty, bs, mode))
        for mode in MODES:
            out = te.costvol_argmin(dev(im), p, D, bs, ty, 0.5, subpixel=mode)
            assert len(out) == 4 and torch.equal(out[0], vol.argmin(1))
            assert_bits(out[2], out[3], fit_reference(vol, out[0], False, mode), "costvol_argmin %s bs %d" % (ty, bs))
    out = te.costvol_argmin(dev(im), dev(pat), D, bs, ty, 0.5, return_rescored=True, subpixel="parabola")
    assert len(out) == 5 and out[3].dtype == torch.float32 and out[4].dtype == torch.uint8


def test_cost_odd_block_beyond_nine_and_squeezed(te):
    rs = np.random.RandomState(11)
    pat = rs.randn(19, 47).astype(np.float32)
    im = np.roll(pat, 4, 1)
    vol = te.costvol(dev(im), dev(pat), 10, 11, "sad", 0.5, algo="exact")
    idx, _, disp, refined = te.costvol_argmin(dev(im), dev(pat), 10, 11, "sad", 0.5, subpixel="equiangular")
    assert disp.shape == (19, 47)
    assert_bits(disp[None], refined[None], fit_reference(vol[None], idx[None], False, "equiangular"))


# ---------------------------------------------------------------------------------------------------------------------
# 4. edge cases
# ---------------------------------------------------------------------------------------------------------------------
def test_end_indices_are_not_refined(te):
    fr, pat = frames_for("dots", 1, 16, 40, 10, 3)
    in0, in1 = dev(fr[:, None]), dev(pat[None])
    for d in (0, 9):
        idx = torch.full((1, 16, 40), d, dtype=torch.int64, device="cuda")
        disp, refined = te.xcorrvol_subpixel(in0, in1, idx, 10, 5)
        assert bool((disp == d).all()) and int(refined.sum()) == 0
        disp, refined = te.costvol_subpixel(dev(fr), dev(pat), idx, 10, 5, "sad")
        assert bool((disp == d).all()) and int(refined.sum()) == 0


def test_constant_frame_is_not_refined(te):
    """a frame whose reference-order window mean is its value (0 for any block; any value for block 1) has every
    score 0 / (0 + 1e-8) = 0.  (Other constants are not flat in the reference's f32 arithmetic: the mean of bs^2
    quotients x / bs^2 can miss x by an ulp, and the scores are then rounding noise.)"""
    _, pat = frames_for("dots", 1, 16, 40, 10, 4)
    idx = torch.randint(0, 10, (1, 16, 40), generator=torch.Generator().manual_seed(0)).cuda()
    for value, bs in ((0.0, 5), (0.0, 9), (0.75, 1)):
        in0 = torch.full((1, 1, 16, 40), value, device="cuda")
        for mode in MODES:
            disp, refined = te.xcorrvol_subpixel(in0, dev(pat[None]), idx, 10, bs, mode)
            assert torch.equal(disp, idx.float()) and int(refined.sum()) == 0


def _tie_scene(H=20, W=64, X1=30, seed=5):
    """pattern rows r(h) up to column X1, noise right of it; the frame is r(h) everywhere: for pixel (h, w) every
    disparity d >= w + half - X1 sees the same clean window, d = w + half - X1 - 1 a contaminated one"""
    rs = np.random.RandomState(seed)
    r = rs.rand(H, 1).astype(np.float32)
    pat = np.repeat(r, W, 1)
    pat[:, X1 + 1:] = rs.rand(H, W - X1 - 1).astype(np.float32)
    fr = np.repeat(r, W, 1)
    return fr, pat


def test_constructed_tie_gives_exactly_half(te):
    H, W, X1, D, bs = 20, 64, 30, 24, 5
    fr, pat = _tie_scene(H, W, X1)
    half = bs // 2
    dstar = torch.arange(W).view(1, 1, W).expand(1, H, W) + half - X1
    use = (dstar >= 1) & (dstar <= D - 2)
    idx = dstar.clamp(0, D - 1).contiguous().cuda()
    checks = [(te.xcorrvol_batch(dev(fr[None, None]), dev(pat[None]), D, bs, algo="exact"), True,
               lambda mode: te.xcorrvol_subpixel(dev(fr[None, None]), dev(pat[None]), idx, D, bs, mode))]
    for ty in ("sad", "census_sad"):
        checks.append((te.costvol(dev(fr[None]), dev(pat), D, bs, ty, 0.5, algo="exact"), False,
                       lambda mode, ty=ty: te.costvol_subpixel(dev(fr[None]), dev(pat), idx, D, bs, ty, 0.5, mode)))
    for vol, maximum, call in checks:
        v = vol.cpu()
        ic = idx.cpu().unsqueeze(1)
        s0, sp, sm = (v.gather(1, (ic + k).clamp(0, D - 1)).squeeze(1) for k in (0, 1, -1))
        tie = use & (sp == s0) & ((sm < s0) if maximum else (sm > s0))
        assert int(tie.sum()) >= 10 * H
        for mode in MODES:
            disp, refined = call(mode)
            disp, refined = disp.cpu(), refined.cpu()
            assert torch.equal(disp[tie], ic.squeeze(1)[tie].float() + 0.5)
            assert bool((refined[tie] == 1).all())


def test_indices_outside_the_range_give_nan(te):
    fr, pat = frames_for("dots", 1, 16, 40, 10, 6)
    for bad in (-1, 10):
        idx = torch.full((1, 16, 40), bad, dtype=torch.int64, device="cuda")
        idx[0, :, ::2] = 4
        for disp, refined in (te.xcorrvol_subpixel(dev(fr[:, None]), dev(pat[None]), idx, 10, 5),
                              te.costvol_subpixel(dev(fr), dev(pat), idx, 10, 5, "census_sad")):
            assert bool(torch.isnan(disp[0, :, 1::2]).all()) and int(refined[0, :, 1::2].sum()) == 0
            assert not bool(torch.isnan(disp[0, :, ::2]).any())


def test_bad_arguments_raise(te):
    fr, pat = frames_for("dots", 1, 16, 40, 10, 8)
    in0, in1 = dev(fr[:, None]), dev(pat[None])
    idx = torch.zeros((1, 16, 40), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):
        te.xcorrvol_subpixel(in0, in1, idx.int(), 10, 5)                  # idx dtype
    with pytest.raises(RuntimeError):
        te.xcorrvol_subpixel(in0.double(), in1.double(), idx, 10, 5)      # frame dtype
    with pytest.raises(RuntimeError):
        te.xcorrvol_subpixel(in0, in1, idx[:, :8], 10, 5)                 # idx shape
    with pytest.raises(RuntimeError):
        te.xcorrvol_subpixel(in0, in1, idx, 10, 5, "cubic")               # mode
    with pytest.raises(RuntimeError):
        te.xcorrvol_subpixel(in0, in1, idx, 10, 4)                        # even block
    with pytest.raises(RuntimeError):
        te.costvol_subpixel(dev(fr), dev(pat), idx.float(), 10, 5, "sad")
    with pytest.raises(RuntimeError):
        te.costvol_subpixel(dev(fr), dev(pat), idx, 10, 5, "sad", 0.5, "cubic")
    with pytest.raises(RuntimeError):
        te.costvol_subpixel(dev(fr), dev(pat), idx, 10, 5, "nope")
    with pytest.raises(RuntimeError):
        te.xcorrvol_argmax(in0, in1, 10, 5, subpixel="cubic")
    with pytest.raises(RuntimeError):
        te.costvol_argmin(dev(fr), dev(pat), 10, 5, "sad", subpixel="linear")


# ---------------------------------------------------------------------------------------------------------------------
# 5. accuracy on the Kinect pattern shifted by 20 + f pixels
# ---------------------------------------------------------------------------------------------------------------------
FRACTIONS = (0.1, 0.25, 0.5, 0.75, 0.9)


def _shifted_scene(te):
    pat = golden("xcorrvol_cfg1")["kin_pattern_u8"].astype(np.float64) / 255.0
    H, W = pat.shape
    rs = np.random.RandomState(2024)
    cols = np.arange(W, dtype=np.float64)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    frames = []
    for f in FRACTIONS:
        x = cols - (20.0 + f)                                 # frame pixel w matches pattern column w - (20 + f)
        x0 = np.floor(x)
        a = x - x0
        i0 = np.clip(x0.astype(np.int64), 0, W - 1)
        i1 = np.clip(x0.astype(np.int64) + 1, 0, W - 1)
        shifted = (1.0 - a)[None] * pat[:, i0] + a[None] * pat[:, i1]
        ambient = 0.5 + 0.5 * np.sin(xx / 97.0 + f) * np.cos(yy / 61.0)
        ir = 0.6 * shifted + 0.4 * ambient + rs.normal(0, 2.0 / 255, size=(H, W))
        frames.append(np.clip(ir, 0, 1))
    raw = dev(np.stack(frames)[:, None].astype(np.float32))
    y = te.lcn(raw, 5, 0.05)[0]
    pat_lcn = te.lcn(dev(pat[None, None].astype(np.float32)), 5, 0.05)[0][0].contiguous()
    return y, pat_lcn


def _mae(d, f):
    inner = d[:, 16:-16, 64:-16]
    return [float((inner[i] - (20.0 + f_)).abs().mean()) for i, f_ in enumerate(f)]


def test_accuracy_on_shifted_kinect_pattern(te):
    y, pat_lcn = _shifted_scene(te)
    D, bs = 48, 9
    idx, _, disp, refined = te.xcorrvol_argmax(y, pat_lcn, D, bs, subpixel="parabola")
    mae_int = _mae(idx.float(), FRACTIONS)
    mae_ncc = _mae(disp, FRACTIONS)
    c_idx, _, c_disp, _ = te.costvol_argmin(y[:, 0], pat_lcn[0], D, bs, "sad", 0.1, subpixel="equiangular")
    mae_sad = _mae(c_disp, FRACTIONS)
    print("\nsub-pixel MAE (interior pixels), f =", FRACTIONS)
    print("  integer argmax   ", ["%.3f" % v for v in mae_int])
    print("  NCC parabola     ", ["%.3f" % v for v in mae_ncc])
    print("  SAD equiangular  ", ["%.3f" % v for v in mae_sad])
    print("  SAD integer      ", ["%.3f" % v for v in _mae(c_idx.float(), FRACTIONS)])
    assert max(mae_ncc) <= 0.10 and np.mean(mae_ncc) <= 0.07, mae_ncc
    assert np.mean(mae_int) >= 0.2, mae_int
    assert max(mae_sad) <= 0.08, mae_sad


# ---------------------------------------------------------------------------------------------------------------------
# 6. config 2
# ---------------------------------------------------------------------------------------------------------------------
def test_config2_frame0_equals_rule(te):
    N, H, W, D, bs = 16, 432, 512, 128, 9
    raw, pat_lcn = _lcn_inputs(te, N, H, W, D, 2)
    x = te.lcn(raw, 5, 0.05)[0]
    idx, best, disp, refined = te.xcorrvol_argmax(x, pat_lcn, D, bs, subpixel="parabola")
    assert disp.shape == (N, H, W) and not bool(torch.isnan(disp).any())
    vol0 = te.xcorrvol_batch(x[:1], pat_lcn, D, bs, algo="exact")
    assert_bits(disp[:1], refined[:1], fit_reference(vol0, idx[:1], True, "parabola"), "config 2 frame 0")
    assert float(refined.float().mean()) > 0.5
