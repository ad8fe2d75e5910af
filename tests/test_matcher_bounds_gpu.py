"""The fast matchers' error bounds, tested where they are stated, on adversarial frames and against float64.

NCC (ncc_fast.hip and its kernel files): the pre-pass lists every window whose outputs the fast kernel cannot deliver within tolerance, the
fix-up pass recomputes those in the reference's order, and every other output is trusted to |fast - exact| <= 1e-5
|exact| + 1e-6 (C > 1: 1e-5 sum_c |exact_c| + C 1e-6), from the error model |fast - exact| <~ 7 * 2^-24 * sum_c
sqrt(Fa Fb), which kFlagRatio = 1.39 keeps within that bound.  tests/matcher_traps.py restates
the listing rule in float64 and classifies every output: listed outputs must carry the exact kernel's bits, unlisted
ones must meet the bound (and the error model against float64 truth), guard outputs (within 1.5 % of a threshold,
decided by the pre-pass's own rounding) one or the other.  The ranked argmax paths must give the exact kernel's indices
on the same frames.

Cost volumes (costvol_fast.hip, costvol_argmin.hip): the premise of costvol_argmin's proof, |f(d) - x(d)| <= 1e-5
x(d) + 1e-6 for every d, elementwise; indices equal to the exact volume's first-index argmin; and the census-SAD
gradient's sign at census differences next to zero.

The trap generators and their windows' placement are pinned on the CPU (tests/test_f64_refs.py)."""
import numpy as np
import pytest
import torch

from tests import f64_refs as R
from tests import matcher_traps as T
from tests.test_subpixel_gpu import assert_bits, fit_reference
from tests.util import assert_close

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MODEL_C = 7.0                          # the error model's constant (ncc_fixup.hip, above ncc_fixup_kernel)

NCC_SHAPES = T.NCC_SHAPES
NCC_CASES = [(name, 1) + s for name in T.NCC_GENERATORS for s in NCC_SHAPES]
NCC_CASES += [(name, C) + s for name in T.MULTICHANNEL_GENERATORS for C in (2, 3) for s in NCC_SHAPES[:2]]


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _within(a, b, scale, C):
    """the contract of the fast NCC volume: |a - b| <= 1e-5 |b| + 1e-6 for one channel; for C channels the sum of that
    bound over the per-channel NCCs b_c (include/ctd_hip.h), 1e-5 * sum_c |b_c| + C * 1e-6, `scale` = sum_c |b_c|"""
    return np.abs(a - b) <= 1e-5 * scale + 1e-6 * C


def _frames(name, C, bs, H, W):
    gen = {**T.NCC_GENERATORS, **T.MULTICHANNEL_GENERATORS}[name]
    return gen(T.trap_seed(bs, H, C), 2, C, H, W, bs)


@pytest.mark.parametrize("name,C,bs,H,W,D", NCC_CASES)
def test_ncc_fast_volume_bounds(te, name, C, bs, H, W, D):
    """(a) listed outputs carry the exact kernel's bits; (b) unlisted ones are within the contract of `_within`; (c)
    guard outputs do one or the other; (d) against float64 truth t, unlisted outputs meet the error model
    (ncc_fixup.hip, above ncc_fixup_kernel):
        |fast - t| <= |exact - t| + 7 * 2^-24 * sum_c sqrt(Fa Fb) + sum_c |t_c| * 1e-8 / (sa sb)
    the last term being the reference denominator's 1e-8, a relative change of each channel's NCC t_c that the fast
    path's reciprocal deviations leave out (kDevFloor bounds it)"""
    frames, pat = _frames(name, C, bs, H, W)
    A, B = dev(frames), dev(pat)
    fast = te.xcorrvol_batch(A, B, D, bs, algo="fast").cpu().numpy()
    exact = te.xcorrvol_batch(A, B, D, bs, algo="exact").cpu().numpy()
    truth = R.xcorrvol(A, B, D, bs).cpu().numpy()
    # per-channel volumes: the contract's scale for C > 1 (exact) and the 1e-8 term's weights (float64)
    if C == 1:
        scale, t_c = np.abs(exact.astype(np.float64)), np.abs(truth)[:, None]
    else:
        scale = sum(np.abs(te.xcorrvol_batch(A[:, c:c + 1].contiguous(), B[c:c + 1].contiguous(), D, bs,
                                             algo="exact").cpu().numpy().astype(np.float64)) for c in range(C))
        t_c = np.stack([np.abs(R.xcorrvol(A[:, c:c + 1], B[c:c + 1], D, bs).cpu().numpy()) for c in range(C)], 1)
    cls, sqrtF, floor = T.classify(frames, pat, D, bs)
    listed, unlisted, guard = cls == T.LISTED, cls == T.UNLISTED, cls == T.GUARDED
    f, x = fast.astype(np.float64), exact.astype(np.float64)
    ok = _within(f, x, scale, C)
    same = fast == exact
    what = "%s C %d bs %d %dx%d D %d" % (name, C, bs, H, W, D)
    err_x, err_t = np.abs(f - x), np.abs(f - truth)
    print("\n%s: listed %d unlisted %d guard %d; unlisted max |fast-exact| %.3g, max |fast-t| %.3g, max bound %.3g" % (
        what, listed.sum(), unlisted.sum(), guard.sum(), err_x[unlisted].max(initial=0), err_t[unlisted].max(initial=0),
        (1e-5 * scale + 1e-6 * C)[unlisted].max(initial=0)))
    bad = listed & ~same
    assert not bad.any(), "%s: %d of %d listed outputs differ from the exact kernel, max %.3g" % (
        what, bad.sum(), listed.sum(), err_x[bad].max())
    bad = unlisted & ~ok
    assert not bad.any(), "%s: %d of %d unlisted outputs outside the contract, max |a-b| %.3g" % (
        what, bad.sum(), unlisted.sum(), err_x[bad].max())
    bad = guard & ~(same | ok)
    assert not bad.any(), "%s: %d guard outputs neither exact nor within the contract" % (what, bad.sum())
    model = np.abs(x - truth) + MODEL_C * U * sqrtF + (t_c * floor).sum(1)
    bad = unlisted & (err_t > model)
    assert not bad.any(), "%s: %d unlisted outputs break the error model, worst excess %.3g (sqrtF %.3g)" % (
        what, bad.sum(), (err_t - model)[bad].max(), sqrtF[bad].max())
    # on unlisted outputs the reference-order kernel itself is float64 truth to f32 rounding, per channel (listed
    # windows are the ones where the reference's own rounding decides its value)
    bad = unlisted & ~_within(x, truth, scale, C)
    assert not bad.any(), "%s: %d unlisted exact outputs off float64 truth" % (what, bad.sum())


def _idx_cases():
    return [(name, bs, H, W, D) for name, C, bs, H, W, D in NCC_CASES if C == 1]


@pytest.mark.parametrize("name,bs,H,W,D", _idx_cases())
def test_ncc_indices_and_best(te, name, bs, H, W, D):
    """xcorrvol_argmax with and without a volume, with a prepared pattern, and lcn_xcorrvol_argmax (exact and fast
    LCN) give the exact kernel's indices; best stays within tolerance; the parabola fit is the rule applied to the
    exact volume; and wherever the float64 top-two gap exceeds twice the exact volume's error, the index is the float64
    argmax"""
    frames, pat = _frames(name, 1, bs, H, W)
    A, B = dev(frames), dev(pat[0:1])
    what = "%s bs %d %dx%d D %d" % (name, bs, H, W, D)
    idx_e, best_e, vol_e = te.xcorrvol_argmax(A, B, D, bs, return_volume=True, algo="exact")
    tol = vol_e.abs().amax(-3) * 1e-5 + 2e-6
    outs = {"volume": te.xcorrvol_argmax(A, B, D, bs, return_volume=True, algo="fast")[:2],
            "volume-free": te.xcorrvol_argmax(A, B, D, bs, algo="fast")}
    pp = te.prepare_pattern(B, 2, D, bs)
    outs["prepared"] = te.xcorrvol_argmax(A, B, D, bs, algo="fast", prepared=pp)
    for key, (idx, best) in outs.items():
        bad = int((idx != idx_e).sum())
        assert bad == 0, "%s %s: %d of %d indices differ from the exact kernel's" % (what, key, bad, idx.numel())
        assert bool(((best - best_e).abs() <= tol).all()), "%s %s: best" % (what, key)
    # sub-pixel: the rule on the exact volume around the (shared) index
    out = te.xcorrvol_argmax(A, B, D, bs, algo="fast", subpixel="parabola")
    assert torch.equal(out[0], idx_e), what
    assert_bits(out[2], out[3], fit_reference(vol_e, idx_e, True, "parabola"), what + " parabola")
    # float64 truth decides the index where its top-two gap is clear of the exact volume's error
    t = R.xcorrvol(A, B, D, bs)
    top2 = t.topk(2, dim=1).values
    err = (vol_e.double() - t).abs().amax(1)
    clear = (top2[:, 0] - top2[:, 1]) > 2 * err
    assert bool((idx_e == t.argmax(1))[clear].all()), what
    # the fused LCN + matcher call: indices of the exact kernel on the LCN output it returns.  The reference's f32 LCN
    # turns windows whose variance cancels in f32 (E[x^2] - avg^2 below 2^-20 E[x^2]: the plateaus of the flat and
    # clipped-255 frames, far from 0) into NaN, and the matcher has no contract for NaN input; such frames enter this
    # leg centred and scaled to a unit range (an LCN no-op in exact arithmetic), and the leg must then be well posed
    raw = A
    lcn64 = R.lcn(raw.cpu(), 5, 0.05)
    if not bool((lcn64.inter["var"] > 2.0 ** -20 * lcn64.inter["ex2"]).all()):
        raw = ((A - A.mean()) / (A.max() - A.min())).contiguous()
        lcn64 = R.lcn(raw.cpu(), 5, 0.05)
        assert bool((lcn64.inter["var"] > 2.0 ** -20 * lcn64.inter["ex2"]).all()), what
    for lcn_algo in ("exact", "fast"):
        y, _, idx, best = te.lcn_xcorrvol_argmax(raw, B, D, bs, 5, 0.05, lcn_algo=lcn_algo)
        assert bool(torch.isfinite(y).all()), what
        idx_l, best_l = te.xcorrvol_argmax(y, B, D, bs, algo="exact")
        bad = int((idx != idx_l).sum())
        assert bad == 0, "%s lcn %s: %d indices differ" % (what, lcn_algo, bad)
        vol_l = te.xcorrvol_batch(y, B, D, bs, algo="exact")
        assert bool(((best - best_l).abs() <= vol_l.abs().amax(-3) * 1e-5 + 2e-6).all()), what


# ---------------------------------------------------------------------------------------------------------------------
# cost volumes
# ---------------------------------------------------------------------------------------------------------------------
COST_CASES = [(g, ty, eps, bs) for g in T.COST_GENERATORS for ty in ("mse", "sad") for eps in (0.5,) for bs in (3, 5, 7, 9)]
COST_CASES += [(g, ty, eps, bs) for g in T.COST_GENERATORS for ty in ("census_mse", "census_sad")
               for eps in (0.5, 1e-3, 1e-6) for bs in (3, 5, 7, 9)]


@pytest.mark.parametrize("gen,ty,eps,bs", COST_CASES)
def test_costvol_fast_premise_and_argmin(te, gen, ty, eps, bs):
    """costvol_argmin's premise |f(d) - x(d)| <= 1e-5 x(d) + 1e-6 elementwise (fast vs reference-order volume), both
    volumes against float64, and costvol_argmin's indices equal to the exact volume's first-index argmin"""
    H, W, D = 21, 203, 48
    im, pat = T.COST_GENERATORS[gen](bs * 7 + len(ty), 2, H, W)
    I, P = dev(im), dev(pat)
    fast = te.costvol(I, P, D, bs, ty, eps, algo="fast")
    exact = te.costvol(I, P, D, bs, ty, eps, algo="exact")
    truth = R.costvol(I, P, D, bs, ty, float(np.float32(eps))).cpu().numpy()
    f, x = fast.cpu().numpy().astype(np.float64), exact.cpu().numpy().astype(np.float64)
    what = "%s %s eps %g bs %d" % (gen, ty, eps, bs)
    print("\n%s: max |f-x| %.3g, max |f-t| %.3g, max |x-t| %.3g" % (what, np.abs(f - x).max(), np.abs(f - truth).max(),
                                                                  np.abs(x - truth).max()))
    bad = ~(np.abs(f - x) <= 1e-5 * x + 1e-6)
    assert not bad.any(), "%s: %d of %d fast costs break the premise, max |f-x| %.3g" % (what, bad.sum(), bad.size,
                                                                                         np.abs(f - x)[bad].max())
    assert_close(x, truth, what=what + " exact vs f64")
    assert_close(f, truth, rtol=2e-5, atol=2e-6, what=what + " fast vs f64")
    idx, best = te.costvol_argmin(I, P, D, bs, ty, eps)
    ref = exact.argmin(-3)
    bad = int((idx != ref).sum())
    assert bad == 0, "%s: %d of %d indices differ from the exact volume's argmin" % (what, bad, idx.numel())


# ---------------------------------------------------------------------------------------------------------------------
# photometric loss, algo="fast", on the sign traps
# ---------------------------------------------------------------------------------------------------------------------
SIGN_AMBIGUOUS = 2.0 ** -23            # one ulp of 1 + t in the reference's h = 0.5 (1 + t): a census difference this
                                       # close to zero may take either sign in the reference's own arithmetic


def _ambiguous(es, ta, bs, eps):
    """bool [B,1,H,W]: pixels whose gradient takes a census pair (as its centre or as its tap) whose float64
    difference is nonzero and within SIGN_AMBIGUOUS of zero"""
    _, diff = R.block_loss(es.double(), ta.double(), bs, "census_sad", float(np.float32(eps)))
    amb = (diff != 0) & (diff.abs() <= SIGN_AMBIGUOUS)                 # [B, bs*bs, H, W], pair (centre p, tap k)
    out = amb.any(1, keepdim=True)
    h = bs // 2
    H, W = es.shape[-2:]
    for k in range(bs * bs):
        dy, dx = k // bs - h, k % bs - h                              # the tap's pixel: p + (dy, dx), clamped
        ys = (torch.arange(H, device=es.device) + dy).clamp(0, H - 1)
        xs = (torch.arange(W, device=es.device) + dx).clamp(0, W - 1)
        a = amb[:, k]
        for b in range(a.shape[0]):
            rows, cols = torch.nonzero(a[b], as_tuple=True)
            out[b, 0, ys[rows], xs[cols]] = True
    return out


PHOTO_CASES = [(ty, 0.5, bs, scale) for ty in R.PHOTO_TYPES for bs in (3, 5, 7, 9) for scale in (1.0, 1e-2)]


@pytest.mark.parametrize("ty,eps,bs,scale", PHOTO_CASES)
def test_photometric_fast_on_sign_traps(te, ty, eps, bs, scale):
    """forward and backward of algo='fast' against the reference-order kernels at the stated bound, on pairs whose
    differences are 0, +-1 ulp and +-1e-6 (1 +- 0.1); for census_sad, every gradient whose census signs float64
    decides by more than SIGN_AMBIGUOUS must agree with the reference's, and -- the re-evaluation near zero settling
    the rest in the reference's own arithmetic -- so must every other one"""
    es, ta = T.sign_trap_pair(bs * 11 + int(-np.log10(eps)), 2, 37, 150, bs, scale)
    go = np.random.RandomState(bs).rand(2, 1, 37, 150).astype(np.float32)
    E, TA, GO = dev(es), dev(ta), dev(go)
    a, b = E.clone().requires_grad_(True), E.clone().requires_grad_(True)
    fa = te.photometric_loss(a, TA, bs, ty, eps, algo="fast")
    fb = te.photometric_loss(b, TA, bs, ty, eps, algo="exact")
    what = "%s eps %g bs %d scale %g" % (ty, eps, bs, scale)
    assert_close(fa.detach().cpu().numpy(), fb.detach().cpu().numpy(), what=what + " fwd")
    fa.backward(GO)
    fb.backward(GO)
    ga, gb = a.grad, b.grad
    off = (ga - gb).abs() > 1e-5 * gb.abs() + 1e-6
    if ty == "census_sad":
        # where float64 decides every census sign the gradient takes by more than SIGN_AMBIGUOUS, the fast signs must
        # be the reference's; the re-evaluation near zero goes further and settles even the ambiguous ones in the
        # reference's own arithmetic, so the gradient agrees everywhere
        amb = _ambiguous(E, TA, bs, eps)
        assert float(amb.double().mean()) < 0.75, what
        print("\n%s: %d ambiguous pixels, %d / %d gradient entries out of tolerance there / elsewhere" % (
            what, int(amb.sum()), int((off & amb).sum()), int((off & ~amb).sum())))
        assert int((off & ~amb).sum()) == 0, "%s: %d decided gradient entries out of tolerance" % (what, int((off & ~amb).sum()))
    assert int(off.sum()) == 0, "%s: %d of %d gradient entries out of tolerance, max %.3g" % (
        what, int(off.sum()), off.numel(), float(((ga - gb).abs() * off).max()))
