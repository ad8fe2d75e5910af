"""GPU parity of the match-validity ops (torchext.match_validity / xcorrvol_validity / costvol_validity and validity= on
the matchers; ctd_match_validity_f32, ctd_xcorrvol_validity_f32, ctd_costvol_validity_f32) against tests/validity_ref.py
on the reference-order volume (xcorrvol / costvol with algo="exact"): flags and idx_r bit for bit at every pixel with
either algo, gap bit for bit with algo="exact" and on re-scored pixels, within 1e-5 (|s1| + |s2|) + 2e-6 otherwise."""
import numpy as np
import pytest
import torch

from tests import matcher_traps as mt
from tests import validity_ref as vr
from tests import workloads

pytestmark = pytest.mark.gpu

TYPES = ["mse", "sad", "census_mse", "census_sad"]


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def noisy_idx(rs, best_idx, D, share=0.05):
    """the volume's own argbest with a share of entries replaced by anything in [-2, D + 1]"""
    idx = np.array(best_idx, np.int64)
    swap = rs.rand(*idx.shape) < share
    return np.where(swap, rs.randint(-2, D + 2, size=idx.shape), idx)


def check_outputs(got, vol, idx, maximise, lr_tol, min_gap, exact_gap, rescored_pix=None, what=""):
    """got = (flags, idx_r, gap) device tensors; vol = the exact volume (numpy)"""
    flags, idx_r, gap = (host(t) for t in got[:3])
    rf, rr, rg = vr.validity_ref(vol, idx, maximise, lr_tol, min_gap)
    bad_r, bad_f = int((idx_r != rr).sum()), int((flags != rf).sum())
    print("%s: idx_r differs at %d, flags at %d of %d" % (what, bad_r, bad_f, rf.size))
    assert idx_r.dtype == np.int64 and flags.dtype == np.uint8 and gap.dtype == np.float32
    assert bad_r == 0, "%s: %d of %d pattern-side indices differ" % (what, bad_r, rr.size)
    assert bad_f == 0, "%s: %d of %d flag bytes differ" % (what, bad_f, rf.size)
    if exact_gap:
        assert np.array_equal(gap, rg, equal_nan=True), "%s: gap is not the exact volume's" % what
        return
    _, s1, s2 = vr.gap_of(vol, idx, maximise)
    fin = np.isfinite(rg)
    assert np.array_equal(np.isnan(gap), np.isnan(rg)) and np.array_equal(np.isposinf(gap), np.isposinf(rg))
    err = np.abs(gap[fin].astype(np.float64) - rg[fin])
    bound = 1e-5 * (np.abs(s1[fin].astype(np.float64)) + np.abs(s2[fin])) + 2e-6
    print("%s: fast gap error max %.3e, max error / bound %.3f" % (what, err.max() if err.size else 0,
                                                                   (err / bound).max() if err.size else 0))
    assert (err <= bound).all(), "%s: %d fast gaps outside the bound" % (what, int((err > bound).sum()))
    if rescored_pix is not None:
        p = host(rescored_pix)
        assert np.array_equal(gap.reshape(-1)[p], rg.reshape(-1)[p], equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------------
# 1. match_validity on volumes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 17, 13, 61, 5), (1, 96, 20, 301, 9), (2, 128, 9, 258, 7), (1, 40, 6, 23, 3),
                                   (3, 1, 5, 70, 5), (1, 2, 4, 33, 3), (1, 3, 4, 257, 9), (1, 130, 11, 512, 9)])
def test_match_validity_on_exact_volumes(te, shape):
    """W not a multiple of 4 / 64 / 256, D not a multiple of 8 / 64, D = 1, 2, 3, W < D; both families"""
    N, D, H, W, bs = shape
    rs = np.random.RandomState(N * 1000 + D + W)
    in0 = dev(rs.rand(N, 1, H, W).astype(np.float32))
    in1 = dev(rs.rand(1, H, W).astype(np.float32))
    vol = te.xcorrvol_batch(in0, in1, D, bs, algo="exact")
    idx = noisy_idx(rs, host(vol).argmax(1), D)
    for lr_tol, min_gap in ((1, 0.0), (0, 0.05)):
        got = te.match_validity(vol, dev(idx), True, lr_tol, min_gap)
        check_outputs(got, host(vol), idx, True, lr_tol, min_gap, True, what="ncc %s" % (shape,))
    cost = te.costvol(in0[:, 0], in1[0], D, bs, "sad", 0.5, algo="exact")
    idx = noisy_idx(rs, host(cost).argmin(1), D)
    got = te.match_validity(cost, dev(idx), False, 1, 0.01)
    check_outputs(got, host(cost), idx, False, 1, 0.01, True, what="sad %s" % (shape,))
    # a single volume [D,H,W] squeezes
    f1, r1, g1 = te.match_validity(cost[0], dev(idx[0]), False, 1, 0.01)
    assert f1.shape == (H, W) and torch.equal(f1, got[0][0]) and torch.equal(r1, got[1][0])


def test_match_validity_planted_ties(te):
    """a volume of four distinct values: exact ties on the pixel side and along every diagonal"""
    rs = np.random.RandomState(7)
    vol = (rs.randint(0, 4, size=(2, 37, 9, 130)) * 0.25).astype(np.float32)
    idx = noisy_idx(rs, vol.argmax(1), 37, 0.2)
    for maximise in (True, False):
        got = te.match_validity(dev(vol), dev(idx), maximise, 1, 0.0)
        check_outputs(got, vol, idx, maximise, 1, 0.0, True, what="ties max=%s" % maximise)


# ---------------------------------------------------------------------------------------------------------------------
# 2. + 3.  xcorrvol_validity / costvol_validity, exact and fast, on trap frames; both branches of the fast path
# ---------------------------------------------------------------------------------------------------------------------
def periodic_pair(rs, H, W, p, frame_periodic):
    """period-p tie traps.  Pattern periodic, frame its noisy shifted view: V[d] and V[d + p] of a pixel are the same
    bits (pixel-side ties, gap == 0).  Frame periodic, pattern random: the frame windows at x + d and x + d + p are the
    same bits, so the diagonal of pattern column x ties (listed pattern columns)."""
    tile = rs.rand(H, p).astype(np.float32)
    per = np.tile(tile, (1, W // p + 1))[:, :W]
    if frame_periodic:
        return per.copy(), rs.rand(H, W).astype(np.float32)
    frame = np.roll(per, 5, axis=1) + 0.01 * rs.randn(H, W).astype(np.float32)
    return frame.astype(np.float32), per


def check_lists(exp, pix, col, what):
    """rescored lists against the lists expected from the reference volume"""
    P = exp["pix_must"].size
    pm = np.zeros(P, bool)
    pm[host(pix)] = True
    cm = np.zeros(P, bool)
    cm[host(col)] = True
    print("%s: re-scored %d pixels, %d columns of %d; must %d / %d, never %d / %d" % (
        what, pm.sum(), cm.sum(), P, exp["pix_must"].sum(), exp["col_must"].sum(), exp["pix_never"].sum(),
        exp["col_never"].sum()))
    assert pm[exp["pix_must"].reshape(-1)].all(), "%s: an exact gap tie was not re-scored" % what
    assert cm[exp["col_must"].reshape(-1)].all(), "%s: an exact diagonal tie was not re-scored" % what
    assert not pm[exp["pix_never"].reshape(-1)].any(), "%s: a pixel decided by 4 x the bound was re-scored" % what
    assert not cm[exp["col_never"].reshape(-1)].any(), "%s: a column decided by 4 x the bound was re-scored" % what
    return pm, cm


NCC_CASES = [("flat", 0), ("dots", 0), ("staircase", 0), ("dots", 1), ("staircase", 2), ("pix_ties", 0), ("col_ties", 0),
             ("synth_ir", 0)]


def ncc_case(name, shape_no):
    bs, H, W, D = mt.NCC_SHAPES[shape_no]
    rs = np.random.RandomState(len(name) * 31 + shape_no)
    if name in ("pix_ties", "col_ties"):
        pairs = [periodic_pair(rs, H, W, 16, name == "col_ties") for _ in range(2)]
        return np.stack([f for f, _ in pairs])[:, None], np.stack([p for _, p in pairs])[:, None], bs, D
    if name == "synth_ir":
        pat = workloads.syn_dot_pattern(H, W)
        return np.stack([workloads.synth_ir(pat, rs, min(D, 128), (8, 64))[0] for _ in range(2)])[:, None], pat[None], bs, D
    frames, pat = mt.NCC_GENERATORS[name](mt.trap_seed(bs, H, 1), 2, 1, H, W, bs)
    return frames.astype(np.float32), pat.astype(np.float32), bs, D


@pytest.mark.parametrize("case", NCC_CASES, ids=lambda c: "%s-%d" % c)
def test_xcorrvol_validity_exact_and_fast(te, case):
    name, shape_no = case
    frames, pat, bs, D = ncc_case(name, shape_no)
    in0, in1 = dev(frames), dev(pat)
    vol = host(te.xcorrvol_batch(in0, in1, D, bs, algo="exact"))
    rs = np.random.RandomState(3)
    idx = noisy_idx(rs, vol.argmax(1), D)
    for min_gap in (0.0, 0.05):
        got = te.xcorrvol_validity(in0, in1, dev(idx), D, bs, 1, min_gap, algo="exact", return_rescored=True)
        assert got[3].numel() == 0 and got[4].numel() == 0
        check_outputs(got, vol, idx, True, 1, min_gap, True, what="%s exact" % name)
        got = te.xcorrvol_validity(in0, in1, dev(idx), D, bs, 1, min_gap, algo="fast", return_rescored=True)
        check_outputs(got, vol, idx, True, 1, min_gap, False, got[3], what="%s fast min_gap %g" % (name, min_gap))
        exp = vr.expected_lists(vol, idx, True, min_gap)
        pm, cm = check_lists(exp, got[3], got[4], "%s min_gap %g" % (name, min_gap))
        if name == "pix_ties" and min_gap == 0.0:
            assert exp["pix_must"].any() and exp["pix_never"].any() and 0 < pm.sum() < pm.size
        if name == "col_ties":
            assert exp["col_must"].any() and cm.sum() > 0
        if name == "synth_ir":
            assert exp["pix_never"].any() and exp["col_never"].any() and pm.sum() < pm.size and cm.sum() < cm.size


@pytest.mark.parametrize("ty", TYPES)
@pytest.mark.parametrize("name", ["ulp", "pix_ties", "col_ties"])
def test_costvol_validity_exact_and_fast(te, ty, name):
    H, W, D, N = 21, 203, 61, 2
    rs = np.random.RandomState(len(name) + TYPES.index(ty))
    for bs in (9, 5):
        if name == "ulp":
            ims, pat = mt.COST_GENERATORS["ulp"](bs * 100 + H, N, H, W)
        else:
            pairs = [periodic_pair(rs, H, W, 16, name == "col_ties") for _ in range(N)]
            ims, pat = np.stack([f for f, _ in pairs]), np.stack([p for _, p in pairs])
        im, pt = dev(ims.astype(np.float32)), dev(pat.astype(np.float32))
        vol = host(te.costvol(im, pt, D, bs, ty, 0.5, algo="exact"))
        idx = noisy_idx(rs, vol.argmin(1), D)
        min_gap = 0.0 if bs == 9 else 0.002
        what = "%s %s bs %d" % (name, ty, bs)
        got = te.costvol_validity(im, pt, dev(idx), D, bs, ty, 0.5, 1, min_gap, algo="exact", return_rescored=True)
        assert got[3].numel() == 0 and got[4].numel() == 0
        check_outputs(got, vol, idx, False, 1, min_gap, True, what=what + " exact")
        got = te.costvol_validity(im, pt, dev(idx), D, bs, ty, 0.5, 1, min_gap, algo="fast", return_rescored=True)
        check_outputs(got, vol, idx, False, 1, min_gap, False, got[3], what=what + " fast")
        exp = vr.expected_lists(vol, idx, False, min_gap)
        pm, cm = check_lists(exp, got[3], got[4], what)
        if name == "pix_ties" and min_gap == 0.0:
            assert exp["pix_must"].any() and exp["pix_never"].any() and 0 < pm.sum() < pm.size
        if name == "col_ties":
            assert exp["col_must"].any() and cm.sum() > 0


def test_exact_algo_covers_what_the_fast_path_does_not(te):
    """C = 2 and block 11: algo='fast' takes the exact volume, nothing is re-scored"""
    rs = np.random.RandomState(9)
    for C, bs in ((2, 9), (1, 11)):
        in0, in1 = dev(rs.rand(2, C, 14, 70).astype(np.float32)), dev(rs.rand(C, 14, 70).astype(np.float32))
        vol = host(te.xcorrvol_batch(in0, in1, 24, bs, algo="exact"))
        idx = vol.argmax(1)
        got = te.xcorrvol_validity(in0, in1, dev(idx), 24, bs, 1, 0.02, algo="fast", return_rescored=True)
        assert got[3].numel() == 0 and got[4].numel() == 0
        check_outputs(got, vol, idx, True, 1, 0.02, True, what="C %d bs %d" % (C, bs))


# ---------------------------------------------------------------------------------------------------------------------
# 4. + 6.  the synth_ir set: the expected output is not vacuous, and the filter does what it is for
# ---------------------------------------------------------------------------------------------------------------------
SYNTH_MIN_GAP = 0.05


def synth_set(te):
    H, W, D, bs, N = 96, 320, 128, 9, 2
    rs = np.random.RandomState(2024)
    pat = workloads.syn_dot_pattern(H, W)
    pairs = [workloads.synth_ir(pat, rs, D) for _ in range(N)]
    frames = np.stack([p[0] for p in pairs])[:, None]
    truth = np.stack([p[1] for p in pairs])
    in0, _ = te.lcn(dev(frames), 5, 0.05)
    in1, _ = te.lcn(dev(pat[None, None]), 5, 0.05)
    return in0, in1[0], truth, D, bs


def test_synth_ir_flags_are_not_vacuous_and_filter_errors(te):
    """Expected output from the reference volume alone (2 x 96 x 320 pixels, D 128, block 9, LCN radius 5, idx = the
    exact argmax, lr_tol 1, min_gap 0.05).  Counts (set / clear of 61440 pixels):
    IN_PATTERN 54403 / 7037, LR_OK 39012 / 22428, UNIQUE 53020 / 8420, valid 38595; |idx - truth| > 1 at 14.59 % of
    all pixels and 0.80 % of the valid ones; the fast path re-scores 3 pixels and 10 pattern columns."""
    in0, in1, truth, D, bs = synth_set(te)
    vol = host(te.xcorrvol_batch(in0, in1, D, bs, algo="exact"))
    idx = vol.argmax(1)
    rf, rr, rg = vr.validity_ref(vol, idx, True, 1, SYNTH_MIN_GAP)
    for bit, name in ((vr.IN_PATTERN, "IN_PATTERN"), (vr.LR_OK, "LR_OK"), (vr.UNIQUE, "UNIQUE")):
        n_set = int(((rf & bit) != 0).sum())
        print("%s: %d set, %d clear of %d" % (name, n_set, rf.size - n_set, rf.size))
        assert 0 < n_set < rf.size, "%s is %s everywhere in the expected output" % (name, "set" if n_set else "clear")
    # the kernels reproduce it, from the matcher's own indices, with both algos
    midx, _ = te.xcorrvol_argmax(in0, in1, D, bs)
    assert np.array_equal(host(midx), idx)
    for algo in ("exact", "fast"):
        got = te.xcorrvol_validity(in0, in1, midx, D, bs, 1, SYNTH_MIN_GAP, algo=algo, return_rescored=True)
        check_outputs(got, vol, idx, True, 1, SYNTH_MIN_GAP, algo == "exact", got[3], what="synth_ir " + algo)
    n_pix, n_col = got[3].numel(), got[4].numel()
    print("fast: re-scored %d pixels and %d columns of %d" % (n_pix, n_col, rf.size))
    assert n_pix < rf.size and n_col < rf.size
    # purpose: gross errors are rarer among the valid pixels
    valid = host(got[0]) == 7
    wrong = np.abs(idx - truth) > 1
    share_all, share_valid = wrong.mean(), wrong[valid].mean()
    print("valid %d of %d; |idx - truth| > 1: %.4f of all, %.4f of valid" % (valid.sum(), valid.size, share_all, share_valid))
    assert valid.any()
    assert share_valid < share_all


# ---------------------------------------------------------------------------------------------------------------------
# 5. validity= on the matchers
# ---------------------------------------------------------------------------------------------------------------------
def test_validity_keyword_equals_the_stand_alone_call(te):
    in0, in1, _, D, bs = synth_set(te)
    plain = te.xcorrvol_argmax(in0, in1, D, bs)
    assert len(te.xcorrvol_argmax(in0, in1, D, bs, validity=None)) == 2
    both = te.xcorrvol_argmax(in0, in1, D, bs, subpixel="parabola", validity=dict(lr_tol=2, min_gap=0.03))
    assert len(both) == 7 and torch.equal(both[0], plain[0]) and torch.equal(both[1], plain[1])
    alone = te.xcorrvol_validity(in0, in1, plain[0], D, bs, 2, 0.03)
    sub = te.xcorrvol_subpixel(in0, in1, plain[0], D, bs, "parabola")
    assert all(torch.equal(a, b) for a, b in zip(both[2:4], sub))
    assert all(torch.equal(a, b) for a, b in zip(both[4:], alone))          # (the matcher's idx is in range: no NaN)
    im, pt = in0[:, 0].contiguous(), in1[0].contiguous()
    plain = te.costvol_argmin(im, pt, D, bs, "sad", 0.5)
    assert len(te.costvol_argmin(im, pt, D, bs, "sad", 0.5, validity=None)) == 2
    both = te.costvol_argmin(im, pt, D, bs, "sad", 0.5, validity=dict(min_gap=0.001))
    alone = te.costvol_validity(im, pt, plain[0], D, bs, "sad", 0.5, 1, 0.001)
    assert len(both) == 5 and torch.equal(both[0], plain[0]) and torch.equal(both[1], plain[1])
    assert all(torch.equal(a, b) for a, b in zip(both[2:4], alone[:2]))
    assert torch.equal(both[4], alone[2])
    with pytest.raises(RuntimeError):
        te.xcorrvol_argmax(in0, in1, D, bs, validity=dict(gap=1))


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected(te):
    vol = torch.rand(2, 8, 5, 12, device="cuda")
    idx = torch.zeros(2, 5, 12, dtype=torch.int64, device="cuda")
    in0, in1 = torch.rand(2, 1, 5, 12, device="cuda"), torch.rand(1, 5, 12, device="cuda")
    calls = [
        lambda **k: te.match_validity(vol, k.pop("idx", idx), True, **k),
        lambda **k: te.xcorrvol_validity(in0, in1, k.pop("idx", idx), 8, 3, **k),
        lambda **k: te.costvol_validity(in0[:, 0], in1[0], k.pop("idx", idx), 8, 3, "sad", 0.5, **k),
    ]
    for call in calls:
        call()                                                            # the good call runs
        for bad in (dict(lr_tol=-1), dict(min_gap=float("nan")), dict(min_gap=-0.5), dict(idx=idx[:, :4]),
                    dict(idx=idx[0]), dict(idx=idx.to(torch.int32)), dict(idx=idx.cpu())):
            with pytest.raises(RuntimeError):
                call(**bad)
    with pytest.raises(RuntimeError):
        te.match_validity(vol.cpu(), idx, True)
    with pytest.raises(RuntimeError):
        te.xcorrvol_validity(in0, in1, idx, 8, 3, algo="quick")
