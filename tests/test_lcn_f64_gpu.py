"""Every LCN path against the float64 restatement of LCN.tforward (tests/f64_refs.py: lcn, model/networks.py:507-533):
lcn(algo='exact') (the compiled radius 5 and the run-time-radius kernel), lcn(algo='fast') at each radius 1 .. 7, and the
LCN outputs of lcn_xcorrvol_argmax with lcn_algo 'exact' and 'fast' (the streaming kernel) -- on uniform frames, DC
offsets, dots on zero and on a low-noise level, flat quantised levels, 8-bit values, negative values, frames that are
dark on some rows and bright on the next, and high dynamic range; at radius min(H, W) - 1, at the edges of the tiles and
of the streaming kernel's strips and bands, and with several frames of different levels.

Rule, one for every case.  u = 2^-24; from the f64 intermediates of each pixel (avg, ex2 = E[x^2], var = ex2 - avg^2 +
1e-6, sd = sqrt(var) + eps):
    kappa_std = ex2 / (2 sqrt(var))               a rounding error u * ex2 in var, through the square root
    kappa_y   = (|y| kappa_std + |x| + |avg|) / sd    that error through the divide, plus the roundings of x and avg
and elementwise, for y and std,
    |k - f64| <= r |f64| + a + C u kappa,    r = 1e-6, a = 1e-6 (4e-6 for the streaming f32 sums, below).
C is one constant per kernel family:
  * f64 box sums and the reference's f32 tail (C_EXACT = 12): the sums are within half an f32 ulp of exact once rounded;
    boxs / n, boxs2 / n, avg * avg, the subtraction and + 1e-6 put at most 2u|avg| into avg and 9u ex2 into var; the
    square root, + eps, x - avg and the divide add at most 3u of the outputs themselves (inside r); the module squares x
    in f32 where the reference squares it in f64 (one more u ex2).
  * f32 box sums of centred samples (C_FAST = 64): at most 40 roundings (a fresh 11-term sum in each direction, 2 per
    step of a sliding sum) of partial sums that hold at most 12 of a window's 11 rows or columns, where the centring
    constant lies between 0 and every sample (|x - c| <= |x|).  The tiled kernel chooses it so and takes fresh sums
    (the "dark_bright" and "bright_dark" frames, whose dark runs are longer than any window, failed a tile-mean
    centring and sliding sums); v_rcp / v_sqrt add 1 ulp each (inside r).  (Radii 1 .. 6 of the tiled kernel failed
    this rule, and lcn(algo='fast') runs the exact kernel there: ctd_lcn_fast_f32 serves radius 7 only.)  The
    streaming kernel centres on the first row a band reads and slides its sums over the band, so its contract
    (include/ctd_hip.h) excludes frames with long dark runs next to bright ones: test_fused_lcn_vs_f64 runs the two
    kinds that have them with lcn_algo 'exact' only, and test_fused_fast_outside_its_contract records the miss.  The streaming kernel's f32 11-row sums slide over a whole band (up to 82
    fed rows): the rounding of a bright square (up to 1 on these frames) that has left the window stays, a random walk
    of 2 roundings a row, about sqrt(164) u in the box sum of x^2, which a window on the 1e-6 variance floor divides by
    121 x 2 sqrt(1e-6).  a = AT_STREAM_FAST = 4e-6 for that family is a per-family floor chosen from that one-sigma
    estimate (3.2e-6) and a measurement (2.7e-6 on dots on a low-noise level): an estimate, not a bound, and tested at
    bands of up to 64 rows (FUSED_SHAPES).
And per case, the kernel's largest error is at most 1.25 times the stock-torch f32 error (the same reference in float32:
ATen's conv2d summation order) plus the floor r max|f64| + a + 2 u max kappa.  The last term is two roundings of the
f32 tail (avg * avg and ex2 - avg^2, where var cancels): the kernels keep the reference's f32 tail, so on frames whose
error is all in that cancellation (a DC level at radius 1) whether a kernel or stock torch comes out lower is a coin
toss.  No masks, no per-case constants, no fractions of pixels.

What the rule cannot see: where the f32 tail itself is ill-conditioned the bound follows it.  For x = 1000 + u,
kappa_std is about 1.7e6, so C u kappa is about 1.2 against a std of about 0.34 -- any std near eps would pass, and the
"dc1000" cases check only that the paths run and stay finite there, not their accuracy.

The streaming kernel's exact variant must carry the oracle's bits wherever the f64 sums are exact in any order
(tests/lcn_traps.py: exact_windows), and the tiled exact kernel, which uses the oracle's summation order, everywhere; the
trap frames of lcn_traps.py check that no rounding outlives its window (the emulation there says how many traps the
device's band layout arms, and the test insists on a minimum)."""
import numpy as np
import pytest
import torch

from tests import f64_refs as R
from tests import lcn_traps as T
from tests import workloads

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
RT, AT = 1e-6, 1e-6
AT_STREAM_FAST = 4e-6    # a of the streaming kernel's f32 sliding sums (module docstring)
C_EXACT, C_FAST = 12.0, 64.0
TAIL = 2.0               # roundings of the f32 tail in the floor of the stock-f32 yardstick
EPS = 0.05
KINDS = ("uniform", "dc10", "dc1000", "dots", "dots_noise", "levels", "u8", "negative", "dark_bright", "bright_dark",
         "hdr")


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frames(kind, N, H, W, seed):
    """[N,1,H,W] f32 inputs; frames of one batch differ in level (frame f gets + f / 4, or x (1 + f) for kinds whose
    zero background matters)"""
    rs = np.random.RandomState(seed)
    u = rs.rand(N, 1, H, W)
    f = np.arange(N, dtype=np.float64).reshape(N, 1, 1, 1)
    if kind == "uniform":
        x = u + f / 4
    elif kind == "dc10":
        x = 10 + 3 * u + f
    elif kind == "dc1000":
        x = 1000 + u + 7 * f
    elif kind == "dots":                   # structured light: zero background, sparse bright dots
        x = (rs.rand(N, 1, H, W) < 0.06) * (0.6 + 0.4 * u) * (1 + f) / N
    elif kind == "dots_noise":             # the same on a low-noise dark level
        x = (rs.rand(N, 1, H, W) < 0.06) * 0.9 + 0.02 + 0.01 * u + f / 8
    elif kind == "levels":                 # flat quantised levels
        x = np.floor(u * 4) / 4 + 0.25 * f
        x = np.repeat(np.repeat(x[:, :, ::8, ::8], 8, 2), 8, 3)[:, :, :H, :W]
    elif kind == "u8":                     # 8-bit values / 255
        x = np.floor(u * 256) / 255 + 0 * f
    elif kind == "negative":
        x = -3 + 2 * u - f
    elif kind == "dark_bright":            # 16 dark rows, then 16 bright ones: dark runs longer than any window
        h = np.arange(H).reshape(1, 1, H, 1)
        x = np.where(h % 32 < 16, 0.02 + 0.01 * u, 0.7 + 0.3 * u) + 0.1 * f
    elif kind == "bright_dark":            # 10 bright rows, then 22 dark ones: a band that starts bright runs into dark
        h = np.arange(H).reshape(1, 1, H, 1)
        x = np.where(h % 32 < 10, 0.7 + 0.3 * u, 0.02 + 0.01 * u) + 0.1 * f
    elif kind == "hdr":
        x = T.hdr_frames(N, H, W, seed).astype(np.float64) * (1 + f)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, np.float32)


def errors(x, radius, y, s, C, at=AT):
    """(worst ratio of |k - f64| to the elementwise bound over y and std, worst ratio of the kernel's largest error to
    1.25 x the stock-f32 error + floor, description)"""
    ref = R.lcn(torch.from_numpy(x), radius, EPS)
    st = R.lcn(torch.from_numpy(x), radius, EPS, dtype=torch.float32)
    y64, s64 = ref.value
    avg, ex2, var = ref.inter["avg"], ref.inter["ex2"], ref.inter["var"]
    kap_s = ex2 / (2 * torch.sqrt(var))
    kap_y = (y64.abs() * kap_s + torch.from_numpy(x).double().abs() + avg.abs()) / s64
    worst_el, worst_st, msg = 0.0, 0.0, []
    for name, k, f, kap, sf in (("y", y, y64, kap_y, st.value[0]), ("std", s, s64, kap_s, st.value[1])):
        k = k.detach().cpu().double()
        err = (k - f).abs()
        bound = RT * f.abs() + at + C * U * kap
        ratio = float((err / bound).max())
        e_st = float((sf.double() - f).abs().max())
        yard = 1.25 * e_st + RT * float(f.abs().max()) + at + TAIL * U * float(kap.max())
        r_st = float(err.max()) / yard
        worst_el, worst_st = max(worst_el, ratio), max(worst_st, r_st)
        msg.append("%s: max err %.3e (%.2f x the elementwise bound), stock f32 max err %.3e (kernel at %.2f x its "
                   "yardstick)" % (name, float(err.max()), ratio, e_st, r_st))
    return worst_el, worst_st, "; ".join(msg)


def assert_rule(x, radius, y, s, C, what, at=AT):
    el, st, msg = errors(x, radius, y, s, C, at)
    assert el <= 1 and st <= 1, "%s: %s" % (what, msg)


def lcn_shapes(radius):
    """radius = min(H, W) - 1 (reflection meets both borders), the 64 x 16 fast and 32 x 32 exact tile edges +- 1, N > 1"""
    return [(1, radius + 1, 70), (2, 40, radius + 1), (3, 33, 65), (1, 16, 64), (2, 17, 129), (1, 15, 63),
            (1, 31, 128), (2, 32, 127), (1, 65, 33)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("radius", [5, 0, 2, 9, 11])
def test_lcn_exact_vs_f64(te, kind, radius):
    for i, (N, H, W) in enumerate(lcn_shapes(radius)):
        x = frames(kind, N, H, W, 100 * radius + i)
        y, s = te.lcn(dev(x), radius, EPS, algo="exact")
        assert_rule(x, radius, y, s, C_EXACT, "exact r%d %s %s" % (radius, kind, (N, H, W)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("radius", [1, 2, 3, 4, 5, 6, 7])
def test_lcn_fast_vs_f64(te, kind, radius):
    for i, (N, H, W) in enumerate(lcn_shapes(radius)):
        x = frames(kind, N, H, W, 100 * radius + i)
        y, s = te.lcn(dev(x), radius, EPS, algo="fast")
        assert_rule(x, radius, y, s, C_FAST, "fast r%d %s %s" % (radius, kind, (N, H, W)))


# strip edges (W = 16, 232, 236, 464, 468), band edges (H = 11, 64, 65, 129) at several frame counts; and, on a 256-CU
# device, bands of 21 rows (as at config 2) and one band of 64 rows, the longest the kernel makes (lcn_traps.stream_layout)
FUSED_SHAPES = [(1, 11, 16), (2, 64, 232), (3, 65, 236), (1, 129, 464), (2, 129, 468), (4, 65, 464), (1, 64, 468),
                (3, 11, 232), (200, 105, 16), (600, 64, 16)]


def fused_lcn(te, x, lcn_algo):
    N, _, H, W = x.shape
    D = 8
    from connecting_the_dots_amd import _lib
    assert _lib.lib().ctd_lcn_xcorrvol_supported(H, W, D, 5, 9), "the fused kernel does not cover %s" % ((N, H, W),)
    pat = te.lcn(dev(workloads.syn_dot_pattern(H, W, seed=3)[None, None]), 5, EPS)[0][0].contiguous()
    y, s, _, _ = te.lcn_xcorrvol_argmax(dev(x), pat, D, 9, 5, EPS, lcn_algo=lcn_algo)
    return y, s


FUSED_FAST_OUTSIDE = ("dark_bright", "bright_dark")     # outside CTD_LCN_FAST's stated contract (module docstring)


@pytest.mark.parametrize("kind,lcn_algo", [(k, "exact") for k in KINDS] +
                         [(k, "fast") for k in KINDS if k not in FUSED_FAST_OUTSIDE])
def test_fused_lcn_vs_f64(te, kind, lcn_algo):
    for i, (N, H, W) in enumerate(FUSED_SHAPES):
        x = frames(kind, N, H, W, 7 + i)
        y, s = fused_lcn(te, x, lcn_algo)
        if lcn_algo == "exact":
            assert_rule(x, 5, y, s, C_EXACT, "fused exact %s %s" % (kind, (N, H, W)))
        else:
            assert_rule(x, 5, y, s, C_FAST, "fused fast %s %s" % (kind, (N, H, W)), at=AT_STREAM_FAST)


TRAP_SHAPES = [(2, 432, 512), (1, 200, 464), (3, 97, 236)]
MIN_ARMED = 0.3          # of the motifs, on the device's band layout (the emulation finds about half armed)


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("N,H,W", TRAP_SHAPES)
def test_stream_exact_bits_on_trap_frames(te, oracle, N, H, W):
    x, motifs = T.trap_frames(N, H, W, seed=H + W)
    armed = T.armed(x, motifs, n_cu())
    assert len(armed) >= MIN_ARMED * len(motifs), "%d of %d traps armed on this layout" % (len(armed), len(motifs))
    y0, s0 = oracle.lcn(x, 5, EPS)
    y, s = fused_lcn(te, x, "exact")
    y, s = y.cpu().numpy(), s.cpu().numpy()
    ex = T.exact_windows(x, 5)
    bad = ex & ((y != y0) | (s != s0))
    assert not bad.any(), "%d pixels with exact f64 sums differ from the oracle's bits (%d of %d traps armed)" % (
        int(bad.sum()), len(armed), len(motifs))
    # the tie windows themselves: 1 + 2^-24 rounds to 1
    for f, p, c in armed:
        assert s[f, 0, p + T.TIE_ROW, c] == s0[f, 0, p + T.TIE_ROW, c]


@pytest.mark.parametrize("N,H,W", [(2, 432, 512), (1, 65, 236)])
def test_stream_exact_bits_on_hdr_frames(te, oracle, N, H, W):
    x = T.hdr_block_frames(N, H, W, seed=W)
    y0, s0 = oracle.lcn(x, 5, EPS)
    y, s = fused_lcn(te, x, "exact")
    ex = T.exact_windows(x, 5)
    assert ex.mean() > 0.5
    bad = ex & ((y.cpu().numpy() != y0) | (s.cpu().numpy() != s0))
    assert not bad.any(), "%d pixels with exact f64 sums differ from the oracle's bits" % int(bad.sum())


@pytest.mark.parametrize("radius", [5, 2])
def test_tiled_exact_bits_on_trap_and_hdr_frames(te, oracle, radius):
    """ctd_lcn_f32 sums in the oracle's order (rows, then columns, ascending, f64): its bits everywhere, exact window or not"""
    for x in (T.trap_frames(2, 200, 300, seed=1)[0], T.hdr_frames(2, 97, 150, seed=2), T.hdr_block_frames(2, 97, 150, seed=3)):
        y0, s0 = oracle.lcn(x, radius, EPS)
        y, s = te.lcn(dev(x), radius, EPS, algo="exact")
        assert np.array_equal(y.cpu().numpy(), y0) and np.array_equal(s.cpu().numpy(), s0)


@pytest.mark.parametrize("W", [232, 230])
def test_fused_plain_argmax_with_volume_runs_the_two_calls(te, W):
    """rerank_eps < 0 with a volume is a plain argmax of the fast scores (xcorrvol_argmax); the fused call gives the
    two-call path's results on a shape the fused kernel covers (W % 4 == 0) and on one it does not"""
    N, H, D = 2, 40, 24
    rs = np.random.RandomState(W)
    x = dev(rs.rand(N, 1, H, W).astype(np.float32))
    pat = te.lcn(dev(workloads.syn_dot_pattern(H, W, seed=3)[None, None]), 5, EPS)[0][0].contiguous()
    y, s, idx, best, vol = te.lcn_xcorrvol_argmax(x, pat, D, 9, 5, EPS, return_volume=True, rerank_eps=-1)
    y2, s2 = te.lcn(x, 5, EPS)
    idx2, best2, vol2 = te.xcorrvol_argmax(y2, pat, D, 9, return_volume=True, algo="fast", rerank_eps=-1)
    assert torch.equal(y, y2) and torch.equal(s, s2)
    assert torch.equal(vol, vol2) and torch.equal(idx, idx2) and torch.equal(best, best2)
    assert torch.equal(idx, te.argmax_disp(vol)[0])                 # the plain argmax of the returned volume


def test_fast_kernel_serves_radius_7_only(te):
    """ctd_lcn_fast_f32 refuses the radii whose f32 sums failed the rule above; lcn(algo='fast') runs the exact kernel"""
    from connecting_the_dots_amd import _lib
    x = dev(frames("dark_bright", 1, 40, 70, 0))
    y, s = torch.empty_like(x), torch.empty_like(x)
    L = _lib.lib()
    for radius in range(1, 8):
        st = L.ctd_lcn_fast_f32(x.data_ptr(), y.data_ptr(), s.data_ptr(), 1, 40, 70, radius, EPS, 0,
                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (st == 0) == (radius == 7), (radius, st)
        if radius != 7:
            assert all(torch.equal(a, b) for a, b in zip(te.lcn(x, radius, EPS, algo="fast"), te.lcn(x, radius, EPS)))


def test_fused_fast_outside_its_contract(te):
    """the header's exclusion is real: on long dark runs under bright rows the fused fast LCN misses the rule (measured:
    std 7.6 x its elementwise bound, 3.3 x the stock-f32 error), while 'exact' meets it (test_fused_lcn_vs_f64); the
    outputs stay finite"""
    worst = 0.0
    for i, (N, H, W) in enumerate(FUSED_SHAPES):
        for kind in FUSED_FAST_OUTSIDE:
            x = frames(kind, N, H, W, 7 + i)
            y, s = fused_lcn(te, x, "fast")
            assert bool(torch.isfinite(y).all() and torch.isfinite(s).all()), "fused fast %s %s" % (kind, (N, H, W))
            el, st, msg = errors(x, 5, y, s, C_FAST, AT_STREAM_FAST)
            worst = max(worst, el)
    assert worst > 1, "the stated exclusion is no longer needed: drop it from include/ctd_hip.h and the tests"
