"""The float64 references of tests/f64_refs.py against the values and autograd gradients captured from the reference
modules (tests/golden/losses.npz, pattern_loss.npz), on the CPU.  The goldens are ATen f32; the tolerances are the
ones tests/test_losses_gpu.py and tests/test_pattern_loss_gpu.py hold the HIP kernels to against the same goldens, so
a reference that passes here restates the reference modules (and not the kernels' own formulas) to within the goldens'
f32 rounding."""
import numpy as np
import pytest
import torch

from tests import f64_refs as R
from tests import matcher_traps as MT
from tests.util import assert_close, golden


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_disp_to_depth_ref():
    g = golden("losses")
    ref = R.disp_to_depth(t(g["d2d_disp"]), float(g["d2d_bf"]), t(g["d2d_go"]))
    assert ref.value.dtype == torch.float64
    assert_close(ref.value.numpy(), g["d2d_depth"], rtol=1e-6, atol=0, what="depth")
    assert_close(ref.grads["disp"].numpy(), g["d2d_grad"], rtol=2e-6, atol=0, what="grad")
    assert (ref.grads["disp"][t(g["d2d_disp"]) <= 0] == 0).all()


def test_sobel_ref():
    g = golden("losses")
    gx, gy = R.sobel(t(g["dl_disp"]).double())
    # the golden's f32 sums run over disparities up to ~70 (ulp 7.6e-6)
    assert_close(torch.cat((gx, gy), 1).numpy(), g["sobel_grad"], rtol=1e-5, atol=1e-5, what="sobel")


def test_disparity_loss_ref_with_edge():
    g = golden("losses")
    ref = R.disparity_loss(t(g["dl_disp"]), t(g["dl_edge"]))
    assert_close(float(ref.value), g["dl_val"], rtol=1e-5, atol=0, what="value")
    assert_close(ref.grads["disp"].numpy(), g["dl_gdisp"], rtol=1e-4, atol=1e-8, what="grad disp")
    assert_close(ref.grads["edge"].numpy(), g["dl_gedge"], rtol=1e-4, atol=1e-9, what="grad edge")


def test_disparity_loss_ref_without_edge():
    g = golden("losses")
    ref = R.disparity_loss(t(g["dl_disp"]))
    assert_close(float(ref.value), g["dl_noedge_val"], rtol=1e-5, atol=0, what="value")
    assert_close(ref.grads["disp"].numpy(), g["dl_noedge_gdisp"], rtol=1e-4, atol=1e-8, what="grad disp")


def test_disparity_loss_ref_logits_chain():
    """edge = 1 - sigmoid(logits): the logits gradient is the edge gradient times -sigmoid'"""
    g = golden("losses")
    e = t(g["dl_edge"]).double().clamp(1e-6, 1 - 1e-6)
    logits = torch.log((1 - e) / e)                          # 1 - sigmoid(logits) == e
    ref = R.disparity_loss(t(g["dl_disp"]), logits=logits)
    s = torch.sigmoid(logits)
    ref_e = R.disparity_loss(t(g["dl_disp"]), edge=1 - s)
    assert torch.allclose(ref.value, ref_e.value, rtol=1e-12, atol=0)
    assert torch.allclose(ref.grads["logits"], -ref_e.grads["edge"] * s * (1 - s), rtol=1e-9, atol=1e-15)
    assert_close(ref.grads["disp"].numpy(), g["dl_gdisp"], rtol=1e-4, atol=1e-8, what="grad disp")


@pytest.mark.parametrize("tag,clamp", [("c", 0.1), ("nc", -1.0)])
def test_geometric_loss_ref(tag, clamp):
    g = golden("losses")
    a = {n: t(g["ge_" + n]) for n in ("depth0", "depth1", "K", "R0", "t0", "R1", "t1")}
    ray = t(g["ge_ray"][0])
    ref = R.geometric_loss(a["depth0"], a["depth1"], a["K"], ray, a["R0"], a["t0"], a["R1"], a["t1"], clamp)
    assert_close(float(ref.value), g["ge_%s_val" % tag], rtol=2e-5, atol=0, what="value")
    assert_close(ref.grads["depth0"].numpy(), g["ge_%s_g0" % tag], rtol=2e-3, atol=2e-7, what="grad depth0")
    assert_close(ref.grads["depth1"].numpy(), g["ge_%s_g1" % tag], rtol=2e-3, atol=2e-7, what="grad depth1")
    # one direction and its intermediates: ProjectionBaseLoss's uv and d, the un-normalised sampling coordinates
    B, _, H, W = g["ge_depth0"].shape
    fwd = ref.inter["fwd"]
    assert_close(fwd["d"].reshape(B, -1, 1).numpy(), g["ge_d"], rtol=1e-5, atol=1e-6, what="d")
    u = (2 * fwd["ix"] + 1) / W * (W - 1) / 2                   # invert the align_corners=False unnormalisation
    v = (2 * fwd["iy"] + 1) / H * (H - 1) / 2
    assert_close(torch.stack((u.reshape(B, -1), v.reshape(B, -1)), 2).numpy(), g["ge_uv"], rtol=1e-5, atol=1e-4,
                 what="uv")
    with torch.no_grad():
        dd = {k: x.double() for k, x in a.items()}
        v01, _ = R.geometric_dir(dd["depth0"], dd["depth1"], dd["K"], ray.double(), dd["R0"], dd["t0"], dd["R1"],
                                 dd["t1"], clamp)
    assert_close(float(v01), g["ge_%s_fwd01" % tag], rtol=2e-5, atol=0, what="one direction")
    assert torch.equal(fwd["diff"], fwd["e"].abs())


@pytest.mark.parametrize("name", ["census_sad", "mse"])
@pytest.mark.parametrize("use_std", [True, False])
def test_pattern_loss_ref(name, use_std):
    g = golden("pattern_loss")
    ref = R.pattern_loss(t(g["disp"]), t(g["im"]), t(g["pattern"]), t(g["std"]) if use_std else None, name, 0.5)
    val, proj = ref.value
    tag = "%s_%d" % (name, use_std)
    assert_close(proj.numpy(), g["proj_" + tag], rtol=1e-5, atol=2e-5, what="proj " + tag)
    assert_close(float(val), g["val_" + tag], rtol=1e-4, atol=0, what="val " + tag)
    assert_close(ref.grads["disp"].numpy(), g["gdisp_" + tag], rtol=2e-3, atol=2e-6, what="grad " + tag)
    B, _, H, W = g["disp"].shape
    assert ref.inter["pair"].shape == (B, 81, H, W)
    assert_close(ref.inter["ix"].numpy(), np.arange(W) * W / (W - 1) - 0.5 - g["disp"].astype(np.float64) * W / (W - 1), rtol=0,
                 atol=1e-9, what="ix")


def test_pattern_loss_ref_upstream_proj_gradient_and_frames():
    """grad_proj adds grad_proj . d proj / d disp; a batch equals its frames run with the shared denominator"""
    g = golden("pattern_loss")
    disp, im, pat, std = (t(g[k]) for k in ("disp", "im", "pattern", "std"))
    gp = torch.from_numpy(np.random.RandomState(3).randn(*g["disp"].shape))
    a = R.pattern_loss(disp, im, pat, std, "census_sad", 0.5)
    b = R.pattern_loss(disp, im, pat, std, "census_sad", 0.5, grad_proj=gp)
    d = disp.double().requires_grad_(True)
    grid, _, _ = R.warp_grid(d, *disp.shape[2:])
    proj = torch.nn.functional.grid_sample(pat.double().mean(1, keepdim=True).expand(2, -1, -1, -1), grid,
                                           padding_mode="border", align_corners=False)
    (gproj,) = torch.autograd.grad((proj * gp).sum(), d)
    assert torch.allclose(b.grads["disp"], a.grads["disp"] + gproj, rtol=1e-10, atol=1e-14)
    # whole-batch composition in one graph
    d = disp.double().requires_grad_(True)
    grid, _, _ = R.warp_grid(d, *disp.shape[2:])
    proj = torch.nn.functional.grid_sample(pat.double().mean(1, keepdim=True).expand(2, -1, -1, -1), grid,
                                           padding_mode="border", align_corners=False)
    diff, _ = R.block_loss(proj, im.double(), 9, "census_sad", 0.5)
    val = (std.double() * diff).sum() / std.double().sum()
    (gd,) = torch.autograd.grad(val, d)
    assert torch.allclose(a.grads["disp"], gd, rtol=1e-10, atol=1e-14)
    assert torch.allclose(a.value[0], val.detach(), rtol=1e-12, atol=0)


def test_block_loss_ref_matches_package_composition():
    """the four loss types against photometric_loss_pytorch, the package's stock-torch formulation"""
    from connecting_the_dots_amd.torchext.functions import photometric_loss_pytorch
    rs = np.random.RandomState(7)
    es, ta = torch.from_numpy(rs.randn(2, 1, 13, 21)), torch.from_numpy(rs.randn(2, 1, 13, 21))
    for name in R.PHOTO_TYPES:
        got, pair = R.block_loss(es, ta, 9, name, 0.5)
        assert torch.allclose(got, photometric_loss_pytorch(es, ta, 9, name, 0.5), rtol=1e-12, atol=1e-15), name
        assert pair.shape == (2, 81, 13, 21)


def test_lcn_ref_vs_reference_golden():
    """the LCN vectors captured from networks.LCN, at the tolerances tests/test_oracle_golden.py holds the oracle to"""
    g = golden("lcn_networks")
    for key, r, eps in (("0", 5, 0.05), ("1", 5, 0.05), ("r2", 2, 0.1)):
        ref = R.lcn(t(g["x_" + key]), r, eps)
        y, s = ref.value
        assert y.dtype == torch.float64
        assert_close(s.numpy(), g["std_" + key], what="std " + key)
        assert_close(y.numpy(), g["y_" + key], rtol=2e-5, atol=2e-6, what="lcn " + key)
        assert torch.allclose(ref.inter["var"], ref.inter["ex2"] - ref.inter["avg"] ** 2 + 1e-6, rtol=0, atol=0)
        f32 = R.lcn(t(g["x_" + key]), r, eps, dtype=torch.float32)
        assert f32.value[0].dtype == torch.float32
        assert_close(f32.value[1].numpy(), g["std_" + key], what="f32 std " + key)


@pytest.mark.parametrize("radius", [0, 1, 5, 9])
def test_lcn_ref_vs_oracle(oracle, radius):
    """the f64 reference against the oracle (f64 sums, f32 tail) on frames with a DC level, and at radius = min(H, W) - 1"""
    rs = np.random.RandomState(radius)
    for x in ((rs.rand(2, 1, 24, 37) * 3 + rs.randn(2, 1, 1, 1)).astype(np.float32),
              rs.rand(1, 1, radius + 1, 30).astype(np.float32), rs.rand(1, 1, 30, radius + 1).astype(np.float32)):
        y0, s0 = oracle.lcn(x, radius, 0.05)
        y, s = R.lcn(t(x), radius, 0.05).value
        assert_close(s.numpy(), s0, what="std r%d" % radius)
        assert_close(y.numpy(), y0, rtol=2e-5, atol=2e-6, what="lcn r%d" % radius)


# ---------------------------------------------------------------------------------------------------------------------
# the matcher references: f64_refs.xcorrvol / costvol, and the listing-rule classifier of tests/matcher_traps.py
# ---------------------------------------------------------------------------------------------------------------------
def _ncc_close(got, ref, C, what):
    """NCC volumes sum C terms of magnitude <= 1: 1e-12 relative, with C * 1e-12 as the floor near zero"""
    assert_close(got, ref, rtol=1e-12, atol=1e-12 * C, what=what)


def test_xcorrvol_ref_vs_oracle_f64_and_goldens():
    """every case of the committed reference volumes: the f64 ones to 1e-12, the f32 ones to their own rounding; and
    the oracle's f64 instantiation on the same (f32-valued) inputs to 1e-12"""
    from oracle import oracle
    g = golden("xcorrvol_small")
    for k, (C, H, W, D, bs) in enumerate(g["cases"]):
        a, b = g["in0_%d" % k], g["in1_%d" % k]
        vol = R.xcorrvol(t(a), t(b), int(D), int(bs))
        assert vol.dtype == torch.float64 and vol.shape == (D, H, W)
        if a.dtype == np.float64:
            _ncc_close(vol.numpy(), g["vol_%d" % k], C, "golden %d" % k)
        else:
            assert_close(vol.numpy(), g["vol_%d" % k], what="golden %d (f32)" % k)
        o64 = oracle.xcorrvol(a.astype(np.float64), b.astype(np.float64), int(D), int(bs))
        _ncc_close(vol.numpy(), o64, C, "oracle f64 %d" % k)


@pytest.mark.parametrize("name", ["staircase", "flat", "clipped255", "scale+3", "chan_cancel"])
def test_xcorrvol_ref_vs_oracle_f64_on_traps(name):
    """batched frames, the left-border run (D > W / 2), odd and even block sizes, on trap frames with DC offsets"""
    from oracle import oracle
    from tests import matcher_traps as T
    C = 2 if name == "chan_cancel" else 1
    gen = {**T.NCC_GENERATORS, **T.MULTICHANNEL_GENERATORS}[name]
    for bs, D in ((9, 23), (4, 7)):
        frames, pat = gen(5, 2, C, 13, 37, bs)
        vol = R.xcorrvol(t(frames), t(pat), D, bs, budget=1 << 16).numpy()
        for f in range(2):
            o64 = oracle.xcorrvol(frames[f].astype(np.float64), pat.astype(np.float64), D, bs)
            _ncc_close(vol[f], o64, C, "%s bs %d frame %d" % (name, bs, f))


def test_costvol_ref_vs_golden():
    """the composition of block_loss against the reference's own (f32) composition: within its f32 rounding"""
    g = golden("costvol")
    for ty, name in enumerate(R.PHOTO_TYPES):
        vol = R.costvol(t(g["im"]), t(g["pat"]), int(g["D"]), int(g["bs"]), name, float(np.float32(0.5)))
        assert vol.dtype == torch.float64
        assert_close(vol.numpy(), g["vol_%d" % ty], rtol=2e-6, atol=1e-7, what=name)
        assert np.array_equal(vol.numpy().argmin(0), g["argmin_%d" % ty]), name


def test_costvol_ref_per_frame_pattern():
    """[N,H,W] frames against a shared and a per-frame pattern: each frame's slice is the single-frame volume"""
    rs = np.random.RandomState(4)
    im, pat = t(rs.rand(2, 9, 30).astype(np.float32)), t(rs.rand(2, 9, 30).astype(np.float32))
    shared = R.costvol(im, pat[0], 12, 5, "census_sad", 0.5, chunk=5)
    per = R.costvol(im, pat, 12, 5, "census_sad", 0.5, chunk=5)
    for f in range(2):
        assert torch.equal(shared[f], R.costvol(im[f], pat[0], 12, 5, "census_sad", 0.5))
        assert torch.equal(per[f], R.costvol(im[f], pat[f], 12, 5, "census_sad", 0.5))


def _recount(img, bs, cols, C):
    """the listing rule window by window, straight from the reference's clamp formulas (ext.h:145-160)"""
    from tests import matcher_traps as T
    H, W = img.shape
    n, h = bs * bs, bs // 2
    x = img.astype(np.float64)
    cval = float(np.float32(sum(x[min(max(H // 2 + k // bs - h, 0), H - 1), min(max(W // 2 + k % bs - h, 0), W - 1)]
                                for k in range(n)) / n))
    out = np.empty((H, len(cols)), np.int8)
    for r in range(H):
        for i, c in enumerate(cols):
            v = np.array([x[min(max(r + bh - h, 0), H - 1), min(max(c + bw - h, 0), W - 1)]
                          for bh in range(bs) for bw in range(bs)])
            m = v.mean()
            V = ((v - m) ** 2).sum()
            st = {"f1": np.array(n * (m - cval) ** 2 / V if V > 0 else np.inf), "dev": np.array(np.sqrt(V)),
                  "flat": np.array(T.K_FLAT * n * m * m / V if V > 0 else np.inf)}
            out[r, i] = T.window_class(st, T.K_FLAG_RATIO / C)
    return out


@pytest.mark.parametrize("name", ["staircase", "devfloor", "flat", "dots"])
def test_classifier_vs_recount(name):
    """classify() against a direct per-window recount, frame side and pattern side (unclamped columns, the left-border
    run included), on a frame that has windows in all three classes"""
    from tests import matcher_traps as T
    bs, D = 5, 9
    frames, pat = T.NCC_GENERATORS[name](1, 1, 1, 11, 45, bs)
    cls, sqrtF, floor = T.classify(frames, pat, D, bs)
    ca = _recount(frames[0, 0], bs, range(45), 1)
    cb = _recount(pat[0], bs, range(-(D - 1), 45), 1)
    want = np.stack([np.maximum(ca, cb[:, np.arange(45) - d + D - 1]) for d in range(D)])
    assert np.array_equal(cls[0], want), name
    assert (sqrtF >= 1).all() and (floor > 0).all()
    if name == "staircase":
        assert {T.LISTED, T.GUARDED, T.UNLISTED} <= set(np.unique(cls).tolist())


@pytest.mark.parametrize("bs,H,W", [shape[:3] for shape in MT.NCC_SHAPES])
def test_trap_placement(bs, H, W):
    """at the GPU suite's own seeds and shapes, the generators put interior windows where they say: F - 1 at
    kFlagRatio / C * r (staircase, C = 1, 2, 3), deviation at kDevFloor * r (devfloor), kFlatRatio n mean^2 / V at r
    (every flat level), for r in 0.9, 0.98, 1.02, 1.1 -- and the staircase's centring window lies inside its level-0
    band, so cval is the tile's mean"""
    from tests import matcher_traps as T
    cases = [("staircase", C, "f1", lambda r, C=C: T.K_FLAG_RATIO / C * r) for C in (1, 2, 3)]
    cases += [("devfloor", 1, "dev", lambda r: T.K_DEV_FLOOR * r)]
    cases += [(name, 1, "flat", lambda r: r) for name in T.FLAT_LEVELS]
    gens = {**T.NCC_GENERATORS, **T.MULTICHANNEL_GENERATORS}
    for name, C, key, target in cases:
        frames, pat = gens[name](T.trap_seed(bs, H, C), 2, C, H, W, bs)
        for img in (frames[0], frames[1], pat):
            st = T.window_stats(img, bs)
            if name == "staircase":
                assert np.abs(st["cval"]).max() < 1e-6, (name, C, bs)
            h = bs // 2                                        # windows clear of the border clamps
            vals = st[key][:, h:H - h, h:W - h].ravel()
            for r in T.RATIOS:
                assert np.isclose(vals, target(r), rtol=2e-3).any(), (name, C, bs, r)
