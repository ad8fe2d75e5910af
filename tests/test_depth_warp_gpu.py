"""GPU parity of forward depth warping and the windowed band (torchext.depth_warp / disparity_band_window,
ctd_depth_warp_f32 / ctd_disparity_band_window_f32) against tests/warp_ref.py: every output equals the numpy restatement
at every element (np.array_equal on the values, the NaN masks and src; no tolerance, no pixel left out -- the
definitions use IEEE add, sub, mul, div, floor, ceil, min, max and compares only, so a mismatch is an ordering bug on one
of the two sides).  Every call runs twice and the two results must be equal bit for bit; the inputs are compared with
clones afterwards."""
import numpy as np
import pytest
import torch

from tests import fusion_ref as fr
from tests import warp_ref as wr

pytestmark = pytest.mark.gpu

# (B, V, H, W): across the 256-pixel chunk of the scatter kernel, a view boundary, H == 1, W == 1, more than one track,
# a single view
WARP_SHAPES = [(1, 2, 5, 7), (2, 3, 17, 65), (1, 5, 33, 130), (1, 2, 4, 63), (1, 2, 4, 64), (1, 3, 9, 257), (2, 2, 1, 75),
               (2, 2, 19, 1), (1, 4, 40, 300), (1, 1, 6, 23)]
# (N, H, W): across the 64 x 4 tile; window 15 is wider than the tile's 4 rows and than H or W of some shapes
BAND_SHAPES = [(1, 5, 7), (2, 17, 65), (1, 4, 63), (1, 4, 64), (1, 9, 257), (2, 1, 75), (2, 19, 1), (1, 40, 300)]


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(t):
    """a float tensor as integers, so that NaN entries compare equal to themselves"""
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_float(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: the NaN positions differ at %d elements" % (
        what, int((np.isnan(got) != np.isnan(want)).sum()))
    a, b = np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0)
    assert np.array_equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.size)


def equal_runs(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)), "%s: two runs differ" % what


def unchanged(t_in, before, what):
    for x, x0 in zip(t_in, before):
        assert x is None or torch.equal(bits(x), bits(x0)), "%s: an input was written" % what


def view_masks(rs, B, V):
    """seeded random sources / targets, then fixed up so that every shape tests the per-view selection: track 0 warps
    from a proper subset of its views (view 0 is a source, view 1 is not) into its last view at least, and its view 0
    is no target; with more than one track the last one has no source at all (single tracks get that as a case of
    its own, NO_SOURCE)"""
    sources = (rs.rand(B, V) < 0.7).astype(np.uint8)
    targets = (rs.rand(B, V) < 0.7).astype(np.uint8)
    targets[0, 0] = 0
    if V > 1:
        sources[0, 0], sources[0, 1] = 1, 0
        targets[0, V - 1] = 1
    if B > 1:
        sources[B - 1] = 0
        targets[B - 1] = 1
    return sources, targets


def check_warp(te, sc, with_valid, masks, splat, what):
    """depth_warp at one setting, twice, with and without src, against the restatement -> z as it came out"""
    valid = sc["valid"] if with_valid else None
    sources, targets = masks
    want_z, want_src = wr.warp(sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], valid, sources, targets, splat)
    t_in = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t")] + [dev(valid), dev(sources), dev(targets)]
    before = [None if x is None else x.clone() for x in t_in]
    got = te.depth_warp(*t_in, splat=splat, return_src=True)
    equal_runs(got, te.depth_warp(*t_in, splat=splat, return_src=True), what)
    z, src = host(got[0]), host(got[1])
    assert src.dtype == np.int64 and src.shape == want_src.shape
    same_float(z, want_z, what + " z")
    assert np.array_equal(src, want_src), "%s: %d src differ" % (what, int((src != want_src).sum()))
    only_z = te.depth_warp(*t_in, splat=splat)                                  # return_src=False: the same z, alone
    assert isinstance(only_z, torch.Tensor)
    equal_runs((only_z,), got[:1], what + " without src")
    unchanged(t_in, before, what)
    if targets is not None:
        off = targets == 0
        assert np.isnan(z[off]).all() and (src[off] == -1).all()
    return z


@pytest.mark.parametrize("shape", WARP_SHAPES)
def test_warp_equals_the_restatement(te, shape):
    B, V, H, W = shape
    seed = 1000 * B + 100 * V + H + W
    masks = view_masks(np.random.RandomState(seed), B, V)
    if V > 1:
        assert 0 < masks[0][0].sum() < V and masks[0][0, 0] == 1 and masks[1][0, V - 1] == 1      # a proper subset warps
    assert masks[1][0, 0] == 0 and (B == 1 or not masks[0][B - 1].any())
    no_source = (np.zeros((B, V), np.uint8), np.ones((B, V), np.uint8))
    for kind in fr.SCENE_KINDS:
        sc = fr.make_scene(kind, B, V, H, W, seed)
        for splat in (0, 1, 2):
            for with_valid in (True, False):
                what = "%s %s splat %d valid %d" % (kind, shape, splat, with_valid)
                z_all = check_warp(te, sc, with_valid, (None, None), splat, what)
                z_sub = check_warp(te, sc, with_valid, masks, splat, what + " masks")
                if V == 1 or kind == "away":
                    assert np.isnan(z_all).all() and np.isnan(z_sub).all(), what
                elif kind == "clean":
                    # the subset lands candidates in track 0's last view, and they are not the unmasked run's
                    assert not np.isnan(z_all).all() and not np.isnan(z_sub[0, V - 1]).all(), what
                    assert not np.array_equal(bits(torch.from_numpy(z_sub)), bits(torch.from_numpy(z_all))), what
                    assert not np.isnan(z_all[0, 0]).all() and np.isnan(z_sub[0, 0]).all(), what
        assert np.isnan(check_warp(te, sc, True, no_source, 1, "%s %s no source" % (kind, shape))).all()


def test_a_view_left_out_of_the_sources_contributes_nothing(te):
    """1 x 4 x 40 x 300, clean: views 0 and 2 warped into view 3 with view 1 left out.  src never points into view 1 (nor
    into the target), it does point into both sources, and some pixels differ from the run that may use view 1"""
    B, V, H, W = 1, 4, 40, 300
    sc = fr.make_scene("clean", B, V, H, W, 31)
    sources, targets = np.array([[1, 0, 1, 0]], np.uint8), np.array([[0, 0, 0, 1]], np.uint8)
    t_in = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t")]
    for splat in (0, 1):
        want = wr.warp(sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], None, sources, targets, splat)
        got = te.depth_warp(*t_in, sources=dev(sources), targets=dev(targets), splat=splat, return_src=True)
        equal_runs(got, te.depth_warp(*t_in, sources=dev(sources), targets=dev(targets), splat=splat, return_src=True), "subset")
        same_float(host(got[0]), want[0], "subset z")
        assert np.array_equal(host(got[1]), want[1])
        src = host(got[1])[0, 3]
        view = src[src >= 0] // (H * W)
        assert set(np.unique(view)) == {0, 2}
        with_1 = te.depth_warp(*t_in, sources=dev(np.array([[1, 1, 1, 0]], np.uint8)), targets=dev(targets), splat=splat,
                               return_src=True)
        src_1 = host(with_1[1])[0, 3]
        assert (src_1[src_1 >= 0] // (H * W) == 1).any() and not np.array_equal(src_1, src)


def test_the_z_buffer_chooses_at_an_occlusion(te):
    """clean 1 x 3 x 33 x 130: background pixels of the sources land behind the patch in the target; the nearer wins, and
    more than one candidate reaches many pixels (else there is nothing to choose)"""
    sc = fr.make_scene("clean", 1, 3, 33, 130, 21)
    z, src = wr.warp(sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"])
    one = [wr.warp(sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], sources=np.eye(3, dtype=np.uint8)[s:s + 1])[0]
           for s in range(3)]
    stack = np.stack(one)[:, 0]                                                # [source, view, H, W]
    n_cand = (~np.isnan(stack)).sum(0)
    assert (n_cand >= 2).mean() > 0.5
    near = np.where(np.isnan(stack), np.inf, stack).min(0)
    far = np.where(np.isnan(stack), -np.inf, stack).max(0)
    differ = (n_cand >= 2) & (far > 1.2 * near)
    assert differ.sum() >= 10                                                  # patch against background
    t_in = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t")]
    got = te.depth_warp(*t_in, return_src=True)
    equal_runs(got, te.depth_warp(*t_in, return_src=True), "occlusion")
    same_float(host(got[0]), z, "occlusion z")
    assert np.array_equal(host(got[1]), src)
    assert np.array_equal(host(got[0])[0][differ], near[differ].astype(np.float32))


def test_a_tie_goes_to_the_lower_view(te):
    """views 0 and 1 with the same pose and depth, view 2 the only target: every candidate comes twice with the same z,
    and src must point into view 0"""
    B, V, H, W = 1, 3, 17, 65
    sc = fr.make_scene("clean", B, V, H, W, 9)
    for k in ("depth", "valid", "R", "t"):
        sc[k][:, 1] = sc[k][:, 0]
    targets = np.array([[0, 0, 1]], np.uint8)
    for splat in (0, 1):
        want_z, want_src = wr.warp(sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], None, None, targets, splat)
        t_in = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t")]
        z, src = te.depth_warp(*t_in, targets=dev(targets), splat=splat, return_src=True)
        equal_runs((z, src), te.depth_warp(*t_in, targets=dev(targets != 0), splat=splat, return_src=True), "tie")
        z, src = host(z), host(src)
        same_float(z, want_z, "tie z")
        assert np.array_equal(src, want_src)
        hit = src[0, 2] >= 0
        assert hit.mean() > 0.5 and (src[0, 2][hit] < H * W).all()             # view 0 of track 0
        assert np.array_equal(hit, ~np.isnan(z[0, 2])) and (src[0, :2] == -1).all()
        # and the winner's depth, pushed through the definition again, is the z that came out
        q = src[0, 2][hit]
        uvd = fr.transform(sc["depth"][0, 0].reshape(-1)[q], sc["ray"][q], sc["R"][0, 0], sc["t"][0, 0], sc["R"][0, 2],
                           sc["t"][0, 2], sc["K"])
        assert np.array_equal(uvd[2], z[0, 2][hit])


def test_garbage_in_the_outputs_and_the_workspace_changes_nothing(te):
    """C ABI: outputs and workspace pre-filled with garbage give the same results; src may be NULL; a short workspace is
    turned down"""
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    B, V, H, W = 2, 3, 17, 65
    sc = fr.make_scene("noisy", B, V, H, W, 12)
    depth, ray, K, R, t, valid = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t", "valid")]
    want = te.depth_warp(depth, ray, K, R, t, valid, splat=1, return_src=True)
    need = L.ctd_depth_warp_workspace_bytes(B, V, H, W)
    assert need == (8 * B * V * H * W + 255) // 256 * 256
    stream = torch.cuda.current_stream().cuda_stream
    for fill in (0x00, 0x7F, 0x01):
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        z = torch.full((B, V, H, W), 7.0, dtype=torch.float32, device="cuda")
        src = torch.full((B, V, H, W), -5, dtype=torch.int64, device="cuda")
        for with_src in (True, False):
            st = L.ctd_depth_warp_f32(depth.data_ptr(), valid.data_ptr(), ray.data_ptr(), K.data_ptr(), R.data_ptr(),
                                      t.data_ptr(), None, None, 1, z.data_ptr(), src.data_ptr() if with_src else None,
                                      B, V, H, W, ws.data_ptr(), need, 0, stream)
            torch.cuda.synchronize()
            assert st == 0
            equal_runs((z, src), want, "filled outputs, fill %#x" % fill)
    st = L.ctd_depth_warp_f32(depth.data_ptr(), valid.data_ptr(), ray.data_ptr(), K.data_ptr(), R.data_ptr(), t.data_ptr(),
                              None, None, 1, z.data_ptr(), None, B, V, H, W, ws.data_ptr(), need - 1, 0, stream)
    assert st == 2                                                             # CTD_ERR_WORKSPACE


def test_argument_errors_and_empty_inputs(te):
    sc = fr.make_scene("clean", 2, 3, 9, 20, 0)
    depth, ray, K, R, t, valid = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t", "valid")]
    ones = torch.ones(2, 3, dtype=torch.bool, device="cuda")
    te.depth_warp(depth, ray, K, R, t, valid, ones, ones, 2, True)
    bad_args = [
        (depth.cpu(), ray.cpu(), K.cpu(), R.cpu(), t.cpu(), valid.cpu()), (depth, ray.cpu(), K, R, t, valid),
        (depth, ray, K, R, t, valid.cpu()), (depth, ray, K, R, t, valid, ones.cpu()), (depth, ray, K, R, t, valid, None, ones.cpu()),
        (depth.double(), ray, K, R, t, valid), (depth, ray, K.double(), R, t, valid), (depth, ray, K, R, t, valid.to(torch.int32)),
        (depth, ray, K, R, t, valid, ones.float()), (depth, ray, K, R, t, valid, None, ones.to(torch.int64)),
        (depth.transpose(2, 3), ray, K, R, t, None), (depth, ray, K, R.transpose(2, 3), t, valid),
        (depth, ray, K, R, t, valid, ones.t().contiguous().t()),
        (depth[0], ray, K, R, t, None), (depth, ray[:-1].contiguous(), K, R, t, valid), (depth, ray, K, R[:1].contiguous(), t, valid),
        (depth, ray, K, R, t, valid[0]), (depth, ray, K, R, t, valid, ones[:1]), (depth, ray, K, R, t, valid, None, ones[:, :2]),
        (depth, ray, K, R, t, valid, None, None, 3), (depth, ray, K, R, t, valid, None, None, -1),
        (torch.empty(1, 2, 0, 5, device="cuda"), ray, K, R, t, None),
        (torch.empty(1, 65, 1, 1, device="cuda"), torch.ones(1, 3, device="cuda"), K,
         torch.zeros(1, 65, 3, 3, device="cuda"), torch.zeros(1, 65, 3, device="cuda"), None),   # more than 64 views
    ]
    for a in bad_args:
        with pytest.raises(RuntimeError):
            te.depth_warp(*a)
    z, src = te.depth_warp(torch.empty(0, 3, 9, 20, device="cuda"), ray, K, torch.empty(0, 3, 3, 3, device="cuda"),
                           torch.empty(0, 3, 3, device="cuda"), return_src=True)      # no tracks: empty results, no launch
    assert z.shape == src.shape == (0, 3, 9, 20) and z.dtype == torch.float32 and src.dtype == torch.int64
    prior = torch.zeros(2, 9, 20, device="cuda")
    for a, kw in (((prior.cpu(), 1.0, 8), {}), ((prior.double(), 1.0, 8), {}), ((prior.transpose(1, 2), 1.0, 8), {}),
                  ((prior[0, 0], 1.0, 8), {}), ((prior, 1.0, 0), {}), ((prior, 1.0, 8), dict(window=2)),
                  ((prior, 1.0, 8), dict(window=17)), ((prior, 1.0, 8), dict(holes="some"))):
        with pytest.raises(RuntimeError):
            te.disparity_band_window(*a, **kw)
    lo, hi = te.disparity_band_window(torch.empty(0, 9, 20, device="cuda"), 1.0, 8)
    assert lo.shape == hi.shape == (0, 9, 20) and lo.dtype == torch.int32


# ---------------------------------------------------------------------------------------------------------------------
# the windowed band
# ---------------------------------------------------------------------------------------------------------------------
def priors(rs, shape, D):
    """name -> prior f32: dense in range; 30 % NaN; all NaN; with +-inf; with values below 0 and above D"""
    dense = rs.uniform(0, D - 1, shape).astype(np.float32)
    step = np.where(np.arange(shape[-1]) < shape[-1] // 2, np.float32(0.25 * D), np.float32(0.75 * D))   # an edge
    dense = np.where(rs.rand(*shape) < 0.5, dense, step + rs.uniform(-1, 1, shape)).astype(np.float32)
    dense[rs.rand(*shape) < 0.2] = np.float32(rs.randint(0, D))            # exact integers: ceil == floor
    nan30 = dense.copy()
    nan30[rs.rand(*shape) < 0.3] = np.nan
    infs = nan30.copy()
    u = rs.rand(*shape)
    infs[u < 0.1] = np.inf
    infs[(u >= 0.1) & (u < 0.2)] = -np.inf
    wide = (dense * 3 - D).astype(np.float32)                              # -D .. 2 D
    wide[rs.rand(*shape) < 0.1] = np.nan
    return {"dense": dense, "nan30": nan30, "all nan": np.full(shape, np.nan, np.float32), "infs": infs, "out of range": wide}


@pytest.mark.parametrize("shape", BAND_SHAPES)
def test_band_window_equals_the_restatement(te, shape):
    rs = np.random.RandomState(sum(shape))
    for D in (1, 64, 128):
        for name, prior in priors(rs, shape, D).items():
            p = dev(prior)
            p0 = p.clone()
            for window in (1, 3, 5, 15):
                for radius in (0.0, 1.0, 2.5):
                    for holes in ("full", "empty"):
                        what = "%s %s D %d window %d radius %g holes %s" % (name, shape, D, window, radius, holes)
                        lo, hi = te.disparity_band_window(p, radius, D, window, holes)
                        assert lo.dtype == torch.int32 and hi.dtype == torch.int32 and lo.shape == p.shape, what
                        want = wr.band_window(prior, radius, D, window, holes)
                        assert np.array_equal(host(lo), want[0]), "%s: %d lo differ" % (what, int((host(lo) != want[0]).sum()))
                        assert np.array_equal(host(hi), want[1]), "%s: %d hi differ" % (what, int((host(hi) != want[1]).sum()))
                        if window == 1 and holes == "empty":
                            equal_runs((lo, hi), te.disparity_band(p, radius, D), what + " against disparity_band")
                        equal_runs((lo, hi), te.disparity_band_window(p, radius, D, window, holes), what)
            unchanged([p], [p0], name)


def test_band_window_radius_edge_cases_and_2d_prior(te):
    rs = np.random.RandomState(3)
    prior = priors(rs, (2, 17, 65), 64)["infs"]
    p = dev(prior)
    for radius in (-1.0, float("nan"), float("-inf"), float("inf"), 1e30):
        for holes in ("full", "empty"):
            lo, hi = te.disparity_band_window(p, radius, 64, 3, holes)
            equal_runs((lo, hi), te.disparity_band_window(p, radius, 64, 3, holes), "radius %r" % radius)
            want = wr.band_window(prior, radius, 64, 3, holes)
            assert np.array_equal(host(lo), want[0]) and np.array_equal(host(hi), want[1]), (radius, holes)
            if not radius >= 0:
                assert bool((lo == 64).all()) and bool((hi == -1).all())
    lo2, hi2 = te.disparity_band_window(p[1], 1.0, 64, 5, "empty")                  # [H,W]
    lo3, hi3 = te.disparity_band_window(p, 1.0, 64, 5, "empty")
    equal_runs((lo2, hi2), te.disparity_band_window(p[1], 1.0, 64, 5, "empty"), "[H,W]")
    assert lo2.shape == (17, 65) and torch.equal(lo2, lo3[1]) and torch.equal(hi2, hi3[1])


# ---------------------------------------------------------------------------------------------------------------------
# the chain: matched views -> warp -> disparity -> band -> band matcher
# ---------------------------------------------------------------------------------------------------------------------
def test_warp_to_band_to_matcher(te):
    """clean 1 x 3 x 33 x 130: views 0, 1 warped into view 2, depth_to_disp, disparity_band_window and costvol_argmin_band
    on a seeded frame and pattern: idx == -1 exactly where the band is empty, lo' <= idx <= hi' elsewhere -- the dtypes
    and layouts of the new ops feed the band matcher as they are"""
    B, V, H, W, D, bf = 1, 3, 33, 130, 64, 100.0
    sc = fr.make_scene("clean", B, V, H, W, 5)
    t_in = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t", "valid")]
    sources = torch.tensor([[1, 1, 0]], dtype=torch.bool, device="cuda")
    targets = torch.tensor([[0, 0, 1]], dtype=torch.bool, device="cuda")
    z = te.depth_warp(*t_in, sources=sources, targets=targets, splat=1)
    equal_runs((z,), (te.depth_warp(*t_in, sources=sources, targets=targets, splat=1),), "chain warp")
    disp = te.depth_to_disp(z[:, 2], bf)
    assert disp.is_cuda and disp.dtype == torch.float32 and disp.shape == (B, H, W) and disp.is_contiguous()
    rs = np.random.RandomState(11)
    im, pattern = dev(rs.rand(B, H, W).astype(np.float32)), dev(rs.rand(H, W).astype(np.float32))
    n_empty = {}
    for holes in ("empty", "full"):
        lo, hi = te.disparity_band_window(disp, 1.0, D, 3, holes)
        equal_runs((lo, hi), te.disparity_band_window(disp, 1.0, D, 3, holes), "chain band")
        idx, best = te.costvol_argmin_band(im, pattern, lo, hi, D, 5, "sad")
        equal_runs((idx, best), te.costvol_argmin_band(im, pattern, lo, hi, D, 5, "sad"), "chain matcher")
        lo_c, hi_c = lo.clamp(min=0).long(), hi.clamp(max=D - 1).long()
        empty = lo_c > hi_c
        assert torch.equal(idx == -1, empty) and torch.equal(torch.isnan(best), empty)
        assert bool(((idx >= lo_c) & (idx <= hi_c))[~empty].all())
        n_empty[holes] = int(empty.sum())
    assert n_empty["empty"] > 0 and n_empty["full"] == 0
