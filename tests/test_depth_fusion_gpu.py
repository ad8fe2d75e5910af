"""GPU parity of the multi-view depth consistency check and the point fusion (torchext.depth_consistency /
depth_fuse_points, ctd_depth_consistency_f32 / ctd_depth_fuse_points_f32) against tests/fusion_ref.py: every output
equals the numpy restatement at every element (np.array_equal on the values, the NaN masks and src; no tolerance, no
pixel left out -- the definition uses IEEE add, sub, mul, div, floor and compares only, so a mismatch is an ordering bug
on one of the two sides).  Every call runs twice and the two results must be equal bit for bit."""
import numpy as np
import pytest
import torch

from tests import fusion_ref as fr

pytestmark = pytest.mark.gpu

# (B, V, H, W): the smallest shapes that cross every tile (64 x 4) and compaction (256-pixel workgroups that never cross
# a view; 64-lane ballots) boundary: W = 63, 64, 65, 257, H = 1 and W = 1, more than one track, a single view
SHAPES = [(1, 2, 5, 7), (2, 3, 17, 65), (1, 5, 33, 130), (1, 2, 4, 63), (1, 2, 4, 64), (1, 3, 9, 257), (2, 2, 1, 75),
          (2, 2, 19, 1), (1, 4, 40, 300), (1, 1, 6, 23)]
PARAMS = [(1.0, 0.01, 1), (0.5, 0.002, 2), (0.0, 0.0, 0)]                    # (max_px, max_rel, min_views)


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
    assert np.array_equal(np.signbit(a), np.signbit(b)), "%s: signed zeros differ" % what


def same_maps(got, want, what):
    count, keep, fused = (host(x) for x in got)
    assert count.dtype == np.uint8 and keep.dtype == np.uint8
    assert np.array_equal(count, want[0]), "%s: %d counts differ" % (what, int((count != want[0]).sum()))
    assert np.array_equal(keep, want[1]), "%s: %d keep flags differ" % (what, int((keep != want[1]).sum()))
    same_float(fused, want[2], what + " fused")


def equal_runs(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(bits(x), bits(y)), "%s: two runs differ" % what


def check_scene(te, sc, with_valid, params, what):
    """both ops at one parameter set, dedupe off and on, each twice, against the restatement"""
    max_px, max_rel, min_views = params
    valid = sc["valid"] if with_valid else None
    t_in = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t")] + [dev(valid)]
    before = [None if x is None else x.clone() for x in t_in]
    matches = fr.all_matches(sc["depth"], valid, sc["ray"], sc["K"], sc["R"], sc["t"], max_px, max_rel)
    n_points = {}
    for dedupe in (False, True):
        pts, src, npt, maps = fr.fuse_points(sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], valid, max_px, max_rel,
                                             min_views, dedupe, matches)
        if not dedupe:
            got = te.depth_consistency(*t_in, max_px, max_rel, min_views)
            equal_runs(got, te.depth_consistency(*t_in, max_px, max_rel, min_views), what)
            same_maps(got, maps, what)
        got = te.depth_fuse_points(*t_in, max_px, max_rel, min_views, dedupe, return_maps=True)
        equal_runs(got, te.depth_fuse_points(*t_in, max_px, max_rel, min_views, dedupe, return_maps=True), what)
        w = "%s dedupe %d" % (what, dedupe)
        g_pts, g_src, g_n = host(got[0]), host(got[1]), host(got[2])
        assert g_src.dtype == np.int64 and g_n.dtype == np.int64 and g_pts.ndim == 2 and g_pts.shape[1] == 3
        assert np.array_equal(g_n, npt), "%s: n_per_track %s, expected %s" % (w, g_n, npt)
        assert np.array_equal(g_src, src), "%s: src differs (%d vs %d points)" % (w, len(g_src), len(src))
        same_float(g_pts, pts, w + " points")
        same_maps(got[3:], maps, w + " maps")
        plain = te.depth_fuse_points(*t_in, max_px, max_rel, min_views, dedupe)       # without the maps: the same points
        assert len(plain) == 3
        equal_runs(plain, got[:3], w)
        n_points[dedupe] = len(src)
    for x, x0 in zip(t_in, before):
        assert x is None or torch.equal(bits(x), bits(x0)), "%s: an input was written" % what
    return n_points


@pytest.mark.parametrize("shape", SHAPES)
def test_every_output_equals_the_restatement(te, shape):
    B, V, H, W = shape
    for kind in fr.SCENE_KINDS:
        sc = fr.make_scene(kind, B, V, H, W, 1000 * B + 100 * V + H + W)
        for with_valid in (True, False):
            for params in PARAMS:
                n = check_scene(te, sc, with_valid, params, "%s %s valid %d %s" % (kind, shape, with_valid, params))
                if V == 1 and params[2] > 0:
                    assert n[False] == 0
                if kind == "away" and params[2] > 0:
                    assert n == {False: 0, True: 0}


def test_more_workgroups_than_one_scan_round(te):
    """1 x 3 x 300 x 300: 3 x 352 = 1056 workgroup counts, more than the 1024 the scan workgroup takes at a time"""
    sc = fr.make_scene("noisy", 1, 3, 300, 300, 4)
    n = check_scene(te, sc, True, PARAMS[0], "1 x 3 x 300 x 300")
    assert 0 < n[True] < n[False]


def test_all_dropped_and_shapes_of_the_results(te):
    sc = fr.make_scene("away", 2, 3, 9, 31, 3)
    t_in = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t", "valid")]
    pts, src, n = te.depth_fuse_points(*t_in)
    assert pts.shape == (0, 3) and pts.dtype == torch.float32 and src.shape == (0,) and src.dtype == torch.int64
    assert n.shape == (2,) and n.dtype == torch.int64 and n.tolist() == [0, 0] and pts.is_cuda and n.is_cuda
    count, keep, fused = te.depth_consistency(*t_in)
    assert count.shape == keep.shape == fused.shape == (2, 3, 9, 31)
    assert not count.any() and not keep.any() and bool(torch.isnan(fused).all())
    # a bool mask is taken as it is; tracks are independent of each other
    sc = fr.make_scene("noisy", 2, 3, 17, 65, 8)
    t_in = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t")]
    v8, vb = dev(sc["valid"]), dev(sc["valid"] != 0)
    a = te.depth_fuse_points(*t_in, v8, return_maps=True)
    b = te.depth_fuse_points(*t_in, vb, return_maps=True)
    equal_runs(a, b, "bool valid")
    n0 = int(a[2][0])
    for tr in range(2):
        one = te.depth_fuse_points(t_in[0][tr:tr + 1].contiguous(), t_in[1], t_in[2], t_in[3][tr:tr + 1].contiguous(),
                                   t_in[4][tr:tr + 1].contiguous(), v8[tr:tr + 1].contiguous())
        sl = slice(0, n0) if tr == 0 else slice(n0, None)
        assert torch.equal(bits(one[0]), bits(a[0][sl])) and torch.equal(one[1] + tr * 3 * 17 * 65, a[1][sl])
        assert int(one[2][0]) == int(a[2][tr])


def test_garbage_in_outputs_and_workspace_changes_nothing(te):
    """C ABI: outputs and workspace pre-filled with garbage give the same results; the entries of points and src from M
    on are left alone; NULL maps are allowed"""
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    B, V, H, W = 2, 3, 17, 65
    n = B * V * H * W
    sc = fr.make_scene("noisy", B, V, H, W, 12)
    depth, ray, K, R, t, valid = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t", "valid")]
    want = te.depth_fuse_points(depth, ray, K, R, t, valid, return_maps=True)
    M = want[0].shape[0]
    assert 0 < M < n
    need = L.ctd_depth_fuse_workspace_bytes(B, V, H, W)
    stream = torch.cuda.current_stream().cuda_stream
    for fill in (0x7F, 0xFF, 0x01):
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        pts = torch.full((n, 3), 123.0, dtype=torch.float32, device="cuda")
        src = torch.full((n,), -5, dtype=torch.int64, device="cuda")
        npt = torch.full((B,), -9, dtype=torch.int64, device="cuda")
        maps = [torch.full((B, V, H, W), fill, dtype=torch.uint8, device="cuda") for _ in range(2)]
        fused = torch.full((B, V, H, W), 7.0, dtype=torch.float32, device="cuda")
        for with_maps in (True, False):
            mp = [maps[0].data_ptr(), maps[1].data_ptr(), fused.data_ptr()] if with_maps else [None] * 3
            st = L.ctd_depth_fuse_points_f32(depth.data_ptr(), valid.data_ptr(), ray.data_ptr(), K.data_ptr(), R.data_ptr(),
                                             t.data_ptr(), 1.0, 0.01, 1, 1, pts.data_ptr(), src.data_ptr(), npt.data_ptr(),
                                             mp[0], mp[1], mp[2], B, V, H, W, ws.data_ptr(), need, 0, stream)
            torch.cuda.synchronize()
            assert st == 0
            assert torch.equal(bits(pts[:M]), bits(want[0])) and torch.equal(src[:M], want[1]) and torch.equal(npt, want[2])
            assert bool((pts[M:] == 123.0).all()) and bool((src[M:] == -5).all())
        equal_runs((maps[0], maps[1], fused), want[3:], "maps into filled outputs")
    st = L.ctd_depth_fuse_points_f32(depth.data_ptr(), valid.data_ptr(), ray.data_ptr(), K.data_ptr(), R.data_ptr(),
                                     t.data_ptr(), 1.0, 0.01, 1, 1, pts.data_ptr(), src.data_ptr(), npt.data_ptr(), None, None,
                                     None, B, V, H, W, ws.data_ptr(), need - 1, 0, stream)
    assert st == 2                                                           # CTD_ERR_WORKSPACE


def test_argument_errors(te):
    sc = fr.make_scene("clean", 2, 3, 9, 20, 0)
    depth, ray, K, R, t, valid = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t", "valid")]
    for fn in (te.depth_consistency, te.depth_fuse_points):
        fn(depth, ray, K, R, t, valid)
        fn(depth, ray, K, R, t)
        for bad in (dict(max_px=-1.0), dict(max_px=float("nan")), dict(max_px=float("inf")), dict(max_rel=-0.1),
                    dict(max_rel=float("inf")), dict(max_rel=float("nan")), dict(min_views=-1), dict(min_views=256),
                    dict(min_views=1.5)):
            with pytest.raises(RuntimeError):
                fn(depth, ray, K, R, t, valid, **bad)
        bad_args = [
            (depth.cpu(), ray.cpu(), K.cpu(), R.cpu(), t.cpu(), valid.cpu()),              # CPU tensors
            (depth, ray.cpu(), K, R, t, valid), (depth, ray, K, R, t, valid.cpu()),
            (depth.double(), ray, K, R, t, valid), (depth, ray, K.double(), R, t, valid),    # dtypes
            (depth, ray, K, R, t, valid.to(torch.int32)),
            (depth.transpose(2, 3), ray, K, R, t, None),                                     # not contiguous
            (depth, ray, K, R.transpose(2, 3), t, valid),
            (depth, ray, K, R, t, valid.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)),
            (depth[0], ray, K, R, t, None),                                                  # [V,H,W]
            (depth, ray[:-1].contiguous(), K, R, t, valid), (depth, ray, K[:2].contiguous(), R, t, valid),   # sizes
            (depth, ray, K, R[:1].contiguous(), t, valid), (depth, ray, K, R, t[:, :2].contiguous(), valid),
            (depth, ray, K, R, t, valid[:, :, :, :19].contiguous()), (depth, ray, K, R, t, valid[0]),
            (torch.empty(1, 2, 0, 5, device="cuda"), ray, K, R, t, None),
            (torch.empty(1, 65, 1, 1, device="cuda"), torch.ones(1, 3, device="cuda"), K,
             torch.zeros(1, 65, 3, 3, device="cuda"), torch.zeros(1, 65, 3, device="cuda"), None),   # more than 64 views
        ]
        for a in bad_args:
            with pytest.raises(RuntimeError):
                fn(*a)
    # no tracks at all: empty results, no launch
    e = te.depth_fuse_points(torch.empty(0, 3, 9, 20, device="cuda"), ray, K, torch.empty(0, 3, 3, 3, device="cuda"),
                             torch.empty(0, 3, 3, device="cuda"))
    assert e[0].shape == (0, 3) and e[1].shape == (0,) and e[2].shape == (0,)


def test_abi_errors_need_no_device():
    """through _lib with NULL / fake pointers and device -1: the invalid-argument, unsupported and workspace codes come
    back without a device being touched (the same checks run on machines without a GPU)"""
    from tests.test_depth_fusion_host import check_abi_errors
    check_abi_errors()


def test_timing_tool_report_at_a_small_shape():
    """tools/time_depth_fusion.py's report, in process, one repetition at 1 x 2 x 17 x 65 (the tool itself times 4 views of
    640 x 480)"""
    from tests.test_depth_fusion_host import timing_tool
    text = timing_tool().report((1, 2, 17, 65), 1)
    assert "depth_fuse_points dedupe on" in text and "fuse_scatter_kernel" in text and "NOT MEASURED" in text
