"""CPU-only checks of the yardstick of the depth-fusion tests: tests/fusion_ref.py, the numpy restatement of
ctd_depth_consistency_f32 / ctd_depth_fuse_points_f32, must itself behave as a consistency check should before the
kernels are held to it bit for bit (tests/test_depth_fusion_gpu.py).  The argument validation of the C ABI, which
happens before any HIP call, is checked here as well.

Pose ranges.  The scenes of fusion_ref.make_scene use rotations of up to 3 degrees about a random axis and translations of
up to 0.05 per component, with the scene 1.8 .. 2.7 away and a focal length of 1.2 * max(H, W).  With these, on the
noise-free single plane and max_px = 1, max_rel = 0.01, EVERY (pixel, source view) pair whose step-a projection lands
on a live source pixel is counted (measured when this file was written: 5557 of 5557 pairs at 1 x 3 x 24 x 40, 77471 of
77471 at 1 x 5 x 33 x 130, 117462 of 117462 at 1 x 4 x 40 x 300, and all 70 at 1 x 2 x 5 x 7): nearest-neighbour sampling
moves the back-projection by at most half a pixel per axis (du^2 + dv^2 <= 0.5 plus the plane's parallax over that half
pixel), and half a pixel along the plane changes its depth by well under 1 %.
"""
import ctypes

import numpy as np
import pytest

from tests import fusion_ref as fr

PLANE_SHAPES = [(1, 3, 24, 40), (2, 3, 17, 65), (1, 5, 33, 130), (1, 2, 5, 7), (1, 4, 40, 300)]


def args(sc, with_valid=True):
    return (sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], sc["valid"] if with_valid else None)


@pytest.mark.parametrize("shape", PLANE_SHAPES)
def test_every_landed_view_is_counted_on_the_noise_free_plane(shape):
    B, V, H, W = shape
    for seed in range(3):
        sc = fr.make_scene("plane", B, V, H, W, seed)
        matches = fr.all_matches(sc["depth"], None, sc["ray"], sc["K"], sc["R"], sc["t"], 1.0, 0.01)
        landed = sum(int(m["landed"].sum()) for m in matches.values())
        assert landed >= B * V * (V - 1) * H * W // 2, "the views hardly overlap: %d pairs landed" % landed
        for key, m in matches.items():
            assert np.array_equal(m["landed"], m["consistent"]), "%s: %d landed, %d counted" % (
                key, int(m["landed"].sum()), int(m["consistent"].sum()))
        count, keep, fused = fr.consistency(*args(sc), 1.0, 0.01, 1, matches)
        want = np.zeros((B, V, H * W), np.int64)
        for (b, r, s), m in matches.items():
            want[b, r] += m["landed"]
        assert np.array_equal(count.reshape(B, V, -1), want)
        # the fused depth is a mean of depths of one plane at (almost) one place
        kept = keep != 0
        assert np.all(np.abs(fused[kept] - sc["depth"][kept]) <= 0.01 * sc["depth"][kept])


def test_a_planted_outlier_is_dropped():
    B, V, H, W = 1, 3, 24, 40
    sc = fr.make_scene("plane", B, V, H, W, 5)
    base_count, _, _ = fr.consistency(*args(sc))
    y, x = 11, 19
    assert base_count[0, 1, y, x] == V - 1                                 # seen by both other views before
    sc["depth"][0, 1, y, x] *= np.float32(1.3)
    count, keep, fused = fr.consistency(*args(sc))
    assert count[0, 1, y, x] == 0 and keep[0, 1, y, x] == 0 and np.isnan(fused[0, 1, y, x])
    _, src, _, _ = fr.fuse_points(*args(sc), dedupe=False)
    flat = ((0 * V + 1) * H + y) * W + x
    assert flat not in set(src.tolist())
    # and nobody else uses it: the views that land on it do not count view 1 there
    others = fr.all_matches(sc["depth"], sc["valid"], sc["ray"], sc["K"], sc["R"], sc["t"], 1.0, 0.01)
    for r in (0, 2):
        m = others[0, r, 1]
        assert not np.any(m["consistent"] & (m["q"] == y * W + x))


@pytest.mark.parametrize("kind", fr.SCENE_KINDS)
def test_min_views_zero_keeps_exactly_the_live_pixels(kind):
    sc = fr.make_scene(kind, 2, 3, 17, 65, 3)
    for with_valid in (True, False):
        count, keep, fused = fr.consistency(*args(sc, with_valid), 1.0, 0.01, 0)
        live = fr.live_mask(sc["depth"], sc["valid"] if with_valid else None)
        assert np.array_equal(keep != 0, live)
        assert np.all(count[~live] == 0) and np.all(np.isnan(fused[~live]))
        alone = live & (count == 0)
        assert alone.any() and np.array_equal(fused[alone], sc["depth"][alone])
        _, src, n, _ = fr.fuse_points(*args(sc, with_valid), 1.0, 0.01, 0, dedupe=False)
        assert np.array_equal(src, np.nonzero(live.reshape(-1))[0])
    # zero tolerances: (almost) nothing is confirmed, nothing breaks
    count, keep, _ = fr.consistency(*args(sc), 0.0, 0.0, 0)
    assert np.array_equal(keep != 0, fr.live_mask(sc["depth"], sc["valid"]))


def test_one_view_and_views_facing_away_give_no_points():
    sc = fr.make_scene("clean", 1, 1, 6, 23, 0)
    count, keep, _ = fr.consistency(*args(sc))
    assert not count.any() and not keep.any()
    pts, src, n, _ = fr.fuse_points(*args(sc))
    assert pts.shape == (0, 3) and pts.dtype == np.float32 and src.shape == (0,) and n.tolist() == [0]
    for V in (2, 3, 4, 5):
        sc = fr.make_scene("away", 2, V, 9, 31, V)
        assert fr.live_mask(sc["depth"], sc["valid"]).all()
        matches = fr.all_matches(sc["depth"], sc["valid"], sc["ray"], sc["K"], sc["R"], sc["t"], 1.0, 0.01)
        assert not any(m["landed"].any() for m in matches.values()), "a projection landed"
        pts, src, n, (count, keep, _) = fr.fuse_points(*args(sc))
        assert pts.shape == (0, 3) and n.tolist() == [0, 0] and not count.any() and not keep.any()


@pytest.mark.parametrize("kind", ("clean", "noisy"))
def test_dedupe_order_and_counts(kind):
    B, V, H, W = 2, 3, 17, 65
    sc = fr.make_scene(kind, B, V, H, W, 7)
    pts0, src0, n0, (_, keep, _) = fr.fuse_points(*args(sc), dedupe=False)
    pts1, src1, n1, _ = fr.fuse_points(*args(sc), dedupe=True)
    assert 0 < len(src1) < len(src0) == int(keep.sum())                    # the views overlap: duplicates are removed
    assert set(src1.tolist()) <= set(src0.tolist())
    for src, n, pts in ((src0, n0, pts0), (src1, n1, pts1)):
        assert np.all(np.diff(src) > 0)                                     # strictly ascending
        assert int(n.sum()) == len(src) == len(pts)
        track = src // (V * H * W)
        assert np.array_equal(np.bincount(track, minlength=B), n)
    for b in range(B):                                                       # view 0's kept pixels are all emitted
        first = np.nonzero(keep[b, 0].reshape(-1))[0] + b * V * H * W
        assert np.isin(first, src1).all()
    # a pixel that dedupe removed is confirmed by an earlier view that keeps what it lands on
    removed = np.setdiff1d(src0, src1)
    assert np.all((removed // (H * W)) % V > 0)


def test_points_are_the_float64_unprojection_of_fused():
    """point = R_r^T (fused * ray - t_r).  In f32 each P_i = fused*ray_i - t_i carries two roundings, at most
    u (|fused ray_i| + |P_i|) with u = 2^-24, and each point_j three products and two sums, at most 3 u |P_i R_ij| each
    to first order: |error_j| <= u sum_i |R_ij| (|fused ray_i| + 4 |P_i|).  Asserted with a factor 2 for the second-order
    terms."""
    B, V, H, W = 2, 3, 17, 65
    sc = fr.make_scene("noisy", B, V, H, W, 9)
    pts, src, _, (_, _, fused) = fr.fuse_points(*args(sc))
    assert len(src) > 100
    view, p = np.divmod(src, H * W)
    R = sc["R"].reshape(-1, 3, 3).astype(np.float64)[view]
    t = sc["t"].reshape(-1, 3).astype(np.float64)[view]
    f = fused.reshape(-1).astype(np.float64)[src]
    fr_ = f[:, None] * sc["ray"].astype(np.float64)[p]
    P = fr_ - t
    want = np.einsum("ni,nij->nj", P, R)
    bound = 2.0 ** -24 * np.einsum("ni,nij->nj", np.abs(fr_) + 4 * np.abs(P), np.abs(R))
    assert np.all(np.abs(pts - want) <= 2 * bound), "worst excess %g" % float((np.abs(pts - want) / bound).max())
    # and they lie on the scene: within 2 % of one of the two planes (outliers never get here with min_views = 1 ...
    # unless two of them agree, which the 10 % of gross outliers make rare)
    n, c = fr.PLANE
    on_plane = np.abs(want @ n - c) < 0.02 * c
    on_patch = np.abs(want @ fr.PATCH[0] - fr.PATCH[1]) < 0.02 * fr.PATCH[1]
    assert (on_plane | on_patch).mean() > 0.99


def check_abi_errors():
    """The error codes of include/ctd_hip.h, returned before any HIP call: fake pointers, device -1, no stream."""
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    OK, INVALID, WORKSPACE, UNSUPPORTED = 0, 1, 2, 3
    B, V, H, W = 2, 3, 8, 16
    n = B * V * H * W
    MB = 1 << 20                                                            # fake buffers, 1 MiB apart
    depth, valid, ray, K, R, t, count, keep, fused, points, src, npt, ws = [ctypes.c_void_p((i + 1) * 16 * MB)
                                                                            for i in range(13)]

    def cons(depth=depth, valid=valid, ray=ray, K=K, R=R, t=t, max_px=1.0, max_rel=0.01, min_views=1, count=count,
             keep=keep, fused=fused, B=B, V=V, H=H, W=W):
        return L.ctd_depth_consistency_f32(depth, valid, ray, K, R, t, max_px, max_rel, min_views, count, keep, fused, B,
                                           V, H, W, -1, None)

    def fuse(depth=depth, valid=valid, ray=ray, K=K, R=R, t=t, max_px=1.0, max_rel=0.01, min_views=1, dedupe=1,
             points=points, src=src, npt=npt, count=count, keep=keep, fused=fused, B=B, V=V, H=H, W=W, ws=ws,
             ws_bytes=1 << 40):
        return L.ctd_depth_fuse_points_f32(depth, valid, ray, K, R, t, max_px, max_rel, min_views, dedupe, points, src,
                                           npt, count, keep, fused, B, V, H, W, ws, ws_bytes, -1, None)

    inf, nan = float("inf"), float("nan")
    for call in (cons, fuse):
        for bad in (dict(max_px=-1.0), dict(max_px=inf), dict(max_px=nan), dict(max_rel=-0.5), dict(max_rel=inf),
                    dict(max_rel=nan), dict(min_views=-1), dict(min_views=256), dict(B=-1), dict(V=0), dict(V=-3),
                    dict(H=0), dict(W=0), dict(W=(1 << 24) + 1), dict(B=1 << 12, V=64, H=1 << 7, W=1 << 6),
                    dict(depth=None), dict(ray=None), dict(K=None), dict(R=None), dict(t=None),
                    dict(fused=depth), dict(keep=valid), dict(keep=ctypes.c_void_p(depth.value + 4 * n - 1)),
                    dict(count=keep), dict(fused=ctypes.c_void_p(R.value + 8)), dict(count=K)):
            assert call(**bad) == INVALID, (call.__name__, bad)
        assert call(V=65) == UNSUPPORTED
        assert call(V=65, H=0) == INVALID                                   # sizes first
        assert call(B=0) == OK                                              # touches nothing
        assert call(B=0, max_px=-1.0) == INVALID
    for bad in (dict(count=None), dict(keep=None), dict(fused=None)):
        assert cons(**bad) == INVALID
    for bad in (dict(points=None), dict(src=None), dict(npt=None), dict(points=fused), dict(src=points),
                dict(npt=ctypes.c_void_p(src.value + 8)), dict(ws=depth), dict(ws=ctypes.c_void_p(points.value + 256))):
        assert fuse(**bad) == INVALID, bad
    need = L.ctd_depth_fuse_workspace_bytes(B, V, H, W)
    assert need >= 6 * n + 4 * (B * V + 1)                                  # keep, fused, emit flags, workgroup counts
    for bad in (dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=ctypes.c_void_p(ws.value + 64))):
        assert fuse(**bad) == WORKSPACE, bad
    assert fuse(B=0, ws=None, ws_bytes=0) == OK
    for rejected in ((0, V, H, W), (-1, V, H, W), (B, 0, H, W), (B, 65, H, W), (B, V, 0, W), (B, V, H, 0),
                     (1 << 12, 64, 1 << 7, 1 << 6), (1, 1, 1, (1 << 24) + 1)):
        assert L.ctd_depth_fuse_workspace_bytes(*rejected) == 0, rejected
    assert L.ctd_depth_fuse_workspace_bytes(1, 64, 1, 1) > 0
    # 2^24 workgroups and more in one launch (2^32 threads): millions of tiny views
    tiny = dict(B=1 << 18, V=64, H=1, W=1)
    assert cons(**tiny) == UNSUPPORTED and fuse(**tiny) == UNSUPPORTED
    assert L.ctd_depth_fuse_workspace_bytes(1 << 18, 64, 1, 1) == 0
    assert L.ctd_depth_fuse_workspace_bytes((1 << 18) - 1, 64, 1, 1) > 0
    assert L.ctd_version() == 5


def test_abi_errors_come_before_any_device_call():
    check_abi_errors()


def test_python_surface():
    from connecting_the_dots_amd import torchext as te
    import torch
    assert callable(te.depth_consistency) and callable(te.depth_fuse_points)
    sc = fr.make_scene("clean", 1, 2, 5, 7, 0)
    cpu = [torch.from_numpy(a) for a in args(sc)]
    for fn in (te.depth_consistency, te.depth_fuse_points):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            fn(*cpu)


def timing_tool():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "time_depth_fusion.py")
    spec = importlib.util.spec_from_file_location("time_depth_fusion", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_timing_tool_host_parts(tmp_path):
    """what tools/time_depth_fusion.py does without a GPU: the compulsory-bytes table, the parsing of a rocprofv3
    kernel_stats.csv and the report lines built from the two"""
    tool = timing_tool()
    shape = (1, 4, 480, 640)
    n = 4 * 480 * 640
    table = {k: b for k, b, _ in tool.compulsory_bytes(shape, 1000)}
    assert list(table) == ["depth_consistency_kernel", "fuse_count_kernel", "fuse_scan_kernel", "fuse_scatter_kernel"]
    assert table["depth_consistency_kernel"] == 11 * n + 12 * 480 * 640
    assert table["fuse_scan_kernel"] == 8 * 4 * 1200 + 8
    assert table["fuse_scatter_kernel"] == n + 4 * 4800 + 36000
    d = tmp_path / "trace" / "host" / "1"
    d.mkdir(parents=True)
    (d / "7_kernel_stats.csv").write_text(
        '"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n'
        '"void ctd::(anonymous namespace)::depth_consistency_kernel(float const*)",23,230000,10000.0,50.0,9000,12000,1.0\n'
        '"void ctd::(anonymous namespace)::fuse_scan_kernel(int*, int)",23,46000,2000.0,10.0,1900,2100,1.0\n')
    stats = tool.kernel_stats(str(tmp_path / "trace"))
    assert len(stats) == 2 and sorted(v[0] for v in stats.values()) == [23, 23]
    lines = tool.kernel_lines(shape, 1000, stats)
    assert len(lines) == 5 and "NOT MEASURED" not in lines[0]
    assert "avg 10.0 us" in lines[1] and "%.2f TB/s" % (table["depth_consistency_kernel"] / 10.0 / 1e6) in lines[1]
    assert lines[2].rstrip().endswith(": -") and "avg 2.0 us" in lines[3]
    assert "NOT MEASURED" in tool.kernel_lines(shape, 1000, None)[0]


def test_wrapper_rejects_odd_parameters_with_runtime_error(monkeypatch):
    """the parameter checks come after the tensor checks, so they are reached with a fake `depth` only through the
    helper; every bad value raises RuntimeError like the neighbouring ops, never ValueError / TypeError / OverflowError"""
    from connecting_the_dots_amd.torchext import _track, multiview
    import torch

    # the tensor checks that `_depth_fusion_inputs` runs first live in `_track_inputs`: let CPU tensors through them
    monkeypatch.setattr(_track, "_f32", lambda x, n: x)
    monkeypatch.setattr(_track, "_same_device", lambda *ts: torch.device("cpu"))
    sc = fr.make_scene("clean", 1, 2, 5, 7, 0)
    a = [torch.from_numpy(sc[k]) for k in ("depth", "ray", "K", "R", "t")]
    ok = multiview._depth_fusion_inputs(*a, None, 1, np.float32(0.01), np.int64(2), "x")
    assert ok[2:] == (1.0, float(np.float32(0.01)), 2)
    for bad in (dict(min_views=float("nan")), dict(min_views=float("inf")), dict(min_views=None), dict(min_views="1"),
                dict(min_views=1.5), dict(min_views=-1), dict(min_views=256), dict(max_px=None), dict(max_px="1"),
                dict(max_px=float("nan")), dict(max_px=float("inf")), dict(max_px=-1.0), dict(max_rel=None),
                dict(max_rel=float("inf")), dict(max_rel=-0.1)):
        kw = dict(max_px=1.0, max_rel=0.01, min_views=1)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            multiview._depth_fusion_inputs(*a, None, kw["max_px"], kw["max_rel"], kw["min_views"], "x")
