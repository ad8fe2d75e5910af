"""CPU-only checks of the depth-map normals and the point-to-plane ICP (include/ctd_hip_icp.h: ctd_depth_normals_f32,
ctd_depth_icp_system_f32, ctd_depth_icp_update_f32; torchext.depth_normals, depth_icp_system, depth_icp_update,
depth_icp): the rules' sentences (the header against its ctypes table and the built library: tests/test_abi_and_host.py),
argument validation before any HIP call and its precedence, the workspace query, the Python surface, and the restatement tests/icp_ref.py
against the truth of its corner scene: normals, convergence from perturbed poses, what the consistency check says
before and after, and the two degenerate scenes.

Measured on the restatement (corner scene of tests/icp_ref.py, B=2, V=3, 48 x 80, seeds 5 / 6 / 7; the tests run seed 5
and pin 2 x its values):
  normals      every pixel whose five stencil pixels lie on one plane (88 % of the pixels) has a normal; the largest
               angle to the true normal is 4.16e-4 / 3.97e-4 / 3.95e-4 degrees (f32 rounding of the depths: a stencil is
               two pixels wide, the depth is good to 2^-24, and 2^-24 * 2.5 / (2 * 2.5 / 96) is 2.9e-6 rad = 1.6e-4 degrees
               per difference).  Pinned at 2 x 4.16e-4 = 8.32e-4 degrees.
  convergence  views 1 and 2 start 1 degree / 1 cm and 2 degrees / 3 cm from the truth (translation errors 0.0099 and
               0.0299 at seed 5).  After 6 rounds (3 are enough, the rest move the last digits): translation error at
               most 8.82e-5 / 1.12e-4 / 1.53e-4, rotation error at most 3.96e-3 / 4.50e-3 / 7.14e-3 degrees, the largest
               ratio of final to initial translation error 0.0089 / 0.0115 / 0.0079 (the bound is 1/20).  What is left
               is the bias of the pixels on the creases, whose normals blend two planes.  Pinned at 2 x 8.82e-5 = 1.764e-4
               and 2 x 3.96e-3 = 7.92e-3 degrees.
  consistency  keep of the consistency rule at max_px 1, max_rel 0.002 as a share of all pixels: 0.9636 at the true
               poses, 0.2813 at the perturbed ones, 0.9636 at the refined ones (seeds 6, 7: 0.9635 / 0.1559 / 0.9635 and
               0.9526 / 0.1807 / 0.9524).
  pivots       the smallest pivot ratio D_j / A_jj over all rounds and views: corner 0.139 / 0.112 / 0.113 (condition
               numbers of A at the true poses 260 .. 348); the single slanted plane of fusion_ref ("plane") 2.8e-10 /
               2.1e-10 / 1.8e-10, at the true poses and at perturbed ones alike; the nearly planar tracks of
               tests/chain_scene.py at their true poses (depth = the float64 truth cast to f32, views 1..3 of both
               tracks against view 0) 2.5e-2, 2.0e-8, 4.1e-2 and 2.6e-8, 2.2e-2, 1.7e-5: three of the six are refused
               at 1e-4, which is why those tracks carry no convergence assertion.
               The default min_pivot = 1e-4 separates the corner from the plane by three orders of magnitude on the
               corner's side and five on the plane's.
"""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

from tests import fusion_ref as fr
from tests import icp_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ICP_HEADER = os.path.join(ROOT, "include", "ctd_hip_icp.h")

OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, 1, 2, 3
NAN = float("nan")

# pinned at 2 x the values measured on the restatement (module docstring); tests/test_depth_icp_gpu.py uses the same
MAX_NORMAL_ANGLE_DEG = 2 * 4.16e-4
MAX_FINAL_T_ERR = 2 * 8.82e-5
MAX_FINAL_ROT_ERR_DEG = 2 * 3.96e-3
CORNER_SHAPE, CORNER_SEED, CORNER_ITERS = (2, 3, 48, 80), 5, 6


@pytest.fixture(scope="module")
def L():
    from connecting_the_dots_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header (header == table == exports: tests/test_abi_and_host.py, for every header)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_rules():
    text = " ".join(open(ICP_HEADER).read().replace("*", " ").split())
    for phrase in ("1 <= x <= W-2 and 1 <= y <= H-2",
                   "Every neighbour satisfies |d_nb - d| <= max_rel d",
                   "a = P(y,x+1) - P(y,x-1) and b = P(y+1,x) - P(y-1,x)",
                   "The pixel gets no normal unless l > 0 and l < inf",
                   "Every other pixel gets three NaNs",
                   "A value outside 0..V-1, or equal to s, skips the view",
                   "The pixel is dropped unless uvd2 > 0",
                   "J = (S x n, n)",
                   "Each product is formed in f64 from its two f32 factors and is therefore exact",
                   "thread i sums the pixels i, i + 256, i + 512, i + 768 of the chunk, ascending",
                   "A second pass sums a view's workgroups ascending. No atomics",
                   "any pivot D_j <= min_pivot A_jj, with A_jj the undamped diagonal entry",
                   "Unchanged means R_out = R and t_out = t bit for bit, with ok = 0",
                   "[R_a|t_a] [R_s'|t_s']^-1 = [Rr|tr] [R_a|t_a] [R_s|t_s]^-1",
                   "rounded to f32 once, at the end, and ok = 1"):
        assert phrase in text, phrase


# ---------------------------------------------------------------------------------------------------------------------
# 2. validation
# ---------------------------------------------------------------------------------------------------------------------
class _Bufs:
    """host buffers standing in for device pointers, 4 KiB apart and 256-byte aligned: validation must reject before any
    of them is ever dereferenced"""

    def __init__(self, names, slot=4096):
        self.raw = ctypes.create_string_buffer(slot * (len(names) + 1))
        base = (ctypes.addressof(self.raw) + 255) // 256 * 256
        self.ptr = {n: base + i * slot for i, n in enumerate(names)}


B, V, H, W = 2, 3, 4, 5                                           # 120 pixels: every buffer fits a 4 KiB slot
BIG_ALL = dict(B=1 << 11, V=1, H=1 << 10, W=1 << 10)              # B * V * H * W = 2^31
BIG_SIDE = dict(B=1, V=1, H=(1 << 24) + 1, W=1)                   # H > 2^24


def test_normals_rejections_need_no_gpu(L):
    bufs = _Bufs(["depth", "valid", "ray", "normal"])

    def call(max_rel=0.02, B=B, V=V, H=H, W=W, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_depth_normals_f32(p["depth"], p["valid"], p["ray"], max_rel, p["normal"], B, V, H, W, -1, None)

    for kw in (dict(V=0), dict(H=0), dict(W=-2), dict(B=-1), dict(V=65, H=1, W=1), dict(max_rel=-0.5), dict(max_rel=NAN),
               dict(max_rel=-math.inf), dict(depth=None), dict(ray=None), dict(normal=None)):
        assert call(**kw) == INVALID_ARG, kw
    assert call(**BIG_ALL) == UNSUPPORTED
    assert call(**BIG_SIDE) == UNSUPPORTED
    assert call(B=1 << 18, V=64, H=1, W=1) == UNSUPPORTED              # 2^24 views of one tile each
    assert call(normal=bufs.ptr["depth"]) == INVALID_ARG             # the output over an input
    assert call(normal=bufs.ptr["depth"] + 4 * B * V * H * W - 4) == INVALID_ARG
    assert call(normal=bufs.ptr["ray"] + 8) == INVALID_ARG
    assert call(normal=bufs.ptr["valid"]) == INVALID_ARG
    # precedence: INVALID_ARG, then UNSUPPORTED, then the overlaps
    assert call(max_rel=NAN, **BIG_ALL) == INVALID_ARG
    assert call(normal=None, **BIG_ALL) == INVALID_ARG
    assert call(normal=bufs.ptr["depth"], **BIG_ALL) == UNSUPPORTED
    # valid may be NULL; no tracks: nothing to do, nothing touched
    assert call(B=0) == OK
    assert call(B=0, valid=None, max_rel=math.inf) == OK
    assert call(B=0, max_rel=-1.0) == INVALID_ARG
    assert call(B=0, depth=None) == INVALID_ARG


def test_system_rejections_need_no_gpu(L):
    nws = L.ctd_depth_icp_workspace_bytes(B, V, H, W)
    assert 29 * 8 * B * V == 1392 and nws == 1536                     # one workgroup per view, 29 f64 each, rounded up to 256
    names = ["depth", "valid", "normal", "ray", "K", "R", "t", "target", "system", "residual", "assoc", "ws"]
    bufs = _Bufs(names)

    def call(max_dist=0.1, B=B, V=V, H=H, W=W, nbytes=None, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_depth_icp_system_f32(p["depth"], p["valid"], p["normal"], p["ray"], p["K"], p["R"], p["t"], p["target"],
                                          max_dist, p["system"], p["residual"], p["assoc"], B, V, H, W, p["ws"],
                                          nws if nbytes is None else nbytes, -1, None)

    required = ("depth", "normal", "ray", "K", "R", "t", "system")
    for kw in (dict(V=0), dict(H=0), dict(W=-2), dict(B=-1), dict(V=65, H=1, W=1), dict(max_dist=-0.5), dict(max_dist=NAN)):
        assert call(**kw) == INVALID_ARG, kw
    for k in required:
        assert call(**{k: None}) == INVALID_ARG, k
    assert call(**BIG_ALL) == UNSUPPORTED
    assert call(**BIG_SIDE) == UNSUPPORTED
    assert call(B=1 << 18, V=64, H=1, W=1) == UNSUPPORTED               # 2^24 workgroups
    for out in ("system", "residual", "assoc", "ws"):
        for other in names:
            if other != out:
                assert call(**{out: bufs.ptr[other]}) == INVALID_ARG, (out, other)
    assert call(system=bufs.ptr["K"] + 32) == INVALID_ARG
    assert call(ws=None) == WORKSPACE                                   # workspace missing, short, misaligned
    assert call(nbytes=nws - 1) == WORKSPACE
    assert call(nbytes=0) == WORKSPACE
    assert call(ws=bufs.ptr["ws"] + 8) == WORKSPACE
    # precedence: INVALID_ARG, then UNSUPPORTED, then the overlaps, then WORKSPACE
    assert call(ws=None, **BIG_ALL) == UNSUPPORTED
    assert call(ws=None, max_dist=NAN, **BIG_ALL) == INVALID_ARG
    assert call(ws=None, system=None, **BIG_ALL) == INVALID_ARG
    assert call(ws=None, residual=bufs.ptr["depth"]) == INVALID_ARG
    assert call(ws=None, V=65) == INVALID_ARG
    # what may be NULL: valid, target, residual and assoc never turn a call down (the workspace does, behind them)
    assert call(valid=None, target=None, residual=None, assoc=None, nbytes=0) == WORKSPACE
    # no tracks: nothing to do, nothing touched, no workspace needed
    assert call(B=0, ws=None, nbytes=0) == OK
    assert call(B=0, ws=None, nbytes=0, valid=None, target=None, residual=None, assoc=None, max_dist=math.inf) == OK
    assert call(B=0, ws=None, nbytes=0, max_dist=-1.0) == INVALID_ARG
    assert call(B=0, ws=None, nbytes=0, depth=None) == INVALID_ARG


def test_icp_workspace_query(L):
    for b, v, h, w in [(4, 4, 432, 512), (1, 2, 5, 7), (2, 3, 48, 80), (1, 4, 33, 130), (1, 1, 1, 1), (1, 64, 3, 3),
                       (3, 5, 1, 1024), (3, 5, 1, 1025)]:
        chunks = (h * w + 1023) // 1024
        assert L.ctd_depth_icp_workspace_bytes(b, v, h, w) == (29 * 8 * b * v * chunks + 255) // 256 * 256 > 0
    for args in ((0, 4, 432, 512), (-1, 4, 432, 512), (1, 0, 432, 512), (1, 4, 0, 512), (1, 4, 432, 0), (1, 4, -3, 512),
                 (1, 65, 4, 4), (1 << 11, 1, 1 << 10, 1 << 10), (1, 1, (1 << 24) + 1, 1), (1 << 18, 64, 1, 1)):
        assert L.ctd_depth_icp_workspace_bytes(*args) == 0, args


def test_update_rejections_need_no_gpu(L):
    names = ["system", "R", "t", "target", "R_out", "t_out", "ok"]
    bufs = _Bufs(names)

    def call(min_count=64, min_pivot=1e-4, damping=0.0, B=B, V=V, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_depth_icp_update_f32(p["system"], p["R"], p["t"], p["target"], min_count, min_pivot, damping, p["R_out"],
                                          p["t_out"], p["ok"], B, V, -1, None)

    for kw in (dict(V=0), dict(B=-1), dict(V=65), dict(min_count=-1), dict(min_pivot=-1e-9), dict(min_pivot=NAN),
               dict(damping=-0.5), dict(damping=NAN)):
        assert call(**kw) == INVALID_ARG, kw
    for k in names:
        if k != "target":
            assert call(**{k: None}) == INVALID_ARG, k
    assert call(B=1 << 18, V=64) == UNSUPPORTED
    for out in ("R_out", "t_out", "ok"):
        for other in names:
            if other != out:
                assert call(**{out: bufs.ptr[other]}) == INVALID_ARG, (out, other)
    assert call(R_out=bufs.ptr["R"]) == INVALID_ARG                     # not in place
    # precedence
    assert call(B=1 << 18, V=64, damping=NAN) == INVALID_ARG
    assert call(B=1 << 18, V=64, ok=None) == INVALID_ARG
    assert call(B=1 << 18, V=64, R_out=bufs.ptr["R"]) == UNSUPPORTED
    assert call(B=0) == OK
    assert call(B=0, target=None, min_count=0, min_pivot=0.0, damping=math.inf) == OK
    assert call(B=0, min_count=-1) == INVALID_ARG
    assert call(B=0, R=None) == INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------
# 3. the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def test_python_signatures_and_docstrings(te):
    def params(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    assert params(te.depth_normals) == [("depth", E), ("ray", E), ("valid", None), ("max_rel", 0.02)]
    assert params(te.depth_icp_system) == [("depth", E), ("normal", E), ("ray", E), ("K", E), ("R", E), ("t", E),
                                           ("valid", None), ("target", None), ("max_dist", 0.1), ("return_maps", False)]
    assert params(te.depth_icp_update) == [("system", E), ("R", E), ("t", E), ("target", None), ("min_count", 64),
                                           ("min_pivot", 1e-4), ("damping", 0.0)]
    assert params(te.depth_icp)[:8] == [("depth", E), ("ray", E), ("K", E), ("R", E), ("t", E), ("valid", None),
                                        ("target", None), ("iters", 10)]
    assert dict(params(te.depth_icp)[8:]) == dict(max_rel=0.02, max_dist=0.1, min_count=64, min_pivot=1e-4, damping=0.0)
    assert "negated when n . P(y,x) > 0" in te.depth_normals.__doc__ and "three NaNs" in te.depth_normals.__doc__
    for fn in (te.depth_icp_system, te.depth_icp_update, te.depth_icp):
        assert "J = (S x n, n)" in fn.__doc__ and "<= min_pivot * A_ii" in fn.__doc__, fn.__name__
        assert "the same bits on every run" in fn.__doc__
    assert "without any host synchronisation" in te.depth_icp.__doc__
    assert "single plane" in te.depth_icp.__doc__


def test_python_surface_errors(te):
    sc = fr.make_scene("clean", 2, 3, 4, 5, 0)
    depth, ray, K, R, t, valid = [torch.from_numpy(sc[k]) for k in ("depth", "ray", "K", "R", "t", "valid")]
    normal = torch.zeros(2, 3, 4, 5, 3)
    system = torch.zeros(2, 3, 29, dtype=torch.float64)
    target = torch.zeros(2, 3, dtype=torch.int32)
    # the numbers, before any tensor is looked at
    for bad in (-1.0, NAN, math.inf, "1", None, True):
        with pytest.raises(RuntimeError, match="max_rel must be a finite number >= 0"):
            te.depth_normals(depth, ray, max_rel=bad)
        with pytest.raises(RuntimeError, match="max_dist must be a finite number >= 0"):
            te.depth_icp_system(depth, normal, ray, K, R, t, max_dist=bad)
        with pytest.raises(RuntimeError, match="min_pivot must be a finite number >= 0"):
            te.depth_icp_update(system, R, t, min_pivot=bad)
        with pytest.raises(RuntimeError, match="damping must be a finite number >= 0"):
            te.depth_icp(depth, ray, K, R, t, damping=bad)
    for bad in (-1, 1.5, 64.0, "1", None, True):
        with pytest.raises(RuntimeError, match="min_count must be an integer >= 0"):
            te.depth_icp_update(system, R, t, min_count=bad)
    for bad in (0, -1, 2.0, None, True):
        with pytest.raises(RuntimeError, match="iters must be an integer >= 1"):
            te.depth_icp(depth, ray, K, R, t, iters=bad)
    # dtype, shape, device (no CPU path: well-formed CPU tensors raise too)
    for args in ((depth.double(), ray), (depth, ray.double()), (depth[0], ray), (depth, ray[:-1]), (depth.numpy(), ray),
                 (depth, ray, valid.float()), (depth, ray, valid[0]), (depth, ray), (depth, ray, valid)):
        with pytest.raises(RuntimeError):
            te.depth_normals(*args)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        te.depth_normals(depth, ray)
    for args in ((depth, normal.double(), ray, K, R, t), (depth, normal, ray, K[:2], R, t), (depth, normal, ray, K, R[:1], t),
                 (depth, normal, ray, K, R, t)):
        with pytest.raises(RuntimeError):
            te.depth_icp_system(*args)
    for args in ((system.float(), R, t), (system, R, t), (system, R.double(), t)):
        with pytest.raises(RuntimeError):
            te.depth_icp_update(*args)
    # depth_icp sizes the update by R and t: the element count alone is not enough, also where the other track ops take it
    for bad_R, bad_t in ((R.reshape(6, 3, 3), t), (R.reshape(18, 3), t), (R.reshape(2, 3, 9), t), (R, t.reshape(6, 3)),
                         (R, t.reshape(-1)), (R[:1], t[:1]), (R.numpy(), t)):
        with pytest.raises(RuntimeError, match=r"R must be shaped \[B,V,3,3\] and t \[B,V,3\]"):
            te.depth_icp(depth, ray, K, bad_R, bad_t)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        te.depth_icp(depth, ray, K, R, t)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        te.depth_icp(depth, ray, K, R, t, valid=valid, target=target, iters=2)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the restatement against the truth of the corner scene
# ---------------------------------------------------------------------------------------------------------------------
def stencils_on_one_plane(plane):
    """bool [B,V,H,W]: the pixel is interior and it and its four axis neighbours carry one plane id"""
    same = np.zeros(plane.shape, bool)
    c = plane[:, :, 1:-1, 1:-1]
    same[:, :, 1:-1, 1:-1] = ((c == plane[:, :, 1:-1, 2:]) & (c == plane[:, :, 1:-1, :-2]) & (c == plane[:, :, 2:, 1:-1]) &
                              (c == plane[:, :, :-2, 1:-1]))
    return same


def normal_angles_deg(normal, truth):
    n = normal.astype(np.float64)
    return np.rad2deg(np.arctan2(np.linalg.norm(np.cross(n, truth), axis=-1), (n * truth).sum(-1)))


@pytest.fixture(scope="module")
def corner():
    """the corner scene and the restatement's run on it, computed once and read only"""
    sc = ir.make_corner(*CORNER_SHAPE, CORNER_SEED)
    sc["run"] = ir.depth_icp(sc["depth"], sc["ray"], sc["K"], sc["R0"], sc["t0"], sc["valid"], iters=CORNER_ITERS)
    return sc


def test_normals_of_the_restatement_against_the_truth(corner):
    """largest angle to the true normal over the pixels whose five stencil pixels share a plane: measured 4.16e-4
    degrees (seeds 6, 7: 3.97e-4, 3.95e-4), pinned at 8.32e-4"""
    normal = ir.normals(corner["depth"], corner["ray"], corner["valid"])
    assert normal.dtype == np.float32 and normal.shape == corner["depth"].shape + (3,)
    has = np.isfinite(normal).all(-1)
    assert np.array_equal(has, ~np.isnan(normal).any(-1))                  # three NaNs or three finite values
    assert not has[:, :, 0].any() and not has[:, :, -1].any() and not has[:, :, :, 0].any() and not has[:, :, :, -1].any()
    same = stencils_on_one_plane(corner["plane"])
    assert same.mean() > 0.85 and len(np.unique(corner["plane"][same])) == 3
    assert has[same].all()
    ang = normal_angles_deg(normal, corner["normal_true"])[same]
    print("largest angle to the true normal: %.3e degrees over %d pixels" % (ang.max(), ang.size))
    assert ang.max() <= MAX_NORMAL_ANGLE_DEG
    n64 = normal[has].astype(np.float64)
    assert np.abs(np.linalg.norm(n64, axis=-1) - 1).max() < 3e-7           # unit length to f32 rounding
    P = (corner["depth"][..., None] * corner["ray"].reshape(CORNER_SHAPE[2], CORNER_SHAPE[3], 3))[has]
    assert ((n64 * P).sum(-1) < 0).all()                                   # facing the camera
    # a hole takes the normals of its four neighbours with it, and max_rel = 0 leaves none on a slanted surface
    depth = corner["depth"].copy()
    depth[0, 1, 20, 30] = np.nan
    holed = np.isfinite(ir.normals(depth, corner["ray"], None)).all(-1)
    gone = has & ~holed
    assert sorted(map(tuple, np.argwhere(gone))) == [(0, 1, 19, 30), (0, 1, 20, 29), (0, 1, 20, 30), (0, 1, 20, 31), (0, 1, 21, 30)]
    assert not np.isfinite(ir.normals(corner["depth"], corner["ray"], None, max_rel=0.0)).any()
    valid = corner["valid"].copy()
    valid[1, 2, 5, 5] = 0
    assert (has & ~np.isfinite(ir.normals(corner["depth"], corner["ray"], valid)).all(-1)).sum() == 5


def test_the_restatement_converges_on_the_corner_scene(corner):
    """B=2, V=3, 48 x 80, views 1 and 2 perturbed by 1 degree / 1 cm and 2 degrees / 3 cm, 6 rounds.  Measured: final
    translation error at most 8.82e-5 (from 0.0099 and 0.0299; ratio at most 0.0089), final rotation error at most
    3.96e-3 degrees; pinned at 1.764e-4 and 7.92e-3 degrees.  Smallest pivot ratio 0.139."""
    R, t, info = corner["run"]
    rot0, tr0 = ir.pose_errors(corner["R0"], corner["t0"], corner["R"], corner["t"])
    rot1, tr1 = ir.pose_errors(R, t, corner["R"], corner["t"])
    assert np.allclose(rot0[:, 1], 1.0, atol=1e-5) and np.allclose(rot0[:, 2], 2.0, atol=1e-5) and (rot0[:, 0] == 0).all()
    assert (np.abs(tr0[:, 1] - 0.01) < 1.5e-3).all() and (np.abs(tr0[:, 2] - 0.03) < 2e-3).all()
    print("translation error %s -> %s, rotation error (degrees) %s -> %s, smallest pivot ratio %.3e" % (
        tr0[:, 1:].ravel(), tr1[:, 1:].ravel(), rot0[:, 1:].ravel(), rot1[:, 1:].ravel(), np.nanmin(info["pivot_ratio"])))
    assert info["ok"].tolist() == [[0, 1, 1], [0, 1, 1]]                   # view 0 is the target: skipped
    assert np.array_equal(R[:, 0], corner["R0"][:, 0]) and np.array_equal(t[:, 0], corner["t0"][:, 0])
    assert (tr1[:, 1:] <= tr0[:, 1:] / 20).all()
    assert tr1.max() <= MAX_FINAL_T_ERR and rot1.max() <= MAX_FINAL_ROT_ERR_DEG
    # three rounds are enough; the count and the rmse say so without the truth
    rot3, tr3 = ir.pose_errors(info["R_steps"][2], info["t_steps"][2], corner["R"], corner["t"])
    assert tr3.max() <= MAX_FINAL_T_ERR and rot3.max() <= MAX_FINAL_ROT_ERR_DEG
    assert (info["count"][:, :, 0] == 0).all() and (info["count"][:, :, 1:] > 3000).all()
    assert (info["rmse"][0, :, 1:] > 3e-3).all() and (info["rmse"][-1, :, 1:] < 5e-4).all()
    assert np.nanmin(info["pivot_ratio"]) > 0.05                           # three orders above min_pivot = 1e-4


def test_the_consistency_check_confirms_the_refined_poses(corner):
    """keep of the consistency rule at max_px 1, max_rel 0.002 as a share of all pixels.  Measured: 0.9636 at the true
    poses, 0.2813 at the perturbed ones, 0.9636 at the refined ones"""
    R, t, _ = corner["run"]
    args = [corner[k] for k in ("depth", "ray", "K")]
    true, pert, refined = (ir.keep_share(*args, Rx, tx) for Rx, tx in ((corner["R"], corner["t"]), (corner["R0"], corner["t0"]),
                                                                       (R, t)))
    print("keep share: true poses %.4f, perturbed %.4f, refined %.4f" % (true, pert, refined))
    assert true > 0.9 and pert < 0.4 * true
    assert refined >= 0.9 * true


def test_targets_other_than_view_0(corner):
    """views 0 and 1 aligned to view 2 (which is perturbed): they end where view 2 sees them, i.e. their pose relative
    to view 2 is the true one; entries that are out of range or the view itself skip"""
    target = np.array([[2, 2, 2], [-1, 1, 7]], np.int32)
    sc = corner
    R, t, info = ir.depth_icp(sc["depth"], sc["ray"], sc["K"], sc["R0"], sc["t0"], sc["valid"], target=target, iters=4)
    assert info["ok"].tolist() == [[1, 1, 0], [0, 0, 0]]
    assert np.array_equal(R[1], sc["R0"][1]) and np.array_equal(t[1], sc["t0"][1]) and np.array_equal(R[0, 2], sc["R0"][0, 2])

    def relative(Rx, tx, s, a):                                         # [R_a|t_a] [R_s|t_s]^-1
        Ra, Rs, ta, ts = (x.astype(np.float64) for x in (Rx[0, a], Rx[0, s], tx[0, a], tx[0, s]))
        return Ra @ Rs.T, ta - Ra @ Rs.T @ ts

    for s in (0, 1):
        Rrel, trel = relative(R, t, s, 2)
        Rtrue, ttrue = relative(sc["R"], sc["t"], s, 2)
        rot, tr = ir.pose_errors(Rrel[None, None], trel[None, None], Rtrue[None, None], ttrue[None, None])
        assert tr.max() <= 2 * MAX_FINAL_T_ERR and rot.max() <= 2 * MAX_FINAL_ROT_ERR_DEG, (s, tr, rot)


# ---------------------------------------------------------------------------------------------------------------------
# 5. degenerate scenes, and the update on hand-made systems
# ---------------------------------------------------------------------------------------------------------------------
def test_a_single_plane_leaves_the_poses_alone():
    """fusion_ref's "plane" scene (one slanted plane): three degrees of freedom slide.  Measured smallest pivot ratio
    2.8e-10 (seeds 6, 7: 2.1e-10, 1.8e-10), largest over the views' smallest 3.0e-10: far below min_pivot = 1e-4"""
    Bb, Vv, Hh, Ww = CORNER_SHAPE
    sc = fr.make_scene("plane", Bb, Vv, Hh, Ww, CORNER_SEED)
    R0, t0 = ir.perturb_poses(sc["R"], sc["t"], np.random.RandomState(CORNER_SEED), {1: (1.0, 0.01), 2: (2.0, 0.03)})
    R, t, info = ir.depth_icp(sc["depth"], sc["ray"], sc["K"], R0, t0, sc["valid"], iters=2)
    assert (info["count"][:, :, 1:] > 3000).all()                          # plenty of pixels: it is the pivots that refuse
    assert not info["ok"].any()
    assert np.array_equal(R.view(np.int32), R0.view(np.int32)) and np.array_equal(t.view(np.int32), t0.view(np.int32))
    ratios = info["pivot_ratio"][:, :, 1:]
    print("single plane: smallest pivot ratios between %.3e and %.3e" % (ratios.min(), ratios.max()))
    assert ratios.max() < 1e-6
    # with the pivot test off (min_pivot = 0) the update goes through, which is why the test is there
    system = ir.icp_system(sc["depth"], ir.normals(sc["depth"], sc["ray"]), sc["ray"], sc["K"], R0, t0)[0]
    assert ir.icp_update(system, R0, t0, min_pivot=0.0)[2][:, 1:].all()
    assert not ir.icp_update(system, R0, t0, min_pivot=1e-4)[2].any()
    # and heavy damping makes every pivot large: A_ii + damping * A_ii
    assert ir.icp_update(system, R0, t0, damping=1.0)[2][:, 1:].all()


def test_views_that_see_nothing_of_each_other():
    """fusion_ref's "away" scene: no projection lands, so the count is 0, the system is zero and the poses stay"""
    sc = fr.make_scene("away", 2, 3, 17, 65, 3)
    normal = ir.normals(sc["depth"], sc["ray"], sc["valid"], max_rel=10.0)
    assert np.isfinite(normal).all(-1).mean() > 0.8
    system, residual, assoc = ir.icp_system(sc["depth"], normal, sc["ray"], sc["K"], sc["R"], sc["t"], sc["valid"])
    assert (system == 0).all() and np.isnan(residual).all() and (assoc == -1).all()
    R, t, ok = ir.icp_update(system, sc["R"], sc["t"], min_count=0)        # count 0 passes min_count 0; the pivots are 0
    assert not ok.any() and np.array_equal(R, sc["R"]) and np.array_equal(t, sc["t"])
    R, t, info = ir.depth_icp(sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], sc["valid"], iters=2, max_rel=10.0)
    assert not info["ok"].any() and (info["count"] == 0).all() and np.isnan(info["rmse"]).all()
    assert np.array_equal(R, sc["R"]) and np.array_equal(t, sc["t"])


def test_the_update_on_hand_made_systems():
    """A = I and g = -xi give the motion xi itself: a pure translation moves t by R_s R_a^T (-v) ... checked in the
    simplest frame, all poses the identity, where the new pose of s is [Rr|tr]^-1"""
    eye = np.tile(np.eye(3, dtype=np.float32), (1, 2, 1, 1))
    zero = np.zeros((1, 2, 3), np.float32)
    system = np.zeros((1, 2, 29))
    for k, (i, j) in enumerate(ir.TRIANGLE):
        system[0, 1, k] = 1.0 if i == j else 0.0
    system[0, 1, 28] = 100
    v = np.array([0.25, -0.5, 0.125])
    system[0, 1, 24:27] = -v                                               # xi = -A^-1 g = (0, v)
    R, t, ok = ir.icp_update(system, eye, zero)
    assert ok.tolist() == [[0, 1]] and np.array_equal(R, eye) and np.array_equal(t[0, 1], (-v).astype(np.float32))
    system[0, 1, 24:27] = 0
    system[0, 1, 21:24] = [0.0, 0.0, -math.pi / 2]                         # a quarter turn about z
    R, t, ok = ir.icp_update(system, eye, zero)
    assert ok.tolist() == [[0, 1]] and (t == 0).all()
    assert np.abs(R[0, 1].astype(np.float64) - np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]])).max() < 1e-7   # Rr^T
    system[0, 1, 21:24] = [-3e-5, 0.0, 0.0]                                # omega = (3e-5, 0, 0), below 1e-4: the series
    R, t, ok = ir.icp_update(system, eye, zero)
    assert ok[0, 1] == 1 and R[0, 1, 2, 1] == np.float32(-3e-5) and R[0, 1, 1, 2] == np.float32(3e-5)
    # what leaves a view unchanged: too few pixels, a zero, negative, NaN or inf pivot, a skipped view
    for edit in (lambda s: s.__setitem__((0, 1, 28), 63), lambda s: s.__setitem__((0, 1, 0), 0.0),
                 lambda s: s.__setitem__((0, 1, 20), -1.0), lambda s: s.__setitem__((0, 1, 6), NAN),
                 lambda s: s.__setitem__((0, 1, 11), math.inf), lambda s: s.__setitem__((0, 1, 28), NAN)):
        bad = system.copy()
        edit(bad)
        R, t, ok = ir.icp_update(bad, eye, zero)
        assert not ok.any() and np.array_equal(R, eye) and np.array_equal(t, zero)
    R, t, ok = ir.icp_update(system, eye, zero, target=np.array([[0, 1]], np.int32))
    assert not ok.any()
