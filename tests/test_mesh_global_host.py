"""CPU checks of the global point-to-mesh registration (include/ext/ctd_hip_mesh_global.h, meshglobal) as
tests/meshglobal_ref.py states it: the header's prototype against meshglobal's table and the library, that the pinned
interface lists did not move, every rejection in the stated order (through the library, no GPU needed: each returns
before any HIP call), the rotation grid, the scoring rule by hand on a 3 x 4 x 5 volume, and the reference pipeline itself
(numpy scoring, tests/meshreg_ref.mesh_icp) on the scene of tests/meshglobal_ref.py, where the plain ICP from the identity
ends more than 100 degrees off.

The thresholds are the project's noisy ones, < 0.1 degrees and < 2e-3 (tests/test_mesh_register_host.py)."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from tests import meshglobal_ref as gr
from tests import meshreg_ref as mr
from tests.abi_headers import parse_header

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "ctd_hip_mesh_global.h")

MAX_ROT_DEG, MAX_T = 0.1, 2e-3                        # the noisy thresholds of tests/test_mesh_register_host.py
FAR_DEG = 30.0                                        # the plain ICP from the identity has to end farther off than this

C_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64}


def test_header_matches_the_module_table_and_the_library():
    from connecting_the_dots_amd import _lib, meshglobal
    functions, structs = parse_header(HEADER)
    assert not structs and list(functions) == list(meshglobal.TABLE) == ["ctd_pose_score_u8"]
    bound = meshglobal.lib()
    assert bound is _lib.lib()
    for name, (ret, params) in functions.items():
        res, args = meshglobal.TABLE[name]
        assert res is C_SCALARS[ret], name
        assert len(args) == len(params), name
        for i, (ctype, declared) in enumerate(zip(args, params)):
            assert (ctype is ctypes.c_void_p) if declared.endswith("*") else (ctype is C_SCALARS[declared]), (name, i)
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype == res, name
    text = open(HEADER).read()
    assert re.findall(r'#\s*include\s*[<"]([^>"]+)[>"]', text) == ["../ctd_hip.h"]
    assert "exact integer" in text and "before any conversion" in text    # what makes the comparison array_equal


def test_the_pinned_interface_did_not_move():
    from connecting_the_dots_amd import _lib, build, meshglobal, meshreg, meshrobust, torchext
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert headers == sorted(_lib.TABLES) and len(headers) == 14
    assert meshglobal.HEADER not in _lib.TABLES and meshglobal.TABLE not in _lib.TABLES.values()
    assert not any(name in table for table in _lib.TABLES.values() for name in meshglobal.TABLE)
    assert not any(name in meshreg.TABLE or name in meshrobust.TABLE for name in meshglobal.TABLE)
    assert len(torchext.functions.__all__) == 65
    assert not any(n in torchext.functions.__all__ for n in (
        "rotation_grid", "offset_grid", "default_box", "distance_levels", "morton_order", "pose_scores", "best_starts",
        "global_mesh_icp", "global_register_mesh", "global_aligned_reconstruction_error"))
    assert HEADER in build._headers()                                   # a stale header rebuilds
    assert _lib.lib().ctd_version() == 5


INVALID = 1


def test_the_entry_point_validates_before_any_hip_call():
    from connecting_the_dots_amd import meshglobal
    L = meshglobal.lib()
    buf = ctypes.create_string_buffer(1 << 17)
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    p = [base + 4096 * i for i in range(20)]                # disjoint 4 KiB host regions: never dereferenced
    nan, inf = float("nan"), float("inf")

    def score(points=p[0], n=10, R=p[1], b=p[2], M=4, offsets=p[3], T=5, levels=p[4], nx=3, ny=4, nz=5, origin=p[5],
              voxel=0.5, out=p[6]):
        return L.ctd_pose_score_u8(points, n, R, b, M, offsets, T, levels, nx, ny, nz, origin, voxel, out, -1, None)

    # each class of error wins over every later one: pair it with a later error and the answer does not change (every
    # answer is INVALID; that no call reaches HIP shows in that none of these host pointers is ever dereferenced)
    classes = [
        [dict(n=-1), dict(n=65537), dict(n=1 << 30)],
        [dict(M=0), dict(M=-1), dict(T=0), dict(T=-3), dict(T=4097), dict(M=1 << 20, T=2048), dict(M=(1 << 31) - 1, T=2)],
        [dict(nx=0), dict(ny=0), dict(nz=0), dict(nx=1025), dict(ny=1025), dict(nz=1025), dict(nx=-1), dict(nz=1 << 30)],
        [dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=nan), dict(voxel=inf), dict(voxel=-inf)],
        [dict(points=None), dict(R=None), dict(b=None), dict(offsets=None), dict(levels=None), dict(origin=None), dict(out=None)],
        [dict(out=p[0]), dict(out=p[1]), dict(out=p[2] + 8), dict(out=p[3] - 8), dict(out=p[4] + 59), dict(out=p[5] - 152),
         dict(out=p[5] + 8)],
    ]
    for i, group in enumerate(classes):
        for bad in group:
            assert score(**bad) == INVALID, bad
            for later in classes[i + 1:]:
                assert score(**{**later[0], **bad}) == INVALID, (bad, later[0])
    # a call that passes every check reaches HIP and is not made here
    # the limits themselves are not rejected by the size checks: a later class answers
    assert score(n=65536, voxel=nan) == INVALID and score(M=(1 << 31) // 4096 - 1, T=4096, voxel=nan) == INVALID
    assert score(nx=1024, ny=1024, nz=1024, out=None) == INVALID
    assert score(n=0, points=None, out=None) == INVALID                 # points may be NULL only without points


def test_the_module_checks_its_arguments_without_a_gpu():
    from connecting_the_dots_amd import meshglobal as mgl
    with pytest.raises(RuntimeError):
        mgl.rotation_grid(0)
    with pytest.raises(RuntimeError):
        mgl.offset_grid(0, 0.1)
    with pytest.raises(RuntimeError):
        mgl.offset_grid(3, -0.1)
    with pytest.raises(RuntimeError):
        mgl.pose_scores(*([None] * 6), 0.1)                             # no CPU path: a tensor that is not CUDA is refused
    assert np.array_equal(mgl.offset_grid(3, 0.1).numpy(), gr.offset_grid(3, 0.1))
    assert mgl.offset_grid(3, 0.1).numpy()[9:18, 0].tolist() == [0.0] * 9 and mgl.offset_grid(3, 0.1)[13].tolist() == [0, 0, 0]
    assert mgl.offset_grid(2, 1.0)[1].tolist() == [-0.5, -0.5, 0.5]     # x slowest
    # the module's grid is the reference's to the last ulp of sin and cos
    assert np.abs(mgl.rotation_grid(1024).numpy().astype(np.float64) - gr.rotation_grid(1024)).max() < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
def nearest_grid_angle(n, samples=2000, seed=0):
    """the angle in degrees from each of `samples` seeded random rotations to its nearest rotation of the grid"""
    rs = np.random.RandomState(seed)
    q = rs.normal(size=(samples, 4))
    x, y, z, w = (q / np.linalg.norm(q, axis=1, keepdims=True)).T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                  2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)
    trace = R @ gr.rotation_grid(n).astype(np.float64).reshape(n, 9).T    # trace(A^T B) is the sum of the products
    return np.degrees(np.arccos(np.clip((trace.max(1) - 1) / 2, -1, 1)))


def test_rotation_grid():
    """Orthonormal with determinant +1 to f32 rounding, no state, and n = 1024 covers SO(3): the largest angle from 2000
    seeded random rotations to their nearest grid rotation is 19.62 degrees (mean 11.80), against 26.74 (14.85) for
    n = 512 and 13.10 (7.76) for n = 4096.  19.62 is inside the basin the scene test relies on (BASIN_DEG = 20: every
    start of the reference runs that began within 30 degrees of the truth ended on it); 26.74 is not, which is why a grid
    of 512 rotations misses on some seeds."""
    for n in (1, 7, 1024):
        R = gr.rotation_grid(n)
        assert R.dtype == F and R.shape == (n, 3, 3)
        R64 = R.astype(np.float64)
        assert np.abs(R64 @ R64.transpose(0, 2, 1) - np.eye(3)).max() < 4e-7
        assert np.abs(np.linalg.det(R64) - 1).max() < 4e-7
        assert np.array_equal(R, gr.rotation_grid(n))
    worst = {n: nearest_grid_angle(n) for n in (512, 1024)}
    print("largest angle to the nearest grid rotation: n = 512: %.2f degrees (mean %.2f), n = 1024: %.2f (mean %.2f)" % (
        worst[512].max(), worst[512].mean(), worst[1024].max(), worst[1024].mean()))
    assert worst[1024].max() < worst[512].max()
    assert worst[1024].max() < gr.BASIN_DEG


def test_the_scoring_rule_by_hand():
    """nx, ny, nz = 3, 4, 5 with levels[z, y, x] = 12 z + 3 y + x, origin (1, -1, 2), voxel 0.5; rotation 0 is the identity,
    rotation 1 turns by 90 degrees about z, (x, y, z) -> (-y + 2, x - 2, z); offset 1 shifts by one voxel along x"""
    levels = np.arange(60, dtype=np.uint8).reshape(5, 4, 3)
    origin, voxel = (1.0, -1.0, 2.0), 0.5
    R = np.array([np.eye(3), [[0, -1, 0], [1, 0, 0], [0, 0, 1]]], F)
    base = np.array([[0, 0, 0], [2, -2, 0]], F)
    offsets = np.array([[0, 0, 0], [0.5, 0, 0]], F)
    nan, inf = np.nan, np.inf
    cases = [                     # the point, then q under (rotation 0: offset 0, offset 1), (rotation 1: offset 0, offset 1)
        ((2, 0.5, 4), 59, 255, 55, 56),          # the centre of voxel (2, 3, 4); one step on it leaves along x
        ((1.25, -1, 2), 1, 2, 255, 255),         # u_x + 0.5 = 1 exactly: the boundary belongs to the upper voxel
        ((0.75, -1, 2), 0, 1, 255, 255),         # u_x + 0.5 = 0 exactly: the lowest point that is inside
        ((0.7, -1, 2), 255, 0, 255, 255),        # g_x = -1, just outside
        ((2.25, -1, 2), 255, 255, 255, 255),     # u_x + 0.5 = 3 exactly: g_x = nx, just outside
        ((2.2, -1, 2), 2, 255, 255, 255),        # g_x = nx - 1
        ((1, 0.75, 2), 255, 255, 1, 2),          # g_y = ny; turned, it lies on the half-voxel boundary of x
        ((1, -1.6, 2), 255, 255, 255, 255),      # g_y = -1
        ((1, -1, 4.25), 255, 255, 255, 255),     # g_z = nz
        ((1, -1, 4.2), 48, 49, 255, 255),        # g_z = nz - 1
        ((nan, -1, 2), 255, 255, 255, 255),
        ((1, inf, 2), 255, 255, 255, 255),
        ((1, -1, -inf), 255, 255, 255, 255),
        ((1, -0.75, 2), 3, 4, 255, 255),         # u_y + 0.5 = 1 exactly
    ]
    pts = np.array([c[0] for c in cases], F)
    want = np.array([[sum(c[1] ** 2 for c in cases), sum(c[2] ** 2 for c in cases)],
                     [sum(c[3] ** 2 for c in cases), sum(c[4] ** 2 for c in cases)]], np.int64)
    got = gr.pose_scores(pts, R, base, offsets, levels, origin, voxel)
    assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
    for i, c in enumerate(cases):                                        # and one point at a time
        one = gr.pose_scores(pts[i:i + 1], R, base, offsets, levels, origin, voxel)
        assert one.tolist() == [[c[1] ** 2, c[2] ** 2], [c[3] ** 2, c[4] ** 2]], (i, c, one)
    assert np.array_equal(gr.pose_scores(pts[::-1].copy(), R, base, offsets, levels, origin, voxel), want)
    assert not gr.pose_scores(pts[:0], R, base, offsets, levels, origin, voxel).any()
    # best_starts: the minimum over the offsets with ties to the lowest j, then a stable sort over the rotations
    score = np.array([[5, 3, 3], [9, 9, 9], [3, 4, 7], [2, 8, 2]], np.int64)
    Rs = np.arange(36, dtype=F).reshape(4, 3, 3)
    bs, offs = np.arange(12, dtype=F).reshape(4, 3), np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F)
    R0, t0, s0, m0 = gr.best_starts(score, Rs, bs, offs, 3)
    assert m0.tolist() == [3, 0, 2] and s0.tolist() == [2, 3, 3]
    assert np.array_equal(R0, Rs[[3, 0, 2]]) and t0.tolist() == [[9, 10, 11], [1, 1, 2], [6, 7, 8]]


# ---------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def reference_run(seed):
    """the reference pipeline on the scene, once per seed and shared (read-only) -> (scene, R, t, info)"""
    if seed not in _RUNS:
        sc = gr.make_scene(seed)
        _RUNS[seed] = (sc,) + gr.global_mesh_icp(sc["points"], sc["verts"], sc["faces"], gr.scene_levels())
    return _RUNS[seed]


def test_the_reference_levels():
    levels = gr.scene_levels()
    verts, _ = gr.scaled_corner()
    assert levels.shape == (40, 40, 40) and levels.dtype == np.uint8
    assert levels[10, 10, 10] == 0                                       # the voxel centred on the corner (0, 0, 0)
    assert levels[10 + 4, 10 + 4, 10] == 0 and levels[10 + 4, 10 + 4, 10 + 2] == 85      # on the square z = 0; 0.1 above it
    assert levels[39, 39, 39] == 255 and levels[0, 0, 0] == 255         # 0.87 and 0.5 * sqrt(3) from the mesh
    assert levels[10, 10, 10 + 20 + 4] == 170                           # (1.2, 0, 0): 0.2 beyond the squares' far end, 2/3 of trunc
    assert float(verts[:, 0].max()) == 1.0 and abs(float(verts[:, 2].max()) - 0.45) < 1e-7


@pytest.mark.parametrize("seed", gr.SCENE_SEEDS)
def test_the_reference_pipeline_finds_the_pose(seed):
    """This f32 reference with the mesh-derived levels, 1024 rotations x 27 offsets, 8 starts, 40 point-metric rounds,
    rotation in degrees / translation: seed 1: 0.038 / 1.6e-4, seed 2: 0.040 / 2.0e-4, seed 3: 0.028 / 2.1e-4 (the
    prototype with an analytic distance field: at most 0.07 / 8e-4).  The best start lies 10.2, 5.9 and 11.6 degrees
    from the truth, and every start that began within 30 degrees of it ended on it.  The plain reference ICP from the
    identity ends 115, 163 and 163 degrees off with ok = 1."""
    sc, R, t, info = reference_run(seed)
    rot, tr = mr.pose_error(R, t, sc["R_true"], sc["t_true"])
    starts = [mr.pose_error(info["start_R"][k], info["start_t"][k], sc["R_true"], sc["t_true"]) for k in range(gr.K_STARTS)]
    ends = [mr.pose_error(info["R"][k], info["t"][k], sc["R_true"], sc["t_true"]) for k in range(gr.K_STARTS)]
    print("seed %d: %.4f degrees / %.2e, best %d; starts (degrees / translation -> refined, final): %s" % (
        seed, rot, tr, info["best"], "; ".join("%.1f / %.2f -> %.3f / %.1e, %.4g" % (s + e + (f,)) for s, e, f in
                                               zip(starts, ends, info["final"]))))
    assert info["ok"][info["best"]] == 1
    assert rot < MAX_ROT_DEG and tr < MAX_T
    assert any(s[0] < gr.BASIN_DEG and s[1] < gr.BASIN_T for s in starts[:3])          # a start in the basin among the best three
    assert info["start_score"].tolist() == sorted(info["start_score"].tolist()) and len(set(info["start_rot"].tolist())) == 8
    # the local method alone, from the identity, on the same input
    eye = np.eye(3, dtype=F)[None], np.zeros((1, 3), F)
    Rp, tp, ip = mr.mesh_icp(sc["points"], sc["verts"], sc["faces"], *eye, iters=gr.ITERS, metric=1)
    rot_p, tr_p = mr.pose_error(Rp[0], tp[0], sc["R_true"], sc["t_true"])
    print("seed %d: mesh_icp from the identity ends %.1f degrees / %.2f off, ok = %d" % (seed, rot_p, tr_p, ip["ok"][0]))
    assert rot_p > FAR_DEG


def test_the_final_ranking_is_not_the_plane_rms():
    """Seed 2, the eight starts refined by 30 plane-metric rounds as well.  This run: all eight end with a plane rms of
    0.00194088 to 0.00194092; the two that end 120.0 degrees from the truth have 0.00194091 and 0.00194092, inside the
    range of the six that end 0.045 to 0.047 degrees from it.  The lowest rms is pose 6, a right one, by 3e-8: a coin toss,
    as in the prototype, where the wrong one won.  The plane residual does not see that the points overhang the squares'
    rims.  The rule `final` (the point metric over all points) picks a pose within the thresholds, and its value
    separates the poses on the truth (0.00193 to 0.00201) from those in the wrong basin 118 degrees away (0.82)."""
    sc, R, t, info = reference_run(2)
    Rp, tp, ip = mr.mesh_icp(sc["points"], sc["verts"], sc["faces"], info["start_R"], info["start_t"], iters=30, metric=0)
    rms = np.where(ip["ok"] != 0, ip["rms"][-1], np.inf)
    k = int(rms.argmin())
    rot_k, tr_k = mr.pose_error(Rp[k], tp[k], sc["R_true"], sc["t_true"])
    errs = [mr.pose_error(Rp[i], tp[i], sc["R_true"], sc["t_true"])[0] for i in range(gr.K_STARTS)]
    print("plane metric: rms %s, degrees off %s; the lowest rms is pose %d, %.3f degrees / %.2e off" % (
        np.array2string(rms, precision=5), np.array2string(np.array(errs), precision=2), k, rot_k, tr_k))
    wrong = [i for i in range(gr.K_STARTS) if errs[i] > FAR_DEG and ip["ok"][i]]
    right = [i for i in range(gr.K_STARTS) if errs[i] < 1.0]
    print("plane rms of the poses more than %g degrees off: %s; of those within 1 degree: %s" % (
        FAR_DEG, rms[wrong], rms[right]))
    # the rule of the pipeline on the point-metric poses
    rot, tr = mr.pose_error(R, t, sc["R_true"], sc["t_true"])
    assert rot < MAX_ROT_DEG and tr < MAX_T
    ends = np.array([mr.pose_error(info["R"][i], info["t"][i], sc["R_true"], sc["t_true"])[0] for i in range(gr.K_STARTS)])
    assert (ends > FAR_DEG).any() and (ends < MAX_ROT_DEG).any()         # both basins are among the eight
    assert info["final"][ends > FAR_DEG].min() > 100 * info["final"][ends < 1.0].max()
    assert info["best"] == int(np.argmin(info["final"]))
    # the rule itself: NaN counts as the cap, a pose with ok = 0 is out, ties go to the lowest k
    ok = np.array([0, 1, 1], np.uint8)
    Rk, tk = np.stack([info["R"][0]] * 3), np.stack([info["t"][0]] * 3)
    final, best = gr.final_scores(sc["points"], Rk, tk, ok, sc["verts"], sc["faces"], max_dist=0.001)
    assert np.isinf(final[0]) and final[1] == final[2] and best == 1
    assert final[1] <= len(sc["points"]) * 0.001 ** 2 * (1 + 1e-6) and final[1] > 0.3 * len(sc["points"]) * 0.001 ** 2
