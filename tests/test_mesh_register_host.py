"""CPU checks of the point-to-mesh ICP (include/ext/ctd_hip_mesh_register.h) as tests/meshreg_ref.py states it: the
header's prototypes against meshreg's table and the library, that the pinned interface lists did not move, every
rejection in the stated order (through the library, no GPU needed: each returns before any HIP call), the reference's
fixed-order sum against math.fsum, and the convergence of the reference itself on the corner scene.

The corner scene: three orthogonal unit squares of 6 x 6 quads (216 faces); 2000 surface samples with every coordinate
< 0.85, displaced by 20 degrees about a random axis and by 0.1; max_dist 0.25.  A float64 prototype of the rule gave, for
the plane metric after 5 rounds, < 1e-4 degrees and < 1e-5 without noise and 0.021 degrees / 4.7e-4 with Gaussian noise
of 0.002, and for the point metric after 30 rounds 0.10 degrees / 1.5e-3.  This reference (f32 poses, seeds 1..3) gives
after 10 rounds of the plane metric 2.6e-7 degrees / 9.3e-9 at worst without noise and 0.0073 .. 0.029 degrees /
1.0e-4 .. 2.6e-4 with it, and for the point metric after 30 rounds 0.022 .. 0.12 degrees / 3.5e-4 .. 1.9e-3: the same
figures within the spread of the draws.  The thresholds below are the issue's: < 0.01 degrees and < 1e-4 without noise,
< 0.1 degrees and < 2e-3 with it (about four times the prototype's)."""
import ctypes
import glob
import math
import os
import re

import numpy as np
import pytest

from tests import meshreg_ref as mr
from tests.abi_headers import parse_header

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "ctd_hip_mesh_register.h")

CORNER_SEED = 1
CORNER_ITERS = 10
MAX_DIST = 0.25
NOISE = 0.002
MAX_ROT_DEG, MAX_T = 0.01, 1e-4                       # without noise
MAX_ROT_DEG_NOISY, MAX_T_NOISY = 0.1, 2e-3            # with Gaussian noise of 0.002

C_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
             "size_t": ctypes.c_size_t}


def identity(K=1):
    return np.tile(np.eye(3, dtype=F), (K, 1, 1)), np.zeros((K, 3), F)


def test_header_matches_the_module_table_and_the_library():
    from connecting_the_dots_amd import _lib, meshreg
    functions, structs = parse_header(HEADER)
    assert not structs and list(functions) == list(meshreg.TABLE)       # the header's order
    bound = meshreg.lib()
    assert bound is _lib.lib()
    for name, (ret, params) in functions.items():
        res, args = meshreg.TABLE[name]
        assert res is C_SCALARS[ret], name
        assert len(args) == len(params), name
        for i, (ctype, declared) in enumerate(zip(args, params)):
            assert (ctype is ctypes.c_void_p) if declared.endswith("*") else (ctype is C_SCALARS[declared]), (name, i)
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype == res, name
    text = open(HEADER).read()
    assert re.findall(r'#\s*include\s*[<"]([^>"]+)[>"]', text) == ["../ctd_hip.h"]


def test_the_pinned_interface_did_not_move():
    from connecting_the_dots_amd import _lib, build, meshreg, torchext
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert headers == sorted(_lib.TABLES) and len(headers) == 14
    assert meshreg.HEADER not in _lib.TABLES and meshreg.TABLE not in _lib.TABLES.values()
    assert not any(name in table for table in _lib.TABLES.values() for name in meshreg.TABLE)
    assert len(torchext.functions.__all__) == 65
    assert not any(n in torchext.functions.__all__ for n in ("mesh_icp", "mesh_icp_system", "mesh_icp_update",
                                                             "register_mesh", "transform_points"))
    assert HEADER in build._headers()                                   # a stale header rebuilds


INVALID, WORKSPACE = 1, 2


def test_entry_points_validate_before_any_hip_call():
    from connecting_the_dots_amd import meshreg
    L = meshreg.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    p = [base + 4096 * i for i in range(12)]                # disjoint 4 KiB host regions: never dereferenced
    nan, inf = float("nan"), float("inf")

    # the workspace query: S, d2, face and closest of every posed point, 29 f64 per workgroup, each part 256-aligned
    up = lambda v: (v + 255) // 256 * 256
    for K, n in ((1, 1), (3, 2500), (64, 1024), (2, 1025)):
        N = K * n
        want = up(12 * N) + up(4 * N) + up(4 * N) + up(12 * N) + up(8 * 29 * K * ((n + 1023) // 1024))
        assert L.ctd_mesh_register_workspace_bytes(K, n) == want, (K, n)
    for bad in ((0, 10), (65, 10), (-1, 10), (1, -1), (1, 0), (64, 1 << 24), (1, 715827883)):
        assert L.ctd_mesh_register_workspace_bytes(*bad) == 0, bad
    assert L.ctd_mesh_register_workspace_bytes(1, 715827882) > 0                        # 3 * n = 2^31 - 2

    need = L.ctd_mesh_register_workspace_bytes(2, 10)

    def system(points=p[0], n=10, R=p[1], t=p[2], K=2, verts=p[3], nv=8, faces=p[4], nf=4, bvh=None, metric=0, max_d2=inf,
               hint=None, out=p[5], face=None, residual=None, closest=None, ws=p[6], nws=need):
        return L.ctd_mesh_register_system_f32(points, n, R, t, K, verts, nv, faces, nf, bvh, metric, max_d2, hint, out, face,
                                              residual, closest, ws, nws, -1, None)

    # each class of error wins over every later one: pair it with a later error and the answer does not change
    later = [dict(K=0), dict(n=1 << 30, K=1), dict(metric=2), dict(max_d2=nan), dict(R=None), dict(bvh=p[7] + 4),
             dict(face=p[5]), dict(ws=None)]
    for bad in (dict(n=-1), dict(nv=-1), dict(nf=-1)):
        assert system(**bad) == INVALID, bad
        for nxt in later:
            assert system(**{**nxt, **bad}) == INVALID
    for bad in (dict(K=0), dict(K=-1), dict(K=65)):
        assert system(**bad) == INVALID, bad
    for bad in (dict(n=1 << 30, K=1), dict(n=1 << 24, K=64), dict(nf=(1 << 28) + 1)):
        assert system(**bad) == INVALID, bad
    for bad in (dict(metric=2), dict(metric=-1)):
        assert system(**bad) == INVALID, bad
    for bad in (dict(max_d2=nan), dict(max_d2=-1.0), dict(max_d2=-inf)):
        assert system(**bad) == INVALID, bad
    for name in ("points", "R", "t", "out", "verts", "faces"):
        assert system(**{name: None}) == INVALID, name
        assert system(ws=None, **{name: None}) == INVALID, name                         # NULLs before the workspace
    assert system(bvh=p[7] + 4) == INVALID and system(bvh=p[7] + 8, ws=None) == INVALID  # a misaligned tree
    for a, b in (("face", p[5]), ("residual", p[0]), ("closest", p[3]), ("out", p[1]), ("face", p[6]), ("ws", p[4])):
        assert system(**{a: b}) == INVALID, (a, b)                                      # an output on another buffer
    assert system(face=p[8], hint=p[8]) == INVALID                                      # this round's faces on its hint
    assert system(face=p[8], residual=p[8] + 40) == INVALID                             # 2 * 10 * 4 bytes of face
    for bad in (dict(ws=None), dict(nws=need - 1), dict(ws=p[6] + 16), dict(nws=0)):
        assert system(**bad) == WORKSPACE, bad
    assert system(face=p[5], ws=None) == INVALID                                        # overlap before the workspace

    def update(sys=p[0], R=p[1], t=p[2], min_count=64, min_pivot=1e-4, damping=0.0, R_out=p[3], t_out=p[4], ok=p[5], K=2):
        return L.ctd_mesh_register_update_f32(sys, R, t, min_count, min_pivot, damping, R_out, t_out, ok, K, -1, None)

    for bad in (dict(K=0), dict(K=65), dict(min_count=-1), dict(min_pivot=-1.0), dict(min_pivot=nan), dict(damping=-0.5),
                dict(damping=nan)):
        assert update(**bad) == INVALID, bad
    for name in ("sys", "R", "t", "R_out", "t_out", "ok"):
        assert update(**{name: None}) == INVALID, name
    for a, b in (("R_out", p[1]), ("t_out", p[2]), ("ok", p[0]), ("R_out", p[4]), ("t_out", p[5])):
        assert update(**{a: b}) == INVALID, (a, b)


def test_the_fixed_order_sum_is_a_sum():
    """the header's order over exact terms lies within (n - 1) * 2^-53 * sum |term| of the correctly rounded sum; one
    row per point and three; sizes below a wavefront, at and around a chunk"""
    rs = np.random.RandomState(0)
    for n in (1, 63, 255, 1024, 1025, 2500):
        for rows in (1, 3):
            terms = rs.normal(size=(n, rows)) * 10.0 ** rs.randint(-3, 4, size=(n, rows))
            got, want = mr.ordered_sum(terms), math.fsum(terms.ravel().tolist())
            assert abs(got - want) <= (n * rows - 1) * 2.0 ** -53 * math.fsum(np.abs(terms).ravel().tolist()) + 0.0, (n, rows)
    assert mr.ordered_sum(np.zeros(0)) == 0.0
    ones = np.ones(2500)
    assert mr.ordered_sum(ones) == 2500.0


def test_transform_points_is_the_rule():
    import torch
    from connecting_the_dots_amd import meshreg
    rs = np.random.RandomState(4)
    pts = rs.normal(size=(300, 3)).astype(F)
    R = np.stack([mr.rotation(rs.normal(size=3), a) for a in (0.0, 17.0, 120.0)]).astype(F)
    t = rs.normal(size=(3, 3)).astype(F)
    got = meshreg.transform_points(torch.from_numpy(pts), torch.from_numpy(R), torch.from_numpy(t)).numpy()
    want = np.stack([np.stack(mr.transform(pts, R[k], t[k]), 1) for k in range(3)])
    assert got.dtype == F and np.array_equal(got.view(np.int32), want.view(np.int32))
    one = meshreg.transform_points(torch.from_numpy(pts), torch.from_numpy(R[1]), torch.from_numpy(t[1])).numpy()
    assert np.array_equal(one.view(np.int32), want[1].view(np.int32))
    with pytest.raises(RuntimeError):
        meshreg.transform_points(torch.from_numpy(pts), torch.from_numpy(R), torch.from_numpy(t[0]))
    with pytest.raises(RuntimeError):
        meshreg.transform_points(torch.from_numpy(pts).double(), torch.from_numpy(R[0]), torch.from_numpy(t[0]))
    z = torch.zeros(4, 3)
    i = torch.zeros(2, 3, dtype=torch.int32)
    for call in (lambda: meshreg.mesh_icp(z, z, i), lambda: meshreg.mesh_icp_system(z, z, i, torch.eye(3), torch.zeros(3)),
                 lambda: meshreg.mesh_icp_update(torch.zeros(29, dtype=torch.float64), torch.eye(3), torch.zeros(3)),
                 lambda: meshreg.register_mesh(z, i, z, i)):
        with pytest.raises(RuntimeError):                                # CPU tensors: there is no CPU path
            call()


def test_corner_mesh_is_the_scene():
    verts, faces = mr.corner_mesh()
    assert verts.shape == (147, 3) and faces.shape == (216, 3) and verts.min() == 0 and verts.max() == 1
    a, b, c = (verts[faces[:, i]].astype(np.float64) for i in range(3))
    n = np.cross(b - a, c - a)
    assert np.allclose(np.linalg.norm(n, axis=1), 1 / 36)                # two triangles per quad of side 1/6
    for axis in range(3):
        assert np.allclose(n[72 * axis:72 * (axis + 1)], np.eye(3)[axis] / 36)      # the normals face into the corner
    P = mr.corner_points(np.random.RandomState(0))
    assert P.shape == (2000, 3) and P.max() < 0.85 and ((P == 0).sum(1) >= 1).all()


def run_corner(noise, metric, iters=CORNER_ITERS, seed=CORNER_SEED):
    sc = mr.make_corner(seed, noise=noise)
    R0, t0 = identity()
    R, t, info = mr.mesh_icp(sc["points"], sc["verts"], sc["faces"], R0, t0, iters=iters, metric=metric, max_dist=MAX_DIST)
    return sc, R, t, info


def test_the_reference_converges_on_the_corner_scene_plane_metric():
    for noise, max_rot, max_t in ((0.0, MAX_ROT_DEG, MAX_T), (NOISE, MAX_ROT_DEG_NOISY, MAX_T_NOISY)):
        sc, R, t, info = run_corner(noise, 0)
        rot0, tr0 = mr.pose_error(np.eye(3), np.zeros(3), sc["R_true"], sc["t_true"])
        rot, tr = mr.pose_error(R[0], t[0], sc["R_true"], sc["t_true"])
        print("noise %g: %.3f degrees / %.3f -> %.3e degrees / %.3e; rms %s" % (noise, rot0, tr0, rot, tr,
                                                                             np.array2string(info["rms"][:, 0], precision=5)))
        assert abs(rot0 - 20.0) < 1e-6 and info["ok"][0] == 1 and info["count"][-1, 0] == 2000
        assert rot < max_rot and tr < max_t


def test_the_reference_point_metric_rms_falls_monotonically():
    sc, R, t, info = run_corner(0.0, 1)
    rms = info["rms"][:, 0]
    print("point metric rms by round: %s" % np.array2string(rms, precision=5))
    assert info["ok"][0] == 1 and (np.diff(rms) < 0).all()
    rot, tr = mr.pose_error(R[0], t[0], sc["R_true"], sc["t_true"])
    assert rot < 20.0 / 4                                                # slower than the plane metric, but on its way


def test_update_refuses_a_single_plane_and_a_low_count():
    """a single plane leaves three degrees of freedom free: the pivots refuse, and the pose comes back bit for bit"""
    rs = np.random.RandomState(2)
    verts, faces = mr.corner_mesh()
    pts = np.zeros((500, 3), F)
    pts[:, 1:] = rs.rand(500, 2).astype(F) * F(0.8) + F(0.1)
    pts[:, 0] = F(0.01)                                                  # over the square x = 0 only, 0.01 above it
    R0, t0 = identity()
    R0[0] = mr.rotation([1, 2, 3], 1.0).astype(F)
    s = mr.system(pts, R0, t0, verts, faces, 0, F(0.05) * F(0.05))[0]
    assert s[0, 28] > 400
    R1, t1, ok = mr.update(s, R0, t0)
    assert ok[0] == 0 and np.array_equal(R1.view(np.int32), R0.view(np.int32)) and np.array_equal(t1, t0)
    sc = mr.make_corner(CORNER_SEED)
    s = mr.system(sc["points"], *identity(), sc["verts"], sc["faces"], 0, F(MAX_DIST) * F(MAX_DIST))[0]
    assert mr.update(s, *identity())[2][0] == 1 and mr.update(s, *identity(), min_count=2001)[2][0] == 0
