"""CPU checks of the robust point-to-mesh ICP (include/ext/ctd_hip_mesh_robust.h) as tests/meshrobust_ref.py states it:
the header's prototypes against meshrobust's table and the library, that the pinned interface lists did not move, every
rejection in the stated order (through the library, no GPU needed: each returns before any HIP call), the reference's
face rim on four meshes, that the reference with every gate off is the plain reference, and the convergence of the
reference itself on the three scenes that the plain ICP fails on.

The scenes (meshrobust_ref.SCENES): the corner of tests/meshreg_ref.py, 2000 samples moved by 5 degrees and 0.03, Gaussian
noise 0.002, max_dist 0.25, seeds 1..3; Tukey rounds take their scale from the round before, the first is unweighted.
A float64 prototype gave (rotation in degrees / translation):
  plane metric, 15 rounds, 10 % box-uniform outliers: plain 0.41-0.68 / 6.6e-3-1.1e-2, Tukey 0.014-0.025 / 1.2e-4-1.9e-4;
  point metric, 30 rounds, samples overhanging by 0.2: plain 0.37-0.47 / 4.2e-2-4.5e-2, rim 0.008-0.029 / 1.5e-4-5.0e-4;
  point metric, 30 rounds, both: plain 0.46-0.56 / 4.2e-2-4.6e-2, rim + Tukey 0.04-0.09 / 0.7e-3-1.7e-3.
This f32 reference prints its own figures (test_the_reference_converges_where_the_plain_one_does_not); its docstring
records them.  The thresholds are the project's noisy ones, < 0.1 degrees and < 2e-3, and the plain reference has to be
at least 5 times worse in translation on the same input."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from tests import meshreg_ref as mr
from tests import meshrobust_ref as rr
from tests import meshsdf_ref as sr
from tests.abi_headers import parse_header

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "ctd_hip_mesh_robust.h")

MAX_ROT_DEG, MAX_T = 0.1, 2e-3                        # the noisy thresholds of tests/test_mesh_register_host.py
PLAIN_WORSE = 5.0                                     # the plain path's translation error over the robust path's

C_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64}


def identity(K=1):
    return np.tile(np.eye(3, dtype=F), (K, 1, 1)), np.zeros((K, 3), F)


def trap_mesh():
    """tests/test_mesh_register_gpu.trap_mesh (which needs torch and is a GPU module): the corner with a zero-area face,
    a face with an out-of-range index and one with a negative index"""
    verts, faces = mr.corner_mesh()
    n = len(verts)
    verts = np.concatenate([verts, np.array([[0.5, 0.5, 0.2], [0.5, 0.5, 0.3], [0.5, 0.5, 0.4]], F)])
    faces = np.concatenate([faces, np.array([[n, n + 1, n + 2], [0, 1, n + 3], [-1, 2, 3]], np.int32)])
    return verts, faces


def test_header_matches_the_module_table_and_the_library():
    from connecting_the_dots_amd import _lib, meshrobust
    functions, structs = parse_header(HEADER)
    assert not structs and list(functions) == list(meshrobust.TABLE)    # the header's order
    bound = meshrobust.lib()
    assert bound is _lib.lib()
    for name, (ret, params) in functions.items():
        res, args = meshrobust.TABLE[name]
        assert res is C_SCALARS[ret], name
        assert len(args) == len(params), name
        for i, (ctype, declared) in enumerate(zip(args, params)):
            assert (ctype is ctypes.c_void_p) if declared.endswith("*") else (ctype is C_SCALARS[declared]), (name, i)
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype == res, name
    text = open(HEADER).read()
    assert re.findall(r'#\s*include\s*[<"]([^>"]+)[>"]', text) == ["../ctd_hip.h"]
    assert "bit for bit" in text and "1.0 * x is exact" in text         # the identity with the plain system is stated


def test_the_pinned_interface_did_not_move():
    from connecting_the_dots_amd import _lib, build, meshreg, meshrobust, torchext
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert headers == sorted(_lib.TABLES) and len(headers) == 14
    assert meshrobust.HEADER not in _lib.TABLES and meshrobust.TABLE not in _lib.TABLES.values()
    assert not any(name in table for table in _lib.TABLES.values() for name in meshrobust.TABLE)
    assert not any(name in meshreg.TABLE for name in meshrobust.TABLE)
    assert len(torchext.functions.__all__) == 65
    assert not any(n in torchext.functions.__all__ for n in ("face_rim", "robust_icp_system", "robust_scale", "robust_mesh_icp",
                                                             "robust_register_mesh", "robust_aligned_reconstruction_error"))
    assert HEADER in build._headers()                                   # a stale header rebuilds


INVALID, WORKSPACE = 1, 2


def test_entry_points_validate_before_any_hip_call():
    from connecting_the_dots_amd import meshreg, meshrobust
    L = meshrobust.lib()
    buf = ctypes.create_string_buffer(1 << 17)
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    p = [base + 4096 * i for i in range(20)]                # disjoint 4 KiB host regions: never dereferenced
    nan, inf = float("nan"), float("inf")

    # the workspace query: the plain call's parts, and one feature byte per posed point before the partial sums
    up = lambda v: (v + 255) // 256 * 256
    for K, n in ((1, 1), (3, 2500), (64, 1024), (2, 1025)):
        N = K * n
        want = up(12 * N) + up(4 * N) + up(4 * N) + up(12 * N) + up(N) + up(8 * 29 * K * ((n + 1023) // 1024))
        assert L.ctd_mesh_robust_workspace_bytes(K, n) == want, (K, n)
        assert want == meshreg.lib().ctd_mesh_register_workspace_bytes(K, n) + up(N)
    for bad in ((0, 10), (65, 10), (-1, 10), (1, -1), (1, 0), (64, 1 << 24), (1, 715827883)):
        assert L.ctd_mesh_robust_workspace_bytes(*bad) == 0, bad
    assert L.ctd_mesh_robust_workspace_bytes(1, 715827882) > 0                          # 3 * n = 2^31 - 2

    need = L.ctd_mesh_robust_workspace_bytes(2, 10)

    def system(points=p[0], n=10, R=p[1], t=p[2], K=2, verts=p[3], nv=8, faces=p[4], nf=4, bvh=None, metric=0, max_d2=inf,
               hint=None, kernel=2, scale=p[9], rim=p[10], normals=p[11], min_cos=0.0, out=p[5], face=None, residual=None,
               weight=None, status=None, closest=None, ws=p[6], nws=need):
        return L.ctd_mesh_robust_system_f32(points, n, R, t, K, verts, nv, faces, nf, bvh, metric, max_d2, hint, kernel, scale,
                                            rim, normals, min_cos, out, face, residual, weight, status, closest, ws, nws, -1,
                                            None)

    # each class of error wins over every later one: pair it with a later error and the answer does not change
    later = [dict(K=0), dict(n=1 << 30, K=1), dict(metric=2), dict(kernel=3), dict(max_d2=nan), dict(min_cos=2.0), dict(R=None),
             dict(scale=None), dict(bvh=p[7] + 4), dict(face=p[5]), dict(ws=None)]
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
    for bad in (dict(kernel=3), dict(kernel=-1)):
        assert system(**bad) == INVALID, bad
    for bad in (dict(max_d2=nan), dict(max_d2=-1.0), dict(max_d2=-inf)):
        assert system(**bad) == INVALID, bad
    for bad in (dict(min_cos=nan), dict(min_cos=1.0000001), dict(min_cos=-1.5), dict(min_cos=inf), dict(min_cos=-inf)):
        assert system(**bad) == INVALID, bad
        assert system(normals=None, **bad) == INVALID, bad                              # checked with the gate off too
    for name in ("points", "R", "t", "out", "verts", "faces", "scale"):
        assert system(**{name: None}) == INVALID, name
        assert system(ws=None, **{name: None}) == INVALID, name                         # NULLs before the workspace
    assert system(kernel=1, scale=None) == INVALID
    assert system(bvh=p[7] + 4) == INVALID and system(bvh=p[7] + 8, ws=None) == INVALID  # a misaligned tree
    for a, b in (("face", p[5]), ("residual", p[0]), ("closest", p[3]), ("out", p[1]), ("face", p[6]), ("ws", p[4]),
                 ("weight", p[9]), ("status", p[10]), ("residual", p[11]), ("weight", p[5]), ("status", p[2]),
                 ("scale", p[6]), ("rim", p[5]), ("normals", p[6] + 256)):
        assert system(**{a: b}) == INVALID, (a, b)                                      # an output on another buffer
    assert system(face=p[8], hint=p[8]) == INVALID                                      # this round's faces on its hint
    assert system(face=p[8], residual=p[8] + 40) == INVALID                             # 2 * 10 * 4 bytes of face
    assert system(weight=p[8], status=p[8] + 79) == INVALID and system(status=p[8], weight=p[8] + 16) == INVALID
    for bad in (dict(ws=None), dict(nws=need - 1), dict(ws=p[6] + 16), dict(nws=0)):
        assert system(**bad) == WORKSPACE, bad
    assert system(face=p[5], ws=None) == INVALID                                        # overlap before the workspace
    assert system(kernel=0, scale=None, rim=None, normals=None, ws=None) == WORKSPACE   # all three may be NULL

    def rim(faces=p[0], nf=4, nv=8, offsets=p[1], ids=p[2], ninc=12, vflags=p[3], out=p[4]):
        return L.ctd_mesh_face_rim_u8(faces, nf, nv, offsets, ids, ninc, vflags, out, -1, None)

    for bad in (dict(nf=-1), dict(nv=-1), dict(ninc=-1), dict(nf=(1 << 28) + 1)):
        assert rim(**bad) == INVALID, bad
        assert rim(faces=None, **bad) == INVALID
    for name in ("faces", "offsets", "ids", "vflags", "out"):
        assert rim(**{name: None}) == INVALID, name
    for b in (p[0], p[1] + 32, p[2] + 47, p[3] + 7):
        assert rim(out=b) == INVALID, b
    assert rim(nf=0, faces=None, offsets=None, ids=None, vflags=None, out=None) == 0    # nothing to do: CTD_OK, no HIP call


# ---------------------------------------------------------------------------------------------------------------------
def test_the_reference_face_rim_on_four_meshes():
    # the corner: each square's border is rim and its interior is not
    for quads in (6, 3):
        verts, faces = mr.corner_mesh(quads)
        rim = rr.face_rim(faces, len(verts))
        V = verts.astype(np.float64)
        per = len(faces) // 3
        for f, tri in enumerate(faces):
            axis = f // per
            uv = np.delete(V[tri], axis, axis=1)                           # the in-plane coordinates of the corners
            on_border = ((uv == 0) | (uv == 1)).any(1)                     # a corner on the square's border
            for bit in range(3):
                assert bool(rim[f] >> bit & 1) == bool(on_border[bit]), (f, bit)
            for bit, (i, j) in zip((3, 4, 5), ((0, 1), (0, 2), (1, 2))):
                along = ((uv[i] == uv[j]) & ((uv[i] == 0) | (uv[i] == 1))).any()   # both ends on the same border line
                assert bool(rim[f] >> bit & 1) == bool(along), (f, bit)
        assert (rim >> 6 == 0).all()
        interior = [f for f in range(len(faces)) if rim[f] == 0]
        assert len(interior) == 3 * 2 * (quads - 2) ** 2                   # the faces that touch the border nowhere
    # a closed cube: no rim
    verts, faces = sr.cube()
    assert (rr.face_rim(faces, len(verts)) == 0).all()
    # three faces on the edge {0, 1}: the triple edge is not rim, and its ends are boundary vertices through other edges
    verts, faces = sr.fan3()
    rim = rr.face_rim(faces, len(verts))
    assert rim.tolist() == [0b110111, 0b110111, 0b110111]                  # ab (bit 3) clear, ac, bc and all corners set
    # the trap mesh: the zero-area face is valid (indices in range and different) and stands alone: all rim; the two faces
    # with an index out of range get 0 and change nothing else
    verts, faces = trap_mesh()
    rim = rr.face_rim(faces, len(verts))
    clean = rr.face_rim(mr.corner_mesh()[1], len(verts))
    assert np.array_equal(rim[:216], clean) and rim[216:].tolist() == [0b111111, 0, 0]
    # rows that hold anything: nothing out of range is read, an empty or a bad row makes no edge rim
    offsets, ids = sr.incident_rows(faces, len(verts))
    bad_ids = ids.copy()
    bad_ids[::5] = [-1, len(faces), 2 ** 31 - 1, -2 ** 31][0]
    bad_offsets = offsets.copy()
    bad_offsets[3] = -7
    got = rr.face_rim(faces, len(verts), rows=(bad_offsets, bad_ids))
    assert got.shape == rim.shape and ((got & 7) == (rim & 7)).all()


def test_with_every_gate_off_the_reference_is_the_plain_one():
    rs = np.random.RandomState(3)
    verts, faces = trap_mesh()
    pts = (mr.corner_points(rs, 1500, limit=0.95) + rs.normal(size=(1500, 3)) * 0.02).astype(F)
    pts[7], pts[8, 1] = [0.5, 0.5, 0.3], np.nan
    R, t = identity(2)
    R[1], t[1] = mr.rotation([1, 2, 3], 2.0).astype(F), np.array([0.01, 0, -0.01], F)
    for metric in (0, 1):
        for max_d2 in (np.inf, F(0.05) * F(0.05)):
            plain = mr.system(pts, R, t, verts, faces, metric, max_d2)
            got = rr.system(pts, R, t, verts, faces, metric, max_d2)
            assert np.array_equal(got["system"].view(np.int64), plain[0].view(np.int64))
            assert np.array_equal(got["status"] == 0, plain[1] >= 0)
            assert np.array_equal(np.isnan(got["residual"]), np.isnan(plain[2]))
            ok = got["status"] == 0
            assert np.array_equal(got["residual"][ok].view(np.int32), plain[2][ok].view(np.int32))
            assert np.array_equal(got["face"][ok], plain[1][ok]) and (got["weight"] == ok).all()
            # Huber and Tukey at c = +inf weigh every point 1: the same bits again
            for kernel in (1, 2):
                inf = rr.system(pts, R, t, verts, faces, metric, max_d2, kernel, np.full(2, np.inf, F))
                assert np.array_equal(inf["system"].view(np.int64), plain[0].view(np.int64))
    assert rr.robust_scale(np.array([[3, -1, np.nan, 2, -4], [np.nan] * 5], F), 2).tolist()[0] == F(2) * F(4.685 * 1.4826)
    assert np.isnan(rr.robust_scale(np.full((1, 4), np.nan, F), 1)[0])


def run_scene(name, seed):
    """-> (scene, robust pose error, plain pose error, robust info)"""
    kw, metric, iters, rob = rr.SCENES[name]
    sc = rr.make_scene(seed, **kw)
    R0, t0 = identity()
    rim = rr.face_rim(sc["faces"], len(sc["verts"])) if rob["rim"] else None
    R, t, info = rr.robust_mesh_icp(sc["points"], sc["verts"], sc["faces"], R0, t0, iters=iters, metric=metric,
                                    kernel=rob["kernel"], rim=rim, max_dist=rr.SCENE_MAX_DIST)
    Rp, tp, _ = mr.mesh_icp(sc["points"], sc["verts"], sc["faces"], R0, t0, iters=iters, metric=metric,
                            max_dist=rr.SCENE_MAX_DIST)
    return (sc, mr.pose_error(R[0], t[0], sc["R_true"], sc["t_true"]), mr.pose_error(Rp[0], tp[0], sc["R_true"], sc["t_true"]),
            info)


@pytest.mark.parametrize("seed", rr.SCENE_SEEDS)
@pytest.mark.parametrize("name", list(rr.SCENES))
def test_the_reference_converges_where_the_plain_one_does_not(name, seed):
    """This f32 reference, seeds 1..3, rotation in degrees / translation, robust against plain on the same input:
      outliers, plane:              0.009-0.033 / 1.1e-4-2.1e-4  against  0.53-1.00 / 8.8e-3-1.6e-2  (41-138 times worse);
      overhang, point:              0.017-0.029 / 3.4e-4-5.0e-4  against  0.37-0.47 / 4.2e-2-4.5e-2  (89-128 times);
      overhang and outliers, point: 0.021-0.050 / 4.7e-4-8.6e-4  against  0.44-0.54 / 3.8e-2-3.9e-2  (46-83 times).
    The prototype's figures within the spread of the draws."""
    sc, (rot, tr), (rot_p, tr_p), info = run_scene(name, seed)
    print("%s, seed %d: robust %.4f degrees / %.2e (used %d of %d, last scale %.4g), plain %.4f degrees / %.2e, %.1f times "
          "worse" % (name, seed, rot, tr, info["used"][-1, 0], len(sc["points"]), info["scale"][-1, 0], rot_p, tr_p, tr_p / tr))
    assert info["ok"][0] == 1
    assert rot < MAX_ROT_DEG and tr < MAX_T
    assert tr_p >= PLAIN_WORSE * tr
