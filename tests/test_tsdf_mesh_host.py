"""CPU-only checks of the mesh extraction (include/ctd_hip_mesh.h: ctd_tsdf_mesh_faces_i32, ctd_tsdf_mesh_case;
connecting_the_dots_amd.mesh): the rule's sentences (the header against its ctypes table and the built library:
tests/test_abi_and_host.py), the triangle table against
the restatement tests/mesh_ref.py and against its generator, the manifoldness the rule promises, argument validation
before any HIP call and its precedence, the workspace query, and the Python module (PLY round trip, import without a
GPU, torchext untouched)."""
import ctypes
import importlib.util
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import tsdf_ref as tr
from tests.test_tsdf_host import _Bufs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_HEADER = os.path.join(ROOT, "include", "ctd_hip_mesh.h")
TABLE_HEADER = os.path.join(ROOT, "connecting_the_dots_amd", "csrc", "ctd_mc_table.h")
GENERATOR = os.path.join(ROOT, "tools", "make_mc_table.py")

OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, 1, 2, 3
NAN, INF = float("nan"), float("inf")
F = np.float32


@pytest.fixture(scope="module")
def L():
    from connecting_the_dots_amd import _lib
    return _lib.lib()


def library_case(L, case):
    edges = (ctypes.c_int32 * 15)(*([-9] * 15))
    n = L.ctd_tsdf_mesh_case(case, edges)
    return n, list(edges)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header, the table (header == ctypes table == exports: tests/test_abi_and_host.py, for every header)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_rule():
    text = " ".join(open(MESH_HEADER).read().replace("*", " ").split())
    for phrase in ("Cell (i,j,k) of track b exists for i < nx-1, j < ny-1, k < nz-1",
                   "Corner n = dx + 2 dy + 4 dz is voxel (i+dx, j+dy, k+dz)",
                   "weight >= min_weight and |tsdf| < 1",
                   "Bit n of the cell's case is set when T_n < 0",
                   "so -0.0 and 0 are outside",
                   "Edge e = 4 c + r runs along axis c from the r-th corner (ascending n) that has coordinate c equal to 0",
                   "src = 3 g(lower corner) + c",
                   "Two crossing edges: one segment joins them",
                   "at each inside corner, the two face edges that meet there are joined",
                   "A loop starts at its lowest e",
                   "(v1-v0) x (v2-v0) of its triangles points from inside (T < 0) towards free space",
                   "The loops of a case come in ascending order of their lowest e",
                   "A loop q of length m is a fan (q0, q_i, q_{i+1}) for i = 1 .. m-2",
                   "the first apex, in loop order from the start, for which no fan diagonal joins two edges of one cell face",
                   "Faces are int32, track-local: index 0 is the track's first surface point",
                   "ascending cell order ((b nz + k) ny + j) nx + i, and within a cell in table order",
                   "Surface points on edges of no meshed cell stay as unreferenced vertices",
                   "exactly 0 can yield zero-area triangles",
                   "With faces == NULL it only counts",
                   "it writes every word of the workspace that it reads",
                   "No atomics, no flag that another workgroup waits on: the same bits on every run"):
        assert phrase in text, phrase


def test_the_library_table_is_the_restatement(L):
    for case in range(256):
        n, edges = library_case(L, case)
        want = [e for t in mr.TABLE[case] for e in t]
        assert n == len(mr.TABLE[case]) and edges == want + [-1] * (15 - len(want)), case
    for bad in (-1, 256, 1 << 20):
        n, edges = library_case(L, bad)
        assert n == -1 and edges == [-9] * 15, bad
    assert L.ctd_tsdf_mesh_case(3, None) == -1


def test_the_table_has_the_counts_of_the_rule():
    n_tri = [len(t) for t in mr.TABLE]
    assert max(n_tri) == 5 and sum(n_tri) == 820
    assert np.bincount(n_tri).tolist() == [2, 16, 50, 80, 76, 32]
    assert n_tri[0] == n_tri[255] == 0
    loops = [mr.case_loops(c) for c in range(256)]
    assert max(len(q) for ls in loops for q in ls) == 7 and min(len(q) for ls in loops for q in ls) == 3
    assert sum(any(mr.loop_fan(q)[1] != 0 for q in ls) for ls in loops) == 18   # an apex other than the loop's start
    for case in range(256):
        crossing = sorted(e for e, (a, b) in enumerate(mr.EDGES) if ((case >> a) & 1) != ((case >> b) & 1))
        assert sorted({e for t in mr.TABLE[case] for e in t}) == crossing, case   # every crossing edge, no other
        firsts = [q[0] for q in loops[case]]
        assert firsts == sorted(firsts) and all(q[0] == min(q) for q in loops[case]), case
        assert all(len(set(t)) == 3 for t in mr.TABLE[case]), case
    assert mr.EDGES == [(0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)]


def test_the_committed_table_header_is_the_generators_output():
    spec = importlib.util.spec_from_file_location("make_mc_table", GENERATOR)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert open(TABLE_HEADER).read() == gen.header()
    assert [[tuple(t) for t in ts] for ts in gen.table()] == [[tuple(t) for t in ts] for ts in mr.TABLE]
    r = subprocess.run([sys.executable, GENERATOR], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout == open(TABLE_HEADER).read(), r.stderr


# ---------------------------------------------------------------------------------------------------------------------
# 2. manifoldness
# ---------------------------------------------------------------------------------------------------------------------
def random_sign_volume(n, seed):
    """random signs inside a positive border, every weight usable"""
    rs = np.random.RandomState(seed)
    T = rs.uniform(-0.9, 0.9, (1, n, n, n)).astype(F)
    T[:, 0] = T[:, -1] = T[:, :, 0] = T[:, :, -1] = T[:, :, :, 0] = T[:, :, :, -1] = F(0.5)
    return T, np.ones_like(T)


def test_random_signs_give_a_closed_oriented_manifold():
    T, w = random_sign_volume(12, 0)
    f, count = mr.faces(T, w)
    assert count.tolist() == [len(f)] and len(f) > 2000
    assert mr.is_closed_oriented_manifold(f)
    case, meshed = mr.cell_cases(T, w)
    assert meshed.all() and len(set(case.reshape(-1).tolist())) > 200
    n_points = tr.surface_points(T, w, np.zeros((1, 3), F), 1.0)[3]
    assert sorted(set(f.reshape(-1).tolist())) == list(range(int(n_points[0])))   # every point is a vertex of the mesh
    # the plain fan, without the apex rule, is not manifold on the same volume: the rule is needed
    plain, _ = mr.faces(T, w, table=mr.PLAIN_TABLE)
    assert len(plain) == len(f) and not mr.is_closed_oriented_manifold(plain)


def test_a_sphere_is_closed_has_euler_characteristic_2_and_faces_outwards():
    T, w, centre = mr.sphere_volume(20, 7.3)
    f, count = mr.faces(T, w)
    points, _, _, n_points = tr.surface_points(T, w, np.zeros((1, 3), F), 1.0)
    assert mr.is_closed_oriented_manifold(f)
    n_edges = len(mr.directed_edge_counts(f)) // 2
    assert int(n_points[0]) - n_edges + len(f) == 2
    p = points.astype(np.float64)
    nrm = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert ((nrm * (p[f].mean(1) - centre)).sum(1) > 0).all()
    # the normals of the surface points point to the same side
    normals = tr.surface_points(T, w, np.zeros((1, 3), F), 1.0)[1].astype(np.float64)
    assert ((normals * (p - centre)).sum(1) > 0).all()


def test_cells_with_an_unusable_corner_are_not_meshed_and_zero_is_outside():
    T, w, _ = mr.sphere_volume(10, 3.2)
    full, _ = mr.faces(T, w)
    w2 = w.copy()
    w2[0, 5, 5, 8] = 0                                             # a voxel at the surface
    case, meshed = mr.cell_cases(T, w2)
    assert (~meshed).sum() == 8 and (case[~meshed] == 0).all()
    holed, count = mr.faces(T, w2)
    assert 0 < len(holed) < len(full) and count.tolist() == [len(holed)]
    assert mr.is_closed_oriented_manifold(full) and not mr.is_closed_oriented_manifold(holed)
    Tz = np.full((1, 2, 2, 2), 0.5, F)
    Tz[0, 0, 0, 0] = -0.0                                          # -0.0 is outside, as in the crossing test
    assert len(mr.faces(Tz, np.ones_like(Tz))[0]) == 0
    Tz[0, 0, 0, 0] = -0.25
    assert mr.faces(Tz, np.ones_like(Tz))[0].tolist() == [[0, 1, 2]]
    Tz[0, 1, 1, 1] = 1.0                                           # |tsdf| == 1: not usable, the cell is not meshed
    assert len(mr.faces(Tz, np.ones_like(Tz))[0]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. validation and workspace
# ---------------------------------------------------------------------------------------------------------------------
B, NX, NY, NZ = 2, 3, 4, 5                                          # 120 voxels: every buffer fits a 4 KiB slot
BIG_GRID = dict(B=1 << 20, nx=2048, ny=1, nz=1)                    # B * nx * ny * nz = 2^31


def mesh_workspace_bytes(b, nx, ny, nz):
    nv = b * nx * ny * nz
    counts = (4 * (b * ((nx * ny * nz + 255) // 256) + 1) + 255) // 256 * 256
    up = lambda v: (v + 255) // 256 * 256                          # noqa: E731
    return up(nv) + counts + up(4 * nv) + up(nv) + counts + up(8 * b)


def test_faces_rejections_need_no_gpu(L):
    nws = L.ctd_tsdf_mesh_workspace_bytes(B, NX, NY, NZ)
    assert nws == 256 + 256 + 512 + 256 + 256 + 256                # flags, offsets, first indices, cases, offsets, counts
    names = ["tsdf", "weight", "faces", "n_faces", "ws"]
    bufs = _Bufs(names, slot=8192)

    def call(min_weight=1.0, capacity=100, B=B, nx=NX, ny=NY, nz=NZ, nbytes=None, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_tsdf_mesh_faces_i32(p["tsdf"], p["weight"], min_weight, p["faces"], p["n_faces"], capacity, B, nx, ny, nz,
                                         p["ws"], nws if nbytes is None else nbytes, -1, None)

    for kw in (dict(nx=0), dict(ny=-1), dict(nz=0), dict(B=-1), dict(capacity=-1)):
        assert call(**kw) == INVALID_ARG, kw
    for bad in (0.0, -1.0, NAN, INF, -INF):
        assert call(min_weight=bad) == INVALID_ARG, bad
    for k in ("tsdf", "weight", "n_faces"):
        assert call(**{k: None}) == INVALID_ARG, k
    for kw in (dict(nx=2049), dict(ny=2049), dict(nz=2049), BIG_GRID, dict(B=1, nx=1024, ny=1024, nz=1024),
               dict(B=1, nx=1024, ny=1024, nz=410),                  # 5 * 2^20 * 410 >= 2^31 > 3 * 2^20 * 410
               dict(B=1 << 24, nx=1, ny=1, nz=1)):                   # 2^24 workgroups
        assert call(**kw) == UNSUPPORTED, kw
    assert call(B=1, nx=1024, ny=1024, nz=409, tsdf=None) == INVALID_ARG   # (5 * 2^20 * 409 < 2^31 gets past the sizes)
    for out in ("faces", "n_faces", "ws"):
        for other in names:
            if other != out:
                assert call(**{out: bufs.ptr[other]}) == INVALID_ARG, (out, other)
    assert call(faces=bufs.ptr["tsdf"] + 476) == INVALID_ARG       # the last float of tsdf
    assert call(faces=bufs.ptr["weight"] - 1196, capacity=100) == INVALID_ARG   # 100 faces end 4 bytes into weight
    assert call(faces=bufs.ptr["weight"] - 1200, capacity=100, ws=None) == WORKSPACE   # (they end where weight starts)
    assert call(ws=None) == WORKSPACE                               # workspace missing, short, misaligned
    assert call(nbytes=nws - 1) == WORKSPACE
    assert call(nbytes=0) == WORKSPACE
    assert call(ws=bufs.ptr["ws"] + 8) == WORKSPACE
    # precedence: INVALID_ARG, then UNSUPPORTED, then the overlaps, then WORKSPACE
    assert call(ws=None, **BIG_GRID) == UNSUPPORTED
    assert call(ws=None, min_weight=NAN, **BIG_GRID) == INVALID_ARG
    assert call(ws=None, n_faces=None, **BIG_GRID) == INVALID_ARG
    assert call(ws=None, faces=bufs.ptr["weight"]) == INVALID_ARG
    # counting only: faces NULL, and then capacity is not looked at
    assert call(faces=None, capacity=-5, nbytes=0) == WORKSPACE
    assert call(faces=None, n_faces=bufs.ptr["tsdf"], nbytes=0) == INVALID_ARG
    # no tracks: nothing to do, nothing touched, no workspace needed
    assert call(B=0, ws=None, nbytes=0) == OK
    assert call(B=0, ws=None, nbytes=0, faces=None) == OK
    assert call(B=0, ws=None, nbytes=0, min_weight=-1.0) == INVALID_ARG
    assert call(B=0, ws=None, nbytes=0, tsdf=None) == INVALID_ARG
    assert call(B=0, ws=None, nbytes=0, n_faces=None) == INVALID_ARG


def test_mesh_workspace_query(L):
    for shape in [(4, 256, 256, 100), (1, 2, 2, 2), (2, 33, 18, 21), (2, 64, 5, 7), (1, 1, 1, 1), (3, 256, 1, 1), (3, 257, 1, 1),
                  (1, 1024, 1024, 409)]:
        assert L.ctd_tsdf_mesh_workspace_bytes(*shape) == mesh_workspace_bytes(*shape) > 0, shape
    for args in ((0, 8, 8, 8), (-1, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 0), (1, 2049, 1, 1), (1 << 20, 2048, 1, 1),
                 (1, 1024, 1024, 1024), (1, 1024, 1024, 410), (1 << 24, 1, 1, 1)):
        assert L.ctd_tsdf_mesh_workspace_bytes(*args) == 0, args


# ---------------------------------------------------------------------------------------------------------------------
# 4. the Python module
# ---------------------------------------------------------------------------------------------------------------------
def test_ply_round_trip_keeps_the_bits(tmp_path):
    from connecting_the_dots_amd import mesh
    rs = np.random.RandomState(3)
    verts = rs.randn(11, 3).astype(F)
    verts[4, 1], verts[7, 0] = np.nan, -0.0
    faces = rs.randint(0, 11, (17, 3)).astype(np.int32)
    normals = rs.randn(11, 3).astype(F)
    normals[2] = np.nan                                            # a surface point without a normal
    colors = rs.randint(0, 256, (11, 3)).astype(np.uint8)
    for k, (nrm, col) in enumerate(((None, None), (normals, None), (None, colors), (normals, colors))):
        path = str(tmp_path / ("m%d.ply" % k))
        mesh.save_ply(path, verts, faces, normals=nrm, colors=col)
        head = open(path, "rb").read(64)
        assert head.startswith(b"ply\nformat binary_little_endian 1.0\n")
        v, f, n, c = mesh.load_ply(path)
        assert v.dtype == F and f.dtype == np.int32 and v.tobytes() == verts.tobytes() and f.tobytes() == faces.tobytes()
        assert (n is None) == (nrm is None) and (c is None) == (col is None)
        assert n is None or (n.dtype == F and n.tobytes() == normals.tobytes())
        assert c is None or (c.dtype == np.uint8 and c.tobytes() == colors.tobytes())
        assert os.path.getsize(path) == len(open(path, "rb").read().split(b"end_header\n")[0]) + 11 + \
            11 * (12 + (12 if nrm is not None else 0) + (3 if col is not None else 0)) + 17 * 13
    # tensors are taken too; an empty mesh is a file
    path = str(tmp_path / "t.ply")
    mesh.save_ply(path, torch.from_numpy(verts), torch.from_numpy(faces))
    assert mesh.load_ply(path)[0].tobytes() == verts.tobytes()
    mesh.save_ply(path, np.zeros((0, 3), F), np.zeros((0, 3), np.int32))
    v, f, n, c = mesh.load_ply(path)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n is None and c is None
    # what it refuses
    for bad in (dict(verts=verts.astype(np.float64)), dict(faces=faces.astype(np.int64)), dict(verts=verts[:, :2]),
                dict(normals=normals[:5]), dict(colors=colors.astype(F)), dict(faces=faces + 11)):
        kw = dict(dict(verts=verts, faces=faces), **bad)
        with pytest.raises(RuntimeError, match="save_ply"):
            mesh.save_ply(path, **kw)
    open(path, "wb").write(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(RuntimeError, match="load_ply"):
        mesh.load_ply(path)
    open(path, "wb").write(b"not a ply")
    with pytest.raises(RuntimeError, match="load_ply"):
        mesh.load_ply(path)


def test_mesh_imports_without_a_gpu_and_leaves_torchext_alone():
    code = ("import sys\n"
            "from connecting_the_dots_amd import torchext as te\n"
            "before = sorted(n for n in vars(te) if not n.startswith('_'))\n"
            "from connecting_the_dots_amd import mesh\n"
            "after = sorted(n for n in vars(te) if not n.startswith('_'))\n"
            "assert before == after, set(after) ^ set(before)\n"
            "assert not hasattr(te, 'tsdf_mesh') and not hasattr(te.functions, 'tsdf_mesh')\n"
            "import torch\n"
            "assert not torch.cuda.is_initialized()\n"
            "print(sorted(n for n in vars(mesh) if not n.startswith('_') and getattr(getattr(mesh, n), '__module__', '') == mesh.__name__))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == str(["TsdfMesh", "load_ply", "save_ply", "tsdf_mesh"])


def test_python_signatures_docstrings_and_host_side_errors():
    from connecting_the_dots_amd import mesh

    def params(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    assert params(mesh.tsdf_mesh) == [("tsdf", E), ("weight", E), ("origin", E), ("voxel", E), ("min_weight", 1.0),
                                      ("return_normals", False)]
    assert params(mesh.save_ply) == [("path", E), ("verts", E), ("faces", E), ("normals", None), ("colors", None)]
    assert params(mesh.load_ply) == [("path", E)]
    assert params(mesh.TsdfMesh.track) == [("self", E), ("b", E)]
    doc = mesh.tsdf_mesh.__doc__
    for phrase in ("one synchronisation", "Not differentiable", "Edge e = 4*c + r", "no fan diagonal joins two edges of one cell",
                   "the same bits on every run"):
        assert phrase in doc, phrase
    tsdf, weight, origin = torch.ones(2, 5, 4, 3), torch.zeros(2, 5, 4, 3), torch.zeros(2, 3)
    for bad in (0.0, -1.0, NAN, INF, "1", None, True):
        with pytest.raises(RuntimeError, match="tsdf_mesh: voxel must be a finite number > 0"):
            mesh.tsdf_mesh(tsdf, weight, origin, bad)
        with pytest.raises(RuntimeError, match="tsdf_mesh: min_weight must be a finite number > 0"):
            mesh.tsdf_mesh(tsdf, weight, origin, 0.1, min_weight=bad)
    with pytest.raises(RuntimeError, match="CUDA tensor"):           # no CPU path: well-formed CPU tensors raise too
        mesh.tsdf_mesh(tsdf, weight, origin, 0.1, return_normals=True)
    with pytest.raises(RuntimeError):
        mesh.tsdf_mesh(tsdf.numpy(), weight, origin, 0.1)
