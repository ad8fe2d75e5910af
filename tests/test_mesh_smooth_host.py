"""CPU-only checks of the mesh connectivity, smoothing and vertex normals (include/ctd_hip_mesh_smooth.h:
ctd_mesh_adjacency_i32, ctd_mesh_smooth_f32, ctd_mesh_vertex_normals_f32; connecting_the_dots_amd.meshsmooth): the rule's
sentences (the header against its ctypes table: tests/test_abi_and_host.py), argument validation before any HIP call and its
precedence, the workspace queries, the Python module, and the restatement tests/meshsmooth_ref.py against hand-made
meshes with known answers and against the truth of the fused scenes.

What 10 iterations of lambda 0.5 | mu -0.53 with the boundary held buy, measured with the restatement on the scenes of
tests/test_tsdf_host.fused_scene meshed by tests/mesh_ref.faces and cleaned with min_faces = 32 (distance of the vertices
to the true surfaces, tests/tsdf_ref.scene_surface_distance, before -> after):
  noisy, seed 5:  median 1.829e-03 -> 1.081e-03, ratio 0.591;  mean 2.853e-03 -> 2.086e-03, ratio 0.731
  noisy, seed 6:  median 1.832e-03 -> 1.035e-03, ratio 0.565;  mean 2.915e-03 -> 2.111e-03, ratio 0.724
  clean, seed 5:  median 2.300e-04 -> 2.271e-04, ratio 0.987;  mean 1.000e-03 -> 1.017e-03, ratio 1.017
The scenes are planar, where smoothing is at its best.  On the noisy unit icosphere (642 vertices, sigma 0.01,
default_rng(0)) the rms radial error goes 0.00990 -> 0.00454 (ratio 0.459) and the volume to 1.0070 of the clean
sphere's; with mu = 0 (plain Laplacian) the volume shrinks to 0.841.

The recomputed normals against the TSDF gradients, on the meshes before clean-up: clean, seed 5: 2465 of 2475 vertices
referenced, all 2465 with a finite recomputed normal, 274 of the 2475 gradients not finite, dot > 0 for 100 % and > 0.9
for 97.4 % of the vertices that have both; noisy, seed 6: 2500 of 2538 referenced, all finite, 425 gradients not finite,
dot > 0 for 100 %, > 0.9 for 97.1 %.  (noisy, seed 5, which is not asserted: 2507 referenced, 387 gradients not finite,
dot > 0 for all but one vertex.)"""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import meshclean_ref as mcr
from tests import meshsmooth_ref as msr
from tests import tsdf_ref as tr
from tests.test_tsdf_host import _Bufs, fused_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTH_HEADER = os.path.join(ROOT, "include", "ctd_hip_mesh_smooth.h")

OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, 1, 2, 3
F = np.float32
NAN, INF = float("nan"), float("inf")

# (kind, seed) -> the measured after / before of the median distance (the docstring above)
MEASURED_MEDIAN_RATIO = {("noisy", 5): 0.591, ("noisy", 6): 0.565, ("clean", 5): 0.987}
MEASURED_SPHERE_RMS_RATIO = 0.459


@pytest.fixture(scope="module")
def L():
    from connecting_the_dots_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header (header == ctypes table == exports: tests/test_abi_and_host.py, for every header)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_rule():
    text = " ".join(open(SMOOTH_HEADER).read().replace("*", " ").split())
    for phrase in ("Its three indices lie in [0, n_verts)",
                   "Its three indices are pairwise different",
                   "Out-of-range indices are never dereferenced",
                   "The incident faces of vertex i are the valid faces that use i, in ascending face index",
                   "the row of a receives b and c, the row of b receives a and c, and the row of c receives a and b",
                   "The one-ring of i is the set of values in its row, ascending, each once",
                   "The multiplicity of j in row i is the number of valid faces that use the edge {i,j}",
                   "An edge is a pair i < j with j in the ring of i",
                   "A boundary edge has multiplicity 1",
                   "A non-manifold edge has multiplicity > 2",
                   "CTD_MESH_VERT_REFERENCED (1): the ring is not empty",
                   "CTD_MESH_VERT_BOUNDARY (2): the vertex is an end of a boundary edge",
                   "CTD_MESH_VERT_NONMANIFOLD (4): the vertex is an end of a non-manifold edge",
                   "nnz, which is 2 x the number of edges",
                   "max_incident, the largest number of valid faces at one vertex",
                   "CTD_MESH_ADJ_MAX_INCIDENT = 1024",
                   "No lane, wavefront or workgroup does work that grows quadratically in a row longer than that",
                   "still returns CTD_OK and always writes the true counts",
                   "all other outputs are then unspecified and must not be used",
                   "every output is exact and the same on every run",
                   "Everything is f32, uncontracted, in the written association",
                   "a row is empty unless 0 <= offsets[i] <= offsets[i+1] <= nnz",
                   "A row entry outside [0, n_verts) is never dereferenced, adds nothing, and does not count",
                   "then out = in, bit for bit",
                   "m_c = s_c / (float)d (IEEE division); out_c = x_c + f (m_c - x_c)",
                   "One iteration is a pass with lambda over all vertices, then a pass with mu over the result",
                   "With mu == 0 the second pass is not run",
                   "With iters == 0 the output is a copy",
                   "Passes ping-pong between the output and the workspace",
                   "No pass reads what it writes",
                   "A NaN or infinite coordinate spreads to its ring and nowhere else per pass",
                   "cx = e1y e2z - e1z e2y; cy = e1z e2x - e1x e2z; cz = e1x e2y - e1y e2x",
                   "This is area weighting: |c| is twice the face's area",
                   "len = sqrtf((ax ax + ay ay) + az az)",
                   "normal = acc / len (three divisions) when len > 0 and len is finite",
                   "Otherwise the normal is three NaNs",
                   "So an unreferenced vertex has a NaN normal",
                   "a vertex with at most 16 incident faces by ONE LANE",
                   "every longer row by THE WORKGROUP",
                   "Atomics are integer add, subtract and or only, whose final results do not depend on their order",
                   "No flag that another workgroup waits on: the same bits on every run",
                   "they write every word of the workspace that they read",
                   "#define CTD_MESH_ADJ_MAX_INCIDENT 1024", "#define CTD_MESH_VERT_REFERENCED 1",
                   "#define CTD_MESH_VERT_BOUNDARY 2", "#define CTD_MESH_VERT_NONMANIFOLD 4"):
        assert phrase in text, phrase


# ---------------------------------------------------------------------------------------------------------------------
# 2. validation and workspace
# ---------------------------------------------------------------------------------------------------------------------
NV, NF = 100, 200                                                   # every buffer fits a 16 KiB slot
TOO_MANY_FACES = (1 << 31) // 6 + 1                                 # 6 * n_faces >= 2^31
SLOT = 16384


def adjacency_workspace_bytes(n, m):
    up = lambda v: (v + 255) // 256 * 256                          # noqa: E731
    chunks = (n + 255) // 256
    return up(4 * n) + up(4 * (n + 1)) + up(4 * n) + up(12 * m) + up(24 * m) + 3 * up(4 * (chunks + 1))


def test_adjacency_rejections_need_no_gpu(L):
    nws = L.ctd_mesh_adjacency_workspace_bytes(NV, NF)
    assert nws == 512 + 512 + 512 + 2560 + 4864 + 3 * 256             # counters, face offsets, ring sizes; ids; rows; chunk sums
    names = ["faces", "offsets", "neighbors", "face_offsets", "face_ids", "vflags", "counts", "ws"]
    bufs = _Bufs(names, slot=SLOT)

    def call(n=NV, m=NF, cap=6 * NF, cap_faces=3 * NF, nbytes=None, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_mesh_adjacency_i32(p["faces"], n, m, p["offsets"], p["neighbors"], cap, p["face_offsets"], p["face_ids"],
                                        cap_faces, p["vflags"], p["counts"], p["ws"], nws if nbytes is None else nbytes, -1, None)

    for kw in (dict(n=-1), dict(m=-1), dict(cap=-1), dict(cap_faces=-1), dict(faces=None), dict(offsets=None), dict(vflags=None),
               dict(counts=None), dict(faces=None, m=0), dict(counts=None, m=0, n=0), dict(vflags=None, n=0)):
        assert call(**kw) == INVALID_ARG, kw
    for kw in (dict(m=TOO_MANY_FACES), dict(n=1 << 31), dict(n=1 << 40), dict(m=1 << 40)):
        assert call(**kw) == UNSUPPORTED, kw
    assert call(m=TOO_MANY_FACES - 1, faces=None) == INVALID_ARG     # (6 * n_faces < 2^31 gets past the sizes)
    for out in names[1:]:
        for other in names:
            if other != out:
                assert call(**{out: bufs.ptr[other]}) == INVALID_ARG, (out, other)
    assert call(offsets=bufs.ptr["faces"] + 12 * NF - 4) == INVALID_ARG         # the last index of faces
    assert call(neighbors=bufs.ptr["faces"] - 40, cap=11) == INVALID_ARG        # 11 entries end 4 bytes into faces
    assert call(neighbors=bufs.ptr["faces"] - 40, cap=10, ws=None) == WORKSPACE
    assert call(face_ids=bufs.ptr["vflags"] - 4 * 3 * NF + 4, cap_faces=1 << 40) == INVALID_ARG   # counts with 3 * n_faces entries
    assert call(face_ids=bufs.ptr["vflags"] - 4 * 3 * NF, cap_faces=1 << 40, ws=None) == WORKSPACE
    assert call(vflags=bufs.ptr["counts"] - NV + 1) == INVALID_ARG
    assert call(counts=bufs.ptr["ws"] - 47) == INVALID_ARG
    assert call(counts=bufs.ptr["ws"] - 48, nbytes=0) == WORKSPACE               # (they end where the workspace starts)
    for kw in (dict(ws=None), dict(nbytes=nws - 1), dict(nbytes=0), dict(ws=bufs.ptr["ws"] + 8), dict(n=0, m=0, ws=None)):
        assert call(**kw) == WORKSPACE, kw
    # precedence: INVALID_ARG, then UNSUPPORTED, then the overlaps, then WORKSPACE
    assert call(ws=None, m=TOO_MANY_FACES) == UNSUPPORTED
    assert call(ws=None, m=TOO_MANY_FACES, cap=-1) == INVALID_ARG
    assert call(ws=None, m=TOO_MANY_FACES, counts=None) == INVALID_ARG
    assert call(ws=None, offsets=bufs.ptr["faces"]) == INVALID_ARG
    # the optional outputs NULL: their capacities are not looked at
    assert call(neighbors=None, face_offsets=None, face_ids=None, cap=-5, cap_faces=-5, nbytes=0) == WORKSPACE
    assert call(neighbors=None, face_offsets=None, face_ids=None, counts=bufs.ptr["faces"], nbytes=0) == INVALID_ARG


def test_smooth_rejections_need_no_gpu(L):
    nws = L.ctd_mesh_smooth_workspace_bytes(NV)
    assert nws == 1280
    nnz = 600
    names = ["verts", "offsets", "neighbors", "vflags", "verts_out", "ws"]
    bufs = _Bufs(names, slot=SLOT)

    def call(n=NV, nnz=nnz, iters=10, lam=0.5, mu=-0.53, fix=1, nbytes=None, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_mesh_smooth_f32(p["verts"], n, p["offsets"], p["neighbors"], nnz, p["vflags"], iters, lam, mu, fix,
                                     p["verts_out"], p["ws"], nws if nbytes is None else nbytes, -1, None)

    for kw in (dict(n=-1), dict(nnz=-1), dict(verts=None), dict(offsets=None), dict(neighbors=None), dict(vflags=None),
               dict(verts_out=None), dict(verts=None, n=0), dict(neighbors=None, nnz=0), dict(iters=-1), dict(iters=1025),
               dict(lam=0.0), dict(lam=-0.5), dict(lam=1.0001), dict(lam=NAN), dict(lam=INF), dict(mu=0.001), dict(mu=-2.001),
               dict(mu=NAN), dict(mu=-INF), dict(mu=INF)):
        assert call(**kw) == INVALID_ARG, kw
    for kw in (dict(n=1 << 31), dict(nnz=1 << 31), dict(n=1 << 40)):
        assert call(**kw) == UNSUPPORTED, kw
    for out in ("verts_out", "ws"):
        for other in names:
            if other != out:
                assert call(**{out: bufs.ptr[other]}) == INVALID_ARG, (out, other)
    assert call(verts_out=bufs.ptr["neighbors"] + 4 * nnz - 1) == INVALID_ARG
    assert call(verts_out=bufs.ptr["neighbors"] + 4 * nnz, ws=None) == WORKSPACE
    assert call(verts_out=bufs.ptr["vflags"], fix=0, vflags=None, ws=None) == WORKSPACE   # vflags is not a buffer of that call
    assert call(verts_out=bufs.ptr["vflags"], fix=0, ws=None) == WORKSPACE
    for kw in (dict(ws=None), dict(nbytes=nws - 1), dict(nbytes=0), dict(ws=bufs.ptr["ws"] + 8), dict(n=0, nnz=0, ws=None),
               dict(lam=1.0, mu=0.0, iters=0, ws=None), dict(mu=-2.0, iters=1024, ws=None)):
        assert call(**kw) == WORKSPACE, kw
    assert call(ws=None, n=1 << 31) == UNSUPPORTED                  # precedence
    assert call(ws=None, n=1 << 31, lam=2.0) == INVALID_ARG
    assert call(ws=None, verts_out=bufs.ptr["verts"]) == INVALID_ARG


def test_normals_rejections_need_no_gpu(L):
    n_inc = 3 * NF
    names = ["verts", "faces", "face_offsets", "face_ids", "normals"]
    bufs = _Bufs(names, slot=SLOT)

    def call(n=NV, m=NF, n_inc=n_inc, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_mesh_vertex_normals_f32(p["verts"], n, p["faces"], m, p["face_offsets"], p["face_ids"], n_inc, p["normals"],
                                             -1, None)

    for kw in (dict(n=-1), dict(m=-1), dict(n_inc=-1), dict(verts=None), dict(faces=None), dict(face_offsets=None),
               dict(face_ids=None), dict(normals=None), dict(normals=None, n=0), dict(faces=None, m=0)):
        assert call(**kw) == INVALID_ARG, kw
    for kw in (dict(m=TOO_MANY_FACES), dict(n=1 << 31), dict(n_inc=1 << 31)):
        assert call(**kw) == UNSUPPORTED, kw
    assert call(m=TOO_MANY_FACES, normals=None) == INVALID_ARG
    for other in names[:-1]:
        assert call(normals=bufs.ptr[other]) == INVALID_ARG, other
    assert call(normals=bufs.ptr["face_ids"] + 4 * n_inc - 1) == INVALID_ARG
    assert call(normals=bufs.ptr["verts"] - 12 * NV + 1) == INVALID_ARG
    assert call(normals=bufs.ptr["verts"], m=TOO_MANY_FACES) == UNSUPPORTED


def test_workspace_queries(L):
    for n, m in [(0, 0), (1, 1), (255, 255), (256, 256), (257, 257), (14832, 15879), (0, 7), (7, 0), (1 << 20, 1 << 21),
                 ((1 << 31) - 1, TOO_MANY_FACES - 1)]:
        assert L.ctd_mesh_adjacency_workspace_bytes(n, m) == adjacency_workspace_bytes(n, m) > 0, (n, m)
        assert L.ctd_mesh_smooth_workspace_bytes(n) == (12 * n + 255) // 256 * 256, n
    for n, m in ((-1, 5), (5, -1), (1 << 31, 5), (5, TOO_MANY_FACES), (-(1 << 40), 0), (0, 1 << 62)):
        assert L.ctd_mesh_adjacency_workspace_bytes(n, m) == 0, (n, m)
    for n in (-1, 1 << 31, 1 << 62, -(1 << 62)):
        assert L.ctd_mesh_smooth_workspace_bytes(n) == 0, n


# ---------------------------------------------------------------------------------------------------------------------
# 3. the Python module
# ---------------------------------------------------------------------------------------------------------------------
def test_meshsmooth_imports_without_a_gpu_and_leaves_the_other_modules_alone():
    code = ("import sys\n"
            "from connecting_the_dots_amd import torchext as te, mesh, meshops, mesheval, meshcolor\n"
            "mods = (te, te.functions, mesh, meshops, mesheval, meshcolor)\n"
            "before = [sorted(vars(m)) for m in mods]\n"
            "n_all = len(te.functions.__all__)\n"
            "from connecting_the_dots_amd import meshsmooth\n"
            "assert [sorted(vars(m)) for m in mods] == before\n"
            "assert len(te.functions.__all__) == n_all\n"
            "assert not hasattr(te, 'mesh_smooth') and not hasattr(meshops, 'mesh_smooth')\n"
            "import torch\n"
            "assert not torch.cuda.is_initialized()\n"
            "print(sorted(n for n in vars(meshsmooth) if not n.startswith('_') and "
            "(n.isupper() or getattr(getattr(meshsmooth, n), '__module__', '') == meshsmooth.__name__)))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == str(["BOUNDARY", "MAX_INCIDENT", "MeshAdjacency", "NONMANIFOLD", "REFERENCED", "mesh_smooth",
                                    "smooth_tsdf_mesh", "vertex_normals"])


def test_python_signatures_docstrings_and_host_side_errors():
    from connecting_the_dots_amd import mesh, meshsmooth as ms

    def params(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    assert (ms.REFERENCED, ms.BOUNDARY, ms.NONMANIFOLD, ms.MAX_INCIDENT) == (1, 2, 4, 1024)
    assert params(ms.MeshAdjacency) == [("faces", E), ("n_verts", E)]
    assert params(ms.MeshAdjacency.matches) == [("self", E), ("faces", E), ("n_verts", E)]
    assert params(ms.mesh_smooth) == [("verts", E), ("faces", E), ("iters", 10), ("lam", 0.5), ("mu", -0.53), ("fix_boundary", True),
                                      ("adjacency", None)]
    assert params(ms.vertex_normals) == [("verts", E), ("faces", E), ("adjacency", None)]
    assert params(ms.smooth_tsdf_mesh) == [("m", E), ("iters", 10), ("lam", 0.5), ("mu", -0.53), ("fix_boundary", True),
                                           ("recompute_normals", True)]
    for obj in (ms.MeshAdjacency, ms.mesh_smooth, ms.vertex_normals):
        for phrase in ("synchronisation", "in ascending face index", "x + f * (m - x)", "three NaNs", "The same bits on every run"):
            assert phrase in obj.__doc__, phrase
    verts, faces = torch.zeros(5, 3), torch.zeros((4, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="mesh_smooth: verts must be a CUDA tensor"):   # no CPU path
        ms.mesh_smooth(verts, faces)
    with pytest.raises(RuntimeError, match="vertex_normals: verts must be a CUDA tensor"):
        ms.vertex_normals(verts, faces)
    with pytest.raises(RuntimeError, match="MeshAdjacency: faces must be a CUDA tensor"):
        ms.MeshAdjacency(faces, 5)
    with pytest.raises(RuntimeError, match="MeshAdjacency: faces must be a tensor"):
        ms.MeshAdjacency(faces.numpy(), 5)
    with pytest.raises(RuntimeError, match="smooth_tsdf_mesh: m must be a mesh.TsdfMesh"):
        ms.smooth_tsdf_mesh((verts, faces))
    empty = mesh.TsdfMesh(verts[:0], torch.zeros(0, dtype=torch.int64), None, faces[:0], torch.zeros(0, dtype=torch.int64),
                          torch.zeros(0, dtype=torch.int64), [])
    for bad in (-1, 1025, 1.0, None, True, "3"):
        with pytest.raises(RuntimeError, match=r"smooth_tsdf_mesh: iters must be an integer in \[0, 1024\]"):
            ms.smooth_tsdf_mesh(empty, iters=bad)
    for bad in (0, 0.0, -0.5, 1.5, NAN, INF, None, True, "1"):
        with pytest.raises(RuntimeError, match="smooth_tsdf_mesh: lam must be a finite number"):
            ms.smooth_tsdf_mesh(empty, lam=bad)
    for bad in (0.1, -2.5, NAN, -INF, None, False, "0"):
        with pytest.raises(RuntimeError, match="smooth_tsdf_mesh: mu must be a finite number"):
            ms.smooth_tsdf_mesh(empty, mu=bad)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(RuntimeError, match="smooth_tsdf_mesh: fix_boundary must be True or False"):
            ms.smooth_tsdf_mesh(empty, fix_boundary=bad)
        with pytest.raises(RuntimeError, match="smooth_tsdf_mesh: recompute_normals must be True or False"):
            ms.smooth_tsdf_mesh(empty, recompute_normals=bad)
    out = ms.smooth_tsdf_mesh(empty, mu=0, lam=1, iters=0)          # no track: nothing is launched
    assert out.verts.shape == (0, 3) and out.faces.shape == (0, 3) and out.normals is None and out._counts == []


# ---------------------------------------------------------------------------------------------------------------------
# 4. the restatement against hand-made meshes with known answers
# ---------------------------------------------------------------------------------------------------------------------
def rings(adj):
    o, nb = adj["offsets"], adj["neighbors"]
    return [nb[o[i]:o[i + 1]].tolist() for i in range(len(o) - 1)]


def incident(adj):
    o, ids = adj["face_offsets"], adj["face_ids"]
    return [ids[o[i]:o[i + 1]].tolist() for i in range(len(o) - 1)]


def test_a_tetrahedron_is_closed_with_euler_2():
    adj = msr.adjacency(msr.TETRA, 5)                               # vertex 4 is unreferenced
    assert adj["counts"].tolist() == [12, 6, 0, 0, 3, 4]
    assert rings(adj) == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], []]
    assert incident(adj) == [[0, 1, 3], [0, 1, 2], [0, 2, 3], [1, 2, 3], []]
    assert adj["vflags"].tolist() == [1, 1, 1, 1, 0] and adj["mult"].tolist() == [2] * 12
    assert msr.topology(adj) == (4, 2, True)
    assert adj["offsets"].dtype == np.int32 and adj["face_ids"].dtype == np.int32 and adj["vflags"].dtype == np.uint8
    # normals of a regular tetrahedron point away from its centre; the unreferenced vertex has none
    verts = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1], [9, 9, 9]], F)
    flip = 1.0 if msr.mesh_volume(verts, msr.TETRA) > 0 else -1.0
    n = msr.vertex_normals(verts, msr.TETRA, adj["face_offsets"], adj["face_ids"])
    assert np.allclose(n[:4] * flip, verts[:4] / np.sqrt(3), atol=1e-6) and np.isnan(n[4]).all()


def test_two_tetrahedra_that_share_a_vertex():
    second = np.where(msr.TETRA == 0, 3, msr.TETRA + 4).astype(np.int32)    # vertices 3, 5, 6, 7
    adj = msr.adjacency(np.concatenate([msr.TETRA, second]), 8)
    assert adj["counts"].tolist() == [24, 12, 0, 0, 6, 8]
    assert rings(adj)[3] == [0, 1, 2, 5, 6, 7] and incident(adj)[3] == [1, 2, 3, 4, 5, 7] and rings(adj)[4] == []
    assert msr.topology(adj) == (7, 3, True)                        # 7 - 12 + 8: two spheres pinched at a vertex


def test_a_3_by_3_grid_patch_has_one_free_vertex():
    verts, faces = msr.grid_patch(3, 3)
    adj = msr.adjacency(faces, 9)
    assert adj["counts"].tolist() == [32, 16, 8, 0, 6, 8] and msr.topology(adj) == (9, 1, False)
    assert adj["vflags"].tolist() == [3, 3, 3, 3, 1, 3, 3, 3, 3]     # the centre is the only vertex not on the boundary
    assert rings(adj)[4] == [0, 1, 3, 5, 7, 8] and rings(adj)[0] == [1, 3, 4] and rings(adj)[2] == [1, 5]
    verts[4] = [1.5, 0.75, 3.0]
    out = msr.smooth_pass(verts, adj["offsets"], adj["neighbors"], 32, adj["vflags"], 0.5, True)
    assert np.array_equal(np.delete(out, 4, 0), np.delete(verts, 4, 0))
    assert out[4].tolist() == [1.25, 0.875, 1.5]                    # halfway to the ring's mean (1, 1, 0)
    free = msr.smooth_pass(verts, adj["offsets"], adj["neighbors"], 32, adj["vflags"], 1.0, False)
    assert free[0].tolist() == [F(2.5) / F(3), F(1.75) / F(3), 1.0] and free[4].tolist() == [1.0, 1.0, 0.0]
    n = msr.vertex_normals(msr.grid_patch(3, 3)[0], faces, adj["face_offsets"], adj["face_ids"])
    assert np.array_equal(n, np.tile(np.array([0, 0, 1], F), (9, 1)))
    # iters = 0 is a copy; mu = 0 runs one pass per iteration
    a = (verts, adj["offsets"], adj["neighbors"], adj["vflags"])
    assert np.array_equal(msr.smooth(*a, iters=0), verts)
    assert np.array_equal(msr.smooth(*a, iters=1, lam=0.5, mu=0.0), out)


def test_a_face_repeated_three_times_is_non_manifold():
    adj = msr.adjacency(np.array([[0, 1, 2]] * 3 + [[2, 1, 3]], np.int32), 4)
    assert adj["counts"].tolist() == [10, 5, 2, 3, 4, 4]            # {0,1}, {0,2} three times; {1,2} four; {1,3}, {2,3} once
    assert adj["vflags"].tolist() == [5, 7, 7, 3] and rings(adj) == [[1, 2], [0, 2, 3], [0, 1, 3], [1, 2]]
    assert incident(adj) == [[0, 1, 2], [0, 1, 2, 3], [0, 1, 2, 3], [3]]
    assert adj["mult"].tolist() == [3, 3, 3, 4, 1, 3, 4, 1, 1, 1]


def test_faces_with_repeated_and_out_of_range_indices_are_invalid():
    faces = np.array([[0, 1, 2], [3, 3, 4], [3, 4, 3], [5, 4, 4], [6, 7, -1], [6, 8, 7], [6, 7, 1 << 30], [8, 6, 7],
                      [-2147483648, 0, 1], [2147483647, 0, 1]], np.int32)
    adj = msr.adjacency(faces, 8)                                   # vertex 8 is out of range
    assert adj["counts"].tolist() == [6, 3, 3, 0, 1, 1] and incident(adj)[:3] == [[0], [0], [0]] and rings(adj)[3:] == [[]] * 5
    adj = msr.adjacency(faces, 9)
    assert adj["counts"].tolist() == [12, 6, 3, 0, 2, 3] and incident(adj)[6] == [5, 7] and rings(adj)[8] == [6, 7]
    assert adj["vflags"].tolist() == [3, 3, 3, 0, 0, 0, 1, 1, 1]     # the triangle (6, 7, 8) twice: no boundary
    none = msr.adjacency(np.zeros((0, 3), np.int32), 0)
    assert none["counts"].tolist() == [0] * 6 and none["offsets"].tolist() == [0] and msr.topology(none) == (0, 0, True)
    # a damaged adjacency: what the rule does not accept is skipped
    verts, g = msr.grid_patch(3, 3)
    adj = msr.adjacency(g, 9)
    verts[4] = [1.5, 0.75, 3.0]
    nb = adj["neighbors"].copy()
    nb[adj["offsets"][4]] = 99                                      # vertex 0 leaves the ring of the centre
    out = msr.smooth_pass(verts, adj["offsets"], nb, 32, adj["vflags"], 1.0, True)
    assert out[4].tolist() == [F(6) / F(5), F(6) / F(5), 0.0]
    off = adj["offsets"].copy()
    off[5] = off[4] - 1                                             # the row of 4 decreases: empty; the row of 5 stays usable
    assert np.array_equal(msr.smooth_pass(verts, off, adj["neighbors"], 32, adj["vflags"], 1.0, True), verts)
    assert np.array_equal(msr.smooth_pass(verts, adj["offsets"], adj["neighbors"], 18, adj["vflags"], 1.0, True), verts)   # past nnz
    bad = verts.copy()
    bad[0, 0] = np.nan                                              # spreads to the ring of 0 and nowhere else
    out = msr.smooth_pass(bad, adj["offsets"], adj["neighbors"], 32, adj["vflags"], 0.5, False)
    assert np.nonzero(np.isnan(out).any(1))[0].tolist() == [0, 1, 3, 4] and np.isnan(out[:, 1:]).sum() == 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. the restatement against the truth
# ---------------------------------------------------------------------------------------------------------------------
def cleaned_fixture(kind, seed):
    sc = fused_scene(kind, seed, masked=True)
    faces, _ = mr.faces(sc["tsdf"], sc["weight"])
    return sc, faces


@pytest.mark.parametrize("kind,seed", sorted(MEASURED_MEDIAN_RATIO))
def test_smoothing_moves_the_noisy_meshes_towards_the_true_surfaces(kind, seed):
    """10 x (0.5 | -0.53), boundary held, on the mesh cleaned with min_faces = 32: after / before of the median distance to
    the true surfaces 0.591 (noisy, 5), 0.565 (noisy, 6), asserted at most halfway to 1; 0.987 (clean, 5), where the ratio
    may not exceed 1 by more than the measured |1 - ratio| plus 0.05"""
    sc, faces = cleaned_fixture(kind, seed)
    c = mcr.clean(faces, len(sc["points"]), min_faces=32)
    verts = sc["points"][c["vert_index"]]
    adj = msr.adjacency(c["faces"], len(verts))
    out = msr.smooth(verts, adj["offsets"], adj["neighbors"], adj["vflags"], 10, 0.5, -0.53, True)
    d0, d1 = tr.scene_surface_distance(verts), tr.scene_surface_distance(out)
    ratio = np.median(d1) / np.median(d0)
    print("%s, seed %d: %d vertices, %d faces, %d boundary edges; median %.3e -> %.3e, ratio %.3f; mean %.3e -> %.3e, ratio %.3f"
          % (kind, seed, len(verts), len(c["faces"]), adj["counts"][2], np.median(d0), np.median(d1), ratio, d0.mean(), d1.mean(),
             d1.mean() / d0.mean()))
    fixed = adj["vflags"] & msr.BOUNDARY != 0
    assert fixed.any() and np.array_equal(out[fixed], verts[fixed]) and not np.array_equal(out[~fixed], verts[~fixed])
    measured = MEASURED_MEDIAN_RATIO[(kind, seed)]
    if kind == "noisy":
        assert ratio <= 0.5 * (measured + 1)
    else:
        assert ratio <= 1 + abs(1 - measured) + 0.05


def test_smoothing_a_noisy_sphere_keeps_its_volume():
    """rms radial error 0.00990 -> 0.00454, ratio 0.459 (asserted at most halfway to 1); volume 1.0070 of the clean sphere's
    (asserted within 2 %); plain Laplacian smoothing shrinks it to 0.841"""
    verts, faces = msr.noisy_icosphere(0.01, 0)
    clean, _ = msr.icosphere()
    adj = msr.adjacency(faces, len(verts))
    assert len(verts) == 642 and adj["counts"].tolist() == [3840, 1920, 0, 0, 6, 1280] and msr.topology(adj) == (642, 2, True)
    out = msr.smooth(verts, adj["offsets"], adj["neighbors"], adj["vflags"], 10, 0.5, -0.53, True)

    def rms(p):
        return np.sqrt(((np.linalg.norm(p.astype(np.float64), axis=1) - 1) ** 2).mean())

    volume = msr.mesh_volume(out, faces) / msr.mesh_volume(clean, faces)
    shrunk = msr.mesh_volume(msr.smooth(verts, adj["offsets"], adj["neighbors"], adj["vflags"], 10, 0.5, 0.0, True), faces)
    print("rms radial error %.5f -> %.5f, ratio %.3f; volume %.4f; with mu = 0: %.4f"
          % (rms(verts), rms(out), rms(out) / rms(verts), volume, shrunk / msr.mesh_volume(clean, faces)))
    assert rms(out) / rms(verts) <= 0.5 * (MEASURED_SPHERE_RMS_RATIO + 1)
    assert abs(volume - 1) <= 0.02
    assert shrunk / msr.mesh_volume(clean, faces) < 0.9
    # the normals of the smoothed sphere point outwards
    n = msr.vertex_normals(out, faces, adj["face_offsets"], adj["face_ids"])
    assert ((n * out).sum(1) > 0.99 * np.linalg.norm(out, axis=1)).all()


@pytest.mark.parametrize("kind,seed", [("clean", 5), ("noisy", 6)])
def test_recomputed_normals_agree_with_the_tsdf_gradients_and_exist_everywhere(kind, seed):
    """on the fixture mesh before clean-up: the dot product with the finite TSDF normals is positive for every referenced
    vertex, and the recomputed normal is finite for every referenced vertex whose faces are not all of zero area"""
    sc, faces = cleaned_fixture(kind, seed)
    pts, grad = sc["points"], sc["normals"]
    adj = msr.adjacency(faces, len(pts))
    n = msr.vertex_normals(pts, faces, adj["face_offsets"], adj["face_ids"])
    referenced = adj["vflags"] & msr.REFERENCED != 0
    p = pts.astype(np.float64)[faces]
    area = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    has_area = np.zeros(len(pts), bool)
    has_area[faces[area > 0].reshape(-1)] = True
    finite, grad_finite = np.isfinite(n).all(1), np.isfinite(grad).all(1)
    both = referenced & finite & grad_finite
    dot = (n[both].astype(np.float64) * grad[both]).sum(1)
    print("%s, seed %d: %d vertices, %d referenced, %d with a face of positive area, %d recomputed normals finite, %d gradients "
          "not finite (%d of them at referenced vertices); dot > 0 for %.2f %%, > 0.9 for %.2f %% of %d"
          % (kind, seed, len(pts), referenced.sum(), has_area.sum(), finite.sum(), (~grad_finite).sum(),
             (~grad_finite & referenced).sum(), 100 * (dot > 0).mean(), 100 * (dot > 0.9).mean(), len(dot)))
    assert finite[referenced & has_area].all() and not finite[~referenced].any()
    assert (~grad_finite & referenced).sum() > 100                  # the rim: vertices that had no normal before
    assert (dot > 0).all() and (dot > 0.9).mean() > 0.9
    assert np.allclose(np.linalg.norm(n[finite].astype(np.float64), axis=1), 1, atol=1e-6)
