"""CPU-only checks of the mesh clean-up (include/ctd_hip_mesh_clean.h: ctd_mesh_components_i32, ctd_mesh_clean_i32;
connecting_the_dots_amd.meshops): the rule's sentences (the header against its ctypes table: tests/test_abi_and_host.py),
argument validation before any HIP call and its precedence, the workspace query, the Python module, and the restatement
tests/meshclean_ref.py against hand-made meshes with known answers and against the truth of the fused scenes.

What removing the components of fewer than 32 faces buys, measured with the restatement on the scenes of
tests/test_tsdf_host.fused_scene meshed by tests/mesh_ref.faces (share of the vertices farther than a voxel from the true
surfaces, tests/tsdf_ref.scene_surface_distance, before -> after; mean distance before -> after):
  clean, seed 5:               2475 vertices, 4522 faces, 5 components (4116, 370, 24, 8, 4 faces)
                               3.11 % -> 1.07 %, ratio 0.345; mean distance 3.05e-03 -> 1.00e-03
  noisy, seed 5, valid=keep:   2551 vertices, 4385 faces, 10 components (4035, 323, 12, 4, 3, 2, ...)
                               3.02 % -> 1.13 %, ratio 0.376; mean distance 4.51e-03 -> 2.85e-03
  noisy, seed 6, valid=keep:   2538 vertices, 4353 faces, 6 components (4058, 277, 8, 4, 4, 2)
                               2.17 % -> 0.93 %, ratio 0.429; mean distance 4.21e-03 -> 2.92e-03
Pinned halfway between the measured ratio and 1.  The largest component holds 91.0 %, 92.0 % and 93.2 % of the faces
(asserted >= 85 %: a scene that has fallen apart would make the ratios meaningless)."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import meshclean_ref as mcr
from tests import tsdf_ref as tr
from tests.test_tsdf_host import _Bufs, fused_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN_HEADER = os.path.join(ROOT, "include", "ctd_hip_mesh_clean.h")

OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, 1, 2, 3
F = np.float32

# (kind, seed) -> the measured after / before of the far share (the docstring above); the pin is halfway to 1
MEASURED_RATIO = {("clean", 5): 0.345, ("noisy", 5): 0.376, ("noisy", 6): 0.429}
MIN_LARGEST_SHARE = 0.85


@pytest.fixture(scope="module")
def L():
    from connecting_the_dots_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header (header == ctypes table == exports: tests/test_abi_and_host.py, for every header)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_rule():
    text = " ".join(open(CLEAN_HEADER).read().replace("*", " ").split())
    for phrase in ("Its three indices lie in [0, n_verts)",
                   "Its three indices are pairwise different",
                   "With drop_degenerate, no two of its vertices have equal positions",
                   "Positions are equal when x, y and z each compare == as f32",
                   "So -0.0 equals 0, and a NaN coordinate equals nothing",
                   "Out-of-range indices are never dereferenced",
                   "a chain of valid faces links them, each sharing a vertex index with the next",
                   "Vertex connectivity is by index, not by position",
                   "A component's label is the smallest vertex index any of its faces uses",
                   "A component's size is the number of its valid faces",
                   "An invalid face has label -1 and size 0",
                   "Its size is at least min_faces",
                   "With keep_largest, its component is the one of largest size",
                   "On a tie that is the one with the smallest label",
                   "min_faces still applies to it",
                   "A vertex is kept when a kept face uses it",
                   "A vertex's new index is the number of kept vertices with a smaller old index",
                   "Kept faces keep their order and their winding, with the indices remapped",
                   "Coincident vertices are not welded",
                   "can therefore open a combinatorial hole of zero size in an otherwise closed mesh",
                   "every output is exact and the same on every run",
                   "counts int64 [4]: kept vertices, kept faces, components, components kept",
                   "always writes the true counts",
                   "with all three NULL the call only counts",
                   "they write every word of the workspace that they read",
                   "Atomics are integer min, add and max only",
                   "No flag that another workgroup waits on: the same bits on every run"):
        assert phrase in text, phrase


# ---------------------------------------------------------------------------------------------------------------------
# 2. validation and workspace
# ---------------------------------------------------------------------------------------------------------------------
NV, NF = 100, 200                                                   # every buffer fits a 4 KiB slot
TOO_MANY_FACES = (1 << 31) // 3 + 1                                 # 3 * n_faces >= 2^31


def clean_workspace_bytes(n, m):
    up = lambda v: (v + 255) // 256 * 256                          # noqa: E731
    chunks = lambda v: (v + 255) // 256                            # noqa: E731
    return 3 * up(4 * n) + up(4 * m) + up(n) + up(m) + up(4 * (chunks(m) + 1)) + up(4 * (chunks(n) + 1)) + 256


def test_clean_rejections_need_no_gpu(L):
    nws = L.ctd_mesh_clean_workspace_bytes(NV, NF)
    assert nws == 3 * 512 + 1024 + 256 + 256 + 256 + 256 + 256      # parent, size, new index; root; flags; offsets; counters
    names = ["faces", "verts", "faces_out", "face_index", "vert_index", "counts", "ws"]
    bufs = _Bufs(names, slot=8192)

    def call(n=NV, m=NF, drop=1, min_faces=1, largest=0, cap_faces=NF, cap_verts=NV, nbytes=None, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_mesh_clean_i32(p["faces"], p["verts"], n, m, drop, min_faces, largest, p["faces_out"], p["face_index"],
                                    cap_faces, p["vert_index"], cap_verts, p["counts"], p["ws"],
                                    nws if nbytes is None else nbytes, -1, None)

    for kw in (dict(n=-1), dict(m=-1), dict(min_faces=0), dict(min_faces=-3), dict(cap_faces=-1), dict(cap_verts=-1),
               dict(faces=None), dict(counts=None), dict(verts=None), dict(faces=None, m=0), dict(counts=None, m=0, n=0)):
        assert call(**kw) == INVALID_ARG, kw
    assert call(cap_faces=-1, faces_out=None) == INVALID_ARG         # face_index still has a capacity
    for kw in (dict(m=TOO_MANY_FACES), dict(n=1 << 31), dict(n=1 << 40), dict(m=1 << 40)):
        assert call(**kw) == UNSUPPORTED, kw
    assert call(m=TOO_MANY_FACES - 1, faces=None) == INVALID_ARG     # (3 * n_faces < 2^31 gets past the sizes)
    for out in ("faces_out", "face_index", "vert_index", "counts", "ws"):
        for other in names:
            if other != out:
                assert call(**{out: bufs.ptr[other]}) == INVALID_ARG, (out, other)
    assert call(faces_out=bufs.ptr["faces"] + 12 * NF - 4) == INVALID_ARG       # the last index of faces
    assert call(counts=bufs.ptr["verts"] + 12 * NV - 1) == INVALID_ARG
    assert call(faces_out=bufs.ptr["verts"] - 1196, cap_faces=100) == INVALID_ARG   # 100 faces end 4 bytes into verts
    assert call(faces_out=bufs.ptr["verts"] - 1200, cap_faces=100, ws=None) == WORKSPACE   # (they end where verts starts)
    assert call(vert_index=bufs.ptr["verts"] - 40, cap_verts=10, ws=None) == WORKSPACE
    assert call(vert_index=bufs.ptr["verts"] - 40, cap_verts=11) == INVALID_ARG
    assert call(vert_index=bufs.ptr["verts"], drop=0, verts=None, ws=None) == WORKSPACE   # verts is not a buffer of that call
    assert call(ws=None) == WORKSPACE                                # workspace missing, short, misaligned
    assert call(nbytes=nws - 1) == WORKSPACE
    assert call(nbytes=0) == WORKSPACE
    assert call(ws=bufs.ptr["ws"] + 8) == WORKSPACE
    assert call(n=0, m=0, ws=None) == WORKSPACE                      # empty meshes still write their counts
    # precedence: INVALID_ARG, then UNSUPPORTED, then the overlaps, then WORKSPACE
    assert call(ws=None, m=TOO_MANY_FACES) == UNSUPPORTED
    assert call(ws=None, m=TOO_MANY_FACES, min_faces=0) == INVALID_ARG
    assert call(ws=None, m=TOO_MANY_FACES, counts=None) == INVALID_ARG
    assert call(ws=None, faces_out=bufs.ptr["verts"]) == INVALID_ARG
    # counting only: the outputs NULL, and then the capacities are not looked at
    assert call(faces_out=None, face_index=None, vert_index=None, cap_faces=-5, cap_verts=-5, nbytes=0) == WORKSPACE
    assert call(faces_out=None, face_index=None, vert_index=None, counts=bufs.ptr["faces"], nbytes=0) == INVALID_ARG
    assert call(drop=0, verts=None, nbytes=0) == WORKSPACE           # verts may be NULL without drop_degenerate


def test_components_rejections_need_no_gpu(L):
    nws = L.ctd_mesh_clean_workspace_bytes(NV, NF)
    names = ["faces", "verts", "label", "size", "n_components", "ws"]
    bufs = _Bufs(names, slot=8192)

    def call(n=NV, m=NF, drop=1, nbytes=None, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_mesh_components_i32(p["faces"], p["verts"], n, m, drop, p["label"], p["size"], p["n_components"], p["ws"],
                                         nws if nbytes is None else nbytes, -1, None)

    for kw in (dict(n=-1), dict(m=-1), dict(faces=None), dict(label=None), dict(size=None), dict(n_components=None),
               dict(verts=None), dict(faces=None, m=0), dict(label=None, m=0)):
        assert call(**kw) == INVALID_ARG, kw
    for kw in (dict(m=TOO_MANY_FACES), dict(n=1 << 31)):
        assert call(**kw) == UNSUPPORTED, kw
    for out in ("label", "size", "n_components", "ws"):
        for other in names:
            if other != out:
                assert call(**{out: bufs.ptr[other]}) == INVALID_ARG, (out, other)
    assert call(label=bufs.ptr["size"] - 4 * NF + 4) == INVALID_ARG
    assert call(label=bufs.ptr["size"] - 4 * NF, ws=None) == WORKSPACE
    assert call(ws=None) == WORKSPACE
    assert call(nbytes=nws - 1) == WORKSPACE
    assert call(ws=bufs.ptr["ws"] + 128) == WORKSPACE
    assert call(drop=0, verts=None, nbytes=0) == WORKSPACE
    assert call(ws=None, m=TOO_MANY_FACES) == UNSUPPORTED
    assert call(ws=None, m=TOO_MANY_FACES, size=None) == INVALID_ARG
    assert call(ws=None, label=bufs.ptr["faces"]) == INVALID_ARG


def test_clean_workspace_query(L):
    for n, m in [(0, 0), (1, 1), (255, 255), (256, 256), (257, 257), (14832, 15879), (0, 7), (7, 0), (1 << 20, 1 << 21),
                 ((1 << 31) - 1, TOO_MANY_FACES - 1)]:
        assert L.ctd_mesh_clean_workspace_bytes(n, m) == clean_workspace_bytes(n, m) > 0, (n, m)
    for n, m in ((-1, 5), (5, -1), (1 << 31, 5), (5, TOO_MANY_FACES), (-(1 << 40), 0), (0, 1 << 62)):
        assert L.ctd_mesh_clean_workspace_bytes(n, m) == 0, (n, m)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the Python module
# ---------------------------------------------------------------------------------------------------------------------
def test_meshops_imports_without_a_gpu_and_leaves_torchext_and_mesh_alone():
    code = ("import sys\n"
            "from connecting_the_dots_amd import torchext as te, mesh\n"
            "before = sorted(n for n in vars(te) if not n.startswith('_'))\n"
            "mesh_before = sorted(vars(mesh))\n"
            "from connecting_the_dots_amd import meshops\n"
            "after = sorted(n for n in vars(te) if not n.startswith('_'))\n"
            "assert before == after, set(after) ^ set(before)\n"
            "assert sorted(vars(mesh)) == mesh_before\n"
            "assert not hasattr(te, 'mesh_clean') and not hasattr(mesh, 'mesh_clean')\n"
            "import torch\n"
            "assert not torch.cuda.is_initialized()\n"
            "print(sorted(n for n in vars(meshops) if not n.startswith('_') and "
            "getattr(getattr(meshops, n), '__module__', '') == meshops.__name__))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == str(["CleanMesh", "clean_tsdf_mesh", "mesh_clean", "mesh_components"])


def test_python_signatures_docstrings_and_host_side_errors():
    from connecting_the_dots_amd import mesh, meshops

    def params(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    assert params(meshops.mesh_components) == [("faces", E), ("n_verts", E), ("verts", None), ("drop_degenerate", False)]
    assert params(meshops.mesh_clean) == [("verts", E), ("faces", E), ("min_faces", 1), ("keep_largest", False),
                                          ("drop_degenerate", True), ("normals", None)]
    assert params(meshops.clean_tsdf_mesh) == [("m", E), ("min_faces", 1), ("keep_largest", False), ("drop_degenerate", True)]
    for fn in (meshops.mesh_components, meshops.mesh_clean):
        for phrase in ("one synchronisation", "smallest vertex index any of its faces uses", "on a tie the one with the smallest label",
                       "The same bits on every run"):
            assert phrase in fn.__doc__, phrase
    verts, faces = torch.zeros(5, 3), torch.zeros((4, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="mesh_clean: verts must be a CUDA tensor"):   # no CPU path
        meshops.mesh_clean(verts, faces)
    with pytest.raises(RuntimeError, match="mesh_components: faces must be a CUDA tensor"):
        meshops.mesh_components(faces, 5)
    with pytest.raises(RuntimeError, match="mesh_components: faces must be a tensor"):
        meshops.mesh_components(faces.numpy(), 5)
    with pytest.raises(RuntimeError, match="clean_tsdf_mesh: m must be a mesh.TsdfMesh"):
        meshops.clean_tsdf_mesh((verts, faces))
    empty = mesh.TsdfMesh(verts[:0], torch.zeros(0, dtype=torch.int64), None, faces[:0], torch.zeros(0, dtype=torch.int64),
                          torch.zeros(0, dtype=torch.int64), [])
    for bad in (0, -1, 1.0, None, True, "3"):
        with pytest.raises(RuntimeError, match="clean_tsdf_mesh: min_faces must be an integer >= 1"):
            meshops.clean_tsdf_mesh(empty, min_faces=bad)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(RuntimeError, match="clean_tsdf_mesh: keep_largest must be True or False"):
            meshops.clean_tsdf_mesh(empty, keep_largest=bad)
        with pytest.raises(RuntimeError, match="clean_tsdf_mesh: drop_degenerate must be True or False"):
            meshops.clean_tsdf_mesh(empty, drop_degenerate=bad)
    out = meshops.clean_tsdf_mesh(empty)                            # no track: nothing is launched
    assert out.verts.shape == (0, 3) and out.faces.shape == (0, 3) and out.normals is None and out._counts == []


# ---------------------------------------------------------------------------------------------------------------------
# 4. the restatement against hand-made meshes with known answers
# ---------------------------------------------------------------------------------------------------------------------
TETRA = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int32)


def test_two_tetrahedra_that_share_no_vertex():
    faces = np.concatenate([TETRA + 4, TETRA])                      # the second one holds the smaller indices
    label, size, n = mcr.components(faces, 8)
    assert label.tolist() == [4] * 4 + [0] * 4 and size.tolist() == [4] * 8 and n == 2
    c = mcr.clean(faces, 10)                                        # vertices 8 and 9 are unreferenced
    assert c["counts"].tolist() == [8, 8, 2, 2] and c["vert_index"].tolist() == list(range(8))
    assert np.array_equal(c["faces"], faces) and c["face_index"].tolist() == list(range(8))
    assert mcr.clean(faces, 8, min_faces=5)["counts"].tolist() == [0, 0, 2, 0]
    # a fifth face on the first makes it the largest; the kept faces keep their order and winding
    more = np.concatenate([faces, [[4, 5, 8]]]).astype(np.int32)
    c = mcr.clean(more, 10, keep_largest=True)
    assert c["counts"].tolist() == [5, 5, 2, 1] and c["vert_index"].tolist() == [4, 5, 6, 7, 8]
    assert c["face_index"].tolist() == [0, 1, 2, 3, 8] and c["faces"].tolist() == TETRA.tolist() + [[0, 1, 4]]
    c = mcr.clean(more, 10, min_faces=5)
    assert c["counts"].tolist() == [5, 5, 2, 1] and c["face_index"].tolist() == [0, 1, 2, 3, 8]
    assert mcr.clean(more, 10, min_faces=6, keep_largest=True)["counts"].tolist() == [0, 0, 2, 0]   # min_faces still applies


def test_two_tetrahedra_that_share_one_vertex_are_one_component():
    second = np.where(TETRA == 0, 3, TETRA + 4).astype(np.int32)    # vertices 3, 5, 6, 7
    faces = np.concatenate([second, TETRA])
    label, size, n = mcr.components(faces, 8)
    assert label.tolist() == [0] * 8 and size.tolist() == [8] * 8 and n == 1
    c = mcr.clean(faces, 8, min_faces=8, keep_largest=True)
    assert c["counts"].tolist() == [7, 8, 1, 1] and c["vert_index"].tolist() == [0, 1, 2, 3, 5, 6, 7]
    assert c["faces"].max() == 6 and np.array_equal(c["vert_index"][c["faces"]], faces)


def test_faces_with_repeated_and_out_of_range_indices_are_invalid():
    faces = np.array([[0, 1, 2], [3, 3, 4], [3, 4, 3], [5, 4, 4], [6, 7, -1], [6, 8, 7], [6, 7, 1 << 30], [8, 6, 7],
                      [-2147483648, 0, 1], [2147483647, 0, 1]], np.int32)
    label, size, n = mcr.components(faces, 8)                       # vertex 8 is out of range
    assert label.tolist() == [0, -1, -1, -1, -1, -1, -1, -1, -1, -1] and size.tolist() == [1] + [0] * 9 and n == 1
    label, size, n = mcr.components(faces, 9)
    assert label.tolist() == [0, -1, -1, -1, -1, 6, -1, 6, -1, -1] and size.tolist() == [1, 0, 0, 0, 0, 2, 0, 2, 0, 0] and n == 2
    c = mcr.clean(faces, 9, min_faces=2)
    assert c["counts"].tolist() == [3, 2, 2, 1] and c["faces"].tolist() == [[0, 2, 1], [2, 0, 1]]
    assert c["vert_index"].tolist() == [6, 7, 8] and c["face_index"].tolist() == [5, 7]
    # invalid faces link nothing: (3, 3, 4) does not join vertex 3 to vertex 4
    assert mcr.components(np.array([[3, 3, 4], [3, 0, 1], [4, 5, 6]], np.int32), 7)[0].tolist() == [-1, 0, 4]
    assert mcr.clean(faces[1:5], 8)["counts"].tolist() == [0, 0, 0, 0]
    assert mcr.clean(np.zeros((0, 3), np.int32), 0)["counts"].tolist() == [0, 0, 0, 0]


def test_coincident_positions_under_different_indices():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-0.0, 0, 0.0], [np.nan, 0, 0], [np.nan, 0, 0], [1, 1, 1]], F)
    faces = np.array([[0, 1, 2], [0, 3, 1], [3, 1, 2], [4, 5, 6], [1, 2, 6]], np.int32)
    assert mcr.valid_faces(faces, 7).all()
    # -0.0 equals 0: (0, 3, 1) has two vertices at one position; a NaN coordinate equals nothing: (4, 5, 6) stays
    assert mcr.valid_faces(faces, 7, verts, True).tolist() == [True, False, True, True, True]
    label, size, n = mcr.components(faces, 7, verts, True)
    assert label.tolist() == [0, -1, 0, 0, 0] and size.tolist() == [4, 0, 4, 4, 4] and n == 1
    # connectivity is by index: vertices 0 and 3 coincide, and (0, 1, 2), (3, 4, 5) share no index
    apart = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    assert mcr.components(apart, 7, verts, True)[0].tolist() == [0, 3]
    c = mcr.clean(faces, 7, verts, drop_degenerate=True)
    assert c["counts"].tolist() == [7, 4, 1, 1] and c["face_index"].tolist() == [0, 2, 3, 4]
    assert mcr.clean(faces, 7, verts, drop_degenerate=False)["counts"].tolist() == [7, 5, 1, 1]


def test_a_tie_for_the_largest_component_goes_to_the_smaller_label():
    faces = np.concatenate([TETRA + 5, TETRA + 1, [[9, 10, 11]]]).astype(np.int32)
    label, size, n = mcr.components(faces, 12)
    assert label.tolist() == [5] * 4 + [1] * 4 + [9] and n == 3
    c = mcr.clean(faces, 12, keep_largest=True)
    assert c["counts"].tolist() == [4, 4, 3, 1] and c["face_index"].tolist() == [4, 5, 6, 7]
    assert c["vert_index"].tolist() == [1, 2, 3, 4] and c["faces"].tolist() == TETRA.tolist()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the restatement against the truth
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,seed", sorted(MEASURED_RATIO))
def test_removing_small_components_removes_the_far_vertices(kind, seed):
    """min_faces = 32 over the mesh of the fused scene: after / before of the share of the vertices farther than a voxel
    from the true surfaces 0.345 (clean, 5), 0.376 (noisy, 5), 0.429 (noisy, 6); asserted at most halfway to 1"""
    sc = fused_scene(kind, seed, masked=True)
    faces, _ = mr.faces(sc["tsdf"], sc["weight"])
    pts = sc["points"]
    d = tr.scene_surface_distance(pts)
    c = mcr.clean(faces, len(pts), min_faces=32)
    sizes = sorted((int(s) for s in np.unique(c["label"][c["label"] >= 0], return_counts=True)[1]), reverse=True)
    kept = c["vert_index"]
    far_before, far_after = (d > sc["voxel"]).mean(), (d[kept] > sc["voxel"]).mean()
    ratio = far_after / far_before
    print("%s, seed %d: %d vertices, %d faces, %d components %s; kept %d vertices, %d faces in %d components; far share "
          "%.2f %% -> %.2f %%, ratio %.3f; mean distance %.2e -> %.2e; largest component %.1f %% of the faces"
          % (kind, seed, len(pts), len(faces), c["counts"][2], sizes[:6], c["counts"][0], c["counts"][1], c["counts"][3],
             100 * far_before, 100 * far_after, ratio, d.mean(), d[kept].mean(), 100 * sizes[0] / len(faces)))
    assert sizes[0] >= MIN_LARGEST_SHARE * len(faces)
    assert ratio <= 0.5 * (MEASURED_RATIO[(kind, seed)] + 1)
    assert d[kept].mean() < d.mean()
