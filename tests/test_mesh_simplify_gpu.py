"""GPU parity of the mesh simplification (meshsimplify.mesh_simplify, simplify_tsdf_mesh; ctd_mesh_simplify_f32 of
include/ctd_hip_mesh_simplify.h) against the restatement tests/meshsimplify_ref.py.

Clusters, kept faces and counts are integer work, so they equal the restatement exactly; the quadrics, the means and the
solve use IEEE + - * / in f64 in the rule's order, so verts_out equals it bit for bit (NaNs compared as NaNs): a mismatch
is an ordering bug on one side.  Every C call runs twice with equal bits, from a workspace and outputs filled with
sentinels, leaves its inputs as they were and writes nothing past the true counts or past a capacity."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import meshsimplify_ref as sr
from tests import meshsmooth_ref as msr
from tests.test_mesh_smooth_gpu import hand_cases                  # the hand-made meshes of the smoothing test
from tests.test_tsdf_host import fused_scene

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0xA5
PAD = 8                                                           # entries past every output that must stay as they were
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def mp():
    from connecting_the_dots_amd import meshsimplify
    return meshsimplify


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_f32(a, b):
    """bit for bit, except that a NaN equals any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == F and b.dtype == F and a.shape == b.shape
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _lib():
    from connecting_the_dots_amd import _lib
    return _lib, _lib.lib()


def _some(t, like):
    """an empty array still gets a pointer (nothing is read through it)"""
    return dev(t) if t.size else torch.zeros(like, dtype=torch.from_numpy(t).dtype, device="cuda")


def bumpy(verts, seed=1, sigma=0.1):
    return (verts + np.random.RandomState(seed).normal(0, sigma, verts.shape)).astype(F)


def simplify_c_call(verts, faces, face_offsets, face_ids, origin, cell, reg, dd, cap_verts=None, cap_faces=None, n_incident=None):
    """ctd_mesh_simplify_f32, twice -> dict of host arrays, -7 where nothing was written"""
    lib, L = _lib()
    n, m = len(verts), len(faces)
    cap_verts = n if cap_verts is None else cap_verts
    cap_faces = m if cap_faces is None else cap_faces
    n_incident = len(face_ids) if n_incident is None else n_incident
    x, f, fo, fi = _some(verts, (1, 3)), _some(faces, (1, 3)), dev(face_offsets), _some(face_ids, (1,))
    ins = [x, f, fo, fi]
    before = [t.clone() for t in ins]
    nws = L.ctd_mesh_simplify_workspace_bytes(n, m)
    assert nws > 0
    o = [float(F(v)) for v in origin]
    runs = []
    for _ in range(2):
        ws = torch.full((nws,), SENTINEL, dtype=torch.uint8, device="cuda")
        out = dict(verts=torch.full((n + PAD, 3), -7.0, dtype=torch.float32, device="cuda"),
                   leader=torch.full((n + PAD,), -7, dtype=torch.int32, device="cuda"),
                   vert_cluster=torch.full((n + PAD,), -7, dtype=torch.int32, device="cuda"),
                   faces=torch.full((m + PAD, 3), -7, dtype=torch.int32, device="cuda"),
                   face_index=torch.full((m + PAD,), -7, dtype=torch.int32, device="cuda"),
                   counts=torch.full((9,), -7, dtype=torch.int64, device="cuda"))
        st = L.ctd_mesh_simplify_f32(x.data_ptr(), n, f.data_ptr(), m, fo.data_ptr(), fi.data_ptr(), n_incident, o[0], o[1], o[2],
                                     float(F(cell)), float(reg), int(dd), out["verts"].data_ptr(), out["leader"].data_ptr(),
                                     cap_verts, out["vert_cluster"].data_ptr(), out["faces"].data_ptr(),
                                     out["face_index"].data_ptr(), cap_faces, out["counts"].data_ptr(), ws.data_ptr(), ws.numel(), 0,
                                     torch.cuda.current_stream().cuda_stream)
        lib.check(st, "ctd_mesh_simplify_f32")
        runs.append({k: host(v) for k, v in out.items()})
    for k in runs[0]:
        if k == "verts":
            assert same_f32(runs[0][k], runs[1][k]), "two runs differ in verts"
        else:
            assert np.array_equal(runs[0][k], runs[1][k]), "two runs differ in " + k
    for t, t0 in zip(ins, before):
        assert torch.equal(t.view(torch.int32), t0.view(torch.int32)), "an input was written"
    r = runs[0]
    assert r["counts"][8] == -7 and (r["vert_cluster"][n:] == -7).all()
    return r


def check_against(got, want, what, cap_verts=None, cap_faces=None):
    """the outputs of a call against the restatement, below the capacities; nothing past them or past the true counts"""
    nv, k = int(want["counts"][0]), int(want["counts"][1])
    hv = nv if cap_verts is None else min(nv, cap_verts)
    hf = k if cap_faces is None else min(k, cap_faces)
    n = len(want["vert_cluster"])
    assert got["counts"][:8].tolist() == want["counts"].tolist(), "%s: counts %s vs %s" % (what, got["counts"], want["counts"])
    assert np.array_equal(got["vert_cluster"][:n], want["vert_cluster"]), what + ": vert_cluster"
    assert np.array_equal(got["leader"][:hv], want["leader"][:hv]) and (got["leader"][hv:] == -7).all(), what + ": leader"
    assert np.array_equal(got["faces"][:hf], want["faces"][:hf]) and (got["faces"][hf:] == -7).all(), what + ": faces"
    assert np.array_equal(got["face_index"][:hf], want["face_index"][:hf]) and (got["face_index"][hf:] == -7).all(), what
    assert same_f32(got["verts"][:hv], want["verts"][:hv]), what + ": verts"
    assert (got["verts"][hv:] == -7).all(), what + ": verts past the count"


def check_simplify(verts, faces, origin, cell, what, regs=(1e-3,), dds=(True,), rows=None, capacities=True, n_incident=None):
    """the full call and a call at half the capacities against the restatement -> the restatement's dict of the last setting"""
    verts, faces = np.ascontiguousarray(verts, F), np.ascontiguousarray(faces, np.int32)
    if rows is None:
        adj = msr.adjacency(faces, len(verts))
        rows = adj["face_offsets"], adj["face_ids"]
    want = None
    for reg in regs:
        for dd in dds:
            want = sr.simplify(verts, faces, rows[0], rows[1], origin, cell, reg, dd, n_incident)
            tag = "%s: reg %g drop_duplicates %s" % (what, reg, dd)
            check_against(simplify_c_call(verts, faces, rows[0], rows[1], origin, cell, reg, dd, n_incident=n_incident), want, tag)
            if capacities:
                hv, hf = int(want["counts"][0]) // 2, int(want["counts"][1]) // 2
                half = simplify_c_call(verts, faces, rows[0], rows[1], origin, cell, reg, dd, hv, hf, n_incident)
                check_against(half, want, tag + " at half the capacities", hv, hf)
    return want


# ---------------------------------------------------------------------------------------------------------------------
# hand-made meshes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_made_meshes(name):
    faces, n = hand_cases()[name]
    verts = np.random.RandomState(5).randn(n, 3).astype(F)
    for cell in (0.5, 8.0):                                        # nearly every vertex its own cell; all in one
        want = check_simplify(verts, faces, (-4, -4, -4), cell, "%s, cell %g" % (name, cell), regs=(1e-3, 0.0), dds=(True, False))
        if name == "tetrahedron" and cell == 8.0:
            assert want["counts"].tolist() == [0, 0, 1, 0, 4, 0, 0, 4]
        if name in ("no faces", "nothing", "no vertices", "all invalid"):
            assert want["counts"].tolist() == [0, 0, 0, len(faces), 0, 0, 0, 0]
    if name == "a face three times":
        want = check_simplify(verts * F(4), faces, (-16, -16, -16), 0.5, name)
        assert want["counts"].tolist() == [4, 2, 4, 0, 0, 2, 0, 1] and want["face_index"].tolist() == [0, 3]


def test_the_restatements_known_answers_on_the_gpu():
    from tests.test_mesh_simplify_host import TETRA_VERTS
    want = check_simplify(TETRA_VERTS * F(8), msr.TETRA, (0, 0, 0), 1.0, "own cells")
    assert want["verts"].tobytes() == (TETRA_VERTS * F(8))[:4].tobytes()
    verts, faces = sr.cube_corner()
    check_simplify(verts, faces, (-0.3125,) * 3, 0.5, "cube corner", regs=(1e-3, 1e-9, 1.0))
    verts, faces = msr.grid_patch(17, 13)
    verts[:, 2] = F(0.5) * verts[:, 0] + F(0.25) * verts[:, 1] + F(3)
    check_simplify(verts, faces, (0, 0, 0), 4.0, "tilted plane", regs=(1e-3, 1e-6, 1.0))


def test_vertices_with_nan_inf_and_cells_out_of_range():
    verts, faces = msr.grid_patch(23, 19)
    verts = bumpy(verts)
    rs = np.random.RandomState(7)
    hit = rs.choice(len(verts), 24, replace=False)
    values = [NAN, INF, -INF, 3e9, -3e9, 3.4e38, -0.75]            # -0.75: a negative cell; 3e9: a cell past 2^20 at cell 2
    for i, v in enumerate(hit):
        verts[v, i % 3] = values[i % len(values)]
    want = check_simplify(verts, faces, (-0.5, -0.5, -0.5), 2.0, "bad coordinates", regs=(1e-3, 1e3))
    assert want["counts"][3] > 24 and (want["vert_cluster"][hit] == -1).all() and np.isfinite(want["verts"]).all()
    edge = msr.grid_patch(4, 4)[0] * F(1 << 18)                    # cells 0, 2^18, 2^19, 3 * 2^18 at cell 1: in range
    check_simplify(edge, msr.grid_patch(4, 4)[1], (0, 0, 0), 1.0, "cells up to 3 * 2^18")
    far = check_simplify(edge * F(2), msr.grid_patch(4, 4)[1], (0, 0, 0), 1.0, "cells up to 3 * 2^19")    # 2^20 is out of range
    assert far["counts"][3] > 0 and far["counts"][0] > 0
    top = np.array([[0, 0, 0], [1048575.5, 3, 0], [5, 1048576.0, 0], [9, 9, 0]], F)    # the last cell in range; the first out
    r = check_simplify(top, np.array([[0, 1, 3], [0, 2, 3]], np.int32), (0, 0, 0), 1.0, "cell 2^20 - 1 and 2^20")
    assert r["counts"].tolist()[:6] == [3, 1, 3, 1, 0, 0] and r["vert_cluster"].tolist() == [0, 1, -1, 2]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_sizes_around_the_chunk(n):
    verts, faces = msr.grid_patch(17, 15) if n == 255 else msr.grid_patch(16, 16)
    verts = np.concatenate([verts, np.ones((n - len(verts), 3), F)])     # 257: one vertex that no face uses
    verts = bumpy(verts)
    want = check_simplify(verts, faces, (-1, -1, -1), 3.0, "n = %d" % n, regs=(1e-3, 0.0))
    assert want["counts"][0] > 20 and want["counts"][7] > 9
    check_simplify(verts, faces, (-1, -1, -1), 0.25, "n = %d, small cells" % n)


def test_one_cell_that_holds_a_16_by_16_grid():
    """a row of 256 members, sorted by the workgroup; every face collapses"""
    verts, faces = msr.grid_patch(16, 16)
    want = check_simplify(bumpy(verts), faces, (-8, -8, -8), 64.0, "16 x 16 in one cell")
    assert want["counts"].tolist() == [0, 0, 1, 0, len(faces), 0, 0, 256]
    two = np.concatenate([bumpy(verts), bumpy(verts, 3) + F(64)])   # a second cell of 256, so that faces between them are kept
    bridge = np.array([[0, 256, 5], [7, 300, 9]], np.int32)
    want = check_simplify(two, np.concatenate([faces, faces + 256, bridge]), (-8, -8, -8), 64.0, "two cells of 256")
    assert want["counts"].tolist()[:3] == [0, 0, 2] and want["counts"][7] == 256


def test_rows_above_and_below_the_4096_members_that_are_sorted_in_lds():
    """three cells of 128: a 72 x 72 patch (5184 members: sorted by the workgroup in global memory, summed in 21 stages of
    256), a 60 x 60 patch (3600: sorted over a copy in LDS) and a 3 x 3 patch (one lane), with faces between the three
    that survive"""
    a, fa = msr.grid_patch(72, 72)
    b, fb = msr.grid_patch(60, 60)
    c, fc = msr.grid_patch(3, 3)
    na, nb = len(a), len(b)
    verts = np.concatenate([bumpy(a, 4), bumpy(b, 5) + np.array([128, 0, 0], F), bumpy(c, 6) + np.array([0, 128, 0], F)]).astype(F)
    bridge = np.array([[0, na, na + nb], [na + nb + 4, na + 7, 5000], [17, na + nb + 8, na + 3599], [na, 0, na + nb]], np.int32)
    faces = np.concatenate([fa, bridge[:2], fb + na, fc + na + nb, bridge[2:]]).astype(np.int32)
    want = check_simplify(verts, faces, (-8, -8, -8), 128.0, "rows of 5184, 3600 and 9 members", regs=(1e-3, 1e3),
                          dds=(True, False))
    assert want["counts"].tolist() == [3, 4, 3, 0, len(faces) - 4, 0, 0, 5184] and want["counts"][7] > 4096
    assert want["leader"].tolist() == [0, na, na + nb] and want["face_index"].tolist() == [len(fa), len(fa) + 1, len(faces) - 2, len(faces) - 1]
    once = sr.simplify_mesh(verts, faces, (-8, -8, -8), 128.0)
    assert once["counts"].tolist()[:6] == [3, 1, 3, 0, len(faces) - 4, 3] and once["face_index"].tolist() == [len(fa)]


def test_the_open_fan_of_1024_in_one_cell_and_in_many():
    verts, faces = msr.open_fan(1024)
    one = check_simplify(verts, faces, (-5, -5, -5), 10.0, "fan of 1024, one cell")
    assert one["counts"].tolist() == [0, 0, 1, 0, 1024, 0, 0, 1026]
    many = check_simplify(verts, faces, (-2, -2, -2), 1.0 / 256, "fan of 1024, many cells", regs=(1e-3, 1e3))
    assert many["counts"].tolist() == [1026, 1024, 1026, 0, 0, 0, 0, 1]
    some = check_simplify(verts, faces, (-2, -2, -2), 0.25, "fan of 1024, some cells", dds=(True, False))
    assert some["counts"][7] > 16 and some["counts"][4] > 0 and some["counts"][1] > 0   # long rows beside short ones


@functools.lru_cache(maxsize=None)
def big_grid():
    verts, faces = msr.grid_patch(520, 520)
    adj = msr.adjacency(faces, len(verts))
    return bumpy(verts, 2, 0.2), faces, (adj["face_offsets"], adj["face_ids"])


def test_a_grid_of_more_chunks_than_one_round_of_the_scan():
    """520 x 520 = 270 400 vertices: 1057 chunks of 256, so the scans of the chunk sums carry; cell = 4 spacings"""
    verts, faces, rows = big_grid()
    assert (len(verts) + 255) // 256 > 1024
    want = check_simplify(verts, faces, (-2, -2, -2), 4.0, "grid 520 x 520", rows=rows, capacities=False)
    assert want["counts"][0] > 16000 and want["counts"][1] > 30000
    hv, hf = 9999, 20001                                           # capacities that end inside a chunk
    half = simplify_c_call(verts, faces, rows[0], rows[1], (-2, -2, -2), 4.0, 1e-3, True, hv, hf)
    check_against(half, want, "grid 520 x 520 at capacities inside a chunk", hv, hf)


def test_the_big_grid_with_every_vertex_in_its_own_cell():
    """a cell of 1/64 spacing: the table holds 270 400 keys, and the output is the input"""
    verts, faces, rows = big_grid()
    want = check_simplify(verts, faces, (-2, -2, -2), 1.0 / 64, "grid 520 x 520, tiny cells", rows=rows, capacities=False)
    assert want["counts"].tolist() == [270400, len(faces), 270400, 0, 0, 0, 0, 1]
    assert np.array_equal(want["faces"], faces)


def test_two_sheets_with_and_without_drop_duplicates():
    verts, faces = sr.two_sheets()
    want = check_simplify(verts, faces, (-0.5, -0.5, -0.5), 2.0, "two sheets", dds=(True, False))
    assert want["counts"][5] == 0 and want["counts"][1] > 0
    once = sr.simplify_mesh(verts, faces, (-0.5, -0.5, -0.5), 2.0)
    assert once["counts"][5] == once["counts"][1] == want["counts"][1] // 2 and (once["face_index"] < len(faces) // 2).all()


def test_random_faces_with_duplicates_and_bad_indices():
    faces = msr.random_faces(300)
    verts = np.random.RandomState(9).randn(300, 3).astype(F)
    for cell in (0.125, 0.7, 2.0):
        want = check_simplify(verts, faces, (-5, -5, -5), cell, "random faces, cell %g" % cell, regs=(1e-3, 0.0), dds=(True, False))
        assert want["counts"][3] > 100
    both = sr.simplify_mesh(verts, faces, (-5, -5, -5), 0.125, drop_duplicates=True)
    assert both["counts"][5] >= 30                                  # the valid ones of the 40 faces that random_faces repeats


@functools.lru_cache(maxsize=None)
def fixture_mesh():
    sc = fused_scene("clean", 5, masked=True)
    faces, _ = mr.faces(sc["tsdf"], sc["weight"])
    return sc["points"], faces, np.asarray(sc["origin"], F).reshape(-1)[:3], float(sc["voxel"])


def test_the_mesh_of_the_fused_scene():
    verts, faces, origin, voxel = fixture_mesh()
    for cells in (2, 4):
        want = check_simplify(verts, faces, origin, cells * voxel, "fused scene, %d voxels" % cells, regs=(0.0, 1e-3, 1e3))
        assert 0 < want["counts"][1] < len(faces) / 2
    assert want["counts"][6] == 0


def test_the_noisy_icosphere():
    verts, faces = msr.noisy_icosphere(0.01, 0)
    want = check_simplify(verts, faces, (-1.5, -1.5, -1.5), 0.25, "icosphere", regs=(0.0, 1e-3, 1e3), dds=(True, False))
    assert want["counts"].tolist()[:6] == [251, 498, 251, 0, 782, 0]
    zero = sr.simplify_mesh(verts, faces, (-1.5, -1.5, -1.5), 0.25, 0.0)
    assert zero["counts"][6] == 251                                 # reg = 0: lambda is not > 0, every cluster at its mean
    adj = msr.adjacency(want["faces"], 251)
    assert msr.topology(adj) == (251, 2, True)


def test_damaged_incident_face_rows_are_read_within_bounds():
    """out-of-range face ids, a decreasing offset, offsets past n_incident and negative offsets: the run finishes and treats
    them as the restatement does (such rows are empty, such entries add nothing); nothing outside the arrays is read, since
    every index is compared with its bound before it is used"""
    verts, faces = msr.grid_patch(23, 19)
    verts = bumpy(verts)
    adj = msr.adjacency(faces, len(verts))
    rs = np.random.RandomState(4)
    fo, fi = adj["face_offsets"].copy(), adj["face_ids"].copy()
    fi[rs.choice(len(fi), 40, replace=False)] = rs.choice([-1, len(faces), 2147483647, -2147483648], 40)
    fi[rs.choice(len(fi), 40, replace=False)] = rs.randint(0, len(faces), 40)   # faces that do not use the vertex; rows out of order
    fo[50] = fo[49] - 1
    fo[150] = len(fi) + 3
    fo[250] = -1
    fo[len(verts)] = len(fi) + 1
    bad_faces = faces.copy()
    bad_faces[rs.choice(len(faces), 20, replace=False), rs.randint(0, 3, 20)] = rs.choice([-1, len(verts), 2147483647], 20)
    for f in (faces, bad_faces):
        check_simplify(verts, f, (-1, -1, -1), 3.0, "damaged rows", rows=(fo, fi), regs=(1e-3, 1e3))
    check_simplify(verts, faces, (-1, -1, -1), 3.0, "half of n_incident", rows=(adj["face_offsets"], adj["face_ids"]),
                   n_incident=len(fi) // 2)
    whole = sr.simplify_mesh(verts, faces, (-1, -1, -1), 3.0)
    broken = sr.simplify(verts, faces, fo, fi, (-1, -1, -1), 3.0)
    assert np.array_equal(whole["faces"], broken["faces"]) and not np.array_equal(whole["verts"], broken["verts"])


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------
def owns_its_size(t):
    return t.is_contiguous() and t.untyped_storage().nbytes() == t.numel() * t.element_size()


def test_the_python_layer_equals_the_c_calls(mp):
    from connecting_the_dots_amd import meshsmooth
    verts, faces, origin, voxel = fixture_mesh()
    v, f = dev(verts), dev(faces)
    cell = float(F(2 * voxel))
    for kw in (dict(), dict(reg=0.0), dict(reg=10.0, drop_duplicates=False)):
        want = sr.simplify_mesh(verts, faces, origin, cell, kw.get("reg", 1e-3), kw.get("drop_duplicates", True))
        s = mp.mesh_simplify(v, f, cell, origin=tuple(float(o) for o in origin), **kw)
        assert same_f32(host(s.verts), want["verts"]), kw
        for k in ("faces", "leader", "vert_cluster", "face_index"):
            t = getattr(s, k)
            assert np.array_equal(host(t), want[k]) and t.dtype == torch.int32 and owns_its_size(t), (k, kw)
        assert owns_its_size(s.verts) and s.normals is None
        assert [s.verts.shape[0], s.faces.shape[0], s.n_clusters, s.n_dropped_faces, s.n_collapsed_faces, s.n_duplicate_faces,
                s.n_mean_fallbacks, s.max_cluster] == want["counts"].tolist()
        assert s.cell == cell and s.origin == tuple(float(o) for o in origin)
    # origin=None: the minimum of the finite coordinates; a tensor as origin; a ready adjacency; normals
    bad = verts.copy()
    bad[7] = [NAN, INF, -INF]
    lo = np.where(np.isfinite(bad), bad, np.inf).min(0).astype(F)
    want = sr.simplify_mesh(bad, faces, lo, cell)
    adj = meshsmooth.MeshAdjacency(f, len(verts))
    s = mp.mesh_simplify(dev(bad), f, cell, adjacency=adj, normals=True)
    assert s.origin == tuple(float(o) for o in lo) and same_f32(host(s.verts), want["verts"]) and np.array_equal(host(s.faces), want["faces"])
    a = msr.adjacency(want["faces"], len(want["verts"]))
    assert same_f32(host(s.normals), msr.vertex_normals(want["verts"], want["faces"], a["face_offsets"], a["face_ids"]))
    t = mp.mesh_simplify(dev(bad), f, cell, origin=dev(lo))
    assert torch.equal(t.verts.view(torch.int32), s.verts.view(torch.int32)) and torch.equal(t.faces, s.faces)
    with pytest.raises(RuntimeError, match="mesh_simplify: adjacency was built for other faces"):
        mp.mesh_simplify(v, f.clone(), cell, adjacency=adj)
    with pytest.raises(RuntimeError, match="mesh_simplify: adjacency must be a MeshAdjacency"):
        mp.mesh_simplify(v, f, cell, adjacency=(adj.face_offsets, adj.face_ids))
    with pytest.raises(RuntimeError, match=r"mesh_simplify: faces must be shaped \[m,3\]"):
        mp.mesh_simplify(v, f.reshape(-1), cell)
    with pytest.raises(RuntimeError, match="mesh_simplify: verts: unsupported dtype"):
        mp.mesh_simplify(v.double(), f, cell)
    with pytest.raises(RuntimeError, match="mesh_simplify: cell must be a finite number > 0"):
        mp.mesh_simplify(v, f, 0.0)
    with pytest.raises(RuntimeError, match="mesh_simplify: normals must be True or False"):
        mp.mesh_simplify(v, f, cell, normals=1)
    with pytest.raises(RuntimeError, match="mesh_simplify: the mesh spans 1048576 cells or more on an axis"):
        mp.mesh_simplify(v, f, 1e-7)
    far = mp.mesh_simplify(v, f, 1e-7, origin=(0, 0, 0))           # with an origin of the caller's it is never an error
    assert far.faces.shape == (0, 3) and far.n_dropped_faces == len(faces) and (far.vert_cluster == -1).all()
    # empty meshes
    ev, ef = torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    e = mp.mesh_simplify(ev, ef, 0.5, normals=True)
    assert e.verts.shape == (0, 3) and e.faces.shape == (0, 3) and e.normals.shape == (0, 3) and e.vert_cluster.shape == (0,)
    assert e.origin == (0.0, 0.0, 0.0) and e.n_clusters == 0
    lone = mp.mesh_simplify(v, ef, 0.5)                             # vertices without faces: nothing is clusterable
    assert lone.verts.shape == (0, 3) and (lone.vert_cluster == -1).all() and lone.n_clusters == 0


def test_simplify_tsdf_mesh_works_track_by_track(mp, tmp_path):
    """two tracks (the clean and a noisy fused scene): each equals the per-track restatement; src is gathered at the
    leaders, the counts are rebuilt, and the result goes into renderer.MeshBVH, mesh.save_ply, meshsmooth.MeshAdjacency and
    meshops.clean_tsdf_mesh as it is; mesheval.reconstruction_error against the input mesh is printed"""
    from connecting_the_dots_amd import mesh, mesheval, meshops, meshsmooth, renderer
    parts = []
    for kind, seed in (("clean", 5), ("noisy", 6)):
        sc = fused_scene(kind, seed, masked=True)
        faces, _ = mr.faces(sc["tsdf"], sc["weight"])
        parts.append((sc["points"], faces, sc["normals"], sc["src"]))
    origin, voxel = np.asarray(sc["origin"], F).reshape(-1)[:3], float(sc["voxel"])
    cell = float(F(2 * voxel))
    counts = [(len(p[0]), len(p[1])) for p in parts]
    m = mesh.TsdfMesh(dev(np.concatenate([p[0] for p in parts])), dev(np.concatenate([p[3] for p in parts])),
                      dev(np.concatenate([p[2] for p in parts])), dev(np.concatenate([p[1] for p in parts])),
                      dev(np.array([c[0] for c in counts], np.int64)), dev(np.array([c[1] for c in counts], np.int64)), counts)
    out = mp.simplify_tsdf_mesh(m, cell, origin=tuple(float(o) for o in origin))
    assert out.n_tracks == 2 and out.n_verts_per_track.tolist() == [c[0] for c in out._counts]
    assert out.n_faces_per_track.tolist() == [c[1] for c in out._counts] and out.verts.shape[0] == sum(c[0] for c in out._counts)
    for b, (verts, faces, _, src) in enumerate(parts):
        want = sr.simplify_mesh(verts, faces, origin, cell)
        v, f, nrm = out.track(b)
        assert out._counts[b] == (len(want["verts"]), len(want["faces"])) and out._counts[b][1] < counts[b][1] / 2
        assert same_f32(host(v), want["verts"]) and np.array_equal(host(f), want["faces"])
        a = msr.adjacency(want["faces"], len(want["verts"]))
        assert same_f32(host(nrm), msr.vertex_normals(want["verts"], want["faces"], a["face_offsets"], a["face_ids"]))
        v0 = sum(c[0] for c in out._counts[:b])
        assert np.array_equal(host(out.src[v0:v0 + len(want["verts"])]), src[want["leader"]])
        bvh = renderer.MeshBVH(v, f)
        assert bvh.usable and bvh.matches(v, f)
        adj = meshsmooth.MeshAdjacency(f, v.shape[0])
        assert adj.n_valid_faces == f.shape[0] and adj.n_referenced == v.shape[0]
        vin, fin, _ = m.track(b)
        err = mesheval.reconstruction_error(v, f, vin, fin, [0.25 * voxel, voxel])
        print("track %d: %d -> %d faces; against the input mesh: chamfer %.3e, accuracy median %.3e max %.3e, completeness "
              "median %.3e max %.3e, f-score at voxel / 4 and at a voxel %s"
              % (b, counts[b][1], f.shape[0], err["chamfer"], err["accuracy"]["median"], err["accuracy"]["max"],
                 err["completeness"]["median"], err["completeness"]["max"], err["fscore"]))
        assert err["accuracy"]["max"] <= 2 * 3 ** 0.5 * cell           # a cluster's vertex and its members share a box of 2 cells
    path = str(tmp_path / "simplified.ply")
    v, f, nrm = out.track(1)
    mesh.save_ply(path, v, f, normals=nrm)
    pv, pf, pn, _ = mesh.load_ply(path)
    assert pv.tobytes() == host(v).tobytes() and pf.tobytes() == host(f).tobytes() and same_f32(pn, host(nrm))
    cleaned = meshops.clean_tsdf_mesh(out, min_faces=8)
    assert cleaned.n_tracks == 2 and 0 < cleaned.faces.shape[0] <= out.faces.shape[0]
    bare = mesh.TsdfMesh(m.verts, m.src, None, m.faces, m.n_verts_per_track, m.n_faces_per_track, counts)
    auto = mp.simplify_tsdf_mesh(bare, cell)                        # every track its own origin; no normals
    assert auto.normals is None and auto.n_tracks == 2 and 0 < auto.faces.shape[0] < m.faces.shape[0] / 2
