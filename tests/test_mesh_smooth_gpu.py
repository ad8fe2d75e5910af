"""GPU parity of the mesh connectivity, smoothing and vertex normals (meshsmooth.MeshAdjacency, mesh_smooth,
vertex_normals, smooth_tsdf_mesh; ctd_mesh_adjacency_i32, ctd_mesh_smooth_f32, ctd_mesh_vertex_normals_f32 of
include/ctd_hip_mesh_smooth.h) against the restatement tests/meshsmooth_ref.py.

The adjacency is integer work, so it equals the restatement exactly; the sums of the smoothing and of the normals run in
the rule's order in f32, so verts_out and normals equal it bit for bit (NaNs compared as NaNs, whatever their payload).
Every C call runs twice with equal bits, from a workspace filled with a sentinel, leaves its inputs as they were and
leaves what lies past the true counts unwritten."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import meshsmooth_ref as msr
from tests.test_tsdf_host import fused_scene

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0xA5
PAD = 8                                                           # entries past every output that must stay as they were


@pytest.fixture(scope="module")
def ms():
    from connecting_the_dots_amd import meshsmooth
    return meshsmooth


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


def adjacency_c_call(faces, n, cap=None, cap_faces=None, optional=True):
    """ctd_mesh_adjacency_i32, twice -> dict of host arrays, -7 where nothing was written (None without `optional`)"""
    lib, L = _lib()
    m = len(faces)
    cap = 6 * m if cap is None else cap
    cap_faces = 3 * m if cap_faces is None else cap_faces
    f = _some(faces, (1, 3))
    f0 = f.clone()
    nws = L.ctd_mesh_adjacency_workspace_bytes(n, m)
    assert nws > 0
    runs = []
    for _ in range(2):
        ws = torch.full((nws,), SENTINEL, dtype=torch.uint8, device="cuda")
        out = dict(offsets=torch.full((n + 1 + PAD,), -7, dtype=torch.int32, device="cuda"),
                   neighbors=torch.full((6 * m + PAD,), -7, dtype=torch.int32, device="cuda"),
                   face_offsets=torch.full((n + 1 + PAD,), -7, dtype=torch.int32, device="cuda"),
                   face_ids=torch.full((3 * m + PAD,), -7, dtype=torch.int32, device="cuda"),
                   vflags=torch.full((n + PAD,), 0x77, dtype=torch.uint8, device="cuda"),
                   counts=torch.full((7,), -7, dtype=torch.int64, device="cuda"))
        p = (lambda t: t.data_ptr()) if optional else (lambda t: None)
        st = L.ctd_mesh_adjacency_i32(f.data_ptr(), n, m, out["offsets"].data_ptr(), p(out["neighbors"]), cap,
                                      p(out["face_offsets"]), p(out["face_ids"]), cap_faces, out["vflags"].data_ptr(),
                                      out["counts"].data_ptr(), ws.data_ptr(), ws.numel(), 0, torch.cuda.current_stream().cuda_stream)
        lib.check(st, "ctd_mesh_adjacency_i32")
        runs.append({k: host(v) for k, v in out.items()})
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), "two runs differ in " + k
    assert torch.equal(f, f0), "an input was written"
    r = runs[0]
    assert r["counts"][6] == -7 and (r["offsets"][n + 1:] == -7).all() and (r["vflags"][n:] == 0x77).all()
    return r


def check_adjacency(faces, n, what, want=None, capacities=True):
    """every output against the restatement: the full call, the optional outputs NULL, and capacities of half"""
    faces = np.ascontiguousarray(faces, np.int32)
    m = len(faces)
    want = msr.adjacency(faces, n) if want is None else want
    nnz, n_inc = int(want["counts"][0]), int(3 * want["counts"][5])
    got = adjacency_c_call(faces, n)
    assert got["counts"][:6].tolist() == want["counts"].tolist(), "%s: counts %s vs %s" % (what, got["counts"], want["counts"])
    assert np.array_equal(got["offsets"][:n + 1], want["offsets"]), what + ": offsets"
    assert np.array_equal(got["vflags"][:n], want["vflags"]), what + ": vflags"
    assert np.array_equal(got["neighbors"][:nnz], want["neighbors"]) and (got["neighbors"][nnz:] == -7).all(), what + ": neighbors"
    assert np.array_equal(got["face_offsets"][:n + 1], want["face_offsets"]) and (got["face_offsets"][n + 1:] == -7).all(), what
    assert np.array_equal(got["face_ids"][:n_inc], want["face_ids"]) and (got["face_ids"][n_inc:] == -7).all(), what + ": face_ids"
    if capacities:
        bare = adjacency_c_call(faces, n, -5, -5, optional=False)
        for k in ("counts", "offsets", "vflags"):
            assert np.array_equal(bare[k], got[k]), "%s: %s without the optional outputs" % (what, k)
        for k in ("neighbors", "face_offsets", "face_ids"):
            assert (bare[k] == -7).all()
        hn, hf = nnz // 2, n_inc // 2
        half = adjacency_c_call(faces, n, hn, hf)
        for k in ("counts", "offsets", "vflags", "face_offsets"):
            assert np.array_equal(half[k], got[k]), "%s: %s at half the capacity" % (what, k)
        assert np.array_equal(half["neighbors"][:hn], want["neighbors"][:hn]) and (half["neighbors"][hn:] == -7).all(), what
        assert np.array_equal(half["face_ids"][:hf], want["face_ids"][:hf]) and (half["face_ids"][hf:] == -7).all(), what
    return want


def smooth_c_call(verts, offsets, neighbors, vflags, iters, lam, mu, fix, nnz=None):
    """ctd_mesh_smooth_f32, twice -> verts_out (host)"""
    lib, L = _lib()
    n = len(verts)
    nnz = len(neighbors) if nnz is None else nnz
    x, o, nb = _some(verts, (1, 3)), dev(offsets), _some(neighbors, (1,))
    fl = None if vflags is None else _some(vflags, (1,))
    x0 = x.clone()
    nws = L.ctd_mesh_smooth_workspace_bytes(n)
    runs = []
    for _ in range(2):
        ws = torch.full((max(nws, 256),), SENTINEL, dtype=torch.uint8, device="cuda")
        out = torch.full((n + PAD, 3), -7.0, dtype=torch.float32, device="cuda")
        st = L.ctd_mesh_smooth_f32(x.data_ptr(), n, o.data_ptr(), nb.data_ptr(), nnz, None if fl is None else fl.data_ptr(), iters,
                                   lam, mu, int(fix), out.data_ptr(), ws.data_ptr(), ws.numel(), 0,
                                   torch.cuda.current_stream().cuda_stream)
        lib.check(st, "ctd_mesh_smooth_f32")
        runs.append(host(out))
    assert same_f32(runs[0], runs[1]), "two runs differ"
    assert torch.equal(x.view(torch.int32), x0.view(torch.int32)), "an input was written"
    assert (runs[0][n:] == -7).all()
    return runs[0][:n]


def normals_c_call(verts, faces, face_offsets, face_ids, n_incident=None):
    """ctd_mesh_vertex_normals_f32, twice -> normals (host)"""
    lib, L = _lib()
    n, m = len(verts), len(faces)
    n_incident = len(face_ids) if n_incident is None else n_incident
    x, f, fo, fi = _some(verts, (1, 3)), _some(faces, (1, 3)), dev(face_offsets), _some(face_ids, (1,))
    runs = []
    for _ in range(2):
        out = torch.full((n + PAD, 3), -7.0, dtype=torch.float32, device="cuda")
        st = L.ctd_mesh_vertex_normals_f32(x.data_ptr(), n, f.data_ptr(), m, fo.data_ptr(), fi.data_ptr(), n_incident,
                                           out.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
        lib.check(st, "ctd_mesh_vertex_normals_f32")
        runs.append(host(out))
    assert same_f32(runs[0], runs[1]), "two runs differ"
    assert (runs[0][n:] == -7).all()
    return runs[0][:n]


def check_smooth(verts, adj, what, settings=((10, 0.5, -0.53, True),)):
    for iters, lam, mu, fix in settings:
        want = msr.smooth(verts, adj["offsets"], adj["neighbors"], adj["vflags"], iters, lam, mu, fix)
        got = smooth_c_call(verts, adj["offsets"], adj["neighbors"], adj["vflags"], iters, lam, mu, fix)
        assert same_f32(got, want), "%s: iters %d lam %g mu %g fix_boundary %s" % (what, iters, lam, mu, fix)
        if not fix:                                                # vflags is not read then
            assert same_f32(smooth_c_call(verts, adj["offsets"], adj["neighbors"], None, iters, lam, mu, fix), want), what
    return want


def check_normals(verts, faces, adj, what):
    want = msr.vertex_normals(verts, faces, adj["face_offsets"], adj["face_ids"])
    assert same_f32(normals_c_call(verts, faces, adj["face_offsets"], adj["face_ids"]), want), what + ": normals"
    return want


ALL_SETTINGS = ((0, 0.5, -0.53, True), (1, 0.5, -0.53, True), (10, 0.5, -0.53, True), (10, 0.5, -0.53, False), (3, 0.7, 0.0, True),
                (1, 1.0, 0.0, False), (2, 1.0, -2.0, False))


def bumpy(verts, seed=1, sigma=0.1):
    return (verts + np.random.RandomState(seed).normal(0, sigma, verts.shape)).astype(F)


# ---------------------------------------------------------------------------------------------------------------------
# hand-made meshes
# ---------------------------------------------------------------------------------------------------------------------
def hand_cases():
    second = np.where(msr.TETRA == 0, 3, msr.TETRA + 4).astype(np.int32)
    bad = np.array([[0, 1, 2], [3, 3, 4], [3, 4, 3], [5, 4, 4], [6, 7, -1], [6, 8, 7], [6, 7, 1 << 30], [8, 6, 7],
                    [-2147483648, 0, 1], [2147483647, 0, 1]], np.int32)
    return {"tetrahedron": (msr.TETRA, 5), "two tetrahedra": (np.concatenate([msr.TETRA, second]), 8),
            "grid 3 x 3": (msr.grid_patch(3, 3)[1], 9), "a face three times": (np.array([[0, 1, 2]] * 3 + [[2, 1, 3]], np.int32), 4),
            "bad indices, 8": (bad, 8), "bad indices, 9": (bad, 9), "all invalid": (bad[1:5], 9),
            "no faces": (np.zeros((0, 3), np.int32), 7), "nothing": (np.zeros((0, 3), np.int32), 0), "no vertices": (bad, 0)}


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_made_meshes(name):
    faces, n = hand_cases()[name]
    adj = check_adjacency(faces, n, name)
    verts = np.random.RandomState(5).randn(n, 3).astype(F)
    check_smooth(verts, adj, name, ALL_SETTINGS)
    check_normals(verts, faces, adj, name)
    if name == "tetrahedron":
        assert adj["counts"].tolist() == [12, 6, 0, 0, 3, 4]
    if name == "a face three times":
        assert adj["counts"].tolist() == [10, 5, 2, 3, 4, 4]


@pytest.mark.parametrize("n", [255, 256, 257])
def test_sizes_around_the_chunk(n):
    verts, faces = msr.grid_patch(17, 15) if n == 255 else msr.grid_patch(16, 16)
    verts = np.concatenate([verts, np.ones((n - len(verts), 3), F)])     # 257: one vertex that no face uses
    verts = bumpy(verts)
    adj = check_adjacency(faces, n, "n = %d" % n)
    check_smooth(verts, adj, "n = %d" % n, ALL_SETTINGS)
    normals = check_normals(verts, faces, adj, "n = %d" % n)
    assert np.isnan(normals[len(np.unique(faces)):]).all() and np.isfinite(normals[:len(np.unique(faces))]).all()


@functools.lru_cache(maxsize=None)
def big_grid():
    verts, faces = msr.grid_patch(520, 520)
    return bumpy(verts, 2, 0.2), faces


def test_a_grid_of_more_chunks_than_one_round_of_the_scan():
    """520 x 520 = 270 400 vertices: 1057 chunks of 256, so the scan of the chunk sums carries"""
    verts, faces = big_grid()
    n = len(verts)
    assert (n + 255) // 256 > 1024
    adj = check_adjacency(faces, n, "grid 520 x 520", capacities=False)
    assert adj["counts"].tolist() == [1618242, 809121, 2076, 0, 6, 538722]
    half = adjacency_c_call(faces, n, 800000, 800000)              # capacities that end inside a chunk's rows
    assert np.array_equal(half["neighbors"][:800000], adj["neighbors"][:800000]) and (half["neighbors"][800000:] == -7).all()
    assert np.array_equal(half["face_ids"][:800000], adj["face_ids"][:800000]) and (half["face_ids"][800000:] == -7).all()
    check_smooth(verts, adj, "grid 520 x 520")
    check_normals(verts, faces, adj, "grid 520 x 520")


def test_a_hub_of_exactly_the_cap_passes_and_one_more_raises(ms):
    verts, faces = msr.open_fan(1024)
    adj = check_adjacency(faces, len(verts), "fan of 1024")
    assert adj["counts"].tolist() == [4098, 2049, 1026, 0, 1024, 1024]
    check_smooth(verts, adj, "fan of 1024", ((10, 0.5, -0.53, False), (2, 0.5, -0.53, True)))
    check_normals(verts, faces, adj, "fan of 1024")
    a = ms.MeshAdjacency(dev(faces), len(verts))
    assert a.max_incident == 1024 == ms.MAX_INCIDENT and a.n_boundary_edges == 1026 and not a.closed and a.euler == 1
    # one more: the call still returns CTD_OK and writes the true counts; the Python layer raises
    verts, faces = msr.open_fan(1025)
    want = msr.adjacency(faces, len(verts))
    got = adjacency_c_call(faces, len(verts))
    assert got["counts"][4] == 1025 and got["counts"][:6].tolist() == want["counts"].tolist()
    with pytest.raises(RuntimeError, match="MeshAdjacency: a vertex has 1025 incident faces, more than MAX_INCIDENT = 1024"):
        ms.MeshAdjacency(dev(faces), len(verts))
    with pytest.raises(RuntimeError, match="more than MAX_INCIDENT"):
        ms.mesh_smooth(dev(verts), dev(faces))


def test_random_faces_with_duplicates_and_bad_indices():
    faces = msr.random_faces(300)
    adj = check_adjacency(faces, 300, "random faces")
    valid = msr.valid_faces(faces, 300)
    assert adj["mult"].max() >= 9 and adj["counts"][3] > 0 and adj["counts"][2] > 0 and 0 < valid.sum() < len(faces) - 100
    assert adj["counts"][4] > 16                                   # rows that the workgroup sorts, among rows that a lane sorts
    assert (np.diff(adj["face_offsets"]) <= 16).any()
    assert (faces < 0).any() and (faces == 2147483647).any() and (faces[:, 0] == faces[:, 2]).any()
    verts = np.random.RandomState(9).randn(300, 3).astype(F)
    check_smooth(verts, adj, "random faces", ALL_SETTINGS)
    check_normals(verts, faces, adj, "random faces")


@functools.lru_cache(maxsize=None)
def fixture_mesh():
    sc = fused_scene("clean", 5, masked=True)
    faces, _ = mr.faces(sc["tsdf"], sc["weight"])
    return sc["points"], faces


def test_the_mesh_of_the_fused_scene():
    verts, faces = fixture_mesh()
    adj = check_adjacency(faces, len(verts), "fused scene")
    assert adj["counts"].tolist() == [13966, 6983, 400, 0, 8, 4522] and len(verts) == 2475
    check_smooth(verts, adj, "fused scene", ALL_SETTINGS)
    normals = check_normals(verts, faces, adj, "fused scene")
    assert np.isfinite(normals).all(1).sum() == 2465


def test_the_noisy_icosphere():
    verts, faces = msr.noisy_icosphere(0.01, 0)
    adj = check_adjacency(faces, len(verts), "icosphere")
    assert adj["counts"].tolist() == [3840, 1920, 0, 0, 6, 1280]
    out = check_smooth(verts, adj, "icosphere", ALL_SETTINGS)      # (the last of the settings is returned; the default below)
    out = check_smooth(verts, adj, "icosphere")
    check_normals(out, faces, adj, "icosphere, smoothed")
    rms = lambda p: np.sqrt(((np.linalg.norm(p.astype(np.float64), axis=1) - 1) ** 2).mean())   # noqa: E731
    assert rms(out) / rms(verts) <= 0.5 * (0.459 + 1)              # as tests/test_mesh_smooth_host.py pins the restatement


# ---------------------------------------------------------------------------------------------------------------------
# smoothing: non-finite coordinates and damaged adjacencies
# ---------------------------------------------------------------------------------------------------------------------
def test_a_nan_vertex_spreads_to_its_ring_per_pass():
    verts, faces = msr.grid_patch(23, 19)
    verts = bumpy(verts)
    adj = msr.adjacency(faces, len(verts))
    centre = 9 * 23 + 11
    for value in (np.nan, np.inf, -np.inf):
        bad = verts.copy()
        bad[centre, 1] = value
        for iters, mu in ((1, 0.0), (1, -0.53), (3, -0.53)):
            want = msr.smooth(bad, adj["offsets"], adj["neighbors"], adj["vflags"], iters, 0.5, mu, True)
            got = smooth_c_call(bad, adj["offsets"], adj["neighbors"], adj["vflags"], iters, 0.5, mu, True)
            assert same_f32(got, want), (value, iters, mu)
            if (iters, mu) == (1, 0.0):                            # one pass: the vertex and its ring of six, in y alone
                assert sorted(np.nonzero(~np.isfinite(got).all(1))[0].tolist()) == sorted(
                    [centre] + adj["neighbors"][adj["offsets"][centre]:adj["offsets"][centre + 1]].tolist())
                assert np.isfinite(got[:, [0, 2]]).all()
    check_normals(bad, faces, adj, "a vertex at -inf")


def test_a_damaged_adjacency_is_read_within_bounds():
    """out-of-range neighbours, a decreasing offset, offsets past nnz and negative offsets: the run finishes and treats them
    as the restatement does (such rows are empty, such entries do not count); nothing outside the arrays is read, since
    every index is compared with its bound before it is used"""
    verts, faces = msr.grid_patch(23, 19)
    verts = bumpy(verts)
    n = len(verts)
    adj = msr.adjacency(faces, n)
    rs = np.random.RandomState(4)
    nb, off = adj["neighbors"].copy(), adj["offsets"].copy()
    nnz = len(nb)
    hit = rs.choice(nnz, 60, replace=False)
    nb[hit] = rs.choice([-1, n, n + 5, 2147483647, -2147483648], 60)
    off[40] = off[39] - 3                                          # decreasing
    off[100] = nnz + 7                                             # past nnz: rows 99 and 100 are empty
    off[200] = -4                                                  # negative
    off[n] = nnz + 1                                               # the last row ends past nnz
    for fix in (True, False):
        want = msr.smooth(verts, off, nb, adj["vflags"], 2, 0.5, -0.53, fix)
        assert same_f32(smooth_c_call(verts, off, nb, adj["vflags"], 2, 0.5, -0.53, fix), want), fix
    assert np.array_equal(want[99], verts[99]) and np.array_equal(want[39], verts[39]) and not np.array_equal(want[300], verts[300])
    # a smaller nnz than the array holds: the rows past it are empty
    want = msr.smooth(verts, adj["offsets"], adj["neighbors"], adj["vflags"], 1, 0.5, 0.0, False, nnz=nnz // 2)
    got = smooth_c_call(verts, adj["offsets"], adj["neighbors"], adj["vflags"], 1, 0.5, 0.0, False, nnz=nnz // 2)
    assert same_f32(got, want) and np.array_equal(got[n - 1], verts[n - 1])
    # the normals over damaged rows and ids
    fo, fi = adj["face_offsets"].copy(), adj["face_ids"].copy()
    fi[rs.choice(len(fi), 40, replace=False)] = rs.choice([-1, len(faces), 2147483647, -2147483648], 40)
    fo[50] = fo[49] - 1
    fo[150] = len(fi) + 3
    fo[250] = -1
    bad_faces = faces.copy()
    bad_faces[rs.choice(len(faces), 20, replace=False), rs.randint(0, 3, 20)] = rs.choice([-1, n, 2147483647], 20)
    for f in (faces, bad_faces):
        want = msr.vertex_normals(verts, f, fo, fi)
        assert same_f32(normals_c_call(verts, f, fo, fi), want)
    want = msr.vertex_normals(verts, faces, adj["face_offsets"], adj["face_ids"], n_incident=len(fi) // 2)
    assert same_f32(normals_c_call(verts, faces, adj["face_offsets"], adj["face_ids"], n_incident=len(fi) // 2), want)
    assert np.isnan(want[n - 1]).all()


# ---------------------------------------------------------------------------------------------------------------------
# the Python layer
# ---------------------------------------------------------------------------------------------------------------------
def test_the_python_layer_equals_the_c_calls(ms):
    verts, faces = fixture_mesh()
    n = len(verts)
    want = msr.adjacency(faces, n)
    v, f = dev(verts), dev(faces)
    a = ms.MeshAdjacency(f, n)
    for k in ("offsets", "neighbors", "face_offsets", "face_ids", "vflags"):
        t = getattr(a, k)
        assert np.array_equal(host(t), want[k]) and t.dtype == torch.from_numpy(want[k]).dtype, k
        assert t.is_contiguous() and t.untyped_storage().nbytes() == t.numel() * t.element_size(), k   # owns exactly its size
    n_ref, euler, closed = msr.topology(want)
    assert [a.n_edges, a.n_boundary_edges, a.n_nonmanifold_edges, a.max_incident, a.n_valid_faces] == want["counts"][1:].tolist()
    assert (a.n_referenced, a.euler, a.closed) == (n_ref, euler, closed) == (2465, 4, False)
    assert a.matches(f, n) and not a.matches(f, n + 1) and not a.matches(f.clone(), n) and not a.matches(f[:-1], n)
    for kw in (dict(), dict(iters=3, lam=0.7, mu=0.0, fix_boundary=False), dict(iters=0)):
        full = dict(dict(iters=10, lam=0.5, mu=-0.53, fix_boundary=True), **kw)
        ref = msr.smooth(verts, want["offsets"], want["neighbors"], want["vflags"], full["iters"], full["lam"], full["mu"],
                         full["fix_boundary"])
        assert same_f32(host(ms.mesh_smooth(v, f, adjacency=a, **kw)), ref), kw
        assert same_f32(host(ms.mesh_smooth(v, f, **kw)), ref), kw
    ref = msr.vertex_normals(verts, faces, want["face_offsets"], want["face_ids"])
    assert same_f32(host(ms.vertex_normals(v, f, adjacency=a)), ref) and same_f32(host(ms.vertex_normals(v, f)), ref)
    with pytest.raises(RuntimeError, match="mesh_smooth: adjacency was built for other faces"):
        ms.mesh_smooth(v, f.clone(), adjacency=a)
    with pytest.raises(RuntimeError, match="vertex_normals: adjacency must be a MeshAdjacency"):
        ms.vertex_normals(v, f, adjacency=(a.offsets, a.neighbors))
    with pytest.raises(RuntimeError, match=r"mesh_smooth: faces must be shaped \[m,3\]"):
        ms.mesh_smooth(v, f.reshape(-1))
    with pytest.raises(RuntimeError, match="mesh_smooth: verts: unsupported dtype"):
        ms.mesh_smooth(v.double(), f)
    with pytest.raises(RuntimeError, match="mesh_smooth: lam must be a finite number"):
        ms.mesh_smooth(v, f, lam=1.5)
    with pytest.raises(RuntimeError, match="MeshAdjacency: n_verts must be an integer >= 0"):
        ms.MeshAdjacency(f, -1)
    # closed meshes, empty meshes
    sv, sf = msr.noisy_icosphere()
    s = ms.MeshAdjacency(dev(sf), len(sv))
    assert s.closed and s.euler == 2 and s.n_edges == 1920 and s.n_referenced == 642 and s.max_incident == 6
    ev, ef = torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    e = ms.MeshAdjacency(ef, 0)
    assert e.closed and e.euler == 0 and e.offsets.tolist() == [0] and e.neighbors.shape == (0,) and e.vflags.shape == (0,)
    assert ms.mesh_smooth(ev, ef).shape == (0, 3) and ms.vertex_normals(ev, ef).shape == (0, 3)
    lone = ms.mesh_smooth(v, ef)                                    # vertices without faces stay where they are
    assert torch.equal(lone.view(torch.int32), v.view(torch.int32)) and torch.isnan(ms.vertex_normals(v, ef)).all()


def test_smooth_tsdf_mesh_works_track_by_track(ms, tmp_path):
    """two tracks (the clean and a noisy fused scene): each equals the per-track calls; src, faces and the counts are
    unchanged, and the result goes into renderer.MeshBVH and mesh.save_ply as it is"""
    from connecting_the_dots_amd import mesh, renderer
    parts = []
    for kind, seed in (("clean", 5), ("noisy", 6)):
        sc = fused_scene(kind, seed, masked=True)
        faces, _ = mr.faces(sc["tsdf"], sc["weight"])
        parts.append((sc["points"], faces, sc["normals"], sc["src"]))
    counts = [(len(p[0]), len(p[1])) for p in parts]
    m = mesh.TsdfMesh(dev(np.concatenate([p[0] for p in parts])), dev(np.concatenate([p[3] for p in parts])),
                      dev(np.concatenate([p[2] for p in parts])), dev(np.concatenate([p[1] for p in parts])),
                      dev(np.array([c[0] for c in counts], np.int64)), dev(np.array([c[1] for c in counts], np.int64)), counts)
    out = ms.smooth_tsdf_mesh(m)
    assert out._counts == counts and out.src is m.src and out.faces is m.faces and out.n_verts_per_track is m.n_verts_per_track
    for b, (verts, faces, _, _) in enumerate(parts):
        adj = msr.adjacency(faces, len(verts))
        want = msr.smooth(verts, adj["offsets"], adj["neighbors"], adj["vflags"])
        v, f, nrm = out.track(b)
        assert same_f32(host(v), want) and np.array_equal(host(f), faces)
        assert same_f32(host(nrm), msr.vertex_normals(want, faces, adj["face_offsets"], adj["face_ids"]))
        bvh = renderer.MeshBVH(v, f)
        assert bvh.usable and bvh.matches(v, f)
    path = str(tmp_path / "smooth.ply")
    v, f, nrm = out.track(1)
    mesh.save_ply(path, v, f, normals=nrm)
    pv, pf, pn, _ = mesh.load_ply(path)
    assert pv.tobytes() == host(v).tobytes() and pf.tobytes() == host(f).tobytes() and same_f32(pn, host(nrm))
    kept = ms.smooth_tsdf_mesh(m, iters=2, mu=0.0, fix_boundary=False, recompute_normals=False)
    assert kept.normals is m.normals and not torch.equal(kept.verts, m.verts)
    bare = mesh.TsdfMesh(m.verts, m.src, None, m.faces, m.n_verts_per_track, m.n_faces_per_track, counts)
    assert ms.smooth_tsdf_mesh(bare).normals is None
    same = ms.smooth_tsdf_mesh(m, iters=0)                          # a copy, with the normals of the mesh itself
    assert torch.equal(same.verts.view(torch.int32), m.verts.view(torch.int32)) and same.verts.data_ptr() != m.verts.data_ptr()


def test_recomputed_normals_colour_no_fewer_vertices(ms):
    """track 0 of the scene of tests/chain_scene.py, rendered, fused into a volume and meshed: color_tsdf_mesh with the TSDF
    gradients as normals and with the normals recomputed from the faces; the share of coloured vertices is printed for both
    and may not be smaller with the recomputed ones"""
    from connecting_the_dots_amd import mesh, meshcolor, renderer
    from connecting_the_dots_amd import torchext as te
    from tests import chain_scene as cs
    K = cs.intrinsics()
    scene, pose = cs.meshes()[0], cs.poses()[0]
    verts, colors, faces = dev(scene["verts"]), dev(scene["colors"]), dev(scene["faces"])
    pattern3 = dev(np.ascontiguousarray(np.repeat(cs.pattern01()[:, :, None], 3, 2)))
    shader = renderer.PyShader(*cs.SHADER)
    fx, fy, px, py = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    depth, image = [], []
    for v in range(cs.V):
        cam = renderer.PyCamera(fx, fy, px, py, pose["R"][v], pose["t"][v], cs.W, cs.H)
        proj = renderer.PyCamera(fx, fy, px, py, pose["R"][v], pose["t_proj"][v], cs.W, cs.H)
        d, c, _ = renderer.render_mesh_proj(verts, colors, faces, cam, proj, shader, pattern3, cs.D_ALPHA, cs.D_BETA)
        depth.append(d), image.append(c.permute(2, 0, 1))
    depth, images = torch.stack(depth)[None].contiguous(), torch.stack(image)[None].contiguous()
    R, t = dev(pose["R"][None]), dev(pose["t"][None])
    ray = dev(cs.rays(K))
    # a grid around the points that view 0 sees
    d0 = host(depth[0, 0]).reshape(-1)
    R0, t0 = pose["R"][0].astype(np.float64), pose["t"][0].astype(np.float64)
    X = ((cs.rays(K).astype(np.float64) * d0[:, None])[d0 > 0] - t0) @ R0
    nx, ny, nz, voxel = 96, 40, 64, 0.04
    lo = 0.5 * (X.min(0) + X.max(0)) - 0.5 * voxel * (np.array([nx, ny, nz]) - 1)
    origin = dev(lo[None].astype(F))
    T, w = te.tsdf_volume(1, nx, ny, nz)
    te.tsdf_integrate(T, w, origin, voxel, depth, ray, dev(K), R, t)
    m = mesh.tsdf_mesh(T, w, origin, voxel, return_normals=True)
    assert m._counts[0][1] > 2000
    again = ms.smooth_tsdf_mesh(m, iters=0)                         # the same vertices, the normals recomputed
    share = []
    for which, mm in (("the TSDF gradients", m), ("recomputed normals", again)):
        vc = meshcolor.color_tsdf_mesh(mm, images, dev(K), R, t, 2 * voxel)
        share.append(float((vc.n_views > 0).float().mean()))
        print("%s: %d vertices, %d faces, %d normals not finite, %.2f %% of the vertices coloured"
              % (which, m._counts[0][0], m._counts[0][1], int((~torch.isfinite(mm.normals).all(1)).sum()), 100 * share[-1]))
    assert share[1] >= share[0]
