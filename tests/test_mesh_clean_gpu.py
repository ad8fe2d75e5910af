"""GPU parity of the mesh clean-up (meshops.mesh_components, meshops.mesh_clean, meshops.clean_tsdf_mesh;
ctd_mesh_components_i32, ctd_mesh_clean_i32 of include/ctd_hip_mesh_clean.h) against the restatement
tests/meshclean_ref.py.

Everything is integer work, so labels, sizes, counts, faces and index lists equal the restatement exactly.  Every C call
runs twice with equal bits, from a workspace filled with a sentinel, and leaves its inputs as they were."""
import itertools

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import meshclean_ref as mcr
from tests import tsdf_ref as tr
from tests.test_tsdf_host import CORNER_DIMS, corner_model
from tests.test_tsdf_mesh_gpu import GRIDS, random_volume

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = 0xA5
MIN_FACES = (1, 2, 9, 100)


@pytest.fixture(scope="module")
def mesh():
    from connecting_the_dots_amd import mesh
    return mesh


@pytest.fixture(scope="module")
def meshops():
    from connecting_the_dots_amd import meshops
    return meshops


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def _lib_and_ws(n, m):
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    nws = L.ctd_mesh_clean_workspace_bytes(n, m)
    assert nws > 0
    return _lib, L, torch.full((nws,), SENTINEL, dtype=torch.uint8, device="cuda")


def _inputs(faces, verts):
    """device copies; an empty array still gets a pointer (nothing is read through it)"""
    f = dev(faces) if len(faces) else torch.zeros((1, 3), dtype=torch.int32, device="cuda")
    v = None if verts is None else (dev(verts) if len(verts) else torch.zeros((1, 3), device="cuda"))
    return f, v


def components_c_call(faces, verts, n, drop):
    """ctd_mesh_components_i32, twice -> label, size, n_components (host)"""
    m = len(faces)
    f, v = _inputs(faces, verts)
    f0, v0 = f.clone(), None if v is None else v.clone()
    runs = []
    for _ in range(2):
        _lib, L, ws = _lib_and_ws(n, m)
        label = torch.full((m + 1,), -7, dtype=torch.int32, device="cuda")
        size = torch.full((m + 1,), -7, dtype=torch.int32, device="cuda")
        n_comp = torch.full((2,), -7, dtype=torch.int64, device="cuda")
        st = L.ctd_mesh_components_i32(f.data_ptr(), None if v is None else v.data_ptr(), n, m, int(drop), label.data_ptr(),
                                       size.data_ptr(), n_comp.data_ptr(), ws.data_ptr(), ws.numel(), 0,
                                       torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "ctd_mesh_components_i32")
        runs.append((host(label), host(size), host(n_comp)))
    for a, b in zip(*runs):
        assert np.array_equal(a, b), "two runs differ"
    assert torch.equal(f, f0) and (v is None or torch.equal(v.view(torch.int32), v0.view(torch.int32))), "an input was written"
    label, size, n_comp = runs[0]
    assert label[m] == -7 and size[m] == -7 and n_comp[1] == -7
    return label[:m], size[:m], int(n_comp[0])


def clean_c_call(faces, verts, n, drop, min_faces, largest, cap_faces, cap_verts, outputs=True):
    """ctd_mesh_clean_i32, twice -> faces_out [m+1,3], face_index [m+1], vert_index [n+1] (host, -7 where not written;
    None without outputs) and counts"""
    m = len(faces)
    f, v = _inputs(faces, verts)
    f0, v0 = f.clone(), None if v is None else v.clone()
    runs = []
    for _ in range(2):
        _lib, L, ws = _lib_and_ws(n, m)
        fo = torch.full((m + 1, 3), -7, dtype=torch.int32, device="cuda")
        fi = torch.full((m + 1,), -7, dtype=torch.int32, device="cuda")
        vi = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((5,), -7, dtype=torch.int64, device="cuda")
        p = (lambda t: t.data_ptr()) if outputs else (lambda t: None)
        st = L.ctd_mesh_clean_i32(f.data_ptr(), None if v is None else v.data_ptr(), n, m, int(drop), min_faces, int(largest),
                                  p(fo), p(fi), cap_faces, p(vi), cap_verts, counts.data_ptr(), ws.data_ptr(), ws.numel(), 0,
                                  torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "ctd_mesh_clean_i32")
        runs.append((host(fo), host(fi), host(vi), host(counts)))
    for a, b in zip(*runs):
        assert np.array_equal(a, b), "two runs differ"
    assert torch.equal(f, f0) and (v is None or torch.equal(v.view(torch.int32), v0.view(torch.int32))), "an input was written"
    fo, fi, vi, counts = runs[0]
    assert counts[4] == -7
    return fo, fi, vi, counts[:4]


def check_clean(faces, verts, n, what, min_faces_list=MIN_FACES, drops=(False, True)):
    """labels, sizes, and for every min_faces x keep_largest: the full call, count-only and a capacity of half
    -> {drop: (label, size, n_components)} of the restatement"""
    out = {}
    m = len(faces)
    for drop in drops:
        comps = mcr.components(faces, n, verts, drop)
        out[drop] = comps
        label, size, n_comp = components_c_call(faces, verts if drop else None, n, drop)
        assert np.array_equal(label, comps[0]) and np.array_equal(size, comps[1]) and n_comp == comps[2], "%s drop %s" % (what, drop)
        for min_faces, largest in itertools.product(min_faces_list, (False, True)):
            tag = "%s: drop %s min_faces %d keep_largest %s" % (what, drop, min_faces, largest)
            want = mcr.clean(faces, n, verts, min_faces, largest, drop, comps=comps)
            nv, nf = int(want["counts"][0]), int(want["counts"][1])
            fo, fi, vi, counts = clean_c_call(faces, verts, n, drop, min_faces, largest, m, n)
            assert counts.tolist() == want["counts"].tolist(), "%s: counts %s vs %s" % (tag, counts, want["counts"])
            assert np.array_equal(fo[:nf], want["faces"]) and (fo[nf:] == -7).all(), tag + ": faces_out"
            assert np.array_equal(fi[:nf], want["face_index"]) and (fi[nf:] == -7).all(), tag + ": face_index"
            assert np.array_equal(vi[:nv], want["vert_index"]) and (vi[nv:] == -7).all(), tag + ": vert_index"
            # count only: NULL outputs, whatever the capacities
            _, _, _, counts = clean_c_call(faces, verts, n, drop, min_faces, largest, -5, -5, outputs=False)
            assert counts.tolist() == want["counts"].tolist(), tag + ": count only"
            # a capacity of half: exactly the first half is written, the rest untouched, the counts true
            hf, hv = nf // 2, nv // 2
            fo, fi, vi, counts = clean_c_call(faces, verts, n, drop, min_faces, largest, hf, hv)
            assert counts.tolist() == want["counts"].tolist(), tag + ": half, counts"
            assert np.array_equal(fo[:hf], want["faces"][:hf]) and (fo[hf:] == -7).all(), tag + ": half, faces_out"
            assert np.array_equal(fi[:hf], want["face_index"][:hf]) and (fi[hf:] == -7).all(), tag + ": half, face_index"
            assert np.array_equal(vi[:hv], want["vert_index"][:hv]) and (vi[hv:] == -7).all(), tag + ": half, vert_index"
    return out


# ---------------------------------------------------------------------------------------------------------------------
# meshes from mesh.tsdf_mesh
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", GRIDS)
def test_clean_equals_the_restatement_on_random_volumes(mesh, dims):
    T, w = random_volume(dims, 7)
    origin, voxel = tr.grid_for("clean", T.shape[0], dims)
    seen_faces = 0
    for min_weight in (1.0, 2.0):
        got = mesh.tsdf_mesh(dev(T), dev(w), dev(origin), voxel, min_weight=min_weight)
        verts, faces, _ = got.track(0)
        verts, faces = host(verts), host(faces)
        comps = check_clean(faces, verts, len(verts), "%s min_weight %g" % (dims, min_weight))
        seen_faces += len(faces)
        label, size, n_comp = comps[False]
        sizes = np.unique(label, return_counts=True)[1] if len(label) else np.zeros(0, int)
        if dims == GRIDS[0] and min_weight == 1.0:
            unreferenced = len(verts) - len(np.unique(faces))
            print("%s: %d vertices, %d faces, %d unreferenced vertices, %d components, the largest of %d faces, %d of at most 8"
                  % (dims, len(verts), len(faces), unreferenced, n_comp, sizes.max(), (sizes <= 8).sum()))
            assert (len(verts), len(faces), unreferenced, n_comp) == (14832, 15879, 1885, 368)
            assert sizes.max() == 14008 and (sizes <= 8).sum() == 334
        if dims == (3, 43, 2) and min_weight == 1.0:
            assert n_comp == 19
    if dims == (5, 1, 4):
        assert seen_faces == 0                                      # no cell at all: the calls run on no face


# ---------------------------------------------------------------------------------------------------------------------
# the three-sphere volume
# ---------------------------------------------------------------------------------------------------------------------
SPHERES = ((4.3, (7.13, 7.79, 8.07)), (2.1, (17.2, 16.6, 15.9)), (2.0, (5.0, 18.0, 5.0)))


def three_spheres(n=24):
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    d = np.min([np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r for r, c in SPHERES], 0)
    return np.clip(0.25 * d, -0.9, 0.9).astype(F)[None], np.ones((1, n, n, n), F)


def closed_with_euler_2(faces, n_verts):
    n_edges = len(mr.directed_edge_counts(faces)) // 2
    return mr.is_closed_oriented_manifold(faces) and n_verts - n_edges + len(faces) == 2


def test_three_spheres(mesh, meshops):
    T, w = three_spheres()
    assert (T == 0).sum() == 7
    origin, voxel = tr.grid_for("clean", 1, (24, 24, 24))           # the grid of tests/test_tsdf_mesh_gpu.check_mesh
    got = mesh.tsdf_mesh(dev(T), dev(w), dev(origin), voxel)
    verts, faces, _ = got.track(0)
    hv, hf = host(verts), host(faces)
    assert hv.shape == (488, 3) and hf.shape == (964, 3)
    check_clean(hf, hv, 488, "three spheres", min_faces_list=(1, 105, 157, 705))
    label, size, n_comp = meshops.mesh_components(faces, 488)
    assert n_comp == 3 and sorted(np.unique(host(size)).tolist()) == [104, 156, 704]
    for lb in np.unique(host(label)):                               # three closed components
        assert mr.is_closed_oriented_manifold(hf[host(label) == lb])
    two = meshops.mesh_clean(verts, faces, min_faces=105, drop_degenerate=False)
    assert (two.n_components, two.n_components_kept, two.faces.shape[0]) == (3, 2, 704 + 156)
    one = meshops.mesh_clean(verts, faces, keep_largest=True, drop_degenerate=False)
    assert (one.n_components, one.n_components_kept, one.faces.shape[0]) == (3, 1, 704)
    assert closed_with_euler_2(host(one.faces), one.verts.shape[0])
    assert np.array_equal(host(one.verts).view(np.int32), hv[host(one.vert_index)].view(np.int32))
    # drop_degenerate drops exactly the faces with coincident vertices: 2 of them, at voxels of tsdf exactly 0 (at the
    # others the f32 positions of the crossings differ in their last bits)
    p = hv[hf]
    coincident = ((p[:, 0] == p[:, 1]).all(1) | (p[:, 0] == p[:, 2]).all(1) | (p[:, 1] == p[:, 2]).all(1))
    assert coincident.sum() == 2
    dropped = meshops.mesh_clean(verts, faces)
    assert dropped.faces.shape[0] == 962 and np.array_equal(host(dropped.face_index), np.nonzero(~coincident)[0])
    assert dropped.faces.dtype == torch.int32 and dropped.vert_index.dtype == torch.int32 and dropped.normals is None
    for t, rows in ((dropped.faces, 962), (dropped.face_index, 962), (dropped.vert_index, dropped.verts.shape[0])):
        assert t.is_contiguous() and t.untyped_storage().nbytes() == t.numel() * 4 and t.shape[0] == rows   # owns exactly its size


def test_a_tie_for_the_largest_component_keeps_the_lower_label(meshops, mesh):
    T1, w1, _ = mr.sphere_volume(10, 3.2)
    T, w = np.concatenate([T1, T1], 3), np.concatenate([w1, w1], 3)   # two copies side by side along x
    got = mesh.tsdf_mesh(dev(T), dev(w), dev(np.zeros((1, 3), F)), 1.0)
    verts, faces, _ = got.track(0)
    hv, hf = host(verts), host(faces)
    comps = check_clean(hf, hv, len(hv), "two spheres", min_faces_list=(1,))[False]
    labels, sizes = np.unique(comps[0], return_counts=True)
    assert len(labels) == 2 and sizes[0] == sizes[1] and labels[0] == 0
    c = meshops.mesh_clean(verts, faces, keep_largest=True, drop_degenerate=False)
    assert c.n_components == 2 and c.n_components_kept == 1 and c.faces.shape[0] == sizes[0]
    assert np.array_equal(host(c.face_index), np.nonzero(comps[0] == 0)[0])
    assert closed_with_euler_2(host(c.faces), c.verts.shape[0])


# ---------------------------------------------------------------------------------------------------------------------
# synthetic face lists
# ---------------------------------------------------------------------------------------------------------------------
def strip(m):
    i = np.arange(m)
    return np.stack([i, i + 1, i + 2], 1).astype(np.int32)


@pytest.mark.parametrize("order", ["permuted", "descending"])
def test_a_long_strip_is_one_component_labelled_0(order):
    """4096 faces in a strip: long parent chains whichever way the unions land"""
    m = 4096
    ids = np.random.RandomState(11).permutation(m + 2) if order == "permuted" else np.arange(m + 1, -1, -1)
    faces = ids.astype(np.int32)[strip(m)]
    comps = check_clean(faces, None, m + 2, "strip " + order, min_faces_list=(1, 4096, 4097), drops=(False,))[False]
    assert (comps[0] == 0).all() and (comps[1] == m).all() and comps[2] == 1


BIG = 256 * 1024                                                 # faces of 1024 workgroups: one full round of the scan


def pattern_mesh(m):
    """m faces in blocks of five, each block over ten vertices of its own: a triangle, a quad of two triangles, a
    triangle, and a face made invalid by a repeated index -> faces, n_verts and, by index arithmetic on the pattern,
    label, size and n_components"""
    f = np.arange(m)
    p, r = f // 5, f % 5
    corners = np.array([[0, 1, 2], [3, 4, 5], [3, 5, 6], [7, 8, 9], [7, 7, 8]])
    faces = (10 * p[:, None] + corners[r]).astype(np.int32)
    valid = r != 4
    label = np.where(valid, faces[:, 0], -1).astype(np.int32)     # the first index of a valid face is its block's smallest
    size = valid.astype(np.int32) + ((r == 1) & (f + 1 < m)) + (r == 2)   # (the last quad may lack its second half)
    return faces, 10 * ((m + 4) // 5), label, size, int((valid & (r != 2)).sum())


def straddled_capacity(flags):
    """a capacity one short of where the middle workgroup's kept items end: that workgroup writes some of them, not all"""
    ends = np.cumsum(np.add.reduceat(flags.astype(np.int64), np.arange(0, len(flags), 256)))
    i = len(ends) // 2
    assert ends[i] - ends[i - 1] >= 2
    return int(ends[i]) - 1


def check_pattern_mesh(m):
    """mesh_components and mesh_clean on pattern_mesh(m): more workgroup counts, of faces and of vertices, than one round
    of the scan takes (or exactly as many faces), a chunk of one face at BIG + 1"""
    faces, n, label, size, n_comp = pattern_mesh(m)
    got = components_c_call(faces, None, n, False)
    assert np.array_equal(got[0], label) and np.array_equal(got[1], size) and got[2] == n_comp, "m = %d: components" % m
    first_of_component = np.arange(m) % 5 != 2
    for min_faces in (1, 2):
        tag = "m = %d min_faces %d" % (m, min_faces)
        keep = size >= min_faces
        used = np.zeros(n, bool)
        used[faces[keep].reshape(-1)] = True
        want_vi, want_fi = np.nonzero(used)[0].astype(np.int32), np.nonzero(keep)[0].astype(np.int32)
        want_fo = (np.cumsum(used) - 1)[faces[keep]].astype(np.int32)
        nv, nf = len(want_vi), len(want_fi)
        want_counts = [nv, nf, n_comp, int((keep & first_of_component).sum())]
        assert nf > BIG // 4 and (want_counts[3] < n_comp) == (min_faces == 2)    # the cases are not vacuous
        # capacities: everything, and (min_faces 1) about half, inside a workgroup's kept items
        for cf, cv in ((m, n),) + (((straddled_capacity(keep), straddled_capacity(used)),) if min_faces == 1 else ()):
            fo, fi, vi, counts = clean_c_call(faces, None, n, False, min_faces, False, cf, cv)
            cf, cv = min(cf, nf), min(cv, nv)
            assert counts.tolist() == want_counts, "%s: counts %s vs %s" % (tag, counts, want_counts)
            assert np.array_equal(fo[:cf], want_fo[:cf]) and (fo[cf:] == -7).all(), tag + ": faces_out"
            assert np.array_equal(fi[:cf], want_fi[:cf]) and (fi[cf:] == -7).all(), tag + ": face_index"
            assert np.array_equal(vi[:cv], want_vi[:cv]) and (vi[cv:] == -7).all(), tag + ": vert_index"


@pytest.mark.parametrize("k", [255, 256, 257, 1, BIG - 1, BIG, BIG + 1])
def test_sizes_around_the_chunk(k):
    if k >= BIG - 1:                                               # too many faces for the restatement's union-find
        return check_pattern_mesh(k)
    rs = np.random.RandomState(k)
    n = k if k > 1 else 3
    first = rs.randint(0, n, k)
    faces = np.stack([first, first + rs.randint(0, 3, k), first + rs.randint(0, 4, k)], 1).astype(np.int32)   # some repeat, some leave [0, n)
    verts = rs.randint(0, 4, (n, 3)).astype(F)                       # many coincident positions
    comps = check_clean(faces, verts, n, "k = %d" % k, min_faces_list=(1, 2, 9))
    if k > 1:
        assert comps[False][2] > 3 and (comps[False][0] < 0).any() and comps[True][2] != comps[False][2]
    # k vertices under one face, one vertex under k faces
    check_clean(np.array([[0, k - 1, k // 2]], np.int32), verts, n, "one face", min_faces_list=(1, 2))
    check_clean(faces, verts[:1], 1, "one vertex", min_faces_list=(1,))


def test_invalid_faces_bad_indices_and_empty_meshes(meshops):
    n = 40
    verts = np.random.RandomState(3).randn(n, 3).astype(F)
    bad = np.array([[0, 0, 1], [-1, 2, 3], [4, 5, n], [6, 7, 1 << 30], [8, 9, 8], [-2147483648, 1, 2], [2147483647, 3, 4]], np.int32)
    comps = check_clean(bad, verts, n, "all invalid", min_faces_list=(1, 2))[True]
    assert (comps[0] == -1).all() and (comps[1] == 0).all() and comps[2] == 0
    mixed = np.concatenate([bad, strip(20), bad[::-1], strip(10) + 25]).astype(np.int32)
    comps = check_clean(mixed, verts, n, "mixed", min_faces_list=(1, 11, 21))[True]
    assert comps[2] == 2 and sorted(set(comps[0].tolist())) == [-1, 0, 25]
    check_clean(np.zeros((0, 3), np.int32), verts, n, "no faces", min_faces_list=(1, 2))
    check_clean(np.zeros((0, 3), np.int32), np.zeros((0, 3), F), 0, "no faces, no vertices", min_faces_list=(1,))
    check_clean(bad, np.zeros((0, 3), F), 0, "no vertices", min_faces_list=(1,))
    # the wrappers on empty tensors
    ev, ef = torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    c = meshops.mesh_clean(ev, ef, normals=ev)
    assert c.verts.shape == (0, 3) and c.faces.shape == (0, 3) and c.normals.shape == (0, 3) and c.n_components == 0
    label, size, n_comp = meshops.mesh_components(ef, 0)
    assert label.shape == (0,) and size.shape == (0,) and n_comp == 0
    c = meshops.mesh_clean(dev(verts), ef)
    assert c.verts.shape == (0, 3) and c.vert_index.shape == (0,) and c.n_components_kept == 0
    # host-side errors on device tensors
    f = dev(strip(5))
    with pytest.raises(RuntimeError, match=r"mesh_clean: faces must be shaped \[m,3\]"):
        meshops.mesh_clean(dev(verts), f.reshape(-1))
    with pytest.raises(RuntimeError, match="mesh_clean: faces: unsupported dtype"):
        meshops.mesh_clean(dev(verts), f.long())
    with pytest.raises(RuntimeError, match=r"mesh_clean: normals must be shaped \[40,3\]"):
        meshops.mesh_clean(dev(verts), f, normals=dev(verts[:5]))
    with pytest.raises(RuntimeError, match="mesh_clean: min_faces must be an integer >= 1"):
        meshops.mesh_clean(dev(verts), f, min_faces=0)
    with pytest.raises(RuntimeError, match="mesh_components: drop_degenerate needs verts"):
        meshops.mesh_components(f, n, drop_degenerate=True)
    with pytest.raises(RuntimeError, match=r"mesh_components: verts must be shaped \[41,3\]"):
        meshops.mesh_components(f, n + 1, verts=dev(verts))
    with pytest.raises(RuntimeError, match="contiguous"):
        meshops.mesh_clean(dev(verts), dev(np.zeros((5, 6), np.int32))[:, ::2])


# ---------------------------------------------------------------------------------------------------------------------
# clean_tsdf_mesh on the corner model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_clean_tsdf_mesh_on_the_corner_model(mesh, meshops, tmp_path, masked):
    """the corner model, every pixel integrated (3262 vertices, 6286 faces: one component, no vertex unreferenced, so the
    clean-up returns the mesh as it was) and with the views' keep masks (2957 vertices, 5684 faces: one component and one
    unreferenced vertex, so the indices move)"""
    from connecting_the_dots_amd import renderer
    from connecting_the_dots_amd import torchext as te
    sc = corner_model()
    vw = sc["views"]
    origin = dev(sc["origin"])
    T, w = te.tsdf_volume(1, *CORNER_DIMS)
    te.tsdf_integrate(T, w, origin, sc["voxel"], dev(vw["depth"]), dev(sc["ray"]), dev(sc["K"]), dev(vw["R"]), dev(vw["t"]),
                      valid=dev(vw["keep"]) if masked else None)
    got = mesh.tsdf_mesh(T, w, origin, sc["voxel"], return_normals=True)
    v0, f0, n0 = got.track(0)
    want = mcr.clean(host(f0), v0.shape[0], host(v0), min_faces=32, drop_degenerate=True)
    cleaned = meshops.clean_tsdf_mesh(got, min_faces=32)
    verts, faces, normals = cleaned.track(0)
    nv, nf, n_comp, n_kept = want["counts"].tolist()
    print("corner model: %d vertices, %d faces, %d components -> %d vertices, %d faces, %d components"
          % (v0.shape[0], f0.shape[0], n_comp, nv, nf, n_kept))
    assert 3000 < nf <= f0.shape[0] and (0 < nv < v0.shape[0] if masked else nv == v0.shape[0])
    assert cleaned._counts == [(nv, nf)] and host(cleaned.n_verts_per_track).tolist() == [nv]
    assert host(cleaned.n_faces_per_track).tolist() == [nf] and cleaned.n_faces_per_track.dtype == torch.int64
    assert np.array_equal(host(faces), want["faces"])
    hf = host(faces)
    assert hf.min() == 0 and hf.max() == nv - 1 and len(np.unique(hf)) == nv    # in range, and no vertex is unreferenced
    vi = want["vert_index"]
    for new, old in ((verts, v0), (normals, n0)):
        assert np.array_equal(host(new).view(np.int32), host(old)[vi].view(np.int32))
    assert np.array_equal(host(cleaned.src), host(got.src)[vi]) and cleaned.src.dtype == torch.int64
    bvh = renderer.MeshBVH(verts, faces)
    assert bvh.usable and bvh.matches(verts, faces)
    path = str(tmp_path / "clean.ply")
    mesh.save_ply(path, verts, faces, normals=normals)
    pv, pf, pn, _ = mesh.load_ply(path)
    assert pv.tobytes() == host(verts).tobytes() and pf.tobytes() == hf.tobytes() and pn.tobytes() == host(normals).tobytes()
    # without normals, and keep_largest
    plain = meshops.clean_tsdf_mesh(mesh.tsdf_mesh(T, w, origin, sc["voxel"]), keep_largest=True)
    assert plain.normals is None and plain.track(0)[2] is None
    top = mcr.clean(host(f0), v0.shape[0], host(v0), keep_largest=True, drop_degenerate=True)
    assert np.array_equal(host(plain.faces), top["faces"]) and plain._counts == [tuple(top["counts"][:2].tolist())]


def test_clean_tsdf_mesh_works_track_by_track(mesh, meshops):
    """two tracks of a random volume (109 components in the first): each track is cleaned on its own, its faces stay
    track-local, and verts, normals and src are the old rows of the track at its kept vertices"""
    dims = (64, 5, 7)
    T, w = random_volume(dims, 7)
    origin, voxel = tr.grid_for("clean", T.shape[0], dims)
    got = mesh.tsdf_mesh(dev(T), dev(w), dev(origin), voxel, return_normals=True)
    cleaned = meshops.clean_tsdf_mesh(got, min_faces=9, drop_degenerate=False)
    v_at = 0
    for b in range(T.shape[0]):
        v0, f0, n0 = got.track(b)
        want = mcr.clean(host(f0), v0.shape[0], min_faces=9)
        verts, faces, normals = cleaned.track(b)
        assert 0 < want["counts"][1] < f0.shape[0] and cleaned._counts[b] == tuple(want["counts"][:2].tolist())
        assert np.array_equal(host(faces), want["faces"])
        vi = want["vert_index"]
        for new, old in ((verts, v0), (normals, n0)):
            assert np.array_equal(host(new).view(np.int32), host(old)[vi].view(np.int32))
        k0 = sum(c[0] for c in cleaned._counts[:b])
        assert np.array_equal(host(cleaned.src)[k0:k0 + len(vi)], host(got.src)[v_at:v_at + v0.shape[0]][vi])
        v_at += v0.shape[0]
    assert host(cleaned.n_verts_per_track).tolist() == [c[0] for c in cleaned._counts]
    assert host(cleaned.n_faces_per_track).tolist() == [c[1] for c in cleaned._counts]
    assert cleaned.verts.shape[0] == sum(c[0] for c in cleaned._counts) == cleaned.src.shape[0]
