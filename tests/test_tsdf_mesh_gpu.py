"""GPU parity of the mesh extraction (mesh.tsdf_mesh, ctd_tsdf_mesh_faces_i32; include/ctd_hip_mesh.h) against the
restatement tests/mesh_ref.py, and the reference scene that closes the loop into the ray caster.

Faces and counts equal the restatement exactly (the rule is integer work over signs and flags, so any mismatch is a bug
on one of the two sides); the vertices have the bits of torchext.tsdf_surface_points; every call runs twice with equal
bits, from a workspace filled with a sentinel.

Reference scene, measured on an MI355X (the kernels are deterministic; the factor 2 is slack for later changes of the
scene helpers only).  The corner model of tests/tsdf_ref.make_corner_model with the constants of tests/test_tsdf_host.py
(B=1, views 0..3 of 48 x 80 integrated at their true poses into 72 x 48 x 32 voxels of 0.032), meshed, track(0) put
through renderer.MeshBVH and renderer.render_mesh at the two CAST poses, against tsdf_raycast of the same volume as
camera z:
  pose of view 0: the mesh is hit at 99.840 % of the 3747 pixels the ray cast hits (6 misses, all in the last image
                  row but one, where the cells at the rim of the observed band are not meshed); median
                  |z_mesh - z_cast| = 0.0038 voxel
  pose of view 4: 99.920 % of 3748 (3 misses); 0.0043 voxel
  (3262 vertices, 6286 faces; the restatements tests/tsdf_ref.py, tests/mesh_ref.py and the CPU oracle's ray caster give
  the same figures to every printed digit)
Pinned at 2 x the worse pose: a miss share of 2 x 0.160 %, a median of 2 x 0.0043 voxel."""
import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import tsdf_ref as tr
from tests.test_tsdf_host import CAST, CORNER_DIMS, CORNER_SHAPE, corner_model

pytestmark = pytest.mark.gpu

F = np.float32
B = 2
# (nx, ny, nz): 33 x 18 x 21 = 12474 voxels are 49 chunks of 256 with a ragged last one, and cells straddle every chunk
# border; 64 x 5 x 7 fills rows exactly; 2 x 2 x 2 is one cell in less than a wavefront; 5 x 1 x 4 has no cell at all;
# 3 x 43 x 2 = 258 voxels is one full chunk and a chunk of two voxels
GRIDS = [(33, 18, 21), (64, 5, 7), (2, 2, 2), (5, 1, 4), (3, 43, 2)]
# the one-workgroup scan takes 1024 workgroup counts a round, and the grids above give 98 at most.  64^3 is 1024 chunks a
# track: 2048 counts, two full rounds that meet on the track border; 64 x 64 x 65 is 1040 chunks a track: 2080 counts,
# three rounds, a round border inside track 1.  257 voxels leave one live thread in the last chunk; 64 x 4 is one chunk
SCAN_GRIDS = [(64, 64, 64), (64, 64, 65), (257, 1, 1), (64, 4, 1)]
SENTINEL = 0xA5

MIN_MESH_SHARE = 1 - 2 * 0.00160                                # measured 99.840 % / 99.920 %
MAX_MESH_MEDIAN_VOXELS = 2 * 0.0043                             # measured 0.0038 / 0.0043 voxel


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


@pytest.fixture(scope="module")
def mesh():
    from connecting_the_dots_amd import mesh
    return mesh


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(t):
    a = host(t)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def random_volume(dims, seed, empty_track=None):
    """tsdf uniform in (-0.9, 0.9), a tenth of the weights 0 (the tsdf there is NaN: it is never read); the others 1 or 2"""
    nx, ny, nz = dims
    rs = np.random.RandomState(seed)
    tsdf = rs.uniform(-0.9, 0.9, (B, nz, ny, nx))
    weight = rs.randint(1, 3, (B, nz, ny, nx)) * (rs.rand(B, nz, ny, nx) >= 0.1)
    if empty_track is not None:
        weight[empty_track] = 0
    return np.where(weight == 0, np.nan, tsdf).astype(F), weight.astype(F)


def faces_c_call(T, w, min_weight, faces, capacity):
    """ctd_tsdf_mesh_faces_i32 on device tensors, from a workspace filled with a sentinel (faces None: count only)
    -> n_faces_per_track"""
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    Bb, nz, ny, nx = T.shape
    n_faces = torch.full((Bb,), -1, dtype=torch.int64, device="cuda")
    ws = torch.full((L.ctd_tsdf_mesh_workspace_bytes(Bb, nx, ny, nz),), SENTINEL, dtype=torch.uint8, device="cuda")
    st = L.ctd_tsdf_mesh_faces_i32(T.data_ptr(), w.data_ptr(), min_weight, None if faces is None else faces.data_ptr(),
                                   n_faces.data_ptr(), capacity, Bb, nx, ny, nz, ws.data_ptr(), ws.numel(), 0,
                                   torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "ctd_tsdf_mesh_faces_i32")
    return n_faces


def check_mesh(te, mesh, T, w, min_weight, what):
    """every property of one volume -> (number of faces, set of the cases the restatement met)"""
    Bb, nz, ny, nx = T.shape
    origin, voxel = tr.grid_for("clean", Bb, (nx, ny, nz))
    want_faces, want_count = mr.faces(T, w, min_weight)
    t_in = [dev(T), dev(w), dev(origin)]
    before = [x.clone() for x in t_in]
    got = mesh.tsdf_mesh(*t_in, voxel, min_weight=min_weight, return_normals=True)
    again = mesh.tsdf_mesh(*t_in, voxel, min_weight=min_weight, return_normals=True)
    for x, x0 in zip(t_in, before):
        assert torch.equal(x.view(torch.int32), x0.view(torch.int32)), what + ": an input was written"
    # the faces and their counts
    assert got.faces.dtype == torch.int32 and got.faces.is_contiguous() and got.n_faces_per_track.dtype == torch.int64
    assert np.array_equal(host(got.n_faces_per_track), want_count), "%s: counts %s vs %s" % (what, host(got.n_faces_per_track),
                                                                                           want_count)
    assert got.faces.shape == want_faces.shape and np.array_equal(host(got.faces), want_faces), what + ": faces"
    # the vertices are the surface points, bit for bit
    points, src, n_per_track, normals = te.tsdf_surface_points(*t_in, voxel, min_weight=min_weight, return_normals=True)
    assert np.array_equal(bits(got.verts), bits(points)) and np.array_equal(bits(got.src), bits(src)), what
    assert np.array_equal(bits(got.normals), bits(normals)) and np.array_equal(bits(got.n_verts_per_track), bits(n_per_track))
    assert mesh.tsdf_mesh(*t_in, voxel, min_weight=min_weight).normals is None
    # two runs
    for a, b in ((got.faces, again.faces), (got.n_faces_per_track, again.n_faces_per_track), (got.verts, again.verts)):
        assert np.array_equal(bits(a), bits(b)), what + ": two runs differ"
    # track(b): contiguous slices, every index below the track's number of vertices
    n_verts, f0, v0 = host(n_per_track), 0, 0
    for b in range(Bb):
        vb, fb, nb = got.track(b)
        assert vb.is_contiguous() and fb.is_contiguous() and nb.is_contiguous()
        assert vb.shape == (n_verts[b], 3) and nb.shape == vb.shape and fb.shape == (want_count[b], 3)
        assert np.array_equal(host(fb), want_faces[f0:f0 + want_count[b]]) and np.array_equal(bits(vb), bits(points[v0:v0 + n_verts[b]]))
        if want_count[b]:
            assert 0 <= int(fb.min()) and int(fb.max()) < n_verts[b], what
        f0, v0 = f0 + want_count[b], v0 + n_verts[b]
    # count only, and a capacity below the count: exactly the first faces, nothing past them, the true counts
    m = len(want_faces)
    assert np.array_equal(host(faces_c_call(t_in[0], t_in[1], min_weight, None, 0)), want_count), what
    assert np.array_equal(host(faces_c_call(t_in[0], t_in[1], min_weight, None, -5)), want_count), what
    for cap in sorted({0, m // 2, max(m - 1, 0), m}):
        buf = torch.full((m + 1, 3), -7, dtype=torch.int32, device="cuda")
        assert np.array_equal(host(faces_c_call(t_in[0], t_in[1], min_weight, buf, cap)), want_count), what
        assert np.array_equal(host(buf)[:cap], want_faces[:cap]) and (host(buf)[cap:] == -7).all(), "%s: capacity %d" % (what, cap)
    case, meshed = mr.cell_cases(T, w, min_weight)
    return m, set(case[meshed].tolist())


@pytest.mark.parametrize("dims", GRIDS + SCAN_GRIDS)
def test_faces_equal_the_restatement(te, mesh, dims):
    n_faces, cases = 0, set()
    runs = ((0, 1.0, None), (1, 2.0, None), (2, 1.0, 1), (3, 1.0, 0))
    for seed, min_weight, empty in runs[:1] if dims in SCAN_GRIDS[:2] else runs:    # (one volume of half a million voxels)
        T, w = random_volume(dims, seed, empty_track=empty)
        m, met = check_mesh(te, mesh, T, w, min_weight, "%s seed %d min_weight %g" % (dims, seed, min_weight))
        n_faces += m
        if seed == 0:
            cases = met
    if dims == GRIDS[0]:
        assert cases == set(range(256))                             # the restatement met every case, so the kernel did
        assert n_faces > 10000
    if dims in SCAN_GRIDS[:2]:
        assert n_faces > 100000                                     # the cases are not vacuous
    if dims in ((5, 1, 4), (257, 1, 1), (64, 4, 1)):
        assert n_faces == 0


def test_a_sphere_comes_out_closed_and_facing_outwards(mesh):
    T, w, centre = mr.sphere_volume(20, 7.3)
    origin = np.zeros((1, 3), F)
    got = mesh.tsdf_mesh(dev(T), dev(w), dev(origin), 1.0)
    verts, faces, normals = got.track(0)
    assert normals is None
    f, p = host(faces), host(verts).astype(np.float64)
    assert mr.is_closed_oriented_manifold(f)
    n_edges = len(mr.directed_edge_counts(f)) // 2
    assert len(p) - n_edges + len(f) == 2
    nrm = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert ((nrm * (p[f].mean(1) - centre)).sum(1) > 0).all()


def test_bad_inputs_are_rejected_loudly_and_empty_batches_work(mesh):
    dims = (6, 5, 4)
    T, w = (dev(x) for x in random_volume(dims, 5))
    origin = dev(tr.grid_for("clean", B, dims)[0])
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(RuntimeError, match="voxel must be a finite number > 0"):
            mesh.tsdf_mesh(T, w, origin, bad)
        with pytest.raises(RuntimeError, match="min_weight must be a finite number > 0"):
            mesh.tsdf_mesh(T, w, origin, 0.1, min_weight=bad)
    wide = torch.zeros((B, 4, 5, 12), device="cuda")[..., ::2]
    with pytest.raises(RuntimeError, match="contiguous"):
        mesh.tsdf_mesh(wide, w, origin, 0.1)
    for k in range(3):
        args = [T, w, origin]
        args[k] = args[k].cpu()
        with pytest.raises(RuntimeError):
            mesh.tsdf_mesh(*args, 0.1)
    with pytest.raises(RuntimeError, match=r"tsdf and weight \[B,nz,ny,nx\]"):
        mesh.tsdf_mesh(T[0], w[0], origin, 0.1)
    with pytest.raises(RuntimeError, match=r"origin must be shaped \[B,3\]"):
        mesh.tsdf_mesh(T, w, origin[:1].contiguous(), 0.1)
    with pytest.raises(RuntimeError):
        mesh.tsdf_mesh(T.double(), w, origin, 0.1)
    got = mesh.tsdf_mesh(T, w, origin, 0.1)
    for bad in (-1, B, 0.0, None, True):
        with pytest.raises(RuntimeError, match="b must be an integer in"):
            got.track(bad)
    # B == 0: empty outputs of the right shapes and dtypes, nothing launched
    e = mesh.tsdf_mesh(torch.empty((0, 4, 5, 6), device="cuda"), torch.empty((0, 4, 5, 6), device="cuda"),
                       torch.empty((0, 3), device="cuda"), 0.1, return_normals=True)
    assert e.verts.shape == (0, 3) and e.faces.shape == (0, 3) and e.faces.dtype == torch.int32 and e.normals.shape == (0, 3)
    assert e.src.shape == (0,) and e.n_verts_per_track.shape == (0,) and e.n_faces_per_track.shape == (0,)
    assert e.n_faces_per_track.dtype == torch.int64
    # a volume without a crossing: no vertices, no faces
    none = mesh.tsdf_mesh(torch.ones_like(T), torch.zeros_like(w), origin, 0.1)
    assert none.faces.shape == (0, 3) and host(none.n_faces_per_track).tolist() == [0, 0] and none.track(1)[0].shape == (0, 3)


def test_the_mesh_of_the_corner_model_renders_like_its_ray_cast(te, mesh):
    """tsdf_integrate -> tsdf_mesh -> track(0) -> MeshBVH -> render_mesh at the CAST poses against tsdf_raycast of the
    same volume, as camera z: share of the ray-cast hits the mesh also hits 99.840 % / 99.920 % (pinned at 99.680 %),
    median difference 0.0038 / 0.0043 voxel (pinned at 0.0086)"""
    from connecting_the_dots_amd import renderer
    sc = corner_model()
    vw = sc["views"]
    H, W = CORNER_SHAPE[2:]
    ray, K, origin = dev(sc["ray"]), dev(sc["K"]), dev(sc["origin"])
    T, w = te.tsdf_volume(1, *CORNER_DIMS)
    te.tsdf_integrate(T, w, origin, sc["voxel"], dev(vw["depth"]), ray, K, dev(vw["R"]), dev(vw["t"]))
    cast = te.tsdf_raycast(T, w, origin, sc["voxel"], ray, dev(sc["R_cast"]), dev(sc["t_cast"]), H, W, CAST["d_min"],
                           CAST["step"], CAST["n_steps"])
    z_cast = host(cast)[0].astype(np.float64) * sc["ray"][:, 2].reshape(H, W)
    got = mesh.tsdf_mesh(T, w, origin, sc["voxel"], return_normals=True)
    verts, faces, normals = got.track(0)
    print("corner model: %d vertices, %d faces" % (verts.shape[0], faces.shape[0]))
    assert faces.shape[0] > 3000
    bvh = renderer.MeshBVH(verts, faces)
    assert bvh.usable and bvh.matches(verts, faces)
    Kh = sc["K"]
    shader = renderer.PyShader(0.5, 0.5, 0.0, 1.0)
    for v in range(2):
        cam = renderer.PyCamera(Kh[0, 0], Kh[1, 1], Kh[0, 2], Kh[1, 2], sc["R_cast"][0, v], sc["t_cast"][0, v], W, H)
        z_mesh = host(renderer.render_mesh(verts, torch.ones_like(verts), normals, faces, cam, shader, bvh=bvh)[0])
        hit_cast, hit_mesh = np.isfinite(z_cast[v]), z_mesh > 0
        both = hit_cast & hit_mesh
        share = both.sum() / hit_cast.sum()
        med = float(np.median(np.abs(z_mesh.astype(np.float64) - z_cast[v])[both])) / sc["voxel"]
        print("cast pose %d: the mesh is hit at %.4f %% of the %d pixels the ray cast hits; median |z_mesh - z_cast| %.5f voxel"
              % (v, 100 * share, hit_cast.sum(), med))
        assert hit_cast.sum() > 0.9 * H * W
        assert share >= MIN_MESH_SHARE
        assert med <= MAX_MESH_MEDIAN_VOXELS
