"""BVH ray caster (renderer.MeshBVH, render_mesh_proj / render_mesh with bvh=): every output buffer bit for bit
equal to the brute-force caster, on the goldens and on meshes built to break pruning, ties and the build."""
import numpy as np
import pytest
import torch

from tests import bvh_scenes, workloads
from tests.util import assert_close, golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = ((1, True, (0.5, 1.5, 0.0, 10.0)), (2, True, (0.3, 1.0, 0.4, 8.0)), (3, False, (0.5, 1.5, 0.0, 10.0)))


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cams(K, R, t, W, H):
    from connecting_the_dots_amd import renderer
    return renderer.PyCamera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], R, t, W, H)


def both(verts, colors, faces, cam, proj, shader=(0.5, 1.5, 0.0, 10.0), pat=None, d_alpha=0.0, d_beta=0.35,
         normals=None):
    """renders mesh_proj and mesh by brute force and through a fresh BVH; asserts all six buffers equal bitwise"""
    from connecting_the_dots_amd import renderer
    v = torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(DEV)
    c = torch.from_numpy(np.ascontiguousarray(colors, np.float32)).to(DEV)
    f = torch.from_numpy(np.ascontiguousarray(faces, np.int32).reshape(-1, 3)).to(DEV)
    nrm = c if normals is None else torch.from_numpy(np.ascontiguousarray(normals, np.float32)).to(DEV)
    pc, pp = cams(*cam), cams(*proj)
    sh = renderer.PyShader(*shader)
    pat = bvh_scenes.pattern(pp.height, pp.width) if pat is None else pat
    pt = torch.from_numpy(pat).to(DEV)
    bvh = renderer.MeshBVH(v, f)
    assert bvh.n_faces == f.shape[0]
    ref = renderer.render_mesh_proj(v, c, f, pc, pp, sh, pt, d_alpha, d_beta)
    got = renderer.render_mesh_proj(v, c, f, pc, pp, sh, pt, d_alpha, d_beta, bvh=bvh)
    for name, a, b in zip(("depth", "color", "normal"), ref, got):
        assert np.array_equal(bits(a), bits(b)), "mesh_proj %s differs through the BVH" % name
    ref = renderer.render_mesh(v, c, nrm, f, pc, sh)
    got = renderer.render_mesh(v, c, nrm, f, pc, sh, bvh=bvh)
    for name, a, b in zip(("depth", "color", "normal"), ref, got):
        assert np.array_equal(bits(a), bits(b)), "mesh %s differs through the BVH" % name
    return bvh, ref


@pytest.mark.parametrize("k", range(3))
def test_goldens_through_bvh(k):
    from connecting_the_dots_amd import renderer
    seed, wall, shader = CASES[k]
    sc = workloads.render_scene(seed, wall=wall)
    g = golden("render")
    cam, proj = cams(*sc["cam"]), cams(*sc["proj"])
    data = renderer.PyRenderInput(verts=sc["verts"], colors=sc["colors"], faces=sc["faces"])
    r = renderer.PyRenderer(cam, renderer.PyShader(*shader), engine='gpu', accel='bvh')
    r.mesh_proj(data, proj, sc["pattern"], d_alpha=sc["d_alpha"], d_beta=sc["d_beta"])
    assert np.array_equal(r.depth(), g["depth_%d" % k]) and np.array_equal(r.color(), g["color_%d" % k])
    if shader[2] == 0.0:
        assert np.array_equal(r.normal(), g["normal_%d" % k])
    else:                                   # ks != 0: powf's last bits (as in test_render_gpu.py)
        assert_close(r.normal(), g["normal_%d" % k], rtol=1e-5, atol=1e-6, what="ambient image")
    normals = workloads.render_normals(sc, seed)
    data_m = renderer.PyRenderInput(verts=sc["verts"], colors=sc["colors"], normals=normals, faces=sc["faces"])
    r.mesh(data_m)
    assert np.array_equal(r.depth(), g["mesh_depth_%d" % k]) and np.array_equal(r.normal(), g["mesh_normal_%d" % k])
    if shader[2] == 0.0:
        assert np.array_equal(r.color(), g["mesh_color_%d" % k])
    else:
        assert_close(r.color(), g["mesh_color_%d" % k], rtol=1e-5, atol=1e-6, what="shaded colour")
    # and against the brute-force kernel, bit for bit, whatever ks
    both(sc["verts"], sc["colors"], sc["faces"], sc["cam"], sc["proj"], shader, sc["pattern"], sc["d_alpha"],
         sc["d_beta"], normals=normals)


def test_get_mesh_like_scene():
    """(a) the board x 500 next to four procedural objects of ~10-25 K faces each"""
    v, c, f = bvh_scenes.get_mesh_like(60000, 3)
    for H, W in ((120, 160), (60, 80)):
        bvh, (d, _, _) = both(v, c, f, bvh_scenes.camera(H, W), bvh_scenes.camera(H, W, t=(0.075, 0, 0)))
        assert (d.cpu().numpy() > 0).mean() > 0.9


def test_behind_camera_and_projector():
    """(b) ray_tri does not test t > 0: geometry behind the camera wins with a negative t"""
    rs = np.random.RandomState(1)
    v, f = bvh_scenes.icosphere(2)
    parts, faces, n = [], [], 0
    for z in (-2.0, -0.5, 1.5, 3.0):
        parts.append(v * 0.4 + np.array([rs.uniform(-0.3, 0.3), rs.uniform(-0.3, 0.3), z]))
        faces.append(f + n)
        n += len(v)
    verts = np.concatenate(parts).astype(np.float32)
    faces = np.concatenate(faces)
    colors = rs.uniform(0, 1, verts.shape).astype(np.float32)
    _, (d, _, _) = both(verts, colors, faces, bvh_scenes.camera(24, 32), bvh_scenes.camera(24, 32, t=(0.075, 0, 0)))
    assert (d.cpu().numpy() < 0).any() and (d.cpu().numpy() != -1).any()


def test_duplicate_and_coplanar_faces():
    """(c) equal t: the lowest face index must win, in any visiting order"""
    rs = np.random.RandomState(2)
    quad = np.array([[-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2]], np.float32)
    verts = np.concatenate([quad, quad * [0.5, 0.5, 1], quad * [1.5, 1.5, 1]]).astype(np.float32)
    base = np.array([[0, 1, 2], [0, 2, 3]])
    faces = np.concatenate([base, base + 4, base, base + 8, base + 4, base[::-1]] * 3)
    colors = rs.uniform(0, 1, verts.shape).astype(np.float32)
    both(verts, colors, faces, bvh_scenes.camera(24, 32), bvh_scenes.camera(24, 32, t=(0.075, 0, 0)))


def test_grid_on_pixel_rays():
    """(d) vertices and edges exactly on pixel rays: a grid at z = 1 with one vertex per pixel centre"""
    H, W = 16, 24
    K = bvh_scenes.camera(H, W, f=8.0)
    ys, xs = np.meshgrid(np.arange(H + 1) - 0.5, np.arange(W + 1) - 0.5, indexing="ij")
    verts = np.stack([(xs - K[0][0, 2]) / 8.0, (ys - K[0][1, 2]) / 8.0, np.ones_like(xs)], -1).reshape(-1, 3)
    ys2, xs2 = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    verts = np.concatenate([verts, np.stack([(xs2 - K[0][0, 2]) / 8.0, (ys2 - K[0][1, 2]) / 8.0,
                                             np.full(xs2.shape, 1.5)], -1).reshape(-1, 3)]).astype(np.float32)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    a = (i * (W + 1) + j).reshape(-1)
    faces = np.concatenate([np.stack([a, a + 1, a + W + 2], 1), np.stack([a, a + W + 2, a + W + 1], 1)])
    colors = np.random.RandomState(3).uniform(0, 1, verts.shape).astype(np.float32)
    both(verts, colors, faces, K, bvh_scenes.camera(H, W, t=(0.075, 0, 0), f=8.0))


def test_grazing_faces():
    """(e) faces nearly parallel to the rays: |det| just above and below 1e-6"""
    rs = np.random.RandomState(4)
    verts, faces = [], []
    for k, eps in enumerate(np.geomspace(1e-9, 1e-3, 40)):
        x, y = rs.uniform(-0.4, 0.4, 2)
        z = rs.uniform(1, 3)
        p = np.array([x * z, y * z, z])
        dvec = p / np.linalg.norm(p)
        side = np.cross(dvec, [0, 1, 0])
        side /= np.linalg.norm(side)
        tilt = np.cross(dvec, side)
        s = rs.uniform(0.01, 0.5)
        verts += [p - s * dvec, p + s * dvec + eps * tilt, p + s * side * 0.1]
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
    verts = np.array(verts, np.float32)
    colors = rs.uniform(0, 1, verts.shape).astype(np.float32)
    both(verts, colors, np.array(faces), bvh_scenes.camera(32, 40), bvh_scenes.camera(32, 40, t=(0.075, 0, 0)))


def test_degenerate_and_nonfinite_faces():
    """(f) zero-area faces and faces with NaN / Inf vertices among ordinary ones"""
    rs = np.random.RandomState(5)
    v, f = bvh_scenes.icosphere(2)
    v = (v * 0.5 + [0, 0, 2]).astype(np.float32)
    bad = np.array([[np.nan, 0, 2], [np.inf, 0, 2], [0, -np.inf, 2], [0.1, 0.1, 1.5], [0.1, 0.1, 1.5],
                    [0.2, 0.2, 1.5], [1e30, 1e30, 2], [-1e30, 1e30, 2]], np.float32)
    verts = np.concatenate([v, bad]).astype(np.float32)
    n = len(v)
    extra = np.array([[n, 0, 1], [n + 1, 2, 3], [n + 2, 4, 5], [n + 3, n + 4, n + 5], [n + 3, n + 3, n + 3],
                      [n + 6, n + 7, 6], [0, 1, n + 1]])
    faces = np.concatenate([extra[:3], f, extra[3:]])
    colors = rs.uniform(0, 1, verts.shape).astype(np.float32)
    both(verts, colors, faces, bvh_scenes.camera(24, 32), bvh_scenes.camera(24, 32, t=(0.075, 0, 0)))


@pytest.mark.parametrize("n", [0, 1, 257])
def test_face_counts_and_camera_inside(n):
    """(g) 0, 1 and 257 faces; the camera inside the mesh's bounding box"""
    rs = np.random.RandomState(6 + n)
    verts = rs.uniform(-1, 1, size=(max(3, 3 * n), 3)).astype(np.float32)
    faces = np.arange(3 * n).reshape(-1, 3)
    colors = rs.uniform(0, 1, verts.shape).astype(np.float32)
    _, (d, _, _) = both(verts, colors, faces, bvh_scenes.camera(16, 24), bvh_scenes.camera(16, 24, t=(0.075, 0, 0)))
    if n == 0:
        assert (d.cpu().numpy() == -1).all()


def test_fuzz():
    """(h) ~100 seeded random small scenes: random triangles, poses, sizes; tools/fuzz_render_bvh.py soaks longer"""
    for seed in range(100):
        rs = np.random.RandomState(1000 + seed)
        n = int(rs.choice([2, 5, 17, 60, 200]))
        scale = 10.0 ** rs.uniform(-3, 1)
        centre = rs.normal(size=3) * [1, 1, 2]
        verts = (centre + rs.normal(size=(3 * n, 3)) * scale).astype(np.float32)
        if rs.rand() < 0.3:                                        # shared vertices, i.e. a connected soup
            faces = rs.randint(0, 3 * n, size=(n, 3))
        else:
            faces = np.arange(3 * n).reshape(-1, 3)
        colors = rs.uniform(0, 1, verts.shape).astype(np.float32)
        H, W = int(rs.randint(3, 20)), int(rs.randint(3, 20))
        R = bvh_scenes.rand_rot(rs) if rs.rand() < 0.5 else np.eye(3)
        both(verts, colors, faces, bvh_scenes.camera(H, W, t=rs.normal(size=3) * 0.3, R=R, f=rs.uniform(2, 30)),
             bvh_scenes.camera(H + 1, W + 2, t=rs.normal(size=3) * 0.3, f=rs.uniform(2, 30)))


def test_build_is_deterministic():
    from connecting_the_dots_amd import renderer
    v, c, f = bvh_scenes.get_mesh_like(20000, 7)
    vt, ft = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    a, b = renderer.MeshBVH(vt, ft), renderer.MeshBVH(vt, ft)
    assert a.nbytes == b.nbytes and a.depth == b.depth and 0 < a.depth
    assert torch.equal(a.buffer, b.buffer)


def test_deep_trees_render_identically_or_fall_back():
    """centroids whose Morton codes have distinct top bits form a chain; all-equal codes tie on the face index.
    Either the tree renders bit-exactly or the builder refuses it (usable False) and the renderers fall back."""
    pts = []
    for p in range(62, -1, -1):                      # one centroid per Morton bit: axis p % 3, coordinate bit p // 3
        q = [0.0, 0.0, 0.0]
        q[2 - p % 3] = float(2 ** (p // 3))
        for _ in range(4):
            pts.append(q)
    pts += [[0.0, 0.0, 0.0]] * 64
    pts = np.array(pts, np.float64) * 1e-5 + [0, 0, 1]
    tri = np.array([[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]])
    verts = (pts[:, None, :] + tri[None]).reshape(-1, 3).astype(np.float32)
    faces = np.arange(len(verts)).reshape(-1, 3)
    colors = np.random.RandomState(8).uniform(0, 1, verts.shape).astype(np.float32)
    bvh, _ = both(verts, colors, faces, bvh_scenes.camera(16, 16, f=400), bvh_scenes.camera(16, 16, t=(0.01, 0, 0), f=400))
    assert bvh.usable == (bvh.depth <= 62)
    same = np.tile(np.array([[-0.5, -0.5, 2], [0.5, -0.5, 2], [0, 0.5, 2]], np.float32), (300, 1))
    bvh, _ = both(same, np.ones_like(same), np.arange(900).reshape(-1, 3), bvh_scenes.camera(16, 16),
                  bvh_scenes.camera(16, 16, t=(0.075, 0, 0)))
    assert bvh.usable


def test_track_sample_and_pyrenderer_accel():
    from connecting_the_dots_amd import renderer, synth
    v, c, f = bvh_scenes.get_mesh_like(8000, 9)
    mesh = dict(verts=v, colors=c, faces=f)
    H, W = 48, 64
    K = bvh_scenes.camera(H, W)[0]
    pat = torch.from_numpy(bvh_scenes.pattern(H, W)).to(DEV)
    pats = [p.contiguous() for p in synth.scale_patterns(pat, [(H >> s, W >> s) for s in range(2)])]
    outs = []
    for bvh in (None, "auto"):
        g = torch.Generator(device=DEV)
        g.manual_seed(0)
        outs.append(synth.render_track_sample(mesh, pats, K, np.random.RandomState(0), track_length=2, generator=g,
                                              bvh=bvh))
    assert outs[0].keys() == outs[1].keys()
    for k in outs[0]:
        a, b = outs[0][k], outs[1][k]
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                  b.view(torch.int32) if b.dtype == torch.float32 else b), k
    cam, proj = cams(*bvh_scenes.camera(H, W)), cams(*bvh_scenes.camera(H, W, t=(0.075, 0, 0)))
    data = renderer.PyRenderInput(verts=v, colors=c, faces=f)
    res = []
    for accel in (None, "bvh"):
        r = renderer.PyRenderer(cam, renderer.PyShader(0.5, 1.5, 0.0, 10), accel=accel)
        r.mesh_proj(data, proj, bvh_scenes.pattern(H, W), d_alpha=0, d_beta=0.35)
        res.append([x.copy() for x in (r.depth(), r.color(), r.normal())])
    for a, b in zip(*res):
        assert np.array_equal(bits(a), bits(b))
    assert data._bvh is not None
    data.set_verts(v + 0.25)                       # invalidates the cached tree
    assert data._bvh is None
