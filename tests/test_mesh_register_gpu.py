"""GPU parity of the point-to-mesh ICP (meshreg.mesh_icp_system, mesh_icp_update, mesh_icp, register_mesh,
aligned_reconstruction_error; include/ext/ctd_hip_mesh_register.h) against tests/meshreg_ref.py.

The hinted nearest-face query gives the unhinted one's bits for any hint: face, closest and the point metric's residual
sqrtf(d2) are compared through mesh_icp_system's maps (d2 is a function of the posed point, the face and the closest
point, which are equal), and the unhinted maps against `meshsdf.point_mesh_signed_distance` on the posed points, the
query that stood before.  A mesh with an out-of-range face can only be queried by brute force (`renderer.MeshBVH` refuses
it), which ignores the hint; the tree is fed -1, n_faces and values far outside [0, n_faces) instead.
The system equals the restatement in all 29 entries as int64 (the restatement sums in the header's order), face and
residual equal it at every element, NaN masks included, and two runs give the same bits.  The update is held to what
tests/test_depth_icp_gpu.py holds depth_icp_update to: ok equal, |dR_ij| <= 2^-23, |dt_i| <= 2^-23 * max(1, max |t|), a
refused pose bit for bit.  mesh_icp meets the thresholds of tests/test_mesh_register_host.py."""
import numpy as np
import pytest
import torch

from tests import meshreg_ref as mr
from tests.test_mesh_register_host import (CORNER_ITERS, CORNER_SEED, MAX_DIST, MAX_ROT_DEG, MAX_ROT_DEG_NOISY, MAX_T,
                                           MAX_T_NOISY, NOISE, identity)

pytestmark = pytest.mark.gpu

F = np.float32
ULP = 2.0 ** -23
SIZES = [1, 255, 1024, 1025, 2500]


@pytest.fixture(scope="module")
def mg():
    from connecting_the_dots_amd import meshreg
    return meshreg


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(t):
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def equal_bits(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)), what


def same_float(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: the NaN positions differ at %d elements" % (
        what, int((np.isnan(got) != np.isnan(want)).sum()))
    a, b = np.nan_to_num(got, nan=0.0).view(np.int32), np.nan_to_num(want, nan=0.0).view(np.int32)
    assert np.array_equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.size)


def poses(K, seed=0):
    """the identity, then small motions about the corner"""
    rs = np.random.RandomState(seed)
    R, t = identity(K)
    for k in range(1, K):
        R[k] = mr.rotation(rs.normal(size=3), 2.0 * k).astype(F)
        t[k] = (rs.normal(size=3) * 0.01 * k).astype(F)
    return R, t


def near_corner(rs, n, spread=0.02):
    """n points within about `spread` of the corner's surface"""
    return (mr.corner_points(rs, n, limit=0.95) + rs.normal(size=(n, 3)) * spread).astype(F)


def bisector_points(rs, n):
    """points exactly equidistant from two squares of the corner: two coordinates equal (0.05 .. 0.3), the third 0.35 .. 0.9"""
    a = (rs.randint(50, 300, size=n) / 1000.0).astype(F)
    z = (rs.rand(n) * 0.55 + 0.35).astype(F)
    P = np.empty((n, 3), F)
    which = rs.randint(0, 3, size=n)
    for i in range(n):
        k = which[i]
        P[i, k], P[i, (k + 1) % 3], P[i, (k + 2) % 3] = z[i], a[i], a[i]
    return P


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quads", [6, 29])
def test_a_hint_changes_no_bit(mg, quads):
    """216 and 5046 faces, 2500 points of which 500 lie on the corner's bisector planes; with and without a cutoff, brute
    force and a forced tree, K = 2"""
    from connecting_the_dots_amd import meshsdf
    from connecting_the_dots_amd.renderer import MeshBVH
    rs = np.random.RandomState(quads)
    verts, faces = mr.corner_mesh(quads)
    n_faces, per = len(faces), len(faces) // 3
    pts = np.concatenate([near_corner(rs, 2000, 0.05), bisector_points(rs, 500)])
    R, t = identity(2)
    R[1], t[1] = mr.rotation([1, 2, 3], 1.0).astype(F), np.array([0.004, -0.003, 0.002], F)
    d_pts, d_verts, d_faces, d_R, d_t = dev(pts), dev(verts), dev(faces), dev(R), dev(t)
    tree = MeshBVH(d_verts, d_faces)
    assert tree.usable
    # the nearest face of square 1 alone (the plane y = 0), as an index into the whole mesh: on the bisector of x = y it
    # ties with a face of square 0, which has the lower index and must win whatever the hint says
    sub = mg.mesh_icp_system(d_pts, d_verts, d_faces[per:2 * per].contiguous(), d_R, d_t, metric="point", bvh=None,
                             return_maps=True)
    higher = torch.where(sub[1] >= 0, sub[1] + per, sub[1])
    for max_dist in (None, 0.04):
        base = {m: mg.mesh_icp_system(d_pts, d_verts, d_faces, d_R, d_t, metric=m, max_dist=max_dist, bvh=None,
                                      return_maps=True) for m in ("point", "plane")}
        face, dist = base["point"][1], base["point"][2]
        if max_dist is None:
            tied = (face[0] >= 0) & (face[0] < per) & (bits(dist[0]) == bits(sub[2][0]))
            print("%d faces: %d points tie between square 0 and square 1" % (n_faces, int(tied.sum())))
            assert int(tied[2000:].sum()) >= 100                          # the lowest-index rule is exercised
            assert (face >= 0).all()
        else:
            assert 0 < int((face < 0).sum()) < face.numel()                # the cutoff is hit and missed
        # the unhinted maps are the signed query's on the posed points
        for k in range(2):
            S = mg.transform_points(d_pts, d_R[k], d_t[k]).contiguous()
            sd, f, q = meshsdf.point_mesh_signed_distance(S, d_verts, d_faces, bvh=None, max_dist=max_dist, return_closest=True)
            equal_bits((f, q), (face[k], base["point"][3][k]), "against the signed query")
            assert torch.equal(bits(sd.abs()[f >= 0]), bits(dist[k][f >= 0]))
        hints = {"previous": face, "higher": higher,
                 "random": dev(rs.randint(0, n_faces, size=(2, len(pts))).astype(np.int32)),
                 "minus one": torch.full_like(face, -1), "n_faces": torch.full_like(face, n_faces),
                 "far out": dev(rs.choice(np.array([-2 ** 31, 2 ** 31 - 1, n_faces + 7, -5], np.int64),
                                          size=(2, len(pts))).astype(np.int32))}
        for name, hint in hints.items():
            for bvh in (None, tree):
                for metric in ("point", "plane"):
                    got = mg.mesh_icp_system(d_pts, d_verts, d_faces, d_R, d_t, metric=metric, max_dist=max_dist, bvh=bvh,
                                             hint=hint, return_maps=True)
                    equal_bits(got, base[metric], "%s hint, %s, %s, max_dist %s" % (
                        name, "tree" if bvh is not None else "brute", metric, max_dist))
        if max_dist is None:
            uncut = base["point"]
    # a face with an out-of-range vertex, named by the hint: brute force only (a tree cannot be built over it); the two
    # added faces are skipped, so the maps are those of the mesh without them
    bad = np.concatenate([faces, [[0, 1, len(verts)], [-1, 2, 3]]]).astype(np.int32)
    d_bad = dev(bad)
    for h in (-1, n_faces, n_faces + 1):
        got = mg.mesh_icp_system(d_pts, d_verts, d_bad, d_R, d_t, metric="point", bvh=None, hint=torch.full_like(face, h),
                                 return_maps=True)
        equal_bits(got, uncut, "a hint that names an out-of-range face")


# ---------------------------------------------------------------------------------------------------------------------
def trap_mesh():
    """the corner with a zero-area face (three points of one line, near which some points lie), a face with an
    out-of-range index and one with a negative index"""
    verts, faces = mr.corner_mesh()
    n = len(verts)
    verts = np.concatenate([verts, np.array([[0.5, 0.5, 0.2], [0.5, 0.5, 0.3], [0.5, 0.5, 0.4]], F)])
    faces = np.concatenate([faces, np.array([[n, n + 1, n + 2], [0, 1, n + 3], [-1, 2, 3]], np.int32)])
    return verts, faces


def trap_points(rs, n):
    """near the corner; every 7th near the zero-area face, every 11th far away, and NaN / inf coordinates"""
    P = near_corner(rs, n)
    k = np.arange(n)
    line = np.stack([np.full(n, 0.5), np.full(n, 0.5), 0.2 + 0.2 * rs.rand(n)], 1) + rs.normal(size=(n, 3)) * 0.01
    P = np.where((k % 7 == 3)[:, None], line.astype(F), P)
    P = np.where((k % 11 == 5)[:, None], (P + F(0.6)).astype(F), P)
    if n > 20:
        P[13, 0], P[14, 1], P[15, 2], P[16] = np.nan, np.inf, -np.inf, [np.nan, np.inf, 0]
    return np.ascontiguousarray(P.astype(F))


def check_system(mg, pts, verts, faces, R, t, metric, max_dist, bvh, what):
    max_d2 = np.inf if max_dist is None else F(max_dist) * F(max_dist)
    want = mr.system(pts, R, t, verts, faces, {"plane": 0, "point": 1}[metric], max_d2)
    t_in = [dev(pts), dev(verts), dev(faces), dev(R), dev(t)]
    before = [x.clone() for x in t_in]
    got = mg.mesh_icp_system(*t_in, metric=metric, max_dist=max_dist, bvh=bvh, return_maps=True)
    equal_bits(got, mg.mesh_icp_system(*t_in, metric=metric, max_dist=max_dist, bvh=bvh, return_maps=True), what + ": two runs")
    alone = mg.mesh_icp_system(*t_in, metric=metric, max_dist=max_dist, bvh=bvh)
    assert isinstance(alone, torch.Tensor)
    equal_bits((alone,), got[:1], what + " without the maps")
    equal_bits(t_in, before, what + ": an input was written")
    system, face, residual, closest = (host(x) for x in got)
    assert system.dtype == np.float64 and system.shape == want[0].shape and face.dtype == np.int32
    assert np.array_equal(face, want[1]), "%s: %d faces differ" % (what, int((face != want[1]).sum()))
    same_float(residual, want[2], what + " residual")
    same_float(closest, want[3], what + " closest")
    assert np.array_equal(system[:, 28], want[0][:, 28]), "%s: counts %s vs %s" % (what, system[:, 28], want[0][:, 28])
    differ = system.view(np.int64) != want[0].view(np.int64)
    assert not differ.any(), "%s: %d of %d entries differ, largest difference %.3e" % (
        what, int(differ.sum()), differ.size, np.nanmax(np.abs(system - want[0])))
    return got, want


@pytest.mark.parametrize("metric", ["plane", "point"])
@pytest.mark.parametrize("n", SIZES)
def test_system_equals_the_restatement(mg, n, metric):
    from connecting_the_dots_amd.renderer import MeshBVH
    rs = np.random.RandomState(n)
    verts, faces = trap_mesh()
    clean_v, clean_f = mr.corner_mesh()
    pts = trap_points(rs, n)
    tree = MeshBVH(dev(clean_v), dev(clean_f))
    dropped_by_normal = 0
    for K in (1, 3):
        R, t = poses(K, n)
        for max_dist in (None, 0.05):
            what = "n %d K %d %s max_dist %s" % (n, K, metric, max_dist)
            got, want = check_system(mg, pts, verts, faces, R, t, metric, max_dist, None, what)
            if n >= 255:
                assert want[0][:, 28].min() > 0                            # the case is not vacuous
                if max_dist is not None:
                    assert (want[1][:, ~np.isfinite(pts).all(1)] == -1).all()
                    assert ((want[1] == -1) & np.isfinite(pts).all(1)).any()   # the cutoff is hit, and missed above
            if metric == "plane" and max_dist is None:
                q = mr.system(pts, R, t, verts, faces, 1)[1]                # the point metric keeps the zero-area face
                dropped_by_normal += int(((q == len(clean_f)) & (want[1] == -1)).sum())
        # the clean mesh through a tree that these tensors own
        d_v, d_f = tree.verts, tree.faces
        want = mr.system(pts, R, t, clean_v, clean_f, {"plane": 0, "point": 1}[metric], F(0.05) * F(0.05))
        got = mg.mesh_icp_system(dev(pts), d_v, d_f, dev(R), dev(t), metric=metric, max_dist=0.05, bvh=tree, return_maps=True)
        assert np.array_equal(host(got[0]).view(np.int64), want[0].view(np.int64)) and np.array_equal(host(got[1]), want[1])
        same_float(host(got[2]), want[2], "tree residual")
    if metric == "plane" and n >= 255:
        assert dropped_by_normal > 0                                       # points whose nearest face has no normal


def test_empty_inputs(mg):
    verts, faces = mr.corner_mesh()
    R, t = poses(3)
    none = torch.empty((0, 3), device="cuda")
    for metric in ("plane", "point"):
        s, f, r, q = mg.mesh_icp_system(none, dev(verts), dev(faces), dev(R), dev(t), metric=metric, return_maps=True)
        assert s.shape == (3, 29) and (host(s) == 0).all() and f.shape == (3, 0) and r.shape == (3, 0) and q.shape == (3, 0, 3)
        pts = dev(near_corner(np.random.RandomState(0), 300))
        s, f, r, q = mg.mesh_icp_system(pts, dev(verts), torch.empty((0, 3), dtype=torch.int32, device="cuda"), dev(R), dev(t),
                                        metric=metric, return_maps=True)
        assert (host(s) == 0).all() and (host(f) == -1).all() and np.isnan(host(r)).all() and np.isnan(host(q)).all()
        Ru, tu, ok = mg.mesh_icp_update(s, dev(R), dev(t), min_count=0)
        assert not host(ok).any() and np.array_equal(host(Ru), R) and np.array_equal(host(tu), t)
    s1 = mg.mesh_icp_system(pts, dev(verts), dev(faces), dev(R[0]), dev(t[0]))
    assert s1.shape == (29,)


# ---------------------------------------------------------------------------------------------------------------------
def check_update(mg, system, R, t, what, **kw):
    """mesh_icp_update on the GPU's own system against the restatement on the same numbers"""
    want_R, want_t, want_ok = mr.update(host(system), R, t, **kw)
    t_in = [system, dev(R), dev(t)]
    before = [x.clone() for x in t_in]
    got = mg.mesh_icp_update(*t_in, **kw)
    equal_bits(got, mg.mesh_icp_update(*t_in, **kw), what + ": two runs")
    equal_bits(t_in, before, what + ": an input was written")
    got_R, got_t, got_ok = (host(x) for x in got)
    assert got_R.dtype == np.float32 and got_t.dtype == np.float32 and got_ok.dtype == np.uint8
    assert got_R.shape == R.shape and got_t.shape == t.shape and got_ok.shape == R.shape[:1]
    assert np.array_equal(got_ok, want_ok), "%s: ok %s vs %s" % (what, got_ok.tolist(), want_ok.tolist())
    dR = np.abs(got_R.astype(np.float64) - want_R).max()
    dt = np.abs(got_t.astype(np.float64) - want_t).max()
    t_tol = ULP * max(1.0, float(np.abs(want_t).max()))
    print("%s: ok %s, largest |dR| %.3e (bound %.3e), largest |dt| %.3e (bound %.3e)" % (what, got_ok.tolist(), dR, ULP, dt,
                                                                                        t_tol))
    assert dR <= ULP and dt <= t_tol
    still = got_ok == 0
    assert np.array_equal(got_R[still].view(np.int32), R[still].view(np.int32)), what
    assert np.array_equal(got_t[still].view(np.int32), t[still].view(np.int32)), what
    return got_ok


def test_update_on_the_gpus_own_systems(mg):
    sc = mr.make_corner(CORNER_SEED)
    R, t = poses(3, 7)
    R[2], t[2] = np.eye(3, dtype=F), np.array([5, 5, 5], F)               # out of reach: a count of 0
    args = [dev(sc["points"]), dev(sc["verts"]), dev(sc["faces"]), dev(R), dev(t)]
    for metric in ("plane", "point"):
        system = mg.mesh_icp_system(*args, metric=metric, max_dist=MAX_DIST)
        assert check_update(mg, system, R, t, metric).tolist() == [1, 1, 0]
        assert not check_update(mg, system, R, t, metric + " min_count", min_count=10 ** 6).any()
        assert not check_update(mg, system, R, t, metric + " min_pivot", min_pivot=0.9).any()
        assert check_update(mg, system, R, t, metric + " damped", damping=0.5, min_count=0).tolist() == [1, 1, 0]
    # a single plane leaves three degrees of freedom free: the pivots refuse; so does a count below min_count
    rs = np.random.RandomState(2)
    pts = np.zeros((500, 3), F)
    pts[:, 1:] = rs.rand(500, 2).astype(F) * F(0.8) + F(0.1)
    pts[:, 0] = F(0.01)
    R1, t1 = identity(2)
    R1[0] = mr.rotation([1, 2, 3], 1.0).astype(F)
    R1[1] = mr.rotation([3, 1, -2], 2.0).astype(F)
    system = mg.mesh_icp_system(dev(pts), args[1], args[2], dev(R1), dev(t1), max_dist=0.05)
    assert host(system)[:, 28].min() > 400
    assert not check_update(mg, system, R1, t1, "one plane").any()
    assert not check_update(mg, system, R1, t1, "one plane, few points", min_count=501, min_pivot=0.0).any()
    one = mg.mesh_icp_update(system[0].contiguous(), dev(R1[0]), dev(t1[0]))
    assert one[0].shape == (3, 3) and one[1].shape == (3,) and one[2].shape == () and int(one[2]) == 0


# ---------------------------------------------------------------------------------------------------------------------
def test_mesh_icp_registers_the_corner_scene(mg):
    for noise, max_rot, max_t in ((0.0, MAX_ROT_DEG, MAX_T), (NOISE, MAX_ROT_DEG_NOISY, MAX_T_NOISY)):
        sc = mr.make_corner(CORNER_SEED, noise=noise)
        t_in = [dev(sc["points"]), dev(sc["verts"]), dev(sc["faces"])]
        before = [x.clone() for x in t_in]
        R, t, info = mg.mesh_icp(*t_in, iters=CORNER_ITERS, max_dist=MAX_DIST)
        equal_bits(t_in, before, "mesh_icp: an input was written")
        assert R.shape == (3, 3) and t.shape == (3,) and info["rms"].shape == (CORNER_ITERS,) and info["rms"].is_cuda
        assert info["count"].dtype == torch.float64 and info["ok"].dtype == torch.uint8 and int(info["ok"]) == 1
        assert int(info["best"]) == 0
        rot, tr = mr.pose_error(host(R), host(t), sc["R_true"], sc["t_true"])
        print("noise %g: %.3e degrees, %.3e; rms %s" % (noise, rot, tr, np.array2string(host(info["rms"]), precision=5)))
        assert rot < max_rot and tr < max_t
        # against the restatement's trajectory: printed, not asserted (a face may flip on a last-bit pose difference)
        Rr, tr_, iref = mr.mesh_icp(sc["points"], sc["verts"], sc["faces"], *identity(), iters=CORNER_ITERS, max_dist=MAX_DIST)
        print("difference from the restatement: |dR| %.3e, |dt| %.3e, counts differ by at most %d" % (
            np.abs(host(R).astype(np.float64) - Rr[0]).max(), np.abs(host(t).astype(np.float64) - tr_[0]).max(),
            int(np.abs(host(info["count"]) - iref["count"][:, 0]).max())))
    # the point metric: its rms falls monotonically
    sc = mr.make_corner(CORNER_SEED)
    R, t, info = mg.mesh_icp(dev(sc["points"]), dev(sc["verts"]), dev(sc["faces"]), iters=CORNER_ITERS, metric="point",
                             max_dist=MAX_DIST)
    assert (np.diff(host(info["rms"])) < 0).all() and int(info["ok"]) == 1


def test_mesh_icp_multi_start_hint_and_tolerance(mg):
    from connecting_the_dots_amd.renderer import MeshBVH
    sc = mr.make_corner(CORNER_SEED)
    c = sc["points"].astype(np.float64).mean(0)
    R0, t0 = identity(3)
    t0[0] = [3, 3, 3]                                                      # hopeless: nothing within max_dist
    Q = mr.rotation([1, -2, 0.5], 180.0)                                  # upside down: ends in a local minimum
    R0[2], t0[2] = Q.astype(F), (c - Q @ c).astype(F)
    verts, faces = dev(sc["verts"]), dev(sc["faces"])
    args = [dev(sc["points"]), verts, faces, dev(R0), dev(t0)]
    runs = {}
    for bvh in (None, MeshBVH(verts, faces)):
        for use_hint in (True, False):
            runs[(bvh is not None, use_hint)] = mg.mesh_icp(*args, iters=CORNER_ITERS, max_dist=MAX_DIST, bvh=bvh,
                                                            use_hint=use_hint)
    R, t, info = runs[(True, True)]
    for key, (R2, t2, info2) in runs.items():
        equal_bits((R, t, info["rms"], info["count"], info["ok"], info["best"]),
                   (R2, t2, info2["rms"], info2["count"], info2["ok"], info2["best"]), "tree, hint = %s" % (key,))
    assert R.shape == (3, 3, 3) and info["rms"].shape == (CORNER_ITERS, 3) and info["ok"].shape == (3,)
    print("ok %s, last rms %s, best %d" % (host(info["ok"]).tolist(), host(info["rms"])[-1], int(info["best"])))
    assert int(info["best"]) == 1 and host(info["ok"])[0] == 0 and host(info["count"])[-1, 0] == 0
    assert np.array_equal(host(R)[0], R0[0]) and np.array_equal(host(t)[0], t0[0])
    rot, tr = mr.pose_error(host(R)[1], host(t)[1], sc["R_true"], sc["t_true"])
    assert rot < MAX_ROT_DEG and tr < MAX_T
    # rms_tol ends the loop early, on the same trajectory
    R3, t3, info3 = mg.mesh_icp(args[0], verts, faces, iters=50, max_dist=MAX_DIST, rms_tol=1e-7)
    rounds = info3["rms"].shape[0]
    assert 3 <= rounds < 50 and torch.equal(bits(info3["rms"][:min(rounds, CORNER_ITERS)]),
                                            bits(info["rms"][:min(rounds, CORNER_ITERS), 1]))
    with pytest.raises(RuntimeError):
        mg.mesh_icp(args[0], verts, faces, metric="line")
    with pytest.raises(RuntimeError):
        mg.mesh_icp_system(*args, hint=torch.zeros((3, 5), dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError):
        mg.mesh_icp_system(args[0], verts, faces, torch.eye(3, device="cuda").expand(65, 3, 3).contiguous(),
                           torch.zeros((65, 3), device="cuda"))


def test_aligned_reconstruction_error(mg):
    """the corner moved by 3 degrees and 0.02 against a finer tessellation of the same corner"""
    rs = np.random.RandomState(5)
    verts, faces = mr.corner_mesh(6)
    truth_v, truth_f = mr.corner_mesh(12)
    Q = mr.rotation(rs.normal(size=3), 3.0)
    d = rs.normal(size=3)
    d = d / np.linalg.norm(d) * 0.02
    c = verts.astype(np.float64).mean(0)
    moved = ((verts - c) @ Q.T + c + d).astype(F)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    err = mg.aligned_reconstruction_error(dev(moved), dev(faces), dev(truth_v), dev(truth_f), thresholds=(1e-3, 5e-3),
                                          generator=g, icp_samples=5000)
    print("accuracy mean %.3e -> %.3e; fscore %s -> %s" % (err["before"]["accuracy"]["mean"], err["accuracy"]["mean"],
                                                        err["before"]["fscore"], err["fscore"]))
    assert err["before"]["accuracy"]["mean"] > 5e-3
    assert err["accuracy"]["mean"] < 1e-4
    assert err["R"].shape == (3, 3) and err["t"].shape == (3,) and int(err["icp"]["ok"]) == 1
    rot, tr = mr.pose_error(host(err["R"]), host(err["t"]), Q.T, c - Q.T @ (c + d))
    assert rot < 0.01 and tr < 1e-4
    R, t, info = mg.register_mesh(dev(moved), dev(faces), dev(truth_v), dev(truth_f), n_samples=5000, generator=g, iters=5)
    assert info["rms"].shape == (5,) and int(info["ok"]) == 1
