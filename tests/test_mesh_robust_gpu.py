"""GPU parity of the robust point-to-mesh ICP (meshrobust.face_rim, robust_icp_system, robust_scale, robust_mesh_icp,
robust_register_mesh, robust_aligned_reconstruction_error; include/ext/ctd_hip_mesh_robust.h) against
tests/meshrobust_ref.py.

face_rim equals the restatement at every face.  The system equals it in all 29 entries as int64 (the restatement sums
w * (x * y) in the header's order), face, status, weight, residual and closest equal it at every element, NaN masks
included; two runs give the same bits, no input is written and a hint changes no bit.  With every gate off the system is
meshreg.mesh_icp_system's bit for bit.  robust_mesh_icp meets the thresholds of tests/test_mesh_robust_host.py on its three
scenes, where the plain mesh_icp is at least 5 times worse."""
import itertools

import numpy as np
import pytest
import torch

from tests import meshreg_ref as mr
from tests import meshrobust_ref as rr
from tests import meshsdf_ref as sr
from tests.test_mesh_register_gpu import (SIZES, bits, dev, equal_bits, host, near_corner, poses, same_float, trap_mesh,
                                          trap_points)
from tests.test_mesh_robust_host import MAX_ROT_DEG, MAX_T, PLAIN_WORSE, identity

pytestmark = pytest.mark.gpu

F = np.float32
MIN_COS = 0.5
METRICS = {"plane": 0, "point": 1}
KERNEL_NAMES = ("none", "huber", "tukey")


@pytest.fixture(scope="module")
def mb():
    from connecting_the_dots_amd import meshrobust
    return meshrobust


@pytest.fixture(scope="module")
def mg():
    from connecting_the_dots_amd import meshreg
    return meshreg


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["corner", "cube", "fan3", "trap", "corner 29"])
def test_face_rim_equals_the_restatement(mb, name):
    from connecting_the_dots_amd.meshsmooth import MeshAdjacency
    verts, faces = {"corner": mr.corner_mesh, "cube": sr.cube, "fan3": sr.fan3, "trap": trap_mesh,
                    "corner 29": lambda: mr.corner_mesh(29)}[name]()
    want = rr.face_rim(faces, len(verts))
    d_faces = dev(faces)
    before = d_faces.clone()
    got = mb.face_rim(d_faces, len(verts))
    assert got.dtype == torch.uint8 and got.shape == (len(faces),)
    assert np.array_equal(host(got), want), "%d of %d faces differ" % (int((host(got) != want).sum()), len(faces))
    adj = MeshAdjacency(d_faces, len(verts))
    assert np.array_equal(host(adj.vflags) & rr.BOUNDARY, rr.vertex_flags(faces, len(verts)))   # the reference's flags
    assert torch.equal(mb.face_rim(d_faces, len(verts), adjacency=adj), got) and torch.equal(d_faces, before)
    if name == "corner 29":
        assert len(faces) == 5046 and int((got != 0).sum()) == 3 * (2 * 29 * 29 - 2 * 27 * 27)
    if name == "cube":
        assert not got.any()
    assert mb.face_rim(torch.empty((0, 3), dtype=torch.int32, device="cuda"), 5).shape == (0,)
    with pytest.raises(RuntimeError):
        mb.face_rim(d_faces, len(verts), adjacency=MeshAdjacency(d_faces.clone(), len(verts)))


# ---------------------------------------------------------------------------------------------------------------------
def point_normals(pts):
    """a normal per point: the axis of the square the point is nearest to; every 5th flipped, every 13th with a NaN"""
    n = len(pts)
    a = np.nan_to_num(np.abs(pts), nan=0.0, posinf=1e30).argmin(1)
    N = np.eye(3, dtype=F)[a]
    k = np.arange(n)
    N[k % 5 == 2] *= F(-1)
    N[k % 13 == 6, 1] = np.nan
    return np.ascontiguousarray(N)


def check_robust(mb, d_in, np_in, queries, metric, max_dist, bvh, kernel, scale, rim, normals, what, rerun=False):
    """one configuration against the restatement -> the statuses seen.  d_in: the device tensors (points, verts, faces, R,
    t), np_in the same in numpy; rim and normals: (device, numpy) or None"""
    pts, verts, faces, R, t = np_in
    max_d2 = np.inf if max_dist is None else F(max_dist) * F(max_dist)
    want = rr.system(pts, R, t, verts, faces, METRICS[metric], max_d2, rr.KERNELS[kernel], scale,
                     None if rim is None else rim[1], None if normals is None else normals[1], MIN_COS, queries=queries)
    kw = dict(metric=metric, kernel=kernel, scale=None if scale is None else dev(scale), rim=None if rim is None else rim[0],
              normals=None if normals is None else normals[0], min_cos=MIN_COS, max_dist=max_dist, bvh=bvh)
    extra = [x for x in (kw["scale"], kw["rim"], kw["normals"]) if x is not None]
    before = [x.clone() for x in list(d_in) + extra]
    got = mb.robust_icp_system(*d_in, return_maps=True, **kw)
    equal_bits(list(d_in) + extra, before, what + ": an input was written")
    system, face, residual, weight, status, closest = (host(x) for x in got)
    assert system.dtype == np.float64 and system.shape == want["system"].shape
    assert face.dtype == np.int32 and status.dtype == np.int8 and weight.dtype == np.float32
    assert np.array_equal(face, want["face"]), "%s: %d faces differ" % (what, int((face != want["face"]).sum()))
    assert np.array_equal(status, want["status"]), "%s: %d statuses differ" % (what, int((status != want["status"]).sum()))
    same_float(weight, want["weight"], what + " weight")
    same_float(residual, want["residual"], what + " residual")
    same_float(closest, want["closest"], what + " closest")
    assert np.array_equal(system[:, 28], want["system"][:, 28]), "%s: counts %s vs %s" % (what, system[:, 28],
                                                                                          want["system"][:, 28])
    differ = system.view(np.int64) != want["system"].view(np.int64)
    assert not differ.any(), "%s: %d of %d entries differ, largest difference %.3e" % (
        what, int(differ.sum()), differ.size, np.nanmax(np.abs(system - want["system"])))
    assert np.array_equal(np.isnan(residual), status != 0)
    assert ((weight == 0) | (status == 0)).all() and ((face == -1) == (status == 1)).all()
    # the faces as the next round's hint: no bit changes; and without the maps the system alone comes back
    hinted = mb.robust_icp_system(*d_in, return_maps=True, hint=got[1], **kw)
    equal_bits(hinted, got, what + ": hinted with its own faces")
    if rerun:
        equal_bits(mb.robust_icp_system(*d_in, return_maps=True, **kw), got, what + ": two runs")
        stale = torch.roll(got[1], 7, dims=-1).contiguous()
        equal_bits(mb.robust_icp_system(*d_in, return_maps=True, hint=stale, **kw), got, what + ": a stale hint")
        alone = mb.robust_icp_system(*d_in, **kw)
        assert isinstance(alone, torch.Tensor)
        equal_bits((alone,), got[:1], what + " without the maps")
    return set(np.unique(status).tolist())


@pytest.mark.parametrize("metric", ["plane", "point"])
@pytest.mark.parametrize("n", SIZES)
def test_system_equals_the_restatement(mb, n, metric):
    """the trap mesh and trap points; K 1 and 3, max_dist None and 0.05, with and without rim, with and without normals,
    kernels none / huber / tukey with per-pose scales that take +inf, 0, NaN and 1.5 times the median residual in turn;
    brute force, and the clean mesh through a tree"""
    from connecting_the_dots_amd.renderer import MeshBVH
    rs = np.random.RandomState(n)
    verts, faces = trap_mesh()
    clean_v, clean_f = mr.corner_mesh()
    pts = trap_points(rs, n)
    nrm = point_normals(pts)
    rim = rr.face_rim(faces, len(verts))
    d_pts, d_verts, d_faces, d_nrm, d_rim = dev(pts), dev(verts), dev(faces), dev(nrm), dev(rim)
    assert torch.equal(mb.face_rim(d_faces, len(verts)), d_rim)
    seen, turn = set(), 0
    for K in (1, 3):
        R, t = poses(K, n)
        d_in, np_in = (d_pts, d_verts, d_faces, dev(R), dev(t)), (pts, verts, faces, R, t)
        for max_dist in (None, 0.05):
            max_d2 = np.inf if max_dist is None else F(max_dist) * F(max_dist)
            queries = [rr.pose_query(pts, R[k], t[k], verts, faces, METRICS[metric], max_d2) for k in range(K)]
            r0 = queries[0]["r"][queries[0]["face"] >= 0]
            med = F(1.5) * F(np.median(r0[np.isfinite(r0)])) if np.isfinite(r0).any() else F(0.01)
            values = [med, F(np.inf), F(0), F(np.nan)]
            for use_rim, use_nrm, kernel in itertools.product((False, True), (False, True), KERNEL_NAMES):
                scale = None
                if kernel != "none":
                    scale = np.array([values[(turn + k) % 4] for k in range(K)], F)
                    turn += 1
                what = "n %d K %d %s max_dist %s rim %s normals %s %s scale %s" % (n, K, metric, max_dist, use_rim, use_nrm,
                                                                                   kernel, scale)
                seen |= check_robust(mb, d_in, np_in, queries, metric, max_dist, None, kernel, scale,
                                     (d_rim, rim) if use_rim else None, (d_nrm, nrm) if use_nrm else None, what,
                                     rerun=use_rim and use_nrm and kernel == "tukey")
        # the clean mesh through a tree that these tensors own: every gate on
        tree = MeshBVH(dev(clean_v), dev(clean_f))
        assert tree.usable
        clean_rim = rr.face_rim(clean_f, len(clean_v))
        d_clean = (d_pts, tree.verts, tree.faces, dev(R), dev(t))
        for max_dist, kernel in ((0.05, "tukey"), (None, "huber")):
            scale = np.array([[med, F(np.inf), med][k] for k in range(K)], F)
            seen |= check_robust(mb, d_clean, (pts, clean_v, clean_f, R, t), None, metric, max_dist, tree, kernel, scale,
                                 (dev(clean_rim), clean_rim), (d_nrm, nrm), "tree, n %d K %d %s %s" % (n, K, metric, kernel),
                                 rerun=True)
    print("n %d %s: statuses seen %s" % (n, metric, sorted(seen)))
    if n >= 255:
        assert seen == {0, 1, 2, 3, 4, 5}                                # no branch is vacuous


@pytest.mark.parametrize("metric", ["plane", "point"])
def test_with_every_gate_off_the_system_is_the_plain_one(mb, mg, metric):
    from connecting_the_dots_amd.renderer import MeshBVH
    verts, faces = trap_mesh()
    tree = MeshBVH(*(dev(x) for x in mr.corner_mesh()))
    for n in (1, 1025, 2500):
        pts = trap_points(np.random.RandomState(n), n)
        R, t = poses(3, n)
        for mesh, bvh in (((dev(verts), dev(faces)), None), ((tree.verts, tree.faces), tree)):
            for max_dist in (None, 0.05):
                args = (dev(pts),) + mesh + (dev(R), dev(t))
                plain = mg.mesh_icp_system(*args, metric=metric, max_dist=max_dist, bvh=bvh, return_maps=True)
                got = mb.robust_icp_system(*args, metric=metric, kernel="none", max_dist=max_dist, bvh=bvh, return_maps=True)
                equal_bits(got[:1], plain[:1], "n %d %s max_dist %s" % (n, metric, max_dist))
                assert torch.equal(got[4] == 0, plain[1] >= 0)            # the same points take part
                assert torch.equal(bits(got[2]), bits(plain[2])) and torch.equal(bits(got[5]), bits(plain[3]))
                assert torch.equal(got[1][got[4] == 0], plain[1][got[4] == 0])
                # +inf weighs every point 1: the same bits through the weighted path
                inf = torch.full((3,), float("inf"), device="cuda")
                for kernel in ("huber", "tukey"):
                    again = mb.robust_icp_system(*args, metric=metric, kernel=kernel, scale=inf, max_dist=max_dist, bvh=bvh)
                    equal_bits((again,), plain[:1], "%s at +inf" % kernel)


def test_min_cos_at_its_ends(mb):
    """-1 lets every finite normal pass (the cosine of two unit vectors may round a little below -1: the point normals
    here are axes, whose cosines are exact); 1 passes only the points whose rotated normal is the face's to the bit"""
    verts, faces = mr.corner_mesh()
    pts = near_corner(np.random.RandomState(4), 600)
    nrm = point_normals(pts)
    R, t = identity()
    args = (dev(pts), dev(verts), dev(faces), dev(R[0]), dev(t[0]))
    base = host(mb.robust_icp_system(*args, kernel="none", return_maps=True)[4])
    for min_cos, metric in ((-1.0, "plane"), (-1, "point"), (1.0, "plane"), (1, "point")):
        st = host(mb.robust_icp_system(*args, metric=metric, kernel="none", normals=dev(nrm), min_cos=min_cos, return_maps=True)[4])
        want = rr.system(pts, R, t, verts, faces, METRICS[metric], kernel=0, normals=nrm, min_cos=min_cos)["status"][0]
        assert np.array_equal(st, want)
        if min_cos < 0:
            assert np.array_equal(st == 4, np.isnan(nrm).any(1) & (base == 0)) and (st[base != 0] == base[base != 0]).all()
        else:
            assert 0 < int((st == 0).sum()) < int((base == 0).sum())


def test_empty_inputs(mb, mg):
    verts, faces = mr.corner_mesh()
    R, t = poses(3)
    none = torch.empty((0, 3), device="cuda")
    no_faces = torch.empty((0, 3), dtype=torch.int32, device="cuda")
    scale = torch.full((3,), 0.01, device="cuda")
    for metric in ("plane", "point"):
        s, f, r, w, st, q = mb.robust_icp_system(none, dev(verts), dev(faces), dev(R), dev(t), metric=metric, scale=scale,
                                                 rim=True, normals=none, return_maps=True)
        assert s.shape == (3, 29) and (host(s) == 0).all() and f.shape == (3, 0) and r.shape == (3, 0) and w.shape == (3, 0)
        assert st.shape == (3, 0) and q.shape == (3, 0, 3)
        pts = dev(near_corner(np.random.RandomState(0), 300))
        s, f, r, w, st, q = mb.robust_icp_system(pts, dev(verts), no_faces, dev(R), dev(t), metric=metric, scale=scale, rim=True,
                                                 normals=pts, return_maps=True)
        assert (host(s) == 0).all() and (host(f) == -1).all() and np.isnan(host(r)).all() and np.isnan(host(q)).all()
        assert (host(w) == 0).all() and (host(st) == 1).all()
        Ru, tu, ok = mg.mesh_icp_update(s, dev(R), dev(t), min_count=0)
        assert not host(ok).any() and np.array_equal(host(Ru), R) and np.array_equal(host(tu), t)
    s1 = mb.robust_icp_system(pts, dev(verts), dev(faces), dev(R[0]), dev(t[0]), scale=0.01)
    assert s1.shape == (29,)
    assert torch.equal(bits(s1), bits(mb.robust_icp_system(pts, dev(verts), dev(faces), dev(R[0]), dev(t[0]),
                                                           scale=torch.tensor(0.01, device="cuda"))))
    assert np.isnan(host(mb.robust_scale(torch.empty((3, 0), device="cuda"), "tukey"))).all()
    z, i = dev(verts), dev(faces)
    for bad in (dict(kernel="cauchy"), dict(kernel="tukey"), dict(scale=torch.ones(2, device="cuda")), dict(scale="mad"),
                dict(scale=0.01, min_cos=1.5), dict(scale=0.01, rim=torch.zeros(3, dtype=torch.uint8, device="cuda")),
                dict(scale=0.01, normals=torch.zeros((5, 3), device="cuda")), dict(scale=torch.ones(3))):
        with pytest.raises(RuntimeError):
            mb.robust_icp_system(pts, z, i, dev(R), dev(t), **bad)
    with pytest.raises(RuntimeError):
        mb.robust_mesh_icp(pts, z, i, scale="median")
    with pytest.raises(RuntimeError):
        mb.robust_scale(torch.zeros(5, device="cuda"), "none")
    with pytest.raises(RuntimeError):
        mb.robust_icp_system(pts.cpu(), z.cpu(), i.cpu(), torch.eye(3), torch.zeros(3), scale=0.01)   # there is no CPU path


# ---------------------------------------------------------------------------------------------------------------------
def test_robust_scale_is_the_restatement(mb):
    rs = np.random.RandomState(8)
    res = rs.normal(size=(3, 1001)).astype(F)
    res[0, ::3], res[1, :] = np.nan, np.nan
    res[2, 5] = np.inf
    for kernel in ("huber", "tukey"):
        got = mb.robust_scale(dev(res), kernel)
        assert got.dtype == torch.float32 and got.shape == (3,)
        same_float(host(got), rr.robust_scale(res, rr.KERNELS[kernel]), kernel)
        same_float(host(mb.robust_scale(dev(res[0]), kernel)).reshape(1), rr.robust_scale(res[:1], rr.KERNELS[kernel]), kernel)


@pytest.mark.parametrize("name", list(rr.SCENES))
def test_robust_mesh_icp_on_the_scenes_the_plain_one_fails_on(mb, mg, name):
    kw, metric, iters, rob = rr.SCENES[name]
    metric = "plane" if metric == 0 else "point"
    kernel = KERNEL_NAMES[rob["kernel"]]
    seed = rr.SCENE_SEEDS[0]
    sc = rr.make_scene(seed, **kw)
    t_in = [dev(sc["points"]), dev(sc["verts"]), dev(sc["faces"])]
    before = [x.clone() for x in t_in]
    run = dict(iters=iters, metric=metric, kernel=kernel, rim=True if rob["rim"] else None, max_dist=rr.SCENE_MAX_DIST)
    R, t, info = mb.robust_mesh_icp(*t_in, **run)
    equal_bits(t_in, before, "robust_mesh_icp: an input was written")
    assert R.shape == (3, 3) and t.shape == (3,) and info["rms"].shape == (iters,) and info["rms"].is_cuda
    assert info["used"].dtype == torch.float64 and info["scale"].dtype == torch.float32 and info["scale"].shape == (iters,)
    assert int(info["ok"]) == 1 and int(info["best"]) == 0 and torch.equal(info["used"], info["count"])
    if kernel == "none":
        assert np.isnan(host(info["scale"])).all()
    else:
        assert host(info["scale"])[0] == np.inf and np.isfinite(host(info["scale"])[1:]).all()
    rot, tr = mr.pose_error(host(R), host(t), sc["R_true"], sc["t_true"])
    Rp, tp, _ = mg.mesh_icp(*t_in, iters=iters, metric=metric, max_dist=rr.SCENE_MAX_DIST)
    rot_p, tr_p = mr.pose_error(host(Rp), host(tp), sc["R_true"], sc["t_true"])
    print("%s, seed %d: robust %.4f degrees / %.2e (used %d of %d), plain %.4f degrees / %.2e, %.1f times worse" % (
        name, seed, rot, tr, int(info["used"][-1]), len(sc["points"]), rot_p, tr_p, tr_p / tr))
    assert rot < MAX_ROT_DEG and tr < MAX_T
    assert tr_p >= PLAIN_WORSE * tr
    # scale='mad' is the loop written by hand with robust_scale, bit for bit; use_hint=False gives the same bits
    Rk, tk = dev(identity()[0]), dev(identity()[1])
    rim = mb.face_rim(t_in[2], t_in[1].shape[0]) if rob["rim"] else None
    c = torch.full((1,), float("inf"), device="cuda") if kernel != "none" else None
    rms = []
    for _ in range(iters):
        s, _, residual, _, _, _ = mb.robust_icp_system(*t_in, Rk, tk, metric=metric, kernel=kernel, scale=c, rim=rim,
                                                       max_dist=rr.SCENE_MAX_DIST, return_maps=True)
        Rk, tk, ok = mg.mesh_icp_update(s, Rk, tk)
        rms.append(torch.sqrt(s[0, 27] / s[0, 28]))
        if kernel != "none":
            c = mb.robust_scale(residual, kernel)
    equal_bits((R, t, info["rms"]), (Rk[0], tk[0], torch.stack(rms)), "the loop by hand")
    R2, t2, info2 = mb.robust_mesh_icp(*t_in, use_hint=False, **run)
    equal_bits((R, t, info["rms"], info["used"], info["scale"]), (R2, t2, info2["rms"], info2["used"], info2["scale"]),
               "use_hint=False")


def test_robust_mesh_icp_multi_start_and_tolerance(mb):
    from connecting_the_dots_amd.renderer import MeshBVH
    sc = rr.make_scene(1, outliers=0.1)
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
            runs[(bvh is not None, use_hint)] = mb.robust_mesh_icp(*args, iters=15, max_dist=rr.SCENE_MAX_DIST, bvh=bvh,
                                                                   use_hint=use_hint)
    R, t, info = runs[(True, True)]
    keys = ("rms", "used", "scale", "ok", "best")
    for key, (R2, t2, info2) in runs.items():
        equal_bits((R, t) + tuple(info[k] for k in keys), (R2, t2) + tuple(info2[k] for k in keys), "tree, hint = %s" % (key,))
    assert R.shape == (3, 3, 3) and info["rms"].shape == (15, 3) and info["scale"].shape == (15, 3) and info["ok"].shape == (3,)
    print("ok %s, last rms %s, best %d" % (host(info["ok"]).tolist(), host(info["rms"])[-1], int(info["best"])))
    assert int(info["best"]) == 1 and host(info["ok"])[0] == 0 and host(info["used"])[-1, 0] == 0
    assert np.array_equal(host(R)[0], R0[0]) and np.array_equal(host(t)[0], t0[0])
    assert np.isnan(host(info["scale"])[1:, 0]).all()                      # no residual, no scale: the pose stays gated
    rot, tr = mr.pose_error(host(R)[1], host(t)[1], sc["R_true"], sc["t_true"])
    assert rot < MAX_ROT_DEG and tr < MAX_T
    # a fixed scale, as a number and as a tensor; rms_tol ends the loop early, on the same trajectory
    Ra, ta, ia = mb.robust_mesh_icp(args[0], verts, faces, iters=8, kernel="huber", scale=0.004, max_dist=rr.SCENE_MAX_DIST)
    Rb, tb, ib = mb.robust_mesh_icp(args[0], verts, faces, iters=50, kernel="huber", scale=torch.full((1,), 0.004, device="cuda"),
                                    max_dist=rr.SCENE_MAX_DIST, rms_tol=1e-6)
    rounds = ib["rms"].shape[0]
    assert 3 <= rounds < 50 and torch.equal(bits(ib["rms"][:min(rounds, 8)]), bits(ia["rms"][:min(rounds, 8)]))
    assert (host(ia["scale"]) == F(0.004)).all()


def test_robust_aligned_reconstruction_error(mb):
    """the corner moved by 3 degrees and 0.02 against a finer tessellation of the same corner, as in the plain test; rim
    rejection and the normal gate on"""
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
    err = mb.robust_aligned_reconstruction_error(dev(moved), dev(faces), dev(truth_v), dev(truth_f), thresholds=(1e-3, 5e-3),
                                                 generator=g, icp_samples=5000, kernel="huber", rim=True, use_normals=True,
                                                 min_cos=0.7)
    print("accuracy mean %.3e -> %.3e; fscore %s -> %s; used %s" % (err["before"]["accuracy"]["mean"], err["accuracy"]["mean"],
                                                                  err["before"]["fscore"], err["fscore"],
                                                                  host(err["icp"]["used"]).tolist()))
    assert err["before"]["accuracy"]["mean"] > 5e-3
    assert err["accuracy"]["mean"] < 1e-4
    assert err["R"].shape == (3, 3) and err["t"].shape == (3,) and int(err["icp"]["ok"]) == 1
    rot, tr = mr.pose_error(host(err["R"]), host(err["t"]), Q.T, c - Q.T @ (c + d))
    assert rot < 0.01 and tr < 1e-4
    R, t, info = mb.robust_register_mesh(dev(moved), dev(faces), dev(truth_v), dev(truth_f), n_samples=5000, generator=g,
                                         iters=5, use_normals=True)
    assert info["rms"].shape == (5,) and int(info["ok"]) == 1
    # a refused registration raises: nothing lies within max_dist of the truth
    far = dev((moved + F(5)).astype(F))
    with pytest.raises(RuntimeError):
        mb.robust_aligned_reconstruction_error(far, dev(faces), dev(truth_v), dev(truth_f), thresholds=(1e-3,), generator=g,
                                               icp_samples=2000, max_dist=0.05)
