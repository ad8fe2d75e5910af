"""The second half of the README's chain (depth maps -> normals / ICP -> TSDF fusion -> surface points, ray cast -> mesh ->
clean -> smooth -> simplify -> evaluation -> colours; stages i .. p, after tests/test_chain_truth_host.py's a .. h) against
the float64 truth of the rendered scene, on the CPU.  tests/chain_ref.py runs the chain once from the restatements
(`recon()` on the rendered depths, `recon_matcher()` on the matcher's own depths); tests/chain_scene.py holds the truth:
the true meshes and poses, `recon_grid`, the per-pixel normals, the analytic `field` of the colour images and `occluded64`.
Every restatement is tested against its kernel elsewhere, on scenes that the restatement modules generate themselves;
here they are held against a scene none of them knows, so that a convention which kernel, restatement and scene
generator share wrongly cannot stay green.  The negative controls run the same predicates under each wrong convention
and must score below half the correct score, or above twice the correct distance.

This file establishes every measured figure (the tests print them; run with -s).  The thresholds live in
tests/chain_ref.py (`RECON`, beside the predicates), each the reference's measured figure rounded by its kind: shares down
to three decimals, distances and errors up in the second significant digit, an after / before ratio that shows an
improvement at most halfway to 1.  `hold(..., drift=True)` also checks that no threshold has drifted from its
measurement.  The GPU file asserts the same thresholds.

Measured (the reference chain; voxel 0.025, trunc 4 voxels, grid 144 x 45 x 103 per track; tracks 0 / 1):
  i        depth_normals on 33336 interior pixels: all have a normal, angle to the truth normal median 0.0069 degrees,
           largest 0.029; every normal of every view faces its camera
  j        views 1..3 perturbed by (0.3 degrees, 5 mm), seed 7, max_rel 0.05, 10 rounds: 4 of 6 views end with ok == 1; their
           interior points' median distance to the true mesh falls 8.8e-4 -> 3.3e-6, 1.1e-3 -> 1.2e-5 (track 0, views 1, 3),
           4.7e-3 -> 2.3e-5, 1.4e-3 -> 4.5e-5 (track 1, views 2, 3): largest ratio 0.031, asserted at most halfway to 1.
           Rotation errors 0.3 -> 0.06 .. 0.11 degrees, translation errors 4.2e-3 -> 9.1e-3 (track 0, view 1: it grows, sliding
           along the wall costs a point-to-plane error nothing) and 4.8e-3 .. 6.0e-3 -> 7e-4 .. 1.2e-3: reported, not
           asserted.  The two views with ok == 0: track 0 view 2 never moves (pivot ratio 4.7e-7 in every round); track 1
           view 1 is moved by earlier rounds and comes back 0.55 m from its true pose, its points 0.31 from the mesh
  k        3729 / 591 vertices, 6910 / 1068 faces; vertex distance to the true mesh median 1.2e-4 / 8.1e-5, p99 6.0e-4 /
           7.2e-3, largest 2.4e-2 / 8.3e-3 (creases; below a voxel), none beyond a voxel; truth points of interior pixels at
           most 6.6e-3 / 1.8e-4 from the model; the faces' winding points to every camera that sees their centroid (25047 /
           4244 pairs); the TSDF-gradient normals agree with the face normals at every corner that has both (median angle
           0.11 / 0.26 degrees)
  l        ray cast at the four views and at the mean camera position with view 0's rotation, interior pixels: every ray
           hits, but in view 2 of track 0 0.937 (511 pixels of a box face seen at grazing incidence, where a ray enters the
           band through voxels no view has weighted); |depth - z64| median 0.0023 .. 0.0029 / 0.0013 .. 0.0015 voxel, largest
           0.023 / 0.0076; no depth on any of the 13483 .. 13680 true misses of track 1's poses
  m        clean (min_faces 32): 3710 / 584 vertices, 6899 / 1068 faces, median x 0.994 / 0.978; smooth (10 x 0.5 | -0.53):
           median x 0.903 / 0.765; simplify (cell 2 voxels): 0.236 / 0.232 of the faces, median x 1.054 / 0.990 (no ordering
           asserted on track 0); none beyond a voxel at any step.  Topology (referenced, edges, boundary, non-manifold, valid
           faces, euler): cleaned (3710, 10606, 515, 0, 6899, 3) / (584, 1651, 98, 0, 1068, 1), simplified (941, 2565, 250, 1,
           1627, 3) / (148, 395, 46, 0, 248, 1)
  n        point_mesh_distance of the cleaned model's vertices to the true mesh within 2.4e-7 / 1.2e-9 of float64 (allowed
           by pointmesh_ref.forward_bound: 4.6e-4 / 7.5e-5 at most); of 1808 / 240 truth points moved 2 voxels towards the
           camera all are positive against the model, moved 2 voxels away all negative; mesh_to_tsdf of the true mesh, ray
           cast: the wall is one sheet wound away from the cameras, so only pixels whose true face is wound towards the
           camera are judged (1171 .. 2190 / 802 .. 1014): all hit, median 1.3e-6 .. 6.7e-6 voxel, largest 0.033; 61 .. 78
           depths on true misses of track 1 (rays that graze a box)
  o        colours of the cleaned model (normals from its faces, valid = the truth's hit masks, margin 2 voxels) from
           images of `field`: 14357 / 2222 candidates; grey 0.092 / 0 (cap 0.10); truly occluded candidates that are
           used 43 of 268 / none; truly visible ones dropped: none; colour error median 3.5e-5 / 3.1e-5, p99 0.157 / 4.4e-3;
           0.984 / 0.964 of the vertices get a colour.  The silhouette rule at a reach of one voxel: no occluded candidate is
           used, grey 0.147 / 0.042, over the cap; without the rule 465 of 732 are used (rays grazing a box whose unseen
           side faces the model lacks)
  p        the matcher's depths (disparity about 6 px: 0.07 px are 3.6 cm), median distance to the true mesh of the kept
           per-view points / the model / their ratio, valid = keep of the consistency rule (max_rel 0.01):
             voxel 0.025: 1.78e-2, 3.41e-2 / 3.68e-2, 3.81e-2 / 2.06, 1.12     cleaned: 3.55e-2, 3.96e-2
             voxel 0.05:  1.78e-2, 3.41e-2 / 3.73e-2, 3.89e-2 / 2.09, 1.14     cleaned: 3.83e-2, 4.03e-2
             voxel 0.1:   1.78e-2, 3.41e-2 / 3.70e-2, 3.92e-2 / 2.08, 1.15     cleaned: 4.35e-2, nothing left of track 1
           and with the plain validity mask:
             voxel 0.025: 1.89e-2, 3.31e-2 / 3.77e-2, 2.11e-2 / 2.00, 0.64     cleaned: 3.64e-2, 2.10e-2
             voxel 0.05:  1.89e-2, 3.31e-2 / 3.77e-2, 1.99e-2 / 2.00, 0.60     cleaned: 3.53e-2, 1.71e-2
             voxel 0.1:   1.89e-2, 3.31e-2 / 3.46e-2, 1.75e-2 / 1.84, 0.53     cleaned: 3.75e-2, 1.96e-2
           The README's "0.59 x as far" and "ALWAYS pass keep" do not carry over: the fused surface is farther from the truth
           than the kept points except on track 1 without keep, and keep does not help track 1.  Each figure is asserted
           against its own measurement; no ordering is.  The other figures of k are measured and asserted on each of the
           six models too (tests/chain_ref.py, RECON["p. ..."]): with keep at voxel 0.025 p99 1.4e-1 / 6.0e-2 and largest
           distance 2.2e-1 / 7.0e-2, complete to 1.0e-1 / 6.3e-2, winding share 0.980 / 1.0, gradient agreement 0.986 / 1.0;
           and the cleaned model's vertex count: nothing is left of track 1 at voxel 0.1 with keep (0 vertices, asserted)
  negative controls (correct -> wrong convention)
           R transposed in integrate (k, median vertex distance): 1.2e-4 / 8.1e-5 -> 3.0e-2 / 8.5e-2
           t negated in integrate (k): -> 5.0e-1 / 1.8e-1
           views interleaved as v * B + b (k): -> 9.9e-3 / 4.6e-1; (l, interior pixels with a depth within 0.1 voxel): 0.994 -> 0.081
           TSDF sign flipped before meshing (k, winding share): 1.0 -> 0.0
           winding reversed (n, shares of the moved points with the right sign): 1.0 -> 0.0
           R transposed / t negated / images offset by half a pixel (o, median colour error): 3.5e-5 / 3.1e-5 -> 3.6e-2 /
           3.6e-2, 6.2e-2 / 5.1e-2, 2.3e-3 / 1.7e-3
"""
import numpy as np
import pytest

from tests import chain_ref as cr, chain_scene as cs, icp_ref, meshsdf_ref, tsdf_ref

F = np.float32
VOXEL = cr.VOXEL


@pytest.fixture(scope="module")
def sc():
    return cs.scene()


@pytest.fixture(scope="module")
def ch(oracle):
    return cr.chain()


@pytest.fixture(scope="module")
def rc(ch):
    return cr.recon()


@pytest.fixture(scope="module")
def pm(ch):
    return cr.recon_matcher()


# ---------------------------------------------------------------------------------------------------------------------
# the scene's additions
# ---------------------------------------------------------------------------------------------------------------------
def test_scene_additions(sc):
    origin, dims = cs.recon_grid(VOXEL)
    print("grid at %g: %s, %d voxels per track" % (VOXEL, dims, np.prod(dims)))
    assert origin.shape == (cs.B, 3) and origin.dtype == F and np.prod(dims) < 10 ** 6
    for b in range(cs.B):                                        # every truth point lies at least 4 voxels inside its grid
        X = cs.truth_points(sc, b)
        hi = origin[b] + VOXEL * (np.array(dims) - 1)
        assert (X.min(0) - origin[b] >= 4 * VOXEL - 1e-6).all() and (hi - X.max(0) >= 4 * VOXEL - 1e-6).all()
    X = np.random.RandomState(0).uniform(-3, 3, (1000, 3))
    f = cs.field(X)
    assert f.min() >= 0 and f.max() <= 1 and f.std() > 0.1
    im = cs.field_images(1)
    hit = sc.stack("hit")[cs.V:]
    assert im.shape == (cs.V, 1, cs.H, cs.W) and im.dtype == F and (im[:, 0][~hit] == 0).all() and (~hit).sum() > cs.H * cs.W
    n = cs.truth_normals(sc, 0, 0)
    T = sc.truth[0][0]
    Xc = T["X"] @ sc.R[0, 0].astype(np.float64).T + sc.t[0, 0]
    assert np.allclose(np.linalg.norm(n[T["hit"]], axis=-1), 1) and ((n * Xc).sum(-1)[T["hit"]] < 0).all()


def test_occluded64_on_points_of_known_visibility(sc):
    """the truth points of a view are visible from it; pushed 0.3 behind their surface along the ray they are occluded"""
    margin = cr.margin_of(VOXEL)
    for b in range(cs.B):
        T = sc.truth[b][0]
        X = T["X"][T["interior"]][::7]
        C = -sc.R[b, 0].astype(np.float64).T @ sc.t[b, 0].astype(np.float64)
        u = (X - C) / np.linalg.norm(X - C, axis=1, keepdims=True)
        occ, vis, grey = cs.occluded64(b, 0, X, margin)
        assert vis.all() and not occ.any() and not grey.any()
        occ, vis, grey = cs.occluded64(b, 0, X + 0.3 * u, margin)
        assert (occ | grey).all() and not vis.any() and occ.mean() > 0.9
    X = cs.truth_points(sc, 0)[::97]
    d = cs.mesh_distance(X + 0.01, sc.meshes[0]["verts"], sc.meshes[0]["faces"])
    near = cs.mesh_distance_near(X + 0.01, sc.meshes[0]["verts"], sc.meshes[0]["faces"], k=len(sc.meshes[0]["faces"]))
    assert np.allclose(d, near, atol=1e-12)                       # over all faces the two distances are one


# ---------------------------------------------------------------------------------------------------------------------
# i. normals, j. ICP
# ---------------------------------------------------------------------------------------------------------------------
def test_normals(sc, rc):
    figs, f = cr.figures_i(sc, rc["normal"])
    print("i: %d interior pixels" % f["n"])
    assert f["facing"]
    cr.hold(figs, drift=True)


def test_icp(sc, rc):
    icp = rc["icp"]
    fig = cr.icp_figures(sc, icp)
    rot, tra = icp_ref.pose_errors(icp["R"], icp["t"], sc.R, sc.t)
    rot0, tra0 = icp_ref.pose_errors(icp["R0"], icp["t0"], sc.R, sc.t)
    for f in fig:
        b, v = f["b"], f["v"]
        print("j: track %d view %d: ok %d, median distance %.3e -> %.3e (ratio %.4g); rotation %.3f -> %.3f degrees, "
              "translation %.2e -> %.2e; rmse %.2e -> %.2e, last pivot ratio %.2e (reported, not asserted)"
              % (b, v, f["ok"], f["before"], f["after"], f["ratio"], rot0[b, v], rot[b, v], tra0[b, v], tra[b, v],
                 icp["rmse"][0, b, v], icp["rmse"][-1, b, v], icp["pivot_ratio"][-1, b, v]))
    good = [f for f in fig if f["ok"] == 1]
    assert len(good) >= 3 and len(good) == cr.ICP_OK_VIEWS
    cr.hold({"j.ratio": [max(f["ratio"] for f in good)]}, drift=True)
    # a view that ends with ok == 0 is either where it started or anywhere: one of each here
    bad = [f for f in fig if f["ok"] == 0]
    assert any(f["ratio"] == 1.0 for f in bad) and any(f["ratio"] > 100 for f in bad)


# ---------------------------------------------------------------------------------------------------------------------
# k. integrate + surface points + mesh, l. ray cast, with their controls
# ---------------------------------------------------------------------------------------------------------------------
def test_model(sc, rc):
    m = rc["model"]["mesh"]
    print("k: %s vertices, %s faces" % ([len(v) for v in m["verts"]], [len(f) for f in m["faces"]]))
    cr.hold(cr.figures_k(sc, m), drift=True)


def test_raycast(sc, rc):
    figs, r = cr.figures_l(sc, rc["raycast"])
    print("l: interior pixels %s, true misses %s" % (cr.per(r, "n"), cr.per(r, "misses")))
    cr.hold(figs, drift=True)


def control_models(sc, depth, keep):
    """the wrong conventions of k -> name: model"""
    return {"R transposed": cr.model_of(sc, depth, keep, cr.transposed(sc.R), sc.t, VOXEL),
            "t negated": cr.model_of(sc, depth, keep, sc.R, -sc.t, VOXEL),
            "views interleaved as v * B + b": cr.model_of(sc, cr.interleaved_views(depth), cr.interleaved_views(keep), sc.R,
                                                           sc.t, VOXEL)}


def test_model_controls(sc, ch, rc):
    depth, keep = ch["render"]["depth"], rc["keep"]
    right = cr.per(cr.vertex_figures(sc, rc["model"]["mesh"]["verts"], VOXEL), "median")
    models = control_models(sc, depth, keep)
    for name, model in models.items():
        wrong = cr.per(cr.vertex_figures(sc, model["mesh"]["verts"], VOXEL), "median")
        print("control %s (k): median vertex distance %s -> %s" % (name, right, wrong))
        assert all(w > 2 * r for w, r in zip(wrong, right))
    # the same mix-up of the frames in the ray cast: the model of the interleaved frames, cast at the poses
    il = models["views interleaved as v * B + b"]
    Rc, tc, _ = cr.cast_poses()
    cast = tsdf_ref.raycast(il["tsdf"], il["weight"], il["origin"], VOXEL, sc.ray, Rc, tc, cs.H, cs.W, cr.D_MIN,
                            cr.step_of(VOXEL), cr.N_STEPS)
    good, bad = cr.raycast_figures(sc, rc["raycast"], VOXEL), cr.raycast_figures(sc, cast, VOXEL)
    score = lambda r: float(np.mean(cr.per(r, "close")))
    print("control views interleaved (l): interior pixels with a depth within 0.1 voxel %.4f -> %.4f" % (score(good), score(bad)))
    assert score(bad) < 0.5 * score(good)
    # the TSDF's sign flipped before meshing: the faces turn away from the cameras
    T = rc["model"]["tsdf"]
    flipped = cr.mesh_of(-T, rc["model"]["weight"], rc["model"]["origin"], VOXEL)["mesh"]
    right = [w[0] for w in cr.winding_share(sc, rc["model"]["mesh"], cr.margin_of(VOXEL))]
    wrong = [w[0] for w in cr.winding_share(sc, flipped, cr.margin_of(VOXEL))]
    print("control TSDF sign flipped (k): winding share %s -> %s" % (right, wrong))
    assert all(w < 0.5 * r for w, r in zip(wrong, right))


# ---------------------------------------------------------------------------------------------------------------------
# m. clean -> smooth -> simplify
# ---------------------------------------------------------------------------------------------------------------------
def test_clean_smooth_simplify(sc, rc):
    print("m: faces %s -> %s -> %s; vertices %s -> %s -> %s"
          % tuple([len(x) for x in rc[k][w]] for w in ("faces", "verts") for k in ("clean", "smooth", "simplify")))
    cr.hold(cr.figures_m(sc, rc), drift=True)
    topo = cr.topology_counts(rc)
    print("m: (referenced, edges, boundary, non-manifold, valid faces, euler) %s" % topo)
    assert topo == cr.TOPOLOGY
    for c, v in zip(rc["clean"]["counts"], rc["model"]["mesh"]["verts"]):
        assert c[0] <= len(v) and c[3] <= c[2]
    print("m: components kept %s" % [(int(c[3]), int(c[2])) for c in rc["clean"]["counts"]])


# ---------------------------------------------------------------------------------------------------------------------
# n. evaluation
# ---------------------------------------------------------------------------------------------------------------------
def signed_of(s):
    return np.where(s["sign"] < 0, -1.0, 1.0) * np.sqrt(s["d2"].astype(np.float64))


def test_evaluation(sc, rc):
    ev = rc["eval"]
    fig = cr.eval_figures(sc, rc["clean"]["verts"], [np.sqrt(d) for d in ev["d2"]])
    for b, (diff, tol, ok) in enumerate(fig):
        print("n: track %d: |point_mesh_distance - float64| at most %.3e (allowed at most %.3e)" % (b, diff, tol))
        assert ok
    shares = [cr.signed_shares(*(signed_of(s) for s in ev["signed"][b])) for b in range(cs.B)]
    print("n: %s truth points" % [len(ev["signed"][b][0]["d2"]) for b in range(cs.B)])
    cr.hold({"n.towards": [s[0] for s in shares], "n.away": [s[1] for s in shares]}, drift=True)
    # control: the winding reversed, the signs flip
    for b in range(cs.B):
        wrong = [meshsdf_ref.signed(p, rc["clean"]["verts"][b], rc["clean"]["faces"][b][:, ::-1])
                 for p in cr.moved_truth_points(sc, b, VOXEL)]
        w = cr.signed_shares(*(signed_of(s) for s in wrong))
        print("control winding reversed (n): track %d: shares %s -> %s" % (b, shares[b], w))
        assert w[0] < 0.5 * shares[b][0] and w[1] < 0.5 * shares[b][1]


def test_true_mesh_as_a_volume(sc, rc):
    ex = cr.front_facing_exclusion(sc)
    figs, r = cr.figures_l(sc, rc["truth_raycast"], stage="n.cast", exclude=ex)
    print("n: mesh_to_tsdf of the true mesh, ray cast: interior pixels with a front-facing face %s" % cr.per(r, "n"))
    cr.hold(figs, drift=True)
    # the pixels left out are the wall's and nothing else; there the cast finds nothing
    for b in range(cs.B):
        for v in range(cs.V):
            T = sc.truth[b][v]
            out = ex[b][v] & T["hit"]
            assert (T["face"][out] // 2 == 0).all() and (b == 0 or not out.any())
            assert not np.isfinite(rc["truth_raycast"][b, v][out & T["interior"]]).any()


# ---------------------------------------------------------------------------------------------------------------------
# o. colours
# ---------------------------------------------------------------------------------------------------------------------
def test_colours(sc, rc):
    figs, c = cr.figures_o(sc, rc["colored"], rc["colors"])
    for b, f in enumerate(c):
        print("o: track %d: %d candidates, %d truly occluded and %d truly visible outside grey, %d vertices judged"
              % (b, f["candidates"], f["n_occ"], f["n_vis"], f["n"]))
    cr.hold(figs, drift=True)
    assert all(g <= cr.GREY_CAP for g in figs["o.grey"])
    wide = cr.color_figures(sc, rc["colored"], rc["colors"], cr.margin_of(VOXEL), reach=1.0)
    print("o: at a reach of one voxel: grey %s, occluded but used %s of %s" % (cr.per(wide, "grey"), cr.per(wide, "occ_used"),
                                                                           cr.per(wide, "n_occ")))
    none = cr.color_figures(sc, rc["colored"], rc["colors"], cr.margin_of(VOXEL), reach=0.0)
    print("o: without the silhouette rule: grey %s, occluded but used %s of %s" % (cr.per(none, "grey"), cr.per(none, "occ_used"),
                                                                             cr.per(none, "n_occ")))
    assert max(cr.per(wide, "occ_used")) == 0


def test_colour_controls(sc, rc):
    m, margin = rc["colored"], cr.margin_of(VOXEL)
    right = cr.per(cr.figures_o(sc, m, rc["colors"])[1], "median")
    wrongs = {"R transposed": (rc["images"], cr.transposed(sc.R), sc.t), "t negated": (rc["images"], sc.R, -sc.t),
              "images offset by half a pixel": (cr.half_pixel_images(rc["images"]), sc.R, sc.t)}
    for name, (images, R, t) in wrongs.items():
        col = cr.colors_of(sc, m, images, rc["hit"], R, t, margin)
        wrong = cr.color_median_all(sc, m, col)
        print("control %s (o): median colour error %s -> %s" % (name, right, wrong))
        assert all(w > 2 * r for w, r in zip(wrong, right))


# ---------------------------------------------------------------------------------------------------------------------
# p. the matcher's own depths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voxel", cr.VOXELS_P)
def test_matcher_depths(sc, ch, pm, voxel):
    for name in ("keep", "plain"):
        cr.hold(cr.figures_p(sc, ch["mdepth"], pm["valid"][name], pm["models"][voxel, name], voxel, "p.%g.%s" % (voxel, name)),
                drift=True)
