"""The second half of the README's chain on the GPU against the float64 truth of the rendered scene: the depth maps of the
two tracks through the Python layer (torchext.depth_normals / depth_icp / depth_consistency / tsdf_integrate /
tsdf_surface_points / tsdf_raycast, mesh.tsdf_mesh, meshops.clean_tsdf_mesh, meshsmooth.smooth_tsdf_mesh,
meshsimplify.simplify_tsdf_mesh, mesheval.point_mesh_distance, meshsdf.point_mesh_signed_distance / mesh_to_tsdf,
meshcolor.color_tsdf_mesh), once, in a module fixture, both tracks in one call wherever the API batches: 3729 against 591
vertices, and one track with misses.  Every stage is held to the predicates and thresholds that
tests/test_chain_recon_host.py establishes on the reference chain (tests/chain_ref.py: `recon`, `RECON`), and -- where the
op is bit-exact by contract -- to that chain bit for bit.  Nothing outside the repository is read.

Measured on an MI355X (the tests print the figures; run with -s).  Every figure equals the reference chain's:
  i  depth_normals equal icp_ref.normals bit for bit; 33336 interior pixels, median angle 0.0069 degrees, largest 0.029; all
     face their camera
  j  depth_icp from the reference's perturbed poses (its f64 sums differ from the restatement's in the last bits, so the
     poses are held to the predicate): ok == 1 on the same 4 of 6 views, median distance ratios 0.0037, 0.011, 0.0049,
     0.031; the two views with ok == 0 come back as on the CPU, one unmoved, one 0.31 from the mesh
  k  keep, tsdf, weight, vertices, gradient normals, src and faces equal the restatements bit for bit in the one call over
     both tracks; median 1.2e-4 / 8.1e-5, p99 6.0e-4 / 7.2e-3, largest 2.4e-2 / 8.3e-3, none beyond a voxel; complete to
     6.6e-3 / 1.8e-4; winding and gradient agreement 1.0
  l  tsdf_raycast at the four views and the pose that is no view equals tsdf_ref.raycast bit for bit; hit share 1.0 (0.937
     in view 2 of track 0), |depth - z64| at most 0.023 voxel, no depth on a true miss
  m  clean, smooth and simplify equal their restatements bit for bit (vertices, faces, normals); medians x 0.994 / 0.978,
     x 0.903 / 0.765, x 1.054 / 0.990; 0.236 / 0.232 of the faces; MeshAdjacency counts as on the CPU
  n  every mesh query runs twice, with bvh=None and through an explicit renderer.MeshBVH of its mesh (asserted usable;
     bvh='auto' would build no tree at these sizes: the true meshes have 38 / 36 faces, the cleaned model 6899 / 1068).
     point_mesh_distance equals pointmesh_ref bit for bit and float64 within 2.4e-7; point_mesh_signed_distance: faces
     and distances bit for bit, signs wherever the pseudonormal's dot is clear; all moved truth points on their side
     (control, winding reversed: none); mesh_to_tsdf of the true meshes: the two routes give the same bits, 112651 of
     1334880 voxels within trunc, |tsdf| and the signs (outside 2173 voxels too close to call, where they agree too) as
     the restatement's with torch's own arithmetic on top; its ray cast: all judged pixels hit, at most 0.033 voxel off
  o  color_tsdf_mesh (its own bvh='auto', brute force at these sizes) and view_colors per track by brute force and through
     a MeshBVH equal viewcolor_ref bit for bit (colour, weight, n_views, flags); grey 0.092 / 0, occluded but used 0.160 /
     0, visible but dropped 0 / 0, colour error median 3.5e-5 / 3.1e-5
  p  the matcher's depths at voxel 0.025, 0.05, 0.1, with keep and with the plain mask: volumes, meshes and cleaned meshes
     equal the restatements bit for bit, so every figure (those of k, and the cleaned model's) is the host file's
  controls through the kernels: R transposed, t negated, views interleaved (k, l), TSDF sign flipped, winding reversed (n), R
     transposed, t negated and images offset by half a pixel in the colours: the scores of the host file
"""
import numpy as np
import pytest
import torch

from tests import chain_ref as cr, chain_scene as cs

pytestmark = pytest.mark.gpu

F = np.float32
VOXEL = cr.VOXEL


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_(t):
    return t.detach().cpu().numpy()


def same_floats(a, b):
    """equal, NaN in the same places (a NaN's payload is not part of any contract)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def dsqrt(d2):
    """torch.sqrt on the device, as mesheval and meshsdf take it"""
    return host_(torch.sqrt(dev(d2)))


def mesh_np(m):
    """a mesh.TsdfMesh -> the per-track lists of tests/chain_ref.py"""
    out = dict(verts=[], faces=[], normals=[])
    for b in range(m.n_tracks):
        v, f, n = m.track(b)
        out["verts"].append(host_(v))
        out["faces"].append(host_(f))
        out["normals"].append(None if n is None else host_(n))
    return out


def same_mesh(got, want, normals=True):
    keys = ("verts", "faces", "normals") if normals else ("verts", "faces")
    return all(same_floats(a, b) for k in keys for a, b in zip(got[k], want[k]))


def topology_np(m):
    from connecting_the_dots_amd import meshsmooth
    out = []
    for b in range(m.n_tracks):
        v, f, _ = m.track(b)
        a = meshsmooth.MeshAdjacency(f, v.shape[0])
        out.append((a.n_referenced, a.n_edges, a.n_boundary_edges, a.n_nonmanifold_edges, a.n_valid_faces, a.euler))
    return out


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


def build_model(te, mesh, sc_t, depth, valid, R, t, voxel):
    """tsdf_volume -> tsdf_integrate -> tsdf_mesh, both tracks in one call each"""
    origin, dims = cs.recon_grid(voxel)
    origin = dev(origin)
    tsdf, weight = te.tsdf_volume(cs.B, *dims)
    te.tsdf_integrate(tsdf, weight, origin, voxel, depth, sc_t["ray"], sc_t["K"], R, t, valid=valid)
    return dict(tsdf=tsdf, weight=weight, origin=origin, dims=dims,
                m=mesh.tsdf_mesh(tsdf, weight, origin, voxel, return_normals=True))


@pytest.fixture(scope="module")
def g(sc, ch, rc):
    """the second half of the README's chain on the GPU through the Python layer, once, B = 2 in every batched call"""
    from connecting_the_dots_amd import mesh, meshcolor, mesheval, meshops, meshsdf, meshsimplify, meshsmooth, renderer
    from connecting_the_dots_amd import torchext as te
    out = {}
    depth = dev(ch["render"]["depth"])                            # test_chain_truth_gpu.py: the GPU renders these very bits
    hit = depth > 0
    K, ray, R, t = dev(sc.K), dev(sc.ray), dev(sc.R), dev(sc.t)
    sc_t = dict(K=K, ray=ray)
    out.update(depth=depth, hit=hit, R=R, t=t, sc_t=sc_t)
    # i. normals, j. ICP from the reference's perturbed poses
    out["normal"] = te.depth_normals(depth, ray, hit)
    Ri, ti, info = te.depth_icp(depth, ray, K, dev(rc["icp"]["R0"]), dev(rc["icp"]["t0"]), hit, iters=10, max_rel=cr.ICP_MAX_REL)
    out["icp"] = dict(R0=rc["icp"]["R0"], t0=rc["icp"]["t0"], R=host_(Ri), t=host_(ti), ok=host_(info["ok"]),
                      rmse=host_(info["rmse"]))
    # k. consistency -> integrate -> surface points + mesh
    keep = te.depth_consistency(depth, ray, K, R, t, hit, max_px=cs.MAX_PX, max_rel=cr.RECON_MAX_REL)[1]
    out["keep"] = keep
    model = build_model(te, mesh, sc_t, depth, keep, R, t, VOXEL)
    out["model"] = model
    out["points"] = te.tsdf_surface_points(model["tsdf"], model["weight"], model["origin"], VOXEL, return_normals=True)
    # l. ray cast at the views and at the pose that is no view
    Rc, tc, _ = cr.cast_poses()
    Rc, tc = dev(Rc), dev(tc)
    cast = lambda T, w: te.tsdf_raycast(T, w, model["origin"], VOXEL, ray, Rc, tc, cs.H, cs.W, d_min=cr.D_MIN,
                                        step=cr.step_of(VOXEL), n_steps=cr.N_STEPS)
    out["raycast"] = cast(model["tsdf"], model["weight"])
    # m. clean -> smooth -> simplify
    out["clean"] = meshops.clean_tsdf_mesh(model["m"], min_faces=cr.MIN_FACES)
    out["smooth"] = meshsmooth.smooth_tsdf_mesh(out["clean"])
    out["simplify"] = meshsimplify.simplify_tsdf_mesh(out["smooth"], cell=cr.cell_of(VOXEL))
    # n. evaluation, by brute force and through an explicit tree of each mesh ('auto' would build none: the true meshes
    # have 38 / 36 faces and the cleaned model 6899 / 1068, below every AUTO_BVH_MIN_FACES)
    truth = [(dev(m["verts"]), dev(m["faces"].astype(np.int32))) for m in sc.meshes]
    cleaned = [out["clean"].track(b)[:2] for b in range(cs.B)]
    trees = dict(truth=[renderer.MeshBVH(*m) for m in truth], clean=[renderer.MeshBVH(*m) for m in cleaned])
    out["trees_usable"] = [tr.usable and tr.matches(*m) for key, ms in (("truth", truth), ("clean", cleaned))
                           for tr, m in zip(trees[key], ms)]
    out["eval"], out["truth_volume"], out["truth_raycast"] = {}, {}, {}
    for name in ("brute", "bvh"):
        ev = dict(dist=[], face=[], signed=[])
        for b in range(cs.B):
            cv, cf = cleaned[b]
            dist, face = mesheval.point_mesh_distance(cv, *truth[b], bvh=trees["truth"][b] if name == "bvh" else None)
            ev["dist"].append(host_(dist))
            ev["face"].append(host_(face))
            tree = trees["clean"][b] if name == "bvh" else None
            ev["signed"].append([tuple(host_(a) for a in meshsdf.point_mesh_signed_distance(dev(p), cv, cf, bvh=tree))
                                 for p in cr.moved_truth_points(sc, b, VOXEL)])
        out["eval"][name] = ev
        tv = [meshsdf.mesh_to_tsdf(*truth[b], model["origin"][b].contiguous(), VOXEL, model["dims"], trunc=4 * VOXEL,
                                   bvh=trees["truth"][b] if name == "bvh" else None) for b in range(cs.B)]
        out["truth_volume"][name] = tuple(torch.cat([x[k] for x in tv]).contiguous() for k in (0, 1))
        out["truth_raycast"][name] = cast(*out["truth_volume"][name])
    # control: the winding reversed, the signs flip
    out["control_signed"] = [[host_(meshsdf.point_mesh_signed_distance(dev(p), cleaned[b][0], cleaned[b][1].flip(1).contiguous())[0])
                              for p in cr.moved_truth_points(sc, b, VOXEL)] for b in range(cs.B)]
    # o. colours: the cleaned model with the normals of its faces, valid = the truth's hit masks.  color_tsdf_mesh picks
    # its own route ('auto': brute force at these sizes); view_colors per track by brute force and through a tree
    images, valid = dev(rc["images"]), dev(rc["hit"])
    out["colored"] = meshsmooth.smooth_tsdf_mesh(out["clean"], iters=0)
    margin = cr.margin_of(VOXEL)
    out["colors"] = meshcolor.color_tsdf_mesh(out["colored"], images, K, R, t, margin=margin, valid=valid, return_flags=True)
    out["colors_route"] = {"brute": [], "bvh": []}
    for b in range(cs.B):
        v, f, n = out["colored"].track(b)
        tree = renderer.MeshBVH(v, f)
        out["trees_usable"].append(tree.usable and tree.matches(v, f))
        for name, bvh in (("brute", None), ("bvh", tree)):
            out["colors_route"][name].append(meshcolor.view_colors(v, images[b], K, R[b], t[b], margin, v, f, normals=n,
                                                                   valid=valid[b], bvh=bvh, return_flags=True))
    # the controls through the kernels: wrong poses and frame order in integrate, wrong poses and shifted images in colours
    Rt = R.transpose(-1, -2).contiguous()
    il = lambda a: dev(cr.interleaved_views(host_(a)))
    out["control_models"] = {"R transposed": build_model(te, mesh, sc_t, depth, keep, Rt, t, VOXEL),
                             "t negated": build_model(te, mesh, sc_t, depth, keep, R, -t, VOXEL),
                             "views interleaved as v * B + b": build_model(te, mesh, sc_t, il(depth), il(keep), R, t, VOXEL)}
    cm = out["control_models"]["views interleaved as v * B + b"]
    out["control_raycast"] = cast(cm["tsdf"], cm["weight"])
    out["control_flipped"] = mesh.tsdf_mesh(-model["tsdf"], model["weight"], model["origin"], VOXEL, return_normals=True)
    color = lambda im, R_, t_: meshcolor.color_tsdf_mesh(out["colored"], im, K, R_, t_, margin=margin, valid=valid)
    out["control_colors"] = {"R transposed": color(images, Rt, t), "t negated": color(images, R, -t),
                             "images offset by half a pixel": color(dev(cr.half_pixel_images(rc["images"])), R, t)}
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def gp(sc, ch, pm, g):
    """stage p on the GPU: the matcher's depths of the reference chain (test_chain_truth_gpu.py holds the GPU's to the same
    bits) through depth_consistency, tsdf_integrate, tsdf_mesh and clean_tsdf_mesh at the three voxel sizes"""
    from connecting_the_dots_amd import mesh, meshops, torchext as te
    mdepth, plain = dev(ch["mdepth"]), dev(ch["keep"])
    keep = te.depth_consistency(mdepth, g["sc_t"]["ray"], g["sc_t"]["K"], g["R"], g["t"], plain, max_px=cs.MAX_PX,
                                max_rel=cr.RECON_MAX_REL)[1]
    out = {"valid": {"keep": keep, "plain": plain}, "models": {}}
    for voxel in cr.VOXELS_P:
        for name in ("keep", "plain"):
            model = build_model(te, mesh, g["sc_t"], mdepth, out["valid"][name], g["R"], g["t"], voxel)
            model["clean"] = meshops.clean_tsdf_mesh(model["m"], min_faces=cr.MIN_FACES)
            out["models"][voxel, name] = model
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# i. normals, j. ICP
# ---------------------------------------------------------------------------------------------------------------------
def test_normals(sc, rc, g):
    normal = host_(g["normal"])
    assert same_floats(normal, rc["normal"])
    figs, f = cr.figures_i(sc, normal)
    assert f["facing"]
    cr.hold(figs)


def test_icp(sc, rc, g):
    """the GPU's sums differ from the restatement's in their last bits, so the poses are held to the predicate, not to
    the reference's bits: every view that ends with ok == 1 has moved its points to the true mesh"""
    fig = cr.icp_figures(sc, g["icp"])
    for f in fig:
        print("j: track %d view %d: ok %d, median distance %.3e -> %.3e (ratio %.4g)" % (f["b"], f["v"], f["ok"], f["before"],
                                                                                      f["after"], f["ratio"]))
    good = [f for f in fig if f["ok"] == 1]
    assert len(good) >= 3
    cr.hold({"j.ratio": [max(f["ratio"] for f in good)]})
    assert (g["icp"]["ok"][:, 0] == 0).all() and np.array_equal(g["icp"]["R"][:, 0], sc.R[:, 0])      # view 0 is the target


# ---------------------------------------------------------------------------------------------------------------------
# k. integrate + surface points + mesh, l. ray cast
# ---------------------------------------------------------------------------------------------------------------------
def test_model(sc, rc, g):
    ref, model = rc["model"], g["model"]
    assert same_floats(host_(g["keep"]).astype(np.uint8), rc["keep"])
    assert same_floats(host_(model["tsdf"]), ref["tsdf"]) and same_floats(host_(model["weight"]), ref["weight"])
    m = mesh_np(model["m"])
    assert same_mesh(m, ref["mesh"]) and same_floats(host_(model["m"].src), ref["src"])
    points, src, n, normals = (host_(a) for a in g["points"])
    assert same_floats(points, host_(model["m"].verts)) and same_floats(normals, host_(model["m"].normals))
    assert same_floats(src, ref["src"]) and n.tolist() == [len(v) for v in m["verts"]]
    assert min(n) > 500 and max(n) > 5 * min(n)                   # two tracks of very unequal size in one call
    cr.hold(cr.figures_k(sc, m))


def test_raycast(sc, rc, g):
    cast = host_(g["raycast"])
    assert same_floats(cast, rc["raycast"])
    cr.hold(cr.figures_l(sc, cast)[0])


def test_model_controls(sc, rc, g):
    right = cr.per(cr.vertex_figures(sc, rc["model"]["mesh"]["verts"], VOXEL), "median")
    for name, model in g["control_models"].items():
        wrong = cr.per(cr.vertex_figures(sc, mesh_np(model["m"])["verts"], VOXEL), "median")
        print("control %s (k): median vertex distance %s -> %s" % (name, right, wrong))
        assert all(w > 2 * r for w, r in zip(wrong, right))
    score = lambda d: float(np.mean(cr.per(cr.raycast_figures(sc, d, VOXEL), "close")))
    good, bad = score(host_(g["raycast"])), score(host_(g["control_raycast"]))
    print("control views interleaved (l): interior pixels with a depth within 0.1 voxel %.4f -> %.4f" % (good, bad))
    assert bad < 0.5 * good
    margin = cr.margin_of(VOXEL)
    right = [w[0] for w in cr.winding_share(sc, mesh_np(g["model"]["m"]), margin)]
    wrong = [w[0] for w in cr.winding_share(sc, mesh_np(g["control_flipped"]), margin)]
    print("control TSDF sign flipped (k): winding share %s -> %s" % (right, wrong))
    assert all(w < 0.5 * r for w, r in zip(wrong, right))


# ---------------------------------------------------------------------------------------------------------------------
# m. clean -> smooth -> simplify
# ---------------------------------------------------------------------------------------------------------------------
def test_clean_smooth_simplify(sc, rc, g):
    got = {"model": {"mesh": mesh_np(g["model"]["m"])}}
    for step in ("clean", "smooth", "simplify"):
        got[step] = mesh_np(g[step])
        assert same_mesh(got[step], rc[step], normals=step != "clean"), step
    assert all(same_floats(a, b) for a, b in zip(got["clean"]["normals"], rc["clean"]["normals"]))   # gathered TSDF gradients
    cr.hold(cr.figures_m(sc, got))
    topo = {"smooth": topology_np(g["smooth"]), "simplify": topology_np(g["simplify"])}
    print("m: (referenced, edges, boundary, non-manifold, valid faces, euler) %s" % topo)
    assert topo == cr.TOPOLOGY


# ---------------------------------------------------------------------------------------------------------------------
# n. evaluation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["brute", "bvh"])
def test_evaluation(sc, rc, g, route):
    assert all(g["trees_usable"])                                # the bvh route really goes through a tree of its tensors
    ev, ref = g["eval"][route], rc["eval"]
    verts = mesh_np(g["clean"])["verts"]
    for b in range(cs.B):
        assert same_floats(ev["dist"][b], dsqrt(ref["d2"][b])) and same_floats(ev["face"][b], ref["face"][b])
    for b, (diff, tol, ok) in enumerate(cr.eval_figures(sc, verts, ev["dist"])):
        print("n: track %d: |point_mesh_distance - float64| at most %.3e (allowed at most %.3e)" % (b, diff, tol))
        assert ok
    shares = []
    for b in range(cs.B):
        for (sdist, face), want in zip(ev["signed"][b], ref["signed"][b]):
            assert same_floats(face, want["face"]) and same_floats(np.abs(sdist), dsqrt(want["d2"]))
            clear = np.abs(want["dot"]) > 1e-9 * want["S"]        # tests/meshsdf_ref.py: signs compare where the dot is clear
            assert np.array_equal(np.sign(sdist)[clear], want["sign"][clear].astype(F))
        shares.append(cr.signed_shares(*(s[0] for s in ev["signed"][b])))
    cr.hold({"n.towards": [s[0] for s in shares], "n.away": [s[1] for s in shares]})
    for b in range(cs.B):                                        # control: the winding reversed, the signs flip
        w = cr.signed_shares(*g["control_signed"][b])
        print("control winding reversed (n): track %d: shares %s -> %s" % (b, shares[b], w))
        assert w[0] < 0.5 * shares[b][0] and w[1] < 0.5 * shares[b][1]


@pytest.mark.parametrize("route", ["brute", "bvh"])
def test_true_mesh_as_a_volume(sc, rc, g, route):
    """the volume is held to the restatement's d2 and sign with the layer's own torch arithmetic on top (sqrt, the
    division by trunc, the minimum), the ray cast of it to the truth"""
    assert all(g["trees_usable"])
    T, w = (host_(a) for a in g["truth_volume"][route])
    for a, b in zip(g["truth_volume"]["brute"], g["truth_volume"]["bvh"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))          # the two routes: the same bits
    parts = rc["truth_parts"]
    hit = np.isfinite(parts["d2"])
    assert same_floats(w.reshape(cs.B, -1), hit.astype(F)) and int(hit.sum()) > 10000
    d2, sign = dev(np.where(hit, parts["d2"], F(0))), dev(parts["sign"])
    dist = torch.sqrt(d2)
    want = torch.minimum(torch.ones((), device="cuda"), torch.where(sign < 0, -dist, dist) / torch.tensor(4 * VOXEL, device="cuda"))
    want = host_(torch.where(dev(hit), want, torch.zeros((), device="cuda")))
    got = T.reshape(cs.B, -1)
    clear = parts["clear"]
    print("n: mesh_to_tsdf: %d of %d voxels within trunc, %d of them with a pseudonormal too close to call"
          % (hit.sum(), hit.size, (~clear).sum()))
    assert same_floats(np.abs(got), np.abs(want)) and np.array_equal(got[clear], want[clear])
    assert np.abs(got - rc["truth_volume"][0].reshape(cs.B, -1))[clear].max() <= 2 ** -23     # numpy's sqrt and division: an ulp of 1
    cast = host_(g["truth_raycast"][route])
    cr.hold(cr.figures_l(sc, cast, stage="n.cast", exclude=cr.front_facing_exclusion(sc))[0])


# ---------------------------------------------------------------------------------------------------------------------
# o. colours
# ---------------------------------------------------------------------------------------------------------------------
def colors_np(vc, m):
    n = np.concatenate([[0], np.cumsum([len(v) for v in m["verts"]])])
    return {k: [host_(getattr(vc, k))[n[b]:n[b + 1]] for b in range(cs.B)] for k in ("color", "weight", "n_views", "flags")}


def test_colours(sc, rc, g):
    m = mesh_np(g["colored"])
    assert same_mesh(m, rc["colored"])
    col = colors_np(g["colors"], m)
    assert all(g["trees_usable"])
    for b in range(cs.B):
        for k in ("color", "weight", "n_views", "flags"):
            assert same_floats(col[k][b], rc["colors"][k][b]), (k, b)
            for route in ("brute", "bvh"):
                assert same_floats(host_(getattr(g["colors_route"][route][b], k)), rc["colors"][k][b]), (k, b, route)
    figs, _ = cr.figures_o(sc, m, col)
    cr.hold(figs)
    assert all(x <= cr.GREY_CAP for x in figs["o.grey"])


def test_colour_controls(sc, rc, g):
    m = mesh_np(g["colored"])
    right = cr.per(cr.figures_o(sc, m, colors_np(g["colors"], m))[1], "median")
    for name, vc in g["control_colors"].items():
        n = np.concatenate([[0], np.cumsum([len(v) for v in m["verts"]])])
        col = {"color": [host_(vc.color)[n[b]:n[b + 1]] for b in range(cs.B)]}
        wrong = cr.color_median_all(sc, m, col)
        print("control %s (o): median colour error %s -> %s" % (name, right, wrong))
        assert all(w > 2 * r for w, r in zip(wrong, right))


# ---------------------------------------------------------------------------------------------------------------------
# p. the matcher's own depths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("voxel", cr.VOXELS_P)
def test_matcher_depths(sc, ch, pm, gp, voxel):
    for name in ("keep", "plain"):
        assert same_floats(host_(gp["valid"][name]).astype(np.uint8), pm["valid"][name].astype(np.uint8))
        model, ref = gp["models"][voxel, name], pm["models"][voxel, name]
        assert same_floats(host_(model["tsdf"]), ref["tsdf"]) and same_floats(host_(model["weight"]), ref["weight"])
        got = dict(mesh=mesh_np(model["m"]), clean=mesh_np(model["clean"]))
        assert same_mesh(got["mesh"], ref["mesh"]) and same_mesh(got["clean"], ref["clean"])
        cr.hold(cr.figures_p(sc, ch["mdepth"], pm["valid"][name], got, voxel, "p.%g.%s" % (voxel, name)))
