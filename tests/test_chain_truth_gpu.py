"""The matching-to-fusion chain on the GPU against rendered ground truth: two tracks rendered by
synth.render_track_sample, then the README's chain through the HIP ops, once, in a module fixture.  Every stage is held
against the float64 truth of tests/chain_scene.py with the predicates and thresholds that tests/test_chain_truth_host.py
establishes on the CPU reference chain (tests/chain_ref.py), and -- where the op is bit-exact by contract -- against
that chain bit for bit.

Measured on an MI355X (the tests print the figures; run with -s).  Every figure equals the reference chain's:
  a  renderer.render_mesh_proj, brute force and through a MeshBVH: depth, colour and the three-channel ambient equal
     the oracle bit for bit on all 8 views; render_track_sample (brute force and bvh='auto'): the blended frame and the
     ambient image likewise; disp0 within 2 ulp of f b / depth; the hit mask equals the
     float64 one in every pixel; depth against z64 on interior pixels: largest relative difference 2.913e-07
  b  truth share on 32781 good pixels: exact 0.99994 (32779), fast with a prepared pattern 0.99994 (32779), fused LCN +
     matcher 0.99994 (32779) with an allowance of N = 1 pixel; census_sad 0.99783 (32710); sad 0.99936 (32760); every
     index tensor equals the reference's
  c  offset 4, D = 16: share 1.0; idx_to_depth inside z64 (1 +- 1.5 / d64) on all of them (offset negated: none);
     depth_to_disp gives idx back within 2 ulp
  d  32779 pixels, mean |idx - d64| 0.19387; parabola: mean |disp - d64| 0.072264 (float64 rule 0.072264), signed
     +0.028928 (+0.028928); equiangular: 0.043581 (0.043581), signed +0.017263 (+0.017263); bit-identical to the
     float32 rule on the exact volume
  e  flags, idx_r and gap equal validity_ref bit for bit (the fast route: the same flags, gap within its stated bound);
     truth share among flags == 7 0.98421 against 0.94749 in-pattern; flags == 7 on shadow 0.3595, on good 0.99826;
     idx_r at 658 good pixels across a disparity step: within a pixel of d64 read at column w - round(d64) 1.00000, at
     the pixel's own column 0.3252; idx_r[w - idx] == idx on 0.98032 of 32724 pixels, never off by more than lr_tol = 1
  f  SGM NCC 1.0 against 0.99994 plain, SGM SAD 0.99997 against 0.99937 on 33094 lit interior pixels; disparity_filter
     keeps 0.98552 correct against 0.98421; outputs equal sgm_ref / dispfilter_ref bit for bit
  g  204842 truly visible (pixel, view) pairs outside unsure: all counted, none counted that is not visible; fused
     points at most 3.791e-04 / 7.039e-04 from their own mesh, at least 0.135 / 0.120 from the other track's; geometric loss 0.1213 / 0.1681 at
     the true depths against 0.1662 / 0.1737 (x 1.01) and 0.1680 / 0.1768 (x 0.99)
  h  k = 1 / 3: the warped prior inside the matcher's depth error on all 8264 / 7688 pixels; the band holds round(d64) on
     every good pixel; the band index equals the full search's wherever that lies in the band; truth share 1.0 / 1.0
"""
import numpy as np
import pytest
import torch

from tests import chain_ref as cr, chain_scene as cs, f64_refs, validity_ref

pytestmark = pytest.mark.gpu

F = np.float32
HW = cs.H * cs.W
N = cr.N


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host_(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.shape == b.shape and np.array_equal(a, b)


def same_floats(a, b):
    """equal, NaN in the same places (a NaN's payload is not part of any contract)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


@pytest.fixture(scope="module")
def sc():
    return cs.scene()


@pytest.fixture(scope="module")
def ch(oracle):
    return cr.chain()


@pytest.fixture(scope="module")
def masks(sc):
    return {k: sc.stack(k) for k in ("good", "interior", "lit64", "shadow", "hit", "d64", "z64")}


@pytest.fixture(scope="module")
def g(te, sc):
    """the two tracks rendered and the whole chain run on the GPU, once"""
    from connecting_the_dots_amd import renderer, synth
    out = {}
    pattern3 = dev(sc.pattern3)
    for name, bvh in (("brute", None), ("bvh", "auto")):
        out[name] = [synth.render_track_sample(sc.meshes[b], [pattern3], sc.K, np.random.RandomState(cs.POSE_SEEDS[b]),
                                               track_length=cs.V, baseline=cs.BASELINE, data_aug=False, bvh=bvh)
                     for b in range(cs.B)]
    samples = out["brute"]
    # depth and colour are not part of a sample: the same renders through the renderer's own entry point, at the poses
    # the samples report
    shader = renderer.PyShader(*cs.SHADER)
    fx, fy, px, py = (float(sc.K[0, 0]), float(sc.K[1, 1]), float(sc.K[0, 2]), float(sc.K[1, 2]))
    direct = {"brute": [], "bvh": []}
    for b in range(cs.B):
        m = sc.meshes[b]
        tree = renderer.MeshBVH(dev(m["verts"]), dev(m["faces"]))
        verts, colors, faces = tree.verts, dev(m["colors"]), tree.faces
        R, t = host_(samples[b]["R"]), host_(samples[b]["t"])
        for v in range(cs.V):
            cam = renderer.PyCamera(fx, fy, px, py, R[v], t[v], cs.W, cs.H)
            proj = renderer.PyCamera(fx, fy, px, py, R[v], t[v] + np.array([-cs.BASELINE, 0, 0], F), cs.W, cs.H)
            for name, bvh in (("brute", None), ("bvh", tree)):
                direct[name].append(renderer.render_mesh_proj(verts, colors, faces, cam, proj, shader, pattern3, cs.D_ALPHA,
                                                              cs.D_BETA, bvh=bvh))
    for name, views in direct.items():
        out["direct_" + name] = tuple(torch.stack([r[i] for r in views]).view((cs.B, cs.V) + tuple(views[0][i].shape))
                                      for i in range(3))
    out["depth"] = out["direct_brute"][0]
    frames = torch.cat([s["im0"] for s in samples]).contiguous()                  # [B*V,1,H,W], frame b * V + v
    R = torch.stack([s["R"] for s in samples]).contiguous()
    t = torch.stack([s["t"] for s in samples]).contiguous()
    K, ray = dev(sc.K), dev(sc.ray)
    out.update(frames=frames, R=R, t=t)
    D, bs, bf = cs.D, cs.BLOCK, sc.bf
    # README: LCN -> match
    x = te.lcn(frames, cs.LCN_RADIUS, cs.LCN_EPS)[0]
    pl = te.lcn(dev(sc.pattern[None, None]), cs.LCN_RADIUS, cs.LCN_EPS)[0][0].contiguous()
    out.update(x=x, pl=pl)
    out["exact"] = te.xcorrvol_argmax(x, pl, D, bs, algo="exact")
    handle = te.prepare_pattern(pl, N, D, bs)
    out["fast"] = te.xcorrvol_argmax(x, pl, D, bs, algo="fast", prepared=handle)
    out["fused"] = te.lcn_xcorrvol_argmax(frames, pl, D, bs, cs.LCN_RADIUS, cs.LCN_EPS)
    out["cost"] = {name: te.costvol_argmin(x[:, 0], pl[0], D, bs, name, eps) for name, _, eps in cr.COSTS}
    # c. offset
    pl4 = te.lcn(dev(cr.shifted_pattern(sc.pattern)[None, None]), cs.LCN_RADIUS, cs.LCN_EPS)[0][0].contiguous()
    out["idx4"] = {a: te.xcorrvol_argmax(x, pl4, cr.OFFSET_D, bs, algo=a)[0] for a in ("exact", "fast")}
    out["depth4"] = te.idx_to_depth(out["idx4"]["exact"], bf, float(cr.OFFSET))
    out["depth4_neg"] = te.idx_to_depth(out["idx4"]["exact"], bf, -float(cr.OFFSET))
    out["back4"] = te.depth_to_disp(out["depth4"], bf, float(cr.OFFSET))
    # d. sub-pixel, e. validity
    out["subpixel"] = {m: te.xcorrvol_argmax(x, pl, D, bs, algo="exact", subpixel=m) for m in ("parabola", "equiangular")}
    out["validity"] = te.xcorrvol_argmax(x, pl, D, bs, algo="exact", validity=dict(cr.VALIDITY))
    idx = out["exact"][0]
    out["validity_op"] = {a: te.xcorrvol_validity(x, pl, idx, D, bs, algo=a, **cr.VALIDITY) for a in ("exact", "fast")}
    out["cost_validity"] = {name: te.costvol_validity(x[:, 0], pl[0], out["cost"][name][0], D, bs, name, eps,
                                                      lr_tol=1, min_gap=cr.COST_GAP[name], algo="exact")
                            for name, _, eps in cr.COSTS}
    # f. SGM and the filters
    out["sgm"] = te.xcorrvol_sgm(x, pl, D, bs, cr.SGM_P1, cr.SGM_P2, algo="exact")
    out["sgm_sad"] = te.costvol_sgm(x[:, 0], pl[0], D, bs, "sad", 0.5, cr.SGM_P1, cr.SGM_P2, algo="exact")
    flags = out["validity"][2]
    out["filter"] = te.disparity_filter(idx, flags == 7)
    # g. multi-view on the rendered depths
    hit = out["depth"] > 0
    out["consistency"] = te.depth_consistency(out["depth"], ray, K, R, t, hit, max_px=cs.MAX_PX, max_rel=cs.MAX_REL)
    out["fuse"] = te.depth_fuse_points(out["depth"], ray, K, R, t, hit, max_px=cs.MAX_PX, max_rel=cs.MAX_REL, min_views=1)
    # per (r, s) decisions: a track of the two views alone counts view s for the pixels of r
    pair = {}
    for r in range(cs.V):
        for s in range(cs.V):
            if s != r:
                sel = [r, s]
                pair[r, s] = te.depth_consistency(out["depth"][:, sel].contiguous(), ray, K, R[:, sel].contiguous(),
                                                  t[:, sel].contiguous(), hit[:, sel].contiguous(), max_px=cs.MAX_PX,
                                                  max_rel=cs.MAX_REL)[0][:, 0]
    out["pair"] = pair
    clamp0 = out["depth"].clamp(min=0)
    out["geo"] = {(b, k): float(te.geometric_loss((clamp0[b:b + 1, 0:1] * k).contiguous(), clamp0[b:b + 1, 1:2].contiguous(),
                                                  ray, K, R[b:b + 1, 0].contiguous(), t[b:b + 1, 0].contiguous(),
                                                  R[b:b + 1, 1].contiguous(), t[b:b + 1, 1].contiguous()))
                  for b in range(cs.B) for k in (1.0, 1.01, 0.99)}
    # h. the prior chain, as the README writes it
    disp = out["subpixel"]["parabola"][2]
    mdepth = te.disp_to_depth(torch.nan_to_num(disp), bf).view(cs.B, cs.V, cs.H, cs.W)
    keep = out["filter"][1].view(cs.B, cs.V, cs.H, cs.W)
    out.update(mdepth=mdepth, keep=keep)
    out["prior"] = {}
    for k in (1, cs.V - 1):
        first_k = torch.zeros((cs.B, cs.V), dtype=torch.bool, device="cuda")
        first_k[:, :k] = True
        view_k = torch.zeros((cs.B, cs.V), dtype=torch.bool, device="cuda")
        view_k[:, k] = True
        z, src = te.depth_warp(mdepth, ray, K, R, t, valid=keep, sources=first_k, targets=view_k, splat=1, return_src=True)
        z, src = z[:, k].contiguous(), src[:, k].contiguous()
        prior = te.depth_to_disp(z, bf, 0.0)
        lo, hi = te.disparity_band_window(prior, 1.0, D, window=3)
        xk = x[k::cs.V].contiguous()
        bidx, bbest = te.xcorrvol_argmax_band(xk, pl, lo, hi, D, bs)
        bv = te.xcorrvol_band_validity(xk, pl, lo, hi, D, bs, **cr.VALIDITY)
        out["prior"][k] = dict(z=z, src=src, prior=prior, lo=lo, hi=hi, idx=bidx, best=bbest, validity=bv)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a. render
# ---------------------------------------------------------------------------------------------------------------------
def test_render_equals_the_oracle_and_the_truth(sc, ch, g, masks):
    ref = ch["render"]
    for name in ("brute", "bvh"):
        depth, color, ambient3 = (host_(a) for a in g["direct_" + name])
        assert same_bits(depth, ref["depth"]) and same_bits(color, ref["color"]), name
        assert same_bits(ambient3, ref["ambient3"]), name
    for name in ("brute", "bvh"):
        im = np.concatenate([host_(s["im0"])[:, 0] for s in g[name]])
        amb = np.concatenate([host_(s["ambient0"])[:, 0] for s in g[name]])
        assert same_bits(im, ref["im"]) and same_bits(amb, ref["ambient"]), name
        disp0 = np.concatenate([host_(s["disp0"])[:, 0] for s in g[name]])
        hit = ref["depth"].reshape(N, cs.H, cs.W) > 0
        want = sc.bf / ref["depth"].reshape(N, cs.H, cs.W).astype(np.float64)
        assert (np.abs(disp0.astype(np.float64) - want)[hit] <= 2 * np.spacing(disp0[hit]).astype(np.float64)).all()
        # R and t come back in the order the views were rendered
        for b in range(cs.B):
            assert same_bits(host_(g[name][b]["R"]), sc.R[b]) and same_bits(host_(g[name][b]["t"]), sc.t[b])
    hit = host_(g["depth"]).reshape(N, cs.H, cs.W) > 0
    diff = int((hit != masks["hit"]).sum())
    rel = np.abs(host_(g["depth"]).reshape(N, cs.H, cs.W)[masks["interior"]] / masks["z64"][masks["interior"]] - 1).max()
    print("a: hit masks differ in %d pixels; depth vs z64 on interior: max rel %.3e" % (diff, rel))
    assert diff <= 0.01 * HW and rel < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# b. full search, c. offset
# ---------------------------------------------------------------------------------------------------------------------
def test_full_search(sc, ch, g, masks):
    exact = host_(g["exact"][0])
    assert same_bits(exact, ch["idx"])
    c_exact, n, share = cr.truth_share(exact, sc)
    print("b: exact truth share %.5f (%d of %d)" % (share, c_exact, n))
    assert share >= cr.SHARE_B["ncc"]
    v64 = f64_refs.xcorrvol(torch.from_numpy(ch["x"]), torch.from_numpy(ch["pl"]), cs.D, cs.BLOCK).numpy()
    best, gap = cr.gap64(v64)
    allowance = int((masks["good"] & (gap < 2 * cr.FAST_BOUND(best))).sum())
    assert same_bits(host_(g["fused"][0])[:, 0], ch["x"][:, 0])                 # the fused call's LCN output (exact)
    for name, idx in (("fast, prepared", g["fast"][0]), ("fused LCN + matcher", g["fused"][2])):
        c, _, share = cr.truth_share(host_(idx), sc)
        print("b: %s truth share %.5f (%d); allowance %d" % (name, share, c, allowance))
        assert c >= c_exact - allowance
    for name, _, _ in cr.COSTS:
        idx = host_(g["cost"][name][0])
        assert same_bits(idx, ch["cost"][name]["idx"])                          # the exact volume's argmin, bit for bit
        c, n, share = cr.truth_share(idx, sc)
        print("b: %s truth share %.5f (%d of %d)" % (name, share, c, n))
        assert share >= cr.SHARE_B[name]


def test_offset(sc, ch, g, masks):
    idx4 = host_(g["idx4"]["exact"])
    assert same_bits(idx4, ch["idx4"])
    c, n, share = cr.truth_share(idx4, sc, offset=cr.OFFSET)
    ok = masks["good"] & (np.abs(idx4 + cr.OFFSET - masks["d64"]) <= 1)
    inb = cr.depth_in_bound(host_(g["depth4"]), sc, ok)
    wrong = cr.depth_in_bound(host_(g["depth4_neg"]), sc, ok)
    print("c: offset share %.5f (%d of %d); depth inside the bound %.5f; offset negated %.4f" % (share, c, n, inb, wrong))
    assert share >= cr.SHARE_C and inb == 1.0 and wrong < 0.5 * inb
    assert same_bits(host_(g["depth4"]), ch["depth4"])
    assert cr.round_trip_ok(host_(g["back4"]), idx4)[ok].all()
    cf = cr.truth_share(host_(g["idx4"]["fast"]), sc, offset=cr.OFFSET)[0]
    v64 = f64_refs.xcorrvol(torch.from_numpy(ch["x"]), torch.from_numpy(ch["pl4"]), cr.OFFSET_D, cs.BLOCK).numpy()
    best, gap = cr.gap64(v64)
    assert cf >= c - int((masks["good"] & (gap < 2 * cr.FAST_BOUND(best))).sum())


# ---------------------------------------------------------------------------------------------------------------------
# d. sub-pixel, e. validity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parabola", "equiangular"])
def test_subpixel(sc, ch, g, masks, mode):
    idx, _, disp, refined = (host_(a) for a in g["subpixel"][mode])
    assert same_bits(idx, ch["idx"])
    assert same_floats(disp, ch["subpixel"][mode][0]) and same_bits(refined, ch["subpixel"][mode][1])
    cr.assert_subpixel(cr.subpixel_figures(sc, ch, masks, disp, refined, mode), mode)


def test_validity(sc, ch, g, masks):
    idx, _, flags, idx_r, gap = (host_(a) for a in g["validity"])
    rf, rr, rg = ch["validity"]
    assert same_bits(idx, ch["idx"]) and same_bits(flags, rf) and same_bits(idx_r, rr) and same_floats(gap, rg)
    for got, want in zip(g["validity_op"]["exact"], ch["validity"]):
        assert same_floats(host_(got), want)
    # the fast volume's route: the same flags and idx_r, the gap within the bound include/ctd_hip.h states for it
    ff, fr_, fg = (host_(a) for a in g["validity_op"]["fast"])
    _, s1, s2 = validity_ref.gap_of(ch["vol"], idx, True)
    with np.errstate(invalid="ignore"):
        near = np.abs(fg.astype(np.float64) - rg) <= 1e-5 * (np.abs(s1) + np.abs(s2)) + 2e-6
    assert same_bits(ff, rf) and same_bits(fr_, rr) and (near | (fg == rg)).all()
    fig = cr.validity_figures(sc, masks, idx, flags, idx_r)
    cr.assert_validity(fig, "NCC")
    cr.assert_idx_r(fig)
    for name, _, _ in cr.COSTS:
        got, want = g["cost_validity"][name], ch["cost"][name]["validity"]
        for a, b in zip(got, want):
            assert same_floats(host_(a), b), name
        cr.assert_validity(cr.validity_figures(sc, masks, host_(g["cost"][name][0]), host_(got[0]), host_(got[1])), name)


# ---------------------------------------------------------------------------------------------------------------------
# f. SGM and the filters
# ---------------------------------------------------------------------------------------------------------------------
def test_sgm_and_filter(sc, ch, g, masks):
    for key in ("sgm", "sgm_sad"):
        assert same_bits(host_(g[key][0]), ch[key][0]) and same_bits(host_(g[key][1]), ch[key][1]), key
    fdisp, fkeep = (host_(a) for a in g["filter"])
    assert same_floats(fdisp, ch["filter"][0]) and same_bits(fkeep, ch["filter"][1])
    cr.assert_sgm_and_filter(sc, masks, host_(g["exact"][0]), host_(g["sgm"][0]), host_(g["cost"]["sad"][0]),
                               host_(g["sgm_sad"][0]), host_(g["validity"][2]), fdisp, fkeep)


# ---------------------------------------------------------------------------------------------------------------------
# g. multi-view on the rendered depths
# ---------------------------------------------------------------------------------------------------------------------
def test_consistency_counts_exactly_the_visible_views(sc, ch, g):
    count, keep, fused = (host_(a) for a in g["consistency"])
    rc, rk, rfu = ch["consistency"]
    assert same_bits(count, rc) and same_bits(keep, rk) and same_floats(fused, rfu)
    pair = {k: host_(v) for k, v in g["pair"].items()}
    for (b, r, s), m in ch["matches"].items():
        assert np.array_equal(pair[r, s][b].reshape(-1) != 0, m["consistent"])
    counted, total, wrong = cr.visibility_agreement(sc, lambda b, r, s: pair[r, s][b] != 0)
    print("g: %d truly visible pairs outside unsure: %d counted, %d counted that are not visible" % (total, counted, wrong))
    assert total > 150000 and counted == total and wrong == 0
    for r in range(cs.V):                                        # the count map is the sum of those decisions
        assert np.array_equal(count[:, r], sum(pair[r, s].astype(np.int64) for s in range(cs.V) if s != r))


def test_fused_points_lie_on_their_own_mesh(sc, ch, g):
    points, src, n_per_track = (host_(a) for a in g["fuse"])
    rp, rs, rn = ch["fuse"]
    assert same_bits(points, rp) and same_bits(src, rs) and same_bits(n_per_track, rn)
    o = 0
    for b in range(cs.B):
        p = points[o:o + n_per_track[b]]
        o += n_per_track[b]
        own, other = sc.mesh_distance(b, p), sc.mesh_distance(1 - b, p)
        print("g: track %d: %d fused points at most %.3e from their mesh, at least %.3f from the other track's"
              % (b, len(p), own.max(), other.min()))
        assert own.max() <= cr.FUSE_BOUND[b] and other.min() > cr.FUSE_BOUND[b]


def test_geometric_loss_is_least_at_the_true_depths(g):
    for b in range(cs.B):
        v = [g["geo"][b, k] for k in (1.0, 1.01, 0.99)]
        print("g: geometric loss, track %d: %.4f at the true depths, %.4f at x 1.01, %.4f at x 0.99" % (b, *v))
        assert v[0] < v[1] and v[0] < v[2]


# ---------------------------------------------------------------------------------------------------------------------
# h. the prior chain
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, cs.V - 1])
def test_prior_chain(sc, ch, g, k):
    assert same_bits(host_(g["mdepth"]), ch["mdepth"]) and same_bits(host_(g["keep"]), ch["keep"])
    P, ref = {key: (tuple(host_(a) for a in v) if key == "validity" else host_(v)) for key, v in g["prior"][k].items()}, \
        ch["prior"][k]
    for key in ("z", "prior", "best"):
        assert same_floats(P[key], ref[key]), key
    for key in ("src", "lo", "hi", "idx"):
        assert same_bits(P[key], ref[key]), key
    for a, b in zip(P["validity"], ref["validity"]):
        assert same_floats(a, b)
    cr.assert_prior(cr.prior_figures(sc, ch, k, P), k)
