"""The matching-to-fusion chain against rendered ground truth, on the CPU: tests/chain_ref.py runs the README's chain on
frames rendered by the C oracle, from the project's own restatements; tests/chain_scene.py holds the scene and its
float64 truth.  Every op's restatement is tested against its kernel elsewhere; here the restatements are held against
the geometry they describe, so a convention that a kernel and its restatement share wrongly cannot stay green.  The
negative controls run the same predicates under each wrong convention and must score below half the correct score.

This file establishes every measured figure (printed by the tests, run with -s).  The thresholds live in
tests/chain_ref.py beside the shared predicates: each is the reference's measured value, shares rounded down to three
decimals and the fused points' distance rounded up in its second digit; the tests here also check that a threshold has
not drifted from its measurement.  The GPU file asserts the same thresholds.

Measured (the reference chain; 32781 good pixels of 131072, 8 frames of 64 x 256):
  render   oracle depth against z64 on interior pixels: largest relative difference 2.913e-07; hit masks differ in 0
           pixels; `unsure` at most 0.0107 of the pixels of a view pair (mean 0.0039)
  b        truth share |idx - d64| <= 1 on good: NCC 0.99994 (32779), census_sad 0.99783 (32710), sad 0.99936 (32760);
           good pixels whose float64 top-two NCC gap is below twice the fast bound: N = 1
  c        offset 4, D = 16: share 1.0 (32781); idx_to_depth inside z64 (1 +- 1.5 / d64): 1.0
  d        mean |idx - d64| 0.19387; parabola: mean |disp - d64| 0.072264 (float64 rule 0.072264), signed +0.028928
           (float64 +0.028928); equiangular: 0.043581 (0.043581), signed +0.017263 (+0.017263)
  e        truth share among flags == 7: 0.98421, among in-pattern pixels 0.94749 (hit pixels); flags == 7 on shadow
           0.3595, on good 0.99826; idx_r from the truth alone, at the 658 good pixels across a disparity step: within a
           pixel of d64 read at column w - round(d64) 1.00000, read at the pixel's own column 0.3252 (asserted below
           half); idx_r[w - idx] == idx on good, correct, LR_OK pixels 0.98032 (|difference| <= 1 on all 32724:
           lr_tol = 1 admits a neighbour, so the equality is a share, not an identity)
           census_sad: 0.99066 / 0.93743, shadow 0.5537, good 0.98279; sad: 0.98809 / 0.94313, shadow 0.4215, good 0.99790
  f        lit interior pixels (33094): SGM NCC 1.0 against 0.99994 plain; SGM SAD 0.99997 against 0.99937 plain;
           disparity_filter keeps 0.98552 correct against 0.98421 of flags == 7
  g        204842 truly visible (pixel, view) pairs outside `unsure`: all counted, none counted that is not visible
           (max_px 1, max_rel 0.002); fused points at most 3.791e-04 / 7.039e-04 from their own mesh (tracks 0 / 1; the
           bounds are these, rounded up: 3.8e-04 / 7.1e-04), at least 0.135 / 0.120 from the other track's; float64 geometric loss, tracks 0 / 1: 0.1213 / 0.1681 at the true
           depths, 0.1662 / 0.1737 at x 1.01, 0.1680 / 0.1768 at x 0.99
  h        k = 1 / 3: warped prior inside z64 (1 +- 1.5 / d64) on all 8264 / 7688 finite interior pixels with a visible
           source; band holds round(d64) on good: 1.0 / 1.0; band truth share 1.0 / 1.0 (full search 1.0 / 1.0)
  negative controls (correct score -> wrong convention's score)
           frame and pattern mirrored (b): 0.99994 -> 0.0329
           R transposed (g, share of visible pairs counted): 1.0 -> 0.1811
           t negated (g): 1.0 -> 0.0613
           disp_offset negated (c, depth inside the bound): 1.0 -> 0.0
           views interleaved as v * B + b (g): 1.0 -> 0.0290.  The same mix-up scores 0.5431 on (b): two of the eight
           positions keep their frame and two more only swap views of one static scene, whose disparities differ by
           less than a pixel -- the matching predicate cannot see those, the multi-view one does, so that one is asserted.
"""
import math

import numpy as np
import pytest
import torch

from tests import chain_ref as cr, chain_scene as cs, f64_refs, fusion_ref, workloads

F = np.float32
HW = cs.H * cs.W


@pytest.fixture(scope="module")
def sc():
    return cs.scene()


@pytest.fixture(scope="module")
def ch(oracle):
    return cr.chain()


@pytest.fixture(scope="module")
def masks(sc):
    return {k: sc.stack(k) for k in ("good", "interior", "lit64", "shadow", "hit", "d64", "z64")}


# ---------------------------------------------------------------------------------------------------------------------
# the scene and the renderer
# ---------------------------------------------------------------------------------------------------------------------
def test_truth_masks_and_grey_zone(sc, masks):
    good = masks["good"]
    assert good.reshape(cs.B, -1).sum(1).min() > 3000          # both tracks have pixels to judge
    assert masks["shadow"].sum() > 100 and (~sc.stack("hit")[cs.V:]).sum() > HW     # shadows; track 1 has misses
    worst, total = 0.0, 0.0
    for b in range(cs.B):
        for r in range(cs.V):
            for s in range(cs.V):
                if s != r:
                    u = sc.visibility(b, r, s)[1].mean()
                    worst, total = max(worst, u), total + u
    print("unsure: worst %.4f mean %.4f" % (worst, total / (cs.B * cs.V * (cs.V - 1))))
    assert worst < 0.05


def test_mesh_distance_of_the_truth_points(sc):
    for b in range(cs.B):
        T = sc.truth[b][0]
        d = sc.mesh_distance(b, T["X"][T["hit"]][::7])
        assert d.max() < 1e-12
    v = sc.meshes[0]["verts"].astype(np.float64)
    assert np.allclose(cs.mesh_distance(v[:3].mean(0, keepdims=True) + [[0, 0, 0]], v, sc.meshes[0]["faces"]), 0, atol=1e-12)
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    pts = np.array([[0.2, 0.2, 0.5], [2, 0, 0], [-1, -1, 0], [0.6, 0.6, 0], [0.5, -2, 1]], np.float64)
    ref = [0.5, 1.0, math.sqrt(2), 0.1 * math.sqrt(2), math.sqrt(5)]
    assert np.allclose(cs.mesh_distance(pts, tri, np.array([[0, 1, 2]])), ref, atol=1e-12)


def test_render_against_float64(sc, ch, masks):
    depth = ch["render"]["depth"].reshape(cr.N, cs.H, cs.W)
    hit = depth > 0
    diff = int((hit != masks["hit"]).sum())
    inter = masks["interior"]
    rel = np.abs(depth[inter] / masks["z64"][inter] - 1).max()
    print("render: hit masks differ in %d pixels; depth vs z64 on interior: max rel %.3e" % (diff, rel))
    assert diff <= 0.01 * HW                                    # silhouettes only
    assert rel < 1e-6                                           # a few f32 roundings of an O(1) quantity
    assert (depth[~hit] == -1).all()


def test_plain_renderer_sees_the_same_depth(oracle, sc, ch):
    """oracle.render_mesh (camera rays only) casts the rays of oracle.render_mesh_proj: the same depth, bit for bit"""
    for b in range(cs.B):
        m = sc.meshes[b]
        normals = workloads.render_normals(m, 5 + b)
        for v in (0, cs.V - 1):
            cam = (sc.K, sc.R[b, v], sc.t[b, v], cs.W, cs.H)
            d = oracle.render_mesh(m["verts"], m["colors"], normals, m["faces"], cam, cs.SHADER)[0]
            assert np.array_equal(d, ch["render"]["depth"][b, v])


# ---------------------------------------------------------------------------------------------------------------------
# b. full search, c. offset, and the mirrored control
# ---------------------------------------------------------------------------------------------------------------------
def test_full_search_truth_share(sc, ch):
    c, n, share = cr.truth_share(ch["idx"], sc)
    print("b: NCC truth share %.5f (%d of %d)" % (share, c, n))
    assert share >= cr.SHARE_B["ncc"] and cr.floor3(share) == cr.SHARE_B["ncc"]
    for name in ("census_sad", "sad"):
        c, n, share = cr.truth_share(ch["cost"][name]["idx"], sc)
        print("b: %s truth share %.5f (%d of %d)" % (name, share, c, n))
        assert share >= cr.SHARE_B[name] and cr.floor3(share) == cr.SHARE_B[name]


def test_fast_kernels_may_differ_on_few_good_pixels(sc, ch, masks):
    v64 = f64_refs.xcorrvol(torch.from_numpy(ch["x"]), torch.from_numpy(ch["pl"]), cs.D, cs.BLOCK).numpy()
    best, gap = cr.gap64(v64)
    n = int((masks["good"] & (gap < 2 * cr.FAST_BOUND(best))).sum())
    print("b: good pixels with a float64 top-two gap below twice the fast bound: N = %d" % n)
    assert n <= 10                                              # the allowance stays negligible beside 32781 pixels


def test_mirrored_convention_fails(oracle, sc, ch, masks):
    """pixel w matches pattern column w - d; in the mirror image it would be w + d, which the matcher cannot find"""
    xm = np.ascontiguousarray(ch["x"][..., ::-1])
    pm = np.ascontiguousarray(ch["pl"][..., ::-1])
    idx = cr.ncc_volume(oracle, xm, pm, cs.D).argmax(1)[..., ::-1]
    right, wrong = cr.truth_share(ch["idx"], sc)[2], cr.truth_share(idx, sc)[2]
    print("control mirrored: %.5f -> %.4f" % (right, wrong))
    assert wrong < 0.5 * right


def test_offset(oracle, sc, ch, masks):
    """disparity = idx + disp_offset: the pattern moved 4 columns to the right, D = 16"""
    c, n, share = cr.truth_share(ch["idx4"], sc, offset=cr.OFFSET)
    ok = masks["good"] & (np.abs(ch["idx4"] + cr.OFFSET - masks["d64"]) <= 1)
    inb = cr.depth_in_bound(ch["depth4"], sc, ok)
    neg = oracle.disp_to_depth((ch["idx4"] - cr.OFFSET).astype(F), F(sc.bf))
    wrong = cr.depth_in_bound(neg, sc, ok)
    print("c: offset share %.5f (%d of %d); depth inside the bound %.5f; control offset negated -> %.4f"
          % (share, c, n, inb, wrong))
    assert share >= cr.SHARE_C and inb == 1.0
    assert wrong < 0.5 * inb
    # depth_to_disp gives the index back
    with np.errstate(all="ignore"):
        back = F(sc.bf) / ch["depth4"] - F(cr.OFFSET)
    assert cr.round_trip_ok(back, ch["idx4"])[ok].all()


# ---------------------------------------------------------------------------------------------------------------------
# d. sub-pixel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["parabola", "equiangular"])
def test_subpixel_moves_towards_the_truth(sc, ch, masks, mode):
    disp, refined = ch["subpixel"][mode]
    cr.assert_subpixel(cr.subpixel_figures(sc, ch, masks, disp, refined, mode), mode)


# ---------------------------------------------------------------------------------------------------------------------
# e. validity
# ---------------------------------------------------------------------------------------------------------------------
def test_validity(sc, ch, masks):
    flags, idx_r, _ = ch["validity"]
    fig = cr.validity_figures(sc, masks, ch["idx"], flags, idx_r)
    cr.assert_validity(fig, "NCC")
    cr.assert_idx_r(fig)
    assert cr.floor3(fig["back_equal"]) == cr.SHARE_IDX_R and cr.floor3(fig["step_pattern"]) == cr.SHARE_IDX_R_STEP
    for name in ("census_sad", "sad"):
        c = ch["cost"][name]
        cr.assert_validity(cr.validity_figures(sc, masks, c["idx"], c["validity"][0], c["validity"][1]), name)


# ---------------------------------------------------------------------------------------------------------------------
# f. SGM and the filters
# ---------------------------------------------------------------------------------------------------------------------
def test_sgm_and_filter(sc, ch, masks):
    cr.assert_sgm_and_filter(sc, masks, ch["idx"], ch["sgm"][0], ch["cost"]["sad"]["idx"], ch["sgm_sad"][0],
                          ch["validity"][0], ch["filter"][0], ch["filter"][1])


# ---------------------------------------------------------------------------------------------------------------------
# g. multi-view on the rendered depths, with the pose and frame-order controls
# ---------------------------------------------------------------------------------------------------------------------
def agreement(sc, depth, R, t):
    M = fusion_ref.all_matches(depth, (depth > 0).astype(np.uint8), sc.ray, sc.K, R, t, cs.MAX_PX, cs.MAX_REL)
    return cr.visibility_agreement(sc, lambda b, r, s: M[b, r, s]["consistent"].reshape(cs.H, cs.W))


def test_consistency_counts_exactly_the_visible_views(sc, ch):
    M = ch["matches"]
    counted, total, wrong = cr.visibility_agreement(sc, lambda b, r, s: M[b, r, s]["consistent"].reshape(cs.H, cs.W))
    print("g: %d truly visible pairs outside unsure: %d counted, %d counted that are not visible" % (total, counted, wrong))
    assert total > 150000 and counted == total and wrong == 0
    count = ch["consistency"][0]                                 # the count map is the sum of those decisions
    for b in range(cs.B):
        for r in range(cs.V):
            total_r = sum(M[b, r, s]["consistent"].astype(np.int64) for s in range(cs.V) if s != r)
            assert np.array_equal(count[b, r].reshape(-1), total_r)


def test_pose_and_frame_order_controls(sc, ch):
    depth = ch["render"]["depth"]
    right = agreement(sc, depth, sc.R, sc.t)
    right = right[0] / right[1]
    wrongs = {"R transposed": (depth, np.ascontiguousarray(sc.R.transpose(0, 1, 3, 2)), sc.t),
              "t negated": (depth, sc.R, -sc.t),
              "views interleaved as v * B + b": (cr.interleaved(depth.reshape(cr.N, cs.H, cs.W)).reshape(depth.shape),
                                                 sc.R, sc.t)}
    for name, args in wrongs.items():
        c, n, _ = agreement(sc, *args)
        print("control %s: share of visible pairs counted %.4f -> %.4f" % (name, right, c / n))
        assert c / n < 0.5 * right
    il = cr.truth_share(cr.interleaved(ch["idx"]), sc)[2]
    print("control views interleaved, on the matching predicate (b): %.5f -> %.4f (reported, not asserted)"
          % (cr.truth_share(ch["idx"], sc)[2], il))


def test_fused_points_lie_on_their_own_mesh(sc, ch):
    points, src, n_per_track = ch["fuse"]
    assert int(n_per_track.sum()) == points.shape[0] and (n_per_track > 1000).all()
    o = 0
    for b in range(cs.B):
        p = points[o:o + n_per_track[b]]
        o += n_per_track[b]
        assert ((src[o - n_per_track[b]:o] // (cs.V * HW)) == b).all()
        own, other = sc.mesh_distance(b, p), sc.mesh_distance(1 - b, p)
        print("g: track %d: %d fused points at most %.3e from their mesh, at least %.3f from the other track's"
              % (b, len(p), own.max(), other.min()))
        assert own.max() <= cr.FUSE_BOUND[b] and other.min() > cr.FUSE_BOUND[b]
        assert abs(cr.ceil2(own.max()) - cr.FUSE_BOUND[b]) < 1e-12          # the bound is the measurement, rounded up


def test_geometric_loss_is_least_at_the_true_depths(sc, ch):
    depth = np.maximum(ch["render"]["depth"], 0)
    K, ray = torch.from_numpy(sc.K), torch.from_numpy(sc.ray)
    for b in range(cs.B):
        d0, d1 = (torch.from_numpy(depth[b, v])[None, None] for v in (0, 1))
        R0, t0, R1, t1 = (torch.from_numpy(a)[None] for a in (sc.R[b, 0], sc.t[b, 0], sc.R[b, 1], sc.t[b, 1]))
        v = [float(f64_refs.geometric_loss(d0 * k, d1, K, ray, R0, t0, R1, t1, -1).value) for k in (1.0, 1.01, 0.99)]
        print("g: float64 geometric loss, track %d: %.4f at the true depths, %.4f at x 1.01, %.4f at x 0.99" % (b, *v))
        assert v[0] < v[1] and v[0] < v[2]


# ---------------------------------------------------------------------------------------------------------------------
# h. the prior chain
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, cs.V - 1])
def test_prior_chain(sc, ch, k):
    P = ch["prior"][k]
    cr.assert_prior(cr.prior_figures(sc, ch, k, P), k)
    bv = P["validity"]
    assert np.array_equal(bv[0], P["idx"])                       # the band validity call returns the band match
