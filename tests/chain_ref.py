"""The README's chain (rendered track -> LCN -> match -> sub-pixel / validity -> filter -> depth -> consistency / fusion
-> warp -> band -> band validity) run once on the CPU from the project's restatements and its C oracle, for
tests/test_chain_truth_host.py (which asserts the truth predicates on it and measures every figure) and
tests/test_chain_truth_gpu.py (which holds the HIP outputs against it).  A module, not a test; the scene and the
float64 truth are tests/chain_scene.py's.  The chain never looks at the truth; the predicates at the end do."""
import functools
import math

import numpy as np
import torch

from tests import band_ref, band_validity_ref, chain_scene as cs, dispfilter_ref, f64_refs, fusion_ref, sgm_ref
from tests import validity_ref, warp_ref
from tests.subpixel_ref import fit_reference

F = np.float32
N = cs.B * cs.V
VALIDITY = dict(lr_tol=1, min_gap=0.05)
COST_GAP = {"sad": 0.002, "census_sad": 0.002}          # README: costvol_validity(..., min_gap=0.002)
SGM_P1, SGM_P2 = 0.02, 0.16                              # README's penalties
COSTS = (("census_sad", 3, 0.5), ("sad", 1, 0.5))        # name, the oracle's type number, eps
OFFSET, OFFSET_D = 4, 16
FAST_BOUND = lambda s: 1e-5 * np.abs(s) + 1e-6           # include/ctd_hip.h: |fast - exact| <= 1e-5 |exact| + 1e-6


def render(oracle, sc, nthreads=4):
    """every view of every track through the oracle's projector renderer and synth.finish_render's blend ->
    dict(depth [B,V,H,W], color, ambient3 [B,V,H,W,3], im, ambient [N,H,W], disp0 [N,H,W]) f32"""
    sh = (cs.B, cs.V, cs.H, cs.W)
    depth, color, amb3 = np.zeros(sh, F), np.zeros(sh + (3,), F), np.zeros(sh + (3,), F)
    im, amb = np.zeros((N, cs.H, cs.W), F), np.zeros((N, cs.H, cs.W), F)
    for b in range(cs.B):
        m, blend = sc.meshes[b], sc.poses[b]["blend_im"]
        for v in range(cs.V):
            cam = (sc.K, sc.R[b, v], sc.t[b, v], cs.W, cs.H)
            proj = (sc.K, sc.R[b, v], sc.t_proj[b, v], cs.W, cs.H)
            d, c, n = oracle.render_mesh_proj(m["verts"], m["colors"], m["faces"], cam, proj, cs.SHADER, sc.pattern3,
                                              cs.D_ALPHA, cs.D_BETA, nthreads=nthreads)
            depth[b, v], color[b, v], amb3[b, v] = d, c, n
            imc = ((c[..., 0] + c[..., 1]) + c[..., 2]) / F(3.0)                 # synth.finish_render's order
            a = ((n[..., 0] + n[..., 1]) + n[..., 2]) / F(3.0)
            im[b * cs.V + v] = F(blend) * imc + F(1.0 - blend) * a
            amb[b * cs.V + v] = a
    with np.errstate(divide="ignore"):
        disp0 = F(sc.bf) / depth.reshape(N, cs.H, cs.W)
    return dict(depth=depth, color=color, ambient3=amb3, im=im, ambient=amb, disp0=disp0)


def lcn_pair(oracle, im, pattern):
    """-> frames_lcn [N,1,H,W], pattern_lcn [1,H,W]"""
    return oracle.lcn(im[:, None], cs.LCN_RADIUS, cs.LCN_EPS)[0], oracle.lcn(pattern[None, None], cs.LCN_RADIUS,
                                                                             cs.LCN_EPS)[0][0]


def ncc_volume(oracle, x, pl, D, nthreads=4):
    return np.stack([oracle.xcorrvol(x[n], pl, D, cs.BLOCK, nthreads=nthreads) for n in range(x.shape[0])])


def cost_volume(oracle, x, pl, D, type_no, eps, nthreads=4):
    return np.stack([oracle.costvol(x[n, 0], pl[0], D, cs.BLOCK, type_no, eps, nthreads=nthreads)
                     for n in range(x.shape[0])])


def shifted_pattern(pattern, k=OFFSET):
    """the pattern moved k columns to the right (P'[c] = P[max(c - k, 0)]): pixel w then matches column w - (d - k) of
    P', so the matcher's index is the disparity minus k, disp_offset = +k"""
    return np.ascontiguousarray(pattern[:, np.maximum(np.arange(pattern.shape[1]) - k, 0)])


def gap64(vol64):
    """float64 volume [N,D,H,W] -> (best, best - runner-up over all other disparities)"""
    s = np.sort(vol64, axis=1)
    return s[:, -1], s[:, -1] - s[:, -2]


def subpixel64(x, pl, idx, D, mode):
    """the sub-pixel rule in float64 on f64_refs.xcorrvol scores of the f32 LCN images, at the f32 indices"""
    v = f64_refs.xcorrvol(torch.from_numpy(x), torch.from_numpy(pl), D, cs.BLOCK)
    return v, fit_reference(v, torch.from_numpy(idx), True, mode, dtype=torch.float64)[0].numpy()


def prior_chain(sc, depth, keep, vol, k):
    """The README's prior chain for view k: depth [B,V,H,W] / keep of the views, warped from views 0..k-1 into view k, the
    windowed band, the band match with its validity on vol[k::V], all from the restatements."""
    first_k = np.zeros((cs.B, cs.V), np.uint8)
    first_k[:, :k] = 1
    view_k = np.zeros((cs.B, cs.V), np.uint8)
    view_k[:, k] = 1
    z, src = warp_ref.warp(depth, sc.ray, sc.K, sc.R, sc.t, keep, first_k, view_k, splat=1)
    z, src = z[:, k], src[:, k]
    with np.errstate(all="ignore"):
        live = np.isfinite(z) & (z > 0)
        prior = np.where(live, F(sc.bf) / np.where(live, z, F(1)) - F(0.0), F(np.nan)).astype(F)
    lo, hi = warp_ref.band_window(prior, 1.0, cs.D, window=3, holes="full")
    volk = np.ascontiguousarray(vol[k::cs.V])
    bidx, bbest = band_ref.band_ref(torch.from_numpy(volk), torch.from_numpy(lo), torch.from_numpy(hi), True)
    bv = band_validity_ref.band_validity_ref(volk, lo, hi, True, **VALIDITY)
    return dict(z=z, src=src, prior=prior, lo=lo, hi=hi, idx=bidx.numpy(), best=bbest.numpy(), validity=bv)


def run(oracle, sc, nthreads=4):
    """the whole chain -> dict"""
    out = {"render": render(oracle, sc, nthreads)}
    im = out["render"]["im"]
    x, pl = lcn_pair(oracle, im, sc.pattern)
    out["x"], out["pl"] = x, pl
    # b. full search
    vol = ncc_volume(oracle, x, pl, cs.D, nthreads)
    idx = np.stack([oracle.argmax(v)[0] for v in vol])
    out["vol"], out["idx"] = vol, idx
    out["cost"] = {}
    for name, no, eps in COSTS:
        cv = cost_volume(oracle, x, pl, cs.D, no, eps, nthreads)
        out["cost"][name] = dict(vol=cv, idx=cv.argmin(1).astype(np.int64))
    # c. offset
    pl4 = oracle.lcn(shifted_pattern(sc.pattern)[None, None], cs.LCN_RADIUS, cs.LCN_EPS)[0][0]
    vol4 = ncc_volume(oracle, x, pl4, OFFSET_D, nthreads)
    out["pl4"], out["vol4"], out["idx4"] = pl4, vol4, vol4.argmax(1).astype(np.int64)
    out["depth4"] = oracle.disp_to_depth((out["idx4"] + OFFSET).astype(F), F(sc.bf))
    # d. sub-pixel
    out["subpixel"] = {m: tuple(a.numpy() for a in fit_reference(torch.from_numpy(vol), torch.from_numpy(idx), True, m))
                       for m in ("parabola", "equiangular")}
    # e. validity
    out["validity"] = validity_ref.validity_ref(vol, idx, True, **VALIDITY)
    for name, _, _ in COSTS:
        c = out["cost"][name]
        c["validity"] = validity_ref.validity_ref(c["vol"], c["idx"], False, lr_tol=1, min_gap=COST_GAP[name])
    # f. SGM and the filters
    out["sgm"] = sgm_ref.sgm_ref(vol, SGM_P1, SGM_P2, 8, True)[1:]
    out["sgm_sad"] = sgm_ref.sgm_ref(out["cost"]["sad"]["vol"], SGM_P1, SGM_P2, 8, False)[1:]
    flags = out["validity"][0]
    out["filter"] = dispfilter_ref.disparity_filter(idx.astype(F), (flags == 7).astype(np.uint8))
    # g. multi-view on the rendered depths
    depth = out["render"]["depth"]
    hit = (depth > 0).astype(np.uint8)
    matches = fusion_ref.all_matches(depth, hit, sc.ray, sc.K, sc.R, sc.t, cs.MAX_PX, cs.MAX_REL)
    out["matches"] = matches
    out["consistency"] = fusion_ref.consistency(depth, sc.ray, sc.K, sc.R, sc.t, hit, cs.MAX_PX, cs.MAX_REL, 1, matches)
    out["fuse"] = fusion_ref.fuse_points(depth, sc.ray, sc.K, sc.R, sc.t, hit, cs.MAX_PX, cs.MAX_REL, 1, True, matches)[:3]
    # h. the prior chain from the matcher's own depths
    disp = out["subpixel"]["parabola"][0]
    mdepth = oracle.disp_to_depth(np.nan_to_num(disp), F(sc.bf)).reshape(cs.B, cs.V, cs.H, cs.W)
    keep = out["filter"][1].reshape(cs.B, cs.V, cs.H, cs.W)
    out["mdepth"], out["keep"] = mdepth, keep
    out["prior"] = {k: prior_chain(sc, mdepth, keep, vol, k) for k in (1, cs.V - 1)}
    return out


@functools.lru_cache(maxsize=1)
def chain():
    """the CPU chain of the shared scene, computed once per session (read only)"""
    from oracle import oracle
    oracle.lib()
    return run(oracle, cs.scene())


# ---------------------------------------------------------------------------------------------------------------------
# the truth predicates, shared by the host and the GPU file: each takes outputs of the chain (numpy) and the scene
# ---------------------------------------------------------------------------------------------------------------------
def truth_share(idx, sc, mask=None, offset=0):
    """(correct count, count, share) of |idx + offset - d64| <= 1 over `mask` (default: good), frames in b * V + v order"""
    mask = sc.stack("good") if mask is None else mask
    ok = np.abs(np.asarray(idx, np.float64) + offset - sc.stack("d64")) <= 1
    n = int(mask.sum())
    c = int((ok & mask).sum())
    return c, n, c / max(n, 1)


def depth_in_bound(depth, sc, mask):
    """share of `mask` with depth inside z64 * (1 +- 1.5 / d64)"""
    z, d = sc.stack("z64"), sc.stack("d64")
    with np.errstate(all="ignore"):
        ok = np.abs(np.asarray(depth, np.float64) - z) <= z * 1.5 / d
    return float((ok & mask).sum() / max(int(mask.sum()), 1))


def visibility_agreement(sc, consistent_of):
    """consistent_of(b, r, s) -> bool [H,W].  -> (visible pairs counted, visible pairs, pairs counted without being
    visible), all outside `unsure` and over the hit pixels of r"""
    counted = total = wrong = 0
    for b in range(cs.B):
        for r in range(cs.V):
            for s in range(cs.V):
                if s == r:
                    continue
                vis, uns = sc.visibility(b, r, s)
                sure = sc.truth[b][r]["hit"] & ~uns
                c = consistent_of(b, r, s)
                counted += int((vis & sure & c).sum())
                total += int((vis & sure).sum())
                wrong += int((~vis & sure & c).sum())
    return counted, total, wrong


def interleaved(a):
    """frames [N,...] in b * V + v order -> what a caller who stacked them as v * B + b would read at (b, v)"""
    return a[[(n % cs.B) * cs.V + n // cs.B for n in range(N)]]


def round_trip_ok(back, idx, offset=OFFSET):
    """depth_to_disp(idx_to_depth(idx)) against idx: two f32 divisions of a value near idx + offset, each within half
    an ulp of it, and an exact subtraction -> within 2 ulp of idx + offset"""
    ulp = np.spacing((np.asarray(idx) + offset).astype(F)).astype(np.float64)
    return np.abs(np.asarray(back, np.float64) - idx) <= 2 * ulp


# ---------------------------------------------------------------------------------------------------------------------
# thresholds and figure helpers of the two test files.  A threshold is the reference chain's measured figure
# (tests/test_chain_truth_host.py establishes it and checks it has not drifted): shares that must not fall are rounded
# down to three decimals (`floor3`), the fused points' distance is rounded up in its second significant digit (`ceil2`)
# ---------------------------------------------------------------------------------------------------------------------
HW = cs.H * cs.W
SHARE_B = {"ncc": 0.999, "census_sad": 0.997, "sad": 0.999}
SHARE_C = 1.0
SHARE_IDX_R = 0.980                     # idx_r[w - idx] == idx on good, correct, LR_OK pixels
SHARE_IDX_R_STEP = 1.0                  # |idx_r[w - round(d64)] - d64| <= 1 on good pixels at a disparity step
BAND_HOLDS = {1: 1.0, cs.V - 1: 1.0}
FUSE_BOUND = (3.8e-4, 7.1e-4)           # per track: the reference's fused points' largest distance to their mesh


def ceil2(x):
    """x rounded up in its second significant digit"""
    e = 10.0 ** (math.floor(math.log10(x)) - 1)
    return math.ceil(x / e - 1e-9) * e


def floor3(x):
    return math.floor(x * 1000) / 1000


def subpixel_figures(sc, ch, masks, disp, refined, mode):
    sel = masks["good"] & (np.abs(ch["idx"] - masks["d64"]) <= 1) & (refined != 0)
    _, d64sp = subpixel64(ch["x"], ch["pl"], ch["idx"], cs.D, mode)
    e, e64, ei = (a[sel] - masks["d64"][sel] for a in (disp.astype(np.float64), d64sp, ch["idx"].astype(np.float64)))
    return dict(n=int(sel.sum()), idx=np.abs(ei).mean(), mean=np.abs(e).mean(), mean64=np.abs(e64).mean(),
                signed=e.mean(), signed64=e64.mean())


def assert_subpixel(fig, mode):
    print("d: %s on %d pixels: mean |idx - d64| %.5f, mean |disp - d64| %.6f (float64 rule %.6f), signed %+.6f (%+.6f)"
          % (mode, fig["n"], fig["idx"], fig["mean"], fig["mean64"], fig["signed"], fig["signed64"]))
    assert fig["n"] > 30000
    assert fig["mean"] < fig["idx"]                              # refinement moves towards the truth
    assert fig["mean"] <= 1.1 * fig["mean64"]
    assert abs(fig["signed"] - fig["signed64"]) <= 0.01


def idx_r_at_steps(sc, masks, idx_r):
    """idx_r against the truth alone, where the two readings of its index differ.  Pattern column c is lit through one
    ray, seen by one pixel: for a good pixel w that is c = w - round(d64[w]), so idx_r[c] must be d64[w] to within a
    pixel.  Read at the pixel's own column instead, idx_r[w] is the disparity of the pixel that sees column w, near
    w + round(d64[w]); the pixels judged are the good ones where that pixel is missed or lies at least 2 disparities
    away from d64[w] -- across a disparity step.  -> (pixels, share by pattern column, share by the pixel's column)"""
    d64, good, hit = masks["d64"], masks["good"], masks["hit"]
    cols = np.broadcast_to(np.arange(cs.W)[None, None, :], d64.shape)
    rd = np.round(d64).astype(np.int64)
    p = cols + rd
    pc = np.clip(p, 0, cs.W - 1)
    step = good & (p < cs.W) & (~np.take_along_axis(hit, pc, 2) | (np.abs(np.take_along_axis(d64, pc, 2) - d64) >= 2))
    by_pattern = np.abs(np.take_along_axis(idx_r, np.clip(cols - rd, 0, cs.W - 1), 2) - d64) <= 1
    by_pixel = np.abs(idx_r - d64) <= 1
    return int(step.sum()), by_pattern[step].mean(), by_pixel[step].mean()


def validity_figures(sc, masks, idx, flags, idx_r):
    ok = np.abs(idx - masks["d64"]) <= 1
    hit, f7, inpat = masks["hit"], flags == 7, (flags & 1) != 0
    cols = np.arange(cs.W)[None, None, :]
    sel = masks["good"] & ok & ((flags & 2) != 0)
    back = np.take_along_axis(idx_r, np.clip(cols - idx, 0, cs.W - 1), 2)
    n_step, step_pattern, step_pixel = idx_r_at_steps(sc, masks, idx_r)
    return dict(share7=ok[f7 & hit].mean(), share_in=ok[inpat & hit].mean(), shadow7=f7[masks["shadow"]].mean(),
                good7=f7[masks["good"]].mean(), n_lr=int(sel.sum()), back_equal=(back == idx)[sel].mean(),
                back_max=int(np.abs(back - idx)[sel].max()), n_step=n_step, step_pattern=step_pattern,
                step_pixel=step_pixel)


def assert_idx_r(fig):
    """idx_r is indexed by pattern column: on the truth alone at disparity steps, and against the pixel side's idx"""
    print("e: idx_r at %d good pixels across a disparity step: within a pixel of d64 read at column w - round(d64) %.5f, "
          "read at the pixel's own column %.4f" % (fig["n_step"], fig["step_pattern"], fig["step_pixel"]))
    print("e: idx_r[w - idx] == idx on %d good, correct, LR_OK pixels: %.5f (max |difference| %d)"
          % (fig["n_lr"], fig["back_equal"], fig["back_max"]))
    assert fig["n_step"] > 500
    assert fig["step_pattern"] >= SHARE_IDX_R_STEP
    assert fig["step_pixel"] < 0.5 * fig["step_pattern"]
    assert fig["back_max"] <= VALIDITY["lr_tol"] and fig["back_equal"] >= SHARE_IDX_R


def assert_validity(fig, what):
    print("e: %s: truth share among flags == 7 %.5f, among in-pattern %.5f; flags == 7 on shadow %.4f, on good %.5f"
          % (what, fig["share7"], fig["share_in"], fig["shadow7"], fig["good7"]))
    assert fig["share7"] >= fig["share_in"]
    assert fig["shadow7"] < fig["good7"]


def assert_sgm_and_filter(sc, masks, idx, sgm_idx, sad_idx, sgm_sad_idx, flags, fdisp, fkeep):
    lit = masks["interior"] & masks["lit64"]
    a, b = truth_share(sgm_idx, sc, lit)[2], truth_share(idx, sc, lit)[2]
    c, d = truth_share(sgm_sad_idx, sc, lit)[2], truth_share(sad_idx, sc, lit)[2]
    print("f: lit interior pixels (%d): SGM NCC %.5f against %.5f plain; SGM SAD %.5f against %.5f plain"
          % (lit.sum(), a, b, c, d))
    assert a >= b and c >= d
    ok = np.abs(idx - masks["d64"]) <= 1
    okf = np.abs(np.nan_to_num(fdisp).astype(np.float64) - masks["d64"]) <= 1
    kept, f7 = okf[(fkeep != 0) & masks["hit"]].mean(), ok[(flags == 7) & masks["hit"]].mean()
    print("f: disparity_filter keeps %.5f correct against %.5f of flags == 7" % (kept, f7))
    assert kept >= f7


def prior_figures(sc, ch, k, P):
    Tk = [sc.truth[b][k] for b in range(cs.B)]
    inter, z64, d64, good = (np.stack([T[key] for T in Tk]) for key in ("interior", "z64", "d64", "good"))
    z, src = P["z"], P["src"]
    srcvis = np.zeros(z.shape, bool)
    for b in range(cs.B):
        sv, q = np.divmod(src[b] - b * cs.V * HW, HW)
        for s in range(k):
            vis = sc.visibility(b, s, k)[0].reshape(-1)
            m = (src[b] >= 0) & (sv == s)
            srcvis[b][m] = vis[q[m]]
    sel = np.isfinite(z) & inter & srcvis
    with np.errstate(all="ignore"):
        inb = np.abs(z.astype(np.float64) - z64) <= z64 * 1.5 / d64
    rd = np.round(d64)
    full = ch["idx"][k::cs.V]
    inside = (full >= P["lo"]) & (full <= P["hi"])
    return dict(n=int(sel.sum()), violations=int((sel & ~inb).sum()),
                holds=((rd >= P["lo"]) & (rd <= P["hi"]))[good].mean(),
                equal_inside=bool((P["idx"] == full)[inside].all()), inside=inside.mean(),
                band=(np.abs(P["idx"] - d64) <= 1)[good].mean(), full=(np.abs(full - d64) <= 1)[good].mean())


def assert_prior(fig, k):
    print("h: k = %d: warped prior inside z64 (1 +- 1.5 / d64) on %d finite interior pixels with a visible source "
          "(%d outside); band holds round(d64) on good %.5f; full index inside the band on %.4f of the pixels; band "
          "truth share %.5f (full search %.5f)" % (k, fig["n"], fig["violations"], fig["holds"], fig["inside"],
                                                  fig["band"], fig["full"]))
    assert fig["n"] > 5000 and fig["violations"] == 0
    assert fig["holds"] >= BAND_HOLDS[k]
    assert fig["equal_inside"]
    assert fig["band"] >= fig["full"]
