"""The README's chain (rendered track -> LCN -> match -> sub-pixel / validity -> filter -> depth -> consistency / fusion
-> warp -> band -> band validity) run once on the CPU from the project's restatements and its C oracle, for
tests/test_chain_truth_host.py (which asserts the truth predicates on it and measures every figure) and
tests/test_chain_truth_gpu.py (which holds the HIP outputs against it).  A module, not a test; the scene and the
float64 truth are tests/chain_scene.py's.  The chain never looks at the truth; the predicates at the end do.

The second part of the module does the same for the second half of the README's chain (normals, ICP, TSDF, mesh, clean /
smooth / simplify, evaluation, colours; stages i .. p): `recon()` and `recon_matcher()` for
tests/test_chain_recon_host.py and tests/test_chain_recon_gpu.py, their predicates, and the thresholds in `RECON`."""
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


# =====================================================================================================================
# The second half of the README's chain (depth maps -> normals / ICP -> TSDF -> surface points / ray cast -> mesh ->
# clean -> smooth -> simplify -> evaluation -> colours), run once on the CPU from the restatements for
# tests/test_chain_recon_host.py and tests/test_chain_recon_gpu.py.  Stages continue at i.  A mesh is a dict of per-track
# lists here (`verts` f32 [n,3], `faces` int32 [k,3], `normals` f32 [n,3]), whichever side it comes from.
# =====================================================================================================================
VOXEL = 0.025
RECON_MAX_REL = 0.01                                     # README: depth_consistency(..., max_rel=0.01) -> keep
MIN_FACES = 32                                           # README: clean_tsdf_mesh(m, min_faces=32)
SMOOTH = dict(iters=10, lam=0.5, mu=-0.53)               # README: 10 x Taubin 0.5 | -0.53
D_MIN, N_STEPS = 0.5, 112                                # the ray cast starts in front of every surface (nearest 0.81) and
                                                         # ends at 0.5 + 111 * 1.5 voxel = 4.66, behind the farthest (4.5)
ICP_SEED, ICP_SPEC, ICP_MAX_REL = 7, (0.3, 0.005), 0.05  # views 1..V-1 perturbed by 0.3 degrees and 5 mm
VOXELS_P = (0.025, 0.05, 0.1)


def cell_of(voxel):
    return 2 * voxel                                     # README: simplify_tsdf_mesh(m, cell=2 * voxel)


def margin_of(voxel):
    return 2 * voxel                                     # README: color_tsdf_mesh(..., margin=2 * voxel)


def step_of(voxel):
    return 1.5 * voxel                                   # README: tsdf_raycast(..., step=1.5 * voxel)


def extra_pose(sc):
    """a pose that is no view: the mean camera position of each track with the rotation of view 0 -> R [B,1,3,3], t [B,1,3]
    f32"""
    R64, t64 = sc.R.astype(np.float64), sc.t.astype(np.float64)
    centre = -np.einsum("bvji,bvj->bvi", R64, t64).mean(1)                       # C = -R^T t
    t_new = -np.einsum("bij,bj->bi", R64[:, 0], centre)
    return np.ascontiguousarray(sc.R[:, :1]), np.ascontiguousarray(t_new[:, None].astype(F))


@functools.lru_cache(maxsize=1)
def cast_poses():
    """the poses of stage l: the V views and `extra_pose` -> R [B,V+1,3,3], t [B,V+1,3] f32, and the float64 truth of the
    extra pose per track (chain_scene.cast, with `interior`)"""
    sc = cs.scene()
    Rx, tx = extra_pose(sc)
    truth = []
    for b in range(cs.B):
        T = cs.cast(sc.meshes[b], sc.K, Rx[b, 0], tx[b, 0], tx[b, 0] + np.array([-cs.BASELINE, 0, 0], F))
        T["interior"] = cs.interior_mask(T["face"])
        truth.append(T)
    return np.concatenate([sc.R, Rx], 1), np.concatenate([sc.t, tx], 1), truth


def as_mesh(verts, faces, n_verts, n_faces, normals=None):
    """flat arrays with per-track counts -> the per-track lists"""
    vo, fo = np.concatenate([[0], np.cumsum(n_verts)]), np.concatenate([[0], np.cumsum(n_faces)])
    B = len(n_verts)
    return dict(verts=[verts[vo[b]:vo[b + 1]] for b in range(B)], faces=[faces[fo[b]:fo[b + 1]] for b in range(B)],
                normals=[None if normals is None else normals[vo[b]:vo[b + 1]] for b in range(B)])


def model_of(sc, depth, valid, R, t, voxel):
    """integrate + surface points + faces from the restatements -> dict(tsdf, weight, origin, dims, mesh, src)"""
    from tests import tsdf_ref
    origin, dims = cs.recon_grid(voxel)
    T, w = tsdf_ref.volume(cs.B, *dims)
    T, w = tsdf_ref.integrate(T, w, origin, voxel, depth, sc.ray, sc.K, R, t, valid)
    return dict(tsdf=T, weight=w, origin=origin, dims=dims, **mesh_of(T, w, origin, voxel))


def mesh_of(T, w, origin, voxel):
    from tests import mesh_ref, tsdf_ref
    points, normals, src, n = tsdf_ref.surface_points(T, w, origin, voxel)
    faces, nf = mesh_ref.faces(T, w)
    return dict(mesh=as_mesh(points, faces, n, nf, normals), src=src)


def clean_of(m, min_faces=MIN_FACES):
    """meshops.clean_tsdf_mesh from meshclean_ref (drop_degenerate, the wrapper's default)"""
    from tests import meshclean_ref
    out = dict(verts=[], faces=[], normals=[], counts=[])
    for v, f, n in zip(m["verts"], m["faces"], m["normals"]):
        c = meshclean_ref.clean(f, len(v), v, min_faces=min_faces, drop_degenerate=True)
        out["verts"].append(v[c["vert_index"]])
        out["normals"].append(None if n is None else n[c["vert_index"]])
        out["faces"].append(c["faces"])
        out["counts"].append(c["counts"])
    return out


def smooth_of(m, iters=SMOOTH["iters"]):
    """meshsmooth.smooth_tsdf_mesh from meshsmooth_ref, normals recomputed; also the adjacency counts per track"""
    from tests import meshsmooth_ref as msr
    out = dict(verts=[], faces=m["faces"], normals=[], adj=[])
    for v, f in zip(m["verts"], m["faces"]):
        adj = msr.adjacency(f, len(v))
        x = msr.smooth(v, adj["offsets"], adj["neighbors"], adj["vflags"], iters, SMOOTH["lam"], SMOOTH["mu"], True)
        out["verts"].append(x)
        out["normals"].append(msr.vertex_normals(x, f, adj["face_offsets"], adj["face_ids"]))
        out["adj"].append(topology_of(adj))
    return out


def topology_of(adj):
    from tests import meshsmooth_ref as msr
    n_ref, euler, closed = msr.topology(adj)
    c = adj["counts"]
    return dict(edges=int(c[1]), boundary=int(c[2]), nonmanifold=int(c[3]), valid=int(c[5]), referenced=n_ref, euler=euler,
                closed=closed)


def grid_origin_of(verts):
    """meshsimplify._grid_origin: the per-axis minimum of the finite coordinates"""
    return np.where(np.isfinite(verts), verts, F(np.inf)).min(0).astype(F)


def simplify_of(m, cell):
    """meshsimplify.simplify_tsdf_mesh from meshsimplify_ref (origin None: every track its own)"""
    from tests import meshsimplify_ref, meshsmooth_ref as msr
    out = dict(verts=[], faces=[], normals=[], adj=[])
    for v, f in zip(m["verts"], m["faces"]):
        s = meshsimplify_ref.simplify_mesh(v, f, grid_origin_of(v), float(F(cell)))
        adj = msr.adjacency(s["faces"], len(s["verts"]))
        out["verts"].append(s["verts"])
        out["faces"].append(s["faces"])
        out["normals"].append(msr.vertex_normals(s["verts"], s["faces"], adj["face_offsets"], adj["face_ids"]))
        out["adj"].append(topology_of(adj))
    return out


def colors_of(sc, m, images, valid, R, t, margin):
    """meshcolor.color_tsdf_mesh(..., return_flags=True) from viewcolor_ref -> per-track lists of color, weight, n_views, flags"""
    from tests import viewcolor_ref
    out = dict(color=[], weight=[], n_views=[], flags=[])
    for b, (v, f, n) in enumerate(zip(m["verts"], m["faces"], m["normals"])):
        got = viewcolor_ref.view_colors(v, images[b], sc.K, R[b], t[b], margin, v, f, normals=n, valid=valid[b])
        for key, a in zip(("color", "weight", "n_views", "flags"), got):
            out[key].append(a)
    return out


def moved_truth_points(sc, b, voxel, stride=4):
    """the truth points of every `stride`-th interior pixel of view 0 of track b, moved 2 voxels towards the camera and 2
    voxels away from it along their rays -> (towards, away) f32 [n,3]"""
    T = sc.truth[b][0]
    X = T["X"][T["interior"]][::stride]
    C = -np.asarray(sc.R[b, 0], np.float64).T @ np.asarray(sc.t[b, 0], np.float64)
    u = (X - C) / np.linalg.norm(X - C, axis=1, keepdims=True)
    return (X - 2 * voxel * u).astype(F), (X + 2 * voxel * u).astype(F)


def truth_volume_of(sc, b, origin_b, voxel, dims):
    """meshsdf.mesh_to_tsdf of track b's TRUE mesh from meshsdf_ref -> (tsdf, weight) f32 [1,nz,ny,nx], and per voxel d2,
    sign and `clear` (the pseudonormal's dot stands clear of rounding, tests/meshsdf_ref.py).  Only the centres
    that lie within 1.01 trunc of some face's plane and of that face's bounding box go through the f32 rule: each of the
    two is a lower bound of the distance to the face, so the others cannot qualify (the f32 distance of pointmesh_ref is
    within 1e-5 relative of the exact one at these sizes)."""
    from tests import meshsdf_ref, tsdf_ref
    nx, ny, nz = dims
    m = sc.meshes[b]
    trunc = F(4 * voxel)                                                          # the f32 of the Python number, as the layer
    X = np.stack(tsdf_ref.centres(origin_b, voxel, nx, ny, nz), 1)
    tri = m["verts"].astype(np.float64)[m["faces"]]                               # [k,3,3]
    nrm = cs.face_normals(m)
    near = np.zeros(len(X), bool)
    for k in range(len(tri)):
        box = np.maximum(np.maximum(tri[k].min(0) - X, X - tri[k].max(0)), 0)
        near |= (np.abs((X - tri[k, 0]) @ nrm[k]) <= 1.01 * float(trunc)) & ((box * box).sum(1) <= (1.01 * float(trunc)) ** 2)
    near = np.nonzero(near)[0]
    s = meshsdf_ref.signed(X[near], m["verts"], m["faces"], max_d2=trunc * trunc)
    hit = s["face"] >= 0
    dist = np.sqrt(s["d2"])
    with np.errstate(all="ignore"):
        value = np.minimum(F(1), np.where(s["sign"] < 0, -dist, dist) / trunc).astype(F)
    T, w = np.zeros(nx * ny * nz, F), np.zeros(nx * ny * nz, F)
    T[near], w[near] = np.where(hit, value, F(0)), hit.astype(F)
    d2, sign, clear = np.full(nx * ny * nz, np.inf, F), np.zeros(nx * ny * nz, np.int8), np.ones(nx * ny * nz, bool)
    d2[near], sign[near], clear[near] = s["d2"], s["sign"], np.abs(s["dot"]) > 1e-9 * s["S"]
    return T.reshape(1, nz, ny, nx), w.reshape(1, nz, ny, nx), dict(d2=d2, sign=sign, clear=clear)


def run_recon(sc, ch):
    """stages i .. o on ch["render"]["depth"] -> dict"""
    from tests import fusion_ref, icp_ref, meshsdf_ref, pointmesh_ref, tsdf_ref
    depth = ch["render"]["depth"]
    hit = (depth > 0).astype(np.uint8)
    voxel = VOXEL
    out = {}
    # i. normals
    out["normal"] = icp_ref.normals(depth, sc.ray, hit)
    # j. ICP from perturbed poses
    spec = {v: ICP_SPEC for v in range(1, cs.V)}
    R0, t0 = icp_ref.perturb_poses(sc.R, sc.t, np.random.RandomState(ICP_SEED), spec)
    Ri, ti, info = icp_ref.depth_icp(depth, sc.ray, sc.K, R0, t0, hit, iters=10, max_rel=ICP_MAX_REL)
    out["icp"] = dict(R0=R0, t0=t0, R=Ri, t=ti, ok=info["ok"], rmse=info["rmse"], count=info["count"],
                      pivot_ratio=info["pivot_ratio"])
    # k. integrate + surface points + mesh at the true poses, valid = keep
    keep = fusion_ref.consistency(depth, sc.ray, sc.K, sc.R, sc.t, hit, cs.MAX_PX, RECON_MAX_REL, 1)[1]
    out["keep"] = keep
    model = model_of(sc, depth, keep, sc.R, sc.t, voxel)
    out["model"] = model
    # l. ray cast at the views and at the extra pose
    Rc, tc, _ = cast_poses()
    cast = lambda T, w, origin: tsdf_ref.raycast(T, w, origin, voxel, sc.ray, Rc, tc, cs.H, cs.W, D_MIN, step_of(voxel), N_STEPS)
    out["raycast"] = cast(model["tsdf"], model["weight"], model["origin"])
    # m. clean -> smooth -> simplify
    out["clean"] = clean_of(model["mesh"])
    out["smooth"] = smooth_of(out["clean"])
    out["simplify"] = simplify_of(out["smooth"], cell_of(voxel))
    # n. evaluation: the cleaned model's vertices against the true mesh; signed distances against the cleaned model
    ev = dict(d2=[], face=[], signed=[])
    for b in range(cs.B):
        m = sc.meshes[b]
        d2, face, _ = pointmesh_ref.nearest(out["clean"]["verts"][b], m["verts"], m["faces"])
        ev["d2"].append(d2)
        ev["face"].append(face)
        ev["signed"].append([meshsdf_ref.signed(p, out["clean"]["verts"][b], out["clean"]["faces"][b])
                             for p in moved_truth_points(sc, b, voxel)])
    out["eval"] = ev
    tv = [truth_volume_of(sc, b, model["origin"][b], voxel, model["dims"]) for b in range(cs.B)]
    out["truth_volume"] = tuple(np.concatenate([x[k] for x in tv]) for k in (0, 1))
    out["truth_parts"] = {k: np.stack([x[2][k] for x in tv]) for k in ("d2", "sign", "clear")}
    out["truth_raycast"] = cast(*out["truth_volume"], model["origin"])
    # o. colours: the cleaned model with normals recomputed from its faces (smooth_tsdf_mesh with iters = 0)
    out["images"] = np.stack([cs.field_images(b) for b in range(cs.B)])
    out["hit"] = sc.stack("hit").reshape(cs.B, cs.V, cs.H, cs.W).astype(np.uint8)
    out["colored"] = smooth_of(out["clean"], iters=0)
    out["colors"] = colors_of(sc, out["colored"], out["images"], out["hit"], sc.R, sc.t, margin_of(voxel))
    return out


@functools.lru_cache(maxsize=1)
def recon():
    """the CPU second half on the shared scene and chain, computed once per session (read only)"""
    return run_recon(cs.scene(), chain())


# ---------------------------------------------------------------------------------------------------------------------
# the truth predicates of stages i .. p: each takes outputs of either side (numpy) and the scene, and returns figures
# ---------------------------------------------------------------------------------------------------------------------
def normals_figures(sc, normal):
    """i: depth_normals [B,V,H,W,3] against the truth normals on interior pixels; every normal there is must face its camera
    (normal . ray < 0: the point is depth * ray)"""
    ang, n_int, n_fin, facing = [], 0, 0, True
    ray = sc.ray.astype(np.float64).reshape(cs.H, cs.W, 3)
    for b in range(cs.B):
        for v in range(cs.V):
            n = normal[b, v].astype(np.float64)
            fin = np.isfinite(n).all(-1)
            facing &= bool(((n * ray).sum(-1)[fin] < 0).all())
            m = sc.truth[b][v]["interior"]
            n_int, n_fin = n_int + int(m.sum()), n_fin + int((m & fin).sum())
            cos = (n * cs.truth_normals(sc, b, v)).sum(-1)[m & fin]
            ang.append(np.degrees(np.arccos(np.clip(cos, -1, 1))))
    ang = np.concatenate(ang)
    return dict(n=n_int, share=n_fin / n_int, median=float(np.median(ang)), max=float(ang.max()), facing=facing)


def view_points64(sc, b, v, R, t, stride=4):
    """every `stride`-th interior pixel of view v of track b, back-projected at its true depth with the pose (R, t) -> [n,3]"""
    T = sc.truth[b][v]
    K = sc.K.astype(np.float64)
    ys, xs = np.nonzero(T["interior"])
    ys, xs = ys[::stride], xs[::stride]
    cam = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones(len(xs))], 1) * T["z64"][ys, xs][:, None]
    return (cam - np.asarray(t, np.float64)) @ np.asarray(R, np.float64)


def icp_figures(sc, icp):
    """j: per perturbed view the median distance to the true mesh of its interior points under the perturbed and under the
    refined pose -> list of dict(b, v, ok, before, after, ratio)"""
    out = []
    for b in range(cs.B):
        for v in range(1, cs.V):
            d0 = np.median(sc.mesh_distance(b, view_points64(sc, b, v, icp["R0"][b, v], icp["t0"][b, v])))
            with np.errstate(all="ignore"):
                d1 = np.median(sc.mesh_distance(b, view_points64(sc, b, v, icp["R"][b, v], icp["t"][b, v])))
            out.append(dict(b=b, v=v, ok=int(icp["ok"][b, v]), before=float(d0), after=float(d1), ratio=float(d1 / d0)))
    return out


def vertex_figures(sc, verts, voxel):
    """per track dict(n, median, p99, max, beyond): the vertices' float64 distance to the true mesh; beyond = the share
    farther than a voxel.  No vertices: every distance is inf (a control may leave none)."""
    out = []
    for b in range(cs.B):
        if len(verts[b]) == 0:
            out.append(dict(n=0, median=np.inf, p99=np.inf, max=np.inf, beyond=1.0))
            continue
        d = sc.mesh_distance(b, verts[b])
        out.append(dict(n=len(d), median=float(np.median(d)), p99=float(np.percentile(d, 99)), max=float(d.max()),
                        beyond=float((d > voxel).mean())))
    return out


def completeness(sc, m, stride=4):
    """per track the largest float64 distance from the truth points of every `stride`-th interior pixel (all views) to the
    model's triangles (chain_scene.mesh_distance_near: an upper bound, over the 24 faces with the nearest centroids)"""
    out = []
    for b in range(cs.B):
        if len(m["faces"][b]) == 0:
            out.append(np.inf)
            continue
        X = np.concatenate([view_points64(sc, b, v, sc.R[b, v], sc.t[b, v], stride) for v in range(cs.V)])
        out.append(float(cs.mesh_distance_near(X, m["verts"][b], m["faces"][b]).max()))
    return out


def face_geometry(verts, faces):
    """-> centroids [k,3], unnormalised normals (v1 - v0) x (v2 - v0) [k,3], float64"""
    p = verts.astype(np.float64)[faces]
    return p.mean(1), np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


def winding_share(sc, m, margin):
    """the share of (face, view) pairs, the view truly seeing the face's centroid (chain_scene.occluded64: visible), whose
    face normal (v1 - v0) x (v2 - v0) points to the side of the camera's centre -> per track (share, pairs)"""
    out = []
    for b in range(cs.B):
        c, n = face_geometry(m["verts"][b], m["faces"][b])
        agree = pairs = 0
        for s in range(cs.V):
            C = -np.asarray(sc.R[b, s], np.float64).T @ np.asarray(sc.t[b, s], np.float64)
            vis = cs.occluded64(b, s, c, margin)[1] if len(c) else np.zeros(0, bool)
            agree += int(((n * (C - c)).sum(1) > 0)[vis].sum())
            pairs += int(vis.sum())
        out.append((agree / max(pairs, 1), pairs))
    return out


def gradient_normal_agreement(m):
    """the TSDF-gradient normals of the vertices against the normals of the faces that use them, over the (face, corner)
    pairs where both exist -> per track (pairs, share with a positive cosine, median angle in degrees)"""
    out = []
    for v, f, g in zip(m["verts"], m["faces"], m["normals"]):
        _, n = face_geometry(v, f)
        l = np.linalg.norm(n, axis=1)
        gn = g.astype(np.float64)[f]                                              # [k,3,3]
        with np.errstate(all="ignore"):
            cos = (gn * (n / l[:, None])[:, None, :]).sum(-1)
        ok = np.isfinite(cos) & (l > 0)[:, None]
        ang = np.degrees(np.arccos(np.clip(cos[ok], -1, 1)))
        out.append((int(ok.sum()), float((cos[ok] > 0).mean()), float(np.median(ang))) if ok.any() else (0, 0.0, np.inf))
    return out


def raycast_figures(sc, depth, voxel, exclude=None):
    """l: depth [B,V+1,H,W] at `cast_poses` -> per (b, pose) dict(n, hit, median, max, false): over the interior pixels
    (without `exclude[b][pose]`) the share with a depth and the median and largest |depth - z64| in voxels; false = depths on
    truly missed pixels; close = the share of those pixels with a depth within 0.1 voxel of z64 (four times the largest
    error of the reference chain), the score of the controls"""
    truth_x = cast_poses()[2]
    out = []
    for b in range(cs.B):
        for v in range(cs.V + 1):
            T = sc.truth[b][v] if v < cs.V else truth_x[b]
            m = T["interior"] if exclude is None else T["interior"] & ~exclude[b][v]
            d = depth[b, v].astype(np.float64)
            got = np.isfinite(d)
            with np.errstate(all="ignore"):
                err = np.abs(d - T["z64"])[m & got] / voxel
                close = np.abs(d - T["z64"]) <= 0.1 * voxel
            med, worst = (float(np.median(err)), float(err.max())) if len(err) else (np.inf, np.inf)
            out.append(dict(b=b, v=v, n=int(m.sum()), hit=float(got[m].mean()), median=med, max=worst,
                            false=int((got & ~T["hit"]).sum()), misses=int((~T["hit"]).sum()), close=float(close[m].mean())))
    return out


def eval_figures(sc, verts, dist):
    """n: point_mesh_distance of the model's vertices to the TRUE mesh against the float64 distance of the same f32 points
    -> per track (largest |dist - d64|, largest allowed by pointmesh_ref.forward_bound, all within)"""
    from tests import pointmesh_ref as pr
    out = []
    for b in range(cs.B):
        m = sc.meshes[b]
        d64 = sc.mesh_distance(b, verts[b])
        tol = pr.forward_bound(verts[b], m["verts"], m["faces"], pr.nearest(verts[b], m["verts"], m["faces"], np.float64)[1], d64)
        diff = np.abs(np.asarray(dist[b], np.float64) - d64)
        out.append((float(diff.max()), float(tol.max()), bool((diff <= tol).all())))
    return out


def signed_shares(towards, away):
    """n: signed distances of the truth points moved towards the camera and away from it -> (share > 0, share < 0)"""
    return float((np.asarray(towards) > 0).mean()), float((np.asarray(away) < 0).mean())


def color_figures(sc, m, colors, margin, reach=cs.REACH):
    """o: per track dict.  candidates = (vertex, view) pairs with IN_IMAGE and FACING; against chain_scene.occluded64 outside
    grey: occ_used = the share of truly occluded candidates with UNOCCLUDED, vis_dropped = the share of truly visible ones
    without; grey = the share of candidates in the grey zone.  Colour error |color - field(vertex)| (median, p99) over the
    coloured vertices none of whose used views is truly occluded."""
    from tests import viewcolor_ref as vr
    out = []
    for b in range(cs.B):
        X, flags, color = m["verts"][b], colors["flags"][b], colors["color"][b]
        cand = (flags & (vr.IN_IMAGE | vr.FACING)) == (vr.IN_IMAGE | vr.FACING)
        used = cand & ((flags & vr.UNOCCLUDED) != 0)
        occ, vis, grey = (np.stack(a, 1) for a in zip(*(cs.occluded64(b, s, X, margin, reach) for s in range(cs.V))))
        n_occ, n_vis = int((cand & occ).sum()), int((cand & vis).sum())
        bad = (used & occ).any(1)
        have = np.isfinite(color[:, 0]) & ~bad
        err = np.abs(color[have, 0].astype(np.float64) - cs.field(X[have].astype(np.float64)))
        out.append(dict(candidates=int(cand.sum()), grey=float((cand & grey).sum() / max(int(cand.sum()), 1)), n_occ=n_occ,
                        n_vis=n_vis, occ_used=float((used & occ).sum() / max(n_occ, 1)),
                        vis_dropped=float((cand & vis & ~used).sum() / max(n_vis, 1)), n=int(have.sum()),
                        coloured=float(np.isfinite(color[:, 0]).mean()),
                        median=float(np.median(err)) if have.any() else np.inf,
                        p99=float(np.percentile(err, 99)) if have.any() else np.inf))
    return out


def run_matcher_recon(sc, ch):
    """stage p: the matcher's own depths (ch["mdepth"], ch["keep"] of stage h) fused at VOXELS_P, with valid = the keep of
    the consistency rule at RECON_MAX_REL ("keep") and with the plain validity mask ("plain") -> dict"""
    mdepth, plain = ch["mdepth"], ch["keep"]
    keep = fusion_ref.consistency(mdepth, sc.ray, sc.K, sc.R, sc.t, plain, cs.MAX_PX, RECON_MAX_REL, 1)[1]
    out = {"valid": {"keep": keep, "plain": plain}, "models": {}}
    for voxel in VOXELS_P:
        for name in ("keep", "plain"):
            model = model_of(sc, mdepth, out["valid"][name], sc.R, sc.t, voxel)
            model["clean"] = clean_of(model["mesh"])
            out["models"][voxel, name] = model
    return out


@functools.lru_cache(maxsize=1)
def recon_matcher():
    return run_matcher_recon(cs.scene(), chain())


def kept_points_median(sc, depth, valid):
    """per track the median float64 distance to the true mesh of the per-view points depth * ray of the live pixels of
    `valid`, at the true poses"""
    from tests import tsdf_ref
    live = fusion_ref.live_mask(depth, valid)
    return [float(np.median(sc.mesh_distance(b, tsdf_ref.view_points(depth[b:b + 1], sc.ray, sc.R[b:b + 1], sc.t[b:b + 1],
                                                                  live[b:b + 1])))) for b in range(cs.B)]


# ---------------------------------------------------------------------------------------------------------------------
# the figures of each stage by name -> one value per track (or per view, or per pose), from either side's outputs
# ---------------------------------------------------------------------------------------------------------------------
def per(figs, key):
    return [f[key] for f in figs]


def figures_i(sc, normal):
    f = normals_figures(sc, normal)
    return {"i.share": [f["share"]], "i.median": [f["median"]], "i.max": [f["max"]]}, f


def figures_k(sc, mesh, voxel=VOXEL, stage="k"):
    v = vertex_figures(sc, mesh["verts"], voxel)
    out = {stage + "." + key: per(v, key) for key in ("median", "p99", "max", "beyond")}
    out[stage + ".complete"] = completeness(sc, mesh)
    out[stage + ".winding"] = [w[0] for w in winding_share(sc, mesh, margin_of(voxel))]
    g = gradient_normal_agreement(mesh)
    out[stage + ".gradient"] = [x[1] for x in g]
    out[stage + ".gradient_angle"] = [x[2] for x in g]
    return out


def figures_l(sc, depth, voxel=VOXEL, stage="l", exclude=None):
    r = raycast_figures(sc, depth, voxel, exclude)
    return {stage + "." + key: per(r, key) for key in ("hit", "median", "max", "false")}, r


def figures_m(sc, rc_like, voxel=VOXEL):
    """clean -> smooth -> simplify, each against the step before (the first against the raw model `rc_like["model"]`)"""
    out = {}
    before = vertex_figures(sc, rc_like["model"]["mesh"]["verts"], voxel)
    for step in ("clean", "smooth", "simplify"):
        now = vertex_figures(sc, rc_like[step]["verts"], voxel)
        out["m.%s.median" % step] = per(now, "median")
        out["m.%s.beyond" % step] = per(now, "beyond")
        out["m.%s.ratio" % step] = [a["median"] / b["median"] for a, b in zip(now, before)]
        before = now
    out["m.faces"] = [len(a) / len(b) for a, b in zip(rc_like["simplify"]["faces"], rc_like["smooth"]["faces"])]
    return out


def topology_counts(rc_like):
    """the MeshAdjacency counts of the smoothed (= cleaned) and of the simplified mesh per track, as tuples"""
    keys = ("referenced", "edges", "boundary", "nonmanifold", "valid", "euler")
    return {step: [tuple(int(a[k]) for k in keys) for a in rc_like[step]["adj"]] for step in ("smooth", "simplify")}


def front_facing_exclusion(sc):
    """stage n, mesh_to_tsdf of the TRUE mesh: the pixels to leave out of the ray cast's predicate, from the truth alone ->
    exclude[b][pose] bool [H,W].  The signed distance is positive on the side the face normals point to, and the ray cast
    reports a crossing from + to -.  A closed box is wound outwards, so its faces are met from their positive side; the
    wall is one sheet, wound away from the cameras, so a ray reaches it through negative values and reports nothing.  Left
    out: pixels whose true face has its normal (v1 - v0) x (v2 - v0) pointing away from the camera."""
    Rc, tc, truth_x = cast_poses()
    out = []
    for b in range(cs.B):
        fn = cs.face_normals(sc.meshes[b])
        row = []
        for v in range(cs.V + 1):
            T = sc.truth[b][v] if v < cs.V else truth_x[b]
            C = -Rc[b, v].astype(np.float64).T @ tc[b, v].astype(np.float64)
            row.append(~((fn[np.maximum(T["face"], 0)] * (C - T["X"])).sum(-1) > 0) | ~T["hit"])
        out.append(row)
    return out


def figures_o(sc, mesh, colors, voxel=VOXEL):
    c = color_figures(sc, mesh, colors, margin_of(voxel))
    return {"o." + key: per(c, key) for key in ("median", "p99", "occ_used", "vis_dropped", "grey", "coloured")}, c


def figures_p(sc, mdepth, valid, model, voxel, prefix):
    """p: stage k and the first line of m on a model of the matcher's depths -> named figures, each per track: `points`, the
    kept per-view points' median distance to the true mesh; the figures of k on the raw model (median, p99, max, beyond,
    complete, winding, gradient, gradient_angle); `vs_points`, the model's median over the points'; and of the cleaned
    model its vertex count `clean.n`, `clean.median`, `clean.beyond` and `clean.ratio`, its median over the raw model's"""
    pts = kept_points_median(sc, mdepth, valid)
    out = {prefix + ".points": pts}
    out.update(figures_k(sc, model["mesh"], voxel, prefix))
    out[prefix + ".vs_points"] = [m / p for m, p in zip(out[prefix + ".median"], pts)]
    clean = vertex_figures(sc, model["clean"]["verts"], voxel)
    out[prefix + ".clean.n"] = per(clean, "n")
    out[prefix + ".clean.median"] = per(clean, "median")
    out[prefix + ".clean.beyond"] = per(clean, "beyond")
    out[prefix + ".clean.ratio"] = [c / m for c, m in zip(per(clean, "median"), out[prefix + ".median"])]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the wrong conventions of the negative controls
# ---------------------------------------------------------------------------------------------------------------------
def transposed(R):
    return np.ascontiguousarray(np.swapaxes(R, -1, -2))


def interleaved_views(a):
    """[B,V,...] in (b, v) order -> what a caller who stacked the frames as v * B + b would pass"""
    return interleaved(a.reshape((N,) + a.shape[2:])).reshape(a.shape)


def half_pixel_images(images):
    """[...,H,W] -> the images sampled half a pixel to the right: the mean of horizontal neighbours (the last column kept)"""
    out = images.copy()
    out[..., :-1] = (images[..., :-1] + images[..., 1:]) * F(0.5)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# thresholds of stages i .. p.  RECON[name] = (thresholds, the reference chain's measured figures), one entry per track (or
# per pose, in (b, pose) order; one for both tracks where the figure is one).  The threshold is the measurement rounded by
# the figure's kind (`kind_of` the last part of its name, `threshold_of`); tests/test_chain_recon_host.py measures the
# figures again and checks that no threshold has drifted from them, tests/test_chain_recon_gpu.py asserts the same
# thresholds.
#   max    a distance, an error or a count that must not grow: rounded up in the second significant digit (ceil2)
#   min    a share that must not fall: rounded down to three decimals (floor3)
#   ratio  after / before of a median distance: where the reference shows an improvement (< 1) it is asserted at most
#          halfway to 1 (rounded up to three decimals), as tests/test_mesh_smooth_host.py does; where it shows none, the
#          ratio is a `max`
#   equal  a count that must be the reference's
# ---------------------------------------------------------------------------------------------------------------------
MIN_FIGURES = ("share", "winding", "gradient", "hit", "towards", "away", "coloured")


def kind_of(name):
    last = name.split(".")[-1]
    return "min" if last in MIN_FIGURES else "ratio" if last == "ratio" else "equal" if last == "n" else "max"


def threshold_of(kind, x):
    if kind == "equal":
        return x
    if kind == "min":
        return floor3(x)
    if kind == "ratio" and x < 1:
        return math.ceil((x + 1) / 2 * 1000 - 1e-9) / 1000
    return ceil2(x) if 0 < x < math.inf else float(x)


def hold(figs, drift=False):
    """asserts every named figure against its threshold; with drift also that the threshold is the figure, rounded"""
    for name, values in figs.items():
        values = [float(v) for v in values]
        print("%s: %s" % (name, " ".join("%.4g" % v for v in values)))
        kind, (thresholds, _) = kind_of(name), RECON[name]
        assert len(values) == len(thresholds), name
        for v, th in zip(values, thresholds):
            ok = v >= th if kind == "min" else v == th if kind == "equal" else v <= th
            assert ok, "%s: %r against %r" % (name, v, th)
            if drift and v != th:
                assert abs(threshold_of(kind, v) - th) <= 1e-9 * max(abs(th), 1e-30), "%s: %r drifted from %r" % (name, v, th)


GREY_CAP = 0.10                                          # of the candidates of stage o, both tracks
RECON = {
    "i.share": ((1.000,), (1,)),
    "i.median": ((0.007,), (0.006912,)),
    "i.max": ((0.03,), (0.02929,)),
    "j.ratio": ((0.516,), (0.03124,)),
    "k.median": ((0.00013, 8.2e-05,), (0.0001215, 8.13e-05,)),
    "k.p99": ((0.00061, 0.0073,), (0.0006031, 0.007236,)),
    "k.max": ((0.024, 0.0084,), (0.02385, 0.008325,)),
    "k.beyond": ((0, 0,), (0, 0,)),
    "k.complete": ((0.0066, 0.00019,), (0.006563, 0.0001838,)),
    "k.winding": ((1.000, 1.000,), (1, 1,)),
    "k.gradient": ((1.000, 1.000,), (1, 1,)),
    "k.gradient_angle": ((0.11, 0.27,), (0.1062, 0.2628,)),
    "l.hit": ((1.000, 1.000, 0.936, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000,), (1, 1, 0.9367, 1, 1, 1, 1, 1,
        1, 1,)),
    "l.median": ((0.0028, 0.0027, 0.0024, 0.0029, 0.0026, 0.0015, 0.0015, 0.0013, 0.0015, 0.0015,), (0.002782,
        0.002608, 0.002309, 0.002875, 0.002505, 0.001447, 0.001452, 0.001266, 0.001428, 0.001405,)),
    "l.max": ((0.021, 0.02, 0.021, 0.02, 0.024, 0.0076, 0.0063, 0.0063, 0.0066, 0.0069,), (0.02003, 0.01939, 0.02041,
        0.01924, 0.02348, 0.007573, 0.006226, 0.006277, 0.006533, 0.006867,)),
    "l.false": ((0, 0, 0, 0, 0, 0, 0, 0, 0, 0,), (0, 0, 0, 0, 0, 0, 0, 0, 0, 0,)),
    "m.clean.median": ((0.00013, 8e-05,), (0.0001208, 7.951e-05,)),
    "m.clean.beyond": ((0, 0,), (0, 0,)),
    "m.clean.ratio": ((0.998, 0.990,), (0.9943, 0.978,)),
    "m.smooth.median": ((0.00011, 6.1e-05,), (0.0001091, 6.08e-05,)),
    "m.smooth.beyond": ((0, 0,), (0, 0,)),
    "m.smooth.ratio": ((0.952, 0.883,), (0.903, 0.7646,)),
    "m.simplify.median": ((0.00012, 6.1e-05,), (0.000115, 6.02e-05,)),
    "m.simplify.beyond": ((0, 0,), (0, 0,)),
    "m.simplify.ratio": ((1.1, 0.996,), (1.054, 0.9902,)),
    "m.faces": ((0.24, 0.24,), (0.2358, 0.2322,)),
    "n.towards": ((1.000, 1.000,), (1, 1,)),
    "n.away": ((1.000, 1.000,), (1, 1,)),
    "n.cast.hit": ((1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000, 1.000,), (1, 1, 1, 1, 1, 1, 1, 1,
        1, 1,)),
    "n.cast.median": ((1.4e-06, 6.1e-06, 4.3e-06, 4.1e-06, 3.3e-06, 3.3e-06, 6.7e-06, 6e-06, 5.5e-06, 5.8e-06,),
        (1.316e-06, 6.047e-06, 4.211e-06, 4.017e-06, 3.293e-06, 3.253e-06, 6.667e-06, 5.975e-06, 5.451e-06,
        5.787e-06,)),
    "n.cast.max": ((6.3e-06, 0.011, 8.8e-06, 0.033, 0.029, 1.4e-05, 1.6e-05, 1.4e-05, 1.7e-05, 1.5e-05,), (6.275e-06,
        0.01067, 8.724e-06, 0.03281, 0.02832, 1.343e-05, 1.54e-05, 1.395e-05, 1.628e-05, 1.497e-05,)),
    "n.cast.false": ((0, 0, 0, 0, 0, 63, 61, 66, 70, 78,), (0, 0, 0, 0, 0, 63, 61, 66, 70, 78,)),
    "o.median": ((3.5e-05, 3.2e-05,), (3.494e-05, 3.119e-05,)),
    "o.p99": ((0.16, 0.0045,), (0.1568, 0.004421,)),
    "o.occ_used": ((0.17, 0,), (0.1604, 0,)),
    "o.vis_dropped": ((0, 0,), (0, 0,)),
    "o.grey": ((0.093, 0,), (0.09208, 0,)),
    "o.coloured": ((0.983, 0.964,), (0.9836, 0.964,)),
    "p.0.025.keep.points": ((0.018, 0.035,), (0.01784, 0.03405,)),
    "p.0.025.keep.median": ((0.037, 0.039,), (0.03681, 0.0381,)),
    "p.0.025.keep.p99": ((0.13, 0.06,), (0.1277, 0.0597,)),
    "p.0.025.keep.max": ((0.24, 0.12,), (0.2397, 0.1183,)),
    "p.0.025.keep.beyond": ((0.64, 0.69,), (0.633, 0.6869,)),
    "p.0.025.keep.complete": ((0.087, 0.049,), (0.08621, 0.04827,)),
    "p.0.025.keep.winding": ((0.918, 0.912,), (0.9182, 0.912,)),
    "p.0.025.keep.gradient": ((0.942, 0.998,), (0.9424, 0.9985,)),
    "p.0.025.keep.gradient_angle": ((23, 11,), (22.67, 10.24,)),
    "p.0.025.keep.vs_points": ((2.1, 1.2,), (2.063, 1.119,)),
    "p.0.025.keep.clean.n": ((5591, 837,), (5591, 837,)),
    "p.0.025.keep.clean.median": ((0.036, 0.04,), (0.03547, 0.03963,)),
    "p.0.025.keep.clean.beyond": ((0.62, 0.73,), (0.6171, 0.7204,)),
    "p.0.025.keep.clean.ratio": ((0.982, 1.1,), (0.9637, 1.04,)),
    "p.0.025.plain.points": ((0.019, 0.034,), (0.01885, 0.03313,)),
    "p.0.025.plain.median": ((0.038, 0.022,), (0.03771, 0.02113,)),
    "p.0.025.plain.p99": ((0.15, 0.19,), (0.1483, 0.1842,)),
    "p.0.025.plain.max": ((0.24, 0.2,), (0.2397, 0.1993,)),
    "p.0.025.plain.beyond": ((0.64, 0.36,), (0.6396, 0.352,)),
    "p.0.025.plain.complete": ((0.071, 0.029,), (0.07018, 0.02866,)),
    "p.0.025.plain.winding": ((0.925, 0.938,), (0.9255, 0.9386,)),
    "p.0.025.plain.gradient": ((0.948, 0.984,), (0.9487, 0.9841,)),
    "p.0.025.plain.gradient_angle": ((24, 13,), (23.86, 12.56,)),
    "p.0.025.plain.vs_points": ((2.1, 0.64,), (2.001, 0.6376,)),
    "p.0.025.plain.clean.n": ((6685, 1161,), (6685, 1161,)),
    "p.0.025.plain.clean.median": ((0.037, 0.022,), (0.03642, 0.02103,)),
    "p.0.025.plain.clean.beyond": ((0.64, 0.33,), (0.6326, 0.3247,)),
    "p.0.025.plain.clean.ratio": ((0.983, 0.998,), (0.966, 0.9953,)),
    "p.0.05.keep.points": ((0.018, 0.035,), (0.01784, 0.03405,)),
    "p.0.05.keep.median": ((0.038, 0.039,), (0.03732, 0.03893,)),
    "p.0.05.keep.p99": ((0.13, 0.055,), (0.1286, 0.05466,)),
    "p.0.05.keep.max": ((0.22, 0.074,), (0.2133, 0.07348,)),
    "p.0.05.keep.beyond": ((0.34, 0.02,), (0.3381, 0.01961,)),
    "p.0.05.keep.complete": ((0.093, 0.048,), (0.09249, 0.0472,)),
    "p.0.05.keep.winding": ((0.946, 0.982,), (0.9464, 0.9827,)),
    "p.0.05.keep.gradient": ((0.976, 1.000,), (0.9763, 1,)),
    "p.0.05.keep.gradient_angle": ((17, 6.7,), (16.59, 6.656,)),
    "p.0.05.keep.vs_points": ((2.1, 1.2,), (2.092, 1.143,)),
    "p.0.05.keep.clean.n": ((1044, 130,), (1044, 130,)),
    "p.0.05.keep.clean.median": ((0.039, 0.041,), (0.03828, 0.04026,)),
    "p.0.05.keep.clean.beyond": ((0.34, 0.0077,), (0.3362, 0.007692,)),
    "p.0.05.keep.clean.ratio": ((1.1, 1.1,), (1.026, 1.034,)),
    "p.0.05.plain.points": ((0.019, 0.034,), (0.01885, 0.03313,)),
    "p.0.05.plain.median": ((0.038, 0.02,), (0.03774, 0.01988,)),
    "p.0.05.plain.p99": ((0.17, 0.18,), (0.1668, 0.1729,)),
    "p.0.05.plain.max": ((0.28, 0.19,), (0.2757, 0.186,)),
    "p.0.05.plain.beyond": ((0.36, 0.16,), (0.3543, 0.1549,)),
    "p.0.05.plain.complete": ((0.092, 0.029,), (0.09129, 0.02848,)),
    "p.0.05.plain.winding": ((0.978, 0.952,), (0.9786, 0.9529,)),
    "p.0.05.plain.gradient": ((0.982, 1.000,), (0.982, 1,)),
    "p.0.05.plain.gradient_angle": ((16, 6.7,), (15.4, 6.681,)),
    "p.0.05.plain.vs_points": ((2.1, 0.6,), (2.002, 0.5999,)),
    "p.0.05.plain.clean.n": ((1190, 242,), (1190, 242,)),
    "p.0.05.plain.clean.median": ((0.036, 0.018,), (0.03533, 0.01714,)),
    "p.0.05.plain.clean.beyond": ((0.32, 0.071,), (0.3118, 0.07025,)),
    "p.0.05.plain.clean.ratio": ((0.969, 0.932,), (0.9362, 0.8623,)),
    "p.0.1.keep.points": ((0.018, 0.035,), (0.01784, 0.03405,)),
    "p.0.1.keep.median": ((0.038, 0.04,), (0.03704, 0.03915,)),
    "p.0.1.keep.p99": ((0.12, 0.046,), (0.1198, 0.04561,)),
    "p.0.1.keep.max": ((0.16, 0.046,), (0.1509, 0.04563,)),
    "p.0.1.keep.beyond": ((0.048, 0,), (0.04724, 0,)),
    "p.0.1.keep.complete": ((0.096, 0.049,), (0.09561, 0.04816,)),
    "p.0.1.keep.winding": ((0.986, 1.000,), (0.9866, 1,)),
    "p.0.1.keep.gradient": ((0.998, 1.000,), (0.9988, 1,)),
    "p.0.1.keep.gradient_angle": ((11, 3.8,), (10.13, 3.717,)),
    "p.0.1.keep.vs_points": ((2.1, 1.2,), (2.076, 1.15,)),
    "p.0.1.keep.clean.n": ((215, 0,), (215, 0,)),
    "p.0.1.keep.clean.median": ((0.044, math.inf,), (0.04348, math.inf,)),
    "p.0.1.keep.clean.beyond": ((0.038, 1,), (0.03721, 1,)),
    "p.0.1.keep.clean.ratio": ((1.2, math.inf,), (1.174, math.inf,)),
    "p.0.1.plain.points": ((0.019, 0.034,), (0.01885, 0.03313,)),
    "p.0.1.plain.median": ((0.035, 0.018,), (0.03458, 0.01746,)),
    "p.0.1.plain.p99": ((0.2, 0.06,), (0.192, 0.05993,)),
    "p.0.1.plain.max": ((0.23, 0.061,), (0.2257, 0.06024,)),
    "p.0.1.plain.beyond": ((0.045, 0,), (0.04428, 0,)),
    "p.0.1.plain.complete": ((0.096, 0.03,), (0.09554, 0.02909,)),
    "p.0.1.plain.winding": ((0.996, 1.000,), (0.9966, 1,)),
    "p.0.1.plain.gradient": ((1.000, 1.000,), (1, 1,)),
    "p.0.1.plain.gradient_angle": ((9, 6.5,), (8.909, 6.487,)),
    "p.0.1.plain.vs_points": ((1.9, 0.53,), (1.835, 0.5269,)),
    "p.0.1.plain.clean.n": ((226, 51,), (226, 51,)),
    "p.0.1.plain.clean.median": ((0.038, 0.02,), (0.03748, 0.01959,)),
    "p.0.1.plain.clean.beyond": ((0.0089, 0,), (0.00885, 0,)),
    "p.0.1.plain.clean.ratio": ((1.1, 1.2,), (1.084, 1.122,)),
}
ICP_OK_VIEWS = 4                                         # of the 6 perturbed views end with ok == 1 on the reference
# (referenced vertices, edges, boundary edges, non-manifold edges, valid faces, euler) per track
TOPOLOGY = {'simplify': [(941, 2565, 250, 1, 1627, 3), (148, 395, 46, 0, 248, 1)],
 'smooth': [(3710, 10606, 515, 0, 6899, 3), (584, 1651, 98, 0, 1068, 1)]}


def color_median_all(sc, m, colors):
    """per track the median |color - field(vertex)| over every coloured vertex (inf when none is): the controls' score"""
    out = []
    for b in range(cs.B):
        c = colors["color"][b][:, 0].astype(np.float64)
        have = np.isfinite(c)
        out.append(float(np.median(np.abs(c[have] - cs.field(m["verts"][b][have].astype(np.float64))))) if have.any() else np.inf)
    return out
