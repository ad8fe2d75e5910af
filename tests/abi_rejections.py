"""Calls of the C ABI that the library answers on the host, before any HIP call: the query functions (workspace sizes,
*_supported, *_layout) with good and bad shapes, and for every launching entry point only calls that are REJECTED (or are
empty: frames / N / B == 0) -- never one that passes validation, since the pointers are made up.  The answers recorded
from the library are in tests/golden/abi_rejections.json; tests/test_abi_rejections_host.py holds the built library to
them row by row, which pins every status code and the precedence between them.

The table is data: FUNCS gives each function's parameter names (in the order of include/ctd_hip.h, without the trailing
device / stream of the launching calls, which are always -1 / NULL) and a base call that WOULD pass validation and is
never made; ROWS lists (function, overrides of the base call, kind) with kind "query" (a function that launches nothing),
"rejected" (a launching call that must come back with a non-zero status) or "empty" (a launching call that must come back
CTD_OK without touching anything).  Values:
  * a pointer parameter of the base call is "p": a made-up address, (position + 1) * 16 MiB, so 256-byte aligned and far
    from every other one; an override may be None (NULL), an int, or "@name+offset" (the address of another parameter);
  * "@need" / "@need-1" as a workspace size is the answer of the function's own workspace query for the row's arguments;
  * structures and arrays that the host reads are real ctypes objects: a dict under "tables" / "params" / "out", a list
    under "row_counts" / "levels"; "name.field" overrides one field of such a dict (or of every dict of such a list).
"""
import ctypes

from connecting_the_dots_amd import _lib

NAN, INF = float("nan"), float("inf")
BIG = 1 << 40                       # workspace size of the base calls: never the reason for a rejection
P24 = 1 << 24

_VOL = dict(frames=2, C=1, H=16, W=32, D=8, bs=9)
_VOL1 = dict(frames=2, H=16, W=32, D=8, bs=9)
_IMG = dict(B=2, H=16, W=32)
_FUSION = dict(depth="p", valid="p", ray="p", K="p", R="p", t="p", max_px=1.0, max_rel=0.01, min_views=1)
_GEO = dict(depth0="p", depth1="p", ray="p", K="p", R0="p", t0="p", R1="p", t1="p")
_MESH = dict(n_verts=9, faces="p", n_faces=3, cam="p", cam_w=32, cam_h=16)
_TABLES = dict(nodes=1 << 24, roots=2 << 24, leaf_off=3 << 24, leaf_sum=4 << 24, entries=5 << 24, n_nodes=10, n_leaves=11,
               n_entries=20, row0=0, n_rows=16, n_trees=2, n_classes=64, max_depth=4, reserved=0)
_PARAMS = dict(n_trees=2, max_tree_depth=4, n_test_split_functions=8, n_test_thresholds=4, n_test_samples=16,
               min_samples_to_split=2, min_samples_for_leaf=1, depth_switch=2, n_disp_bins=4, reserved=0, seed=1)
_OUT = dict(nodes=1 << 24, roots=2 << 24, leaf_off=3 << 24, leaf_sum=4 << 24, entries=5 << 24, used=6 << 24, cap_nodes=64,
            cap_leaves=64, cap_entries=256)
_LEVEL = dict(disp=1 << 24, im=2 << 24, mask=0, pattern=3 << 24, pattern_proj=4 << 24, grad_proj=0, grad_disp=5 << 24, B=2,
              H=16, W=32)

# name -> (parameter names, base call, workspace query of the call or None)
FUNCS = {
    "ctd_xcorrvol_workspace_bytes": ("frames C H W D bs algo", dict(_VOL, algo=0), None),
    "ctd_xcorrvol_pattern_prepare_f32": ("in1 stride frames C H W D bs ws ws_bytes",
                                         dict(_VOL, in1="p", stride=0, ws="p", ws_bytes=BIG), None),
    "ctd_xcorrvol_f32": ("in0 in1 stride out frames C H W D bs algo ws ws_bytes",
                         dict(_VOL, in0="p", in1="p", stride=0, out="p", algo=0, ws="p", ws_bytes=BIG),
                         ("ctd_xcorrvol_workspace_bytes", "frames C H W D bs algo")),
    "ctd_xcorrvol_f64": ("in0 in1 stride out frames C H W D bs ws ws_bytes",
                         dict(_VOL, in0="p", in1="p", stride=0, out="p", ws="p", ws_bytes=BIG), None),
    "ctd_argmax_disp_f32": ("vol idx best frames D H W", dict(vol="p", idx="p", best="p", frames=2, D=8, H=16, W=32), None),
    "ctd_xcorrvol_rank_supported": ("C H W D bs", dict(C=1, H=16, W=32, D=8, bs=9), None),
    "ctd_xcorrvol_rank_layout": ("frames H W D per_frame offsets", dict(frames=2, H=16, W=32, D=8, per_frame=0, offsets="out5"),
                                 None),
    "ctd_xcorrvol_argmax_workspace_bytes": ("frames C H W D bs algo", dict(_VOL, algo=1), None),
    "ctd_xcorrvol_argmax_f32": ("in0 in1 stride vol_out idx best frames C H W D bs algo rerank_eps ws ws_bytes",
                                dict(_VOL, in0="p", in1="p", stride=0, vol_out="p", idx="p", best="p", algo=1,
                                     rerank_eps=1e-4, ws="p", ws_bytes=BIG),
                                ("ctd_xcorrvol_argmax_workspace_bytes", "frames C H W D bs algo")),
    "ctd_lcn_xcorrvol_supported": ("H W D radius bs", dict(H=16, W=32, D=8, radius=5, bs=9), None),
    "ctd_lcn_xcorrvol_argmax_f32": ("raw lcn_out std_out radius lcn_eps lcn_algo in1 stride vol_out idx best frames H W D bs "
                                    "algo rerank_eps ws ws_bytes",
                                    dict(_VOL1, raw="p", lcn_out="p", std_out="p", radius=5, lcn_eps=0.05, lcn_algo=0, in1="p",
                                         stride=0, vol_out="p", idx="p", best="p", algo=1, rerank_eps=1e-4, ws="p",
                                         ws_bytes=BIG), None),
    "ctd_costvol_f32": ("im pattern stride cost frames H W D bs type eps",
                        dict(_VOL1, im="p", pattern="p", stride=0, cost="p", type=1, eps=0.5), None),
    "ctd_costvol_workspace_bytes": ("frames H W D bs type per_frame", dict(_VOL1, type=1, per_frame=0), None),
    "ctd_costvol_fast_f32": ("im pattern stride cost frames H W D bs type eps ws ws_bytes",
                             dict(_VOL1, im="p", pattern="p", stride=0, cost="p", type=1, eps=0.5, ws="p", ws_bytes=BIG), None),
    "ctd_costvol_argmin_workspace_bytes": ("frames H W D bs type per_frame", dict(_VOL1, type=1, per_frame=0), None),
    "ctd_costvol_argmin_f32": ("im pattern stride idx best frames H W D bs type eps rerank_rel ws ws_bytes",
                               dict(_VOL1, im="p", pattern="p", stride=0, idx="p", best="p", type=1, eps=0.5, rerank_rel=1e-4,
                                    ws="p", ws_bytes=BIG), None),
    "ctd_xcorrvol_subpixel_workspace_bytes": ("frames H W D bs per_frame", dict(_VOL1, per_frame=0), None),
    "ctd_xcorrvol_subpixel_f32": ("in0 in1 stride idx disp refined frames H W D bs mode ws ws_bytes",
                                  dict(_VOL1, in0="p", in1="p", stride=0, idx="p", disp="p", refined="p", mode=0, ws="p",
                                       ws_bytes=BIG),
                                  ("ctd_xcorrvol_subpixel_workspace_bytes", "frames H W D bs stride")),
    "ctd_costvol_subpixel_f32": ("im pattern stride idx disp refined frames H W D bs type eps mode",
                                 dict(_VOL1, im="p", pattern="p", stride=0, idx="p", disp="p", refined="p", type=1, eps=0.5,
                                      mode=0), None),
    "ctd_match_validity_f32": ("vol maximise idx flags idx_r gap frames D H W lr_tol min_gap",
                               dict(vol="p", maximise=1, idx="p", flags="p", idx_r="p", gap="p", frames=2, D=8, H=16, W=32,
                                    lr_tol=1, min_gap=0.01), None),
    "ctd_xcorrvol_validity_workspace_bytes": ("frames C H W D bs algo", dict(_VOL, algo=1), None),
    "ctd_xcorrvol_validity_f32": ("in0 in1 stride idx flags idx_r gap frames C H W D bs algo lr_tol min_gap ws ws_bytes",
                                  dict(_VOL, in0="p", in1="p", stride=0, idx="p", flags="p", idx_r="p", gap="p", algo=1, lr_tol=1,
                                       min_gap=0.01, ws="p", ws_bytes=BIG),
                                  ("ctd_xcorrvol_validity_workspace_bytes", "frames C H W D bs algo")),
    "ctd_costvol_validity_workspace_bytes": ("frames H W D bs type algo per_frame", dict(_VOL1, type=1, algo=1, per_frame=0),
                                             None),
    "ctd_costvol_validity_f32": ("im pattern stride idx flags idx_r gap frames H W D bs type eps algo lr_tol min_gap ws ws_bytes",
                                 dict(_VOL1, im="p", pattern="p", stride=0, idx="p", flags="p", idx_r="p", gap="p", type=1,
                                      eps=0.5, algo=1, lr_tol=1, min_gap=0.01, ws="p", ws_bytes=BIG),
                                 ("ctd_costvol_validity_workspace_bytes", "frames H W D bs type algo stride")),
    "ctd_sgm_workspace_bytes": ("frames D H W paths want_volume", dict(frames=2, D=8, H=16, W=32, paths=8, want_volume=0), None),
    "ctd_sgm_aggregate_f32": ("vol maximise p1 p2 paths S_out idx best frames D H W ws ws_bytes",
                              dict(vol="p", maximise=0, p1=1.0, p2=8.0, paths=8, S_out=None, idx="p", best="p", frames=2, D=8,
                                   H=16, W=32, ws="p", ws_bytes=BIG),
                              ("ctd_sgm_workspace_bytes", "frames D H W paths 0")),
    "ctd_disp_components_workspace_bytes": ("frames H W", dict(frames=2, H=16, W=32), None),
    "ctd_disp_components_f32": ("disp valid max_diff connectivity label size frames H W ws ws_bytes",
                                dict(disp="p", valid="p", max_diff=1.0, connectivity=4, label="p", size="p", frames=2, H=16, W=32,
                                     ws="p", ws_bytes=BIG),
                                ("ctd_disp_components_workspace_bytes", "frames H W")),
    "ctd_disp_speckle_f32": ("disp valid max_diff max_size connectivity keep size frames H W ws ws_bytes",
                             dict(disp="p", valid="p", max_diff=1.0, max_size=20, connectivity=8, keep="p", size="p", frames=2,
                                  H=16, W=32, ws="p", ws_bytes=BIG),
                             ("ctd_disp_components_workspace_bytes", "frames H W")),
    "ctd_disp_median_f32": ("disp valid window fill_min out valid_out frames H W",
                            dict(disp="p", valid="p", window=3, fill_min=2, out="p", valid_out="p", frames=2, H=16, W=32), None),
    "ctd_depth_consistency_f32": ("depth valid ray K R t max_px max_rel min_views count keep fused B V H W",
                                  dict(_FUSION, count="p", keep="p", fused="p", B=2, V=3, H=8, W=16), None),
    "ctd_depth_fuse_workspace_bytes": ("B V H W", dict(B=2, V=3, H=8, W=16), None),
    "ctd_depth_fuse_points_f32": ("depth valid ray K R t max_px max_rel min_views dedupe points src n_per_track count keep fused "
                                  "B V H W ws ws_bytes",
                                  dict(_FUSION, dedupe=1, points="p", src="p", n_per_track="p", count="p", keep="p", fused="p",
                                       B=2, V=3, H=8, W=16, ws="p", ws_bytes=BIG),
                                  ("ctd_depth_fuse_workspace_bytes", "B V H W")),
    "ctd_disp_to_depth_fwd_f32": ("disp depth n bf", dict(disp="p", depth="p", n=64, bf=10.0), None),
    "ctd_idx_to_depth_f32": ("idx depth n bf disp_offset", dict(idx="p", depth="p", n=64, bf=10.0, disp_offset=0.5), None),
    "ctd_disp_to_depth_bwd_f32": ("disp grad_depth grad_disp n bf", dict(disp="p", grad_depth="p", grad_disp="p", n=64, bf=10.0),
                                  None),
    "ctd_disparity_loss_workspace_bytes": ("B H W", dict(_IMG), None),
    "ctd_disparity_loss_fwd_f32": ("disp edge loss B H W ws ws_bytes", dict(_IMG, disp="p", edge="p", loss="p", ws="p", ws_bytes=BIG),
                                   None),
    "ctd_disparity_loss_bwd_f32": ("disp edge grad_loss grad_disp grad_edge B H W ws ws_bytes",
                                   dict(_IMG, disp="p", edge="p", grad_loss="p", grad_disp="p", grad_edge="p", ws="p",
                                        ws_bytes=BIG), None),
    "ctd_geometric_workspace_bytes": ("B H W", dict(_IMG), None),
    "ctd_geometric_fwd_f32": ("depth0 depth1 ray K R0 t0 R1 t1 loss accumulate B H W clamp ws ws_bytes",
                              dict(_GEO, **_IMG, loss="p", accumulate=0, clamp=1.0, ws="p", ws_bytes=BIG), None),
    "ctd_geometric_sym_fwd_f32": ("depth0 depth1 ray K R0 t0 R1 t1 loss B H W clamp ws ws_bytes ticket",
                                  dict(_GEO, **_IMG, loss="p", clamp=1.0, ws="p", ws_bytes=BIG, ticket="p"), None),
    "ctd_geometric_bwd_f32": ("depth0 depth1 ray K R0 t0 R1 t1 grad_loss grad_depth0 accumulate0 grad_depth1 B H W clamp",
                              dict(_GEO, **_IMG, grad_loss="p", grad_depth0="p", accumulate0=0, grad_depth1="p", clamp=1.0), None),
    "ctd_pattern_loss_workspace_bytes": ("B H W", dict(_IMG), None),
    "ctd_pattern_loss_fwd_f32": ("disp im mask pattern pattern_proj terms B H W type eps ws ws_bytes",
                                 dict(_IMG, disp="p", im="p", mask="p", pattern="p", pattern_proj="p", terms="p", type=3, eps=0.5,
                                      ws="p", ws_bytes=BIG),
                                 ("ctd_pattern_loss_workspace_bytes", "B H W")),
    "ctd_pattern_loss_bwd_f32": ("disp im mask pattern terms grad_val grad_proj grad_disp B H W type eps",
                                 dict(_IMG, disp="p", im="p", mask="p", pattern="p", terms="p", grad_val="p", grad_proj="p",
                                      grad_disp="p", type=3, eps=0.5), None),
    "ctd_pattern_loss_multi_workspace_bytes": ("n_levels levels", dict(n_levels=2, levels=[_LEVEL, _LEVEL]), None),
    "ctd_pattern_loss_multi_fwd_f32": ("n_levels levels terms type eps ws ws_bytes",
                                       dict(n_levels=2, levels=[_LEVEL, _LEVEL], terms="p", type=3, eps=0.5, ws="p", ws_bytes=BIG),
                                       ("ctd_pattern_loss_multi_workspace_bytes", "n_levels levels")),
    "ctd_pattern_loss_multi_bwd_f32": ("n_levels levels terms grad_vals type eps",
                                       dict(n_levels=2, levels=[_LEVEL, _LEVEL], terms="p", grad_vals="p", type=3, eps=0.5), None),
    "ctd_render_mesh_proj_f32": ("verts colors n_verts faces n_faces cam cam_w cam_h proj proj_w proj_h shader pattern d_alpha "
                                 "d_beta depth color normal",
                                 dict(_MESH, verts="p", colors="p", proj="p", proj_w=32, proj_h=16, shader="p", pattern="p",
                                      d_alpha=1.0, d_beta=0.0, depth="p", color="p", normal="p"), None),
    "ctd_render_mesh_f32": ("verts colors normals n_verts faces n_faces cam cam_w cam_h shader depth color normal",
                            dict(_MESH, verts="p", colors="p", normals="p", shader="p", depth="p", color="p", normal="p"), None),
    "ctd_mesh_bvh_bytes": ("n_faces", dict(n_faces=3), None),
    "ctd_mesh_bvh_workspace_bytes": ("n_faces", dict(n_faces=3), None),
    "ctd_mesh_bvh_build_f32": ("verts n_verts faces n_faces bvh bvh_bytes ws ws_bytes depth",
                               dict(verts="p", n_verts=9, faces="p", n_faces=3, bvh="p", bvh_bytes=BIG, ws="p", ws_bytes=BIG,
                                    depth="p"),
                               ("ctd_mesh_bvh_workspace_bytes", "n_faces")),
    "ctd_render_mesh_proj_bvh_f32": ("bvh verts colors n_verts faces n_faces cam cam_w cam_h proj proj_w proj_h shader pattern "
                                     "d_alpha d_beta depth color normal",
                                     dict(_MESH, bvh="p", verts="p", colors="p", proj="p", proj_w=32, proj_h=16, shader="p",
                                          pattern="p", d_alpha=1.0, d_beta=0.0, depth="p", color="p", normal="p"), None),
    "ctd_render_mesh_bvh_f32": ("bvh verts colors normals n_verts faces n_faces cam cam_w cam_h shader depth color normal",
                                dict(_MESH, bvh="p", verts="p", colors="p", normals="p", shader="p", depth="p", color="p",
                                     normal="p"), None),
    "ctd_syn_finish_f32": ("depth color normal blend bf grad_threshold lcn_radius lcn_eps lcn_clip im ambient grad disp mask N H W",
                           dict(depth="p", color="p", normal="p", blend="p", bf=10.0, grad_threshold=0.1, lcn_radius=5, lcn_eps=0.05,
                                lcn_clip=1, im="p", ambient="p", grad="p", disp="p", mask="p", N=2, H=16, W=32), None),
    "ctd_augment_f32": ("img noise noise_f64 params out minmax N H W",
                        dict(img="p", noise="p", noise_f64=0, params="p", out="p", minmax="p", N=2, H=16, W=32), None),
    "ctd_salt_pepper_f32": ("img minmax counts salt pepper kmax N H W",
                            dict(img="p", minmax="p", counts="p", salt="p", pepper="p", kmax=4, N=2, H=16, W=32), None),
    "ctd_nn_f32": ("in0 in1 n0 n1 out", dict(in0="p", in1="p", n0=8, n1=8, out="p"), None),
    "ctd_nn_f64": ("in0 in1 n0 n1 out", dict(in0="p", in1="p", n0=8, n1=8, out="p"), None),
    "ctd_crosscheck": ("in0 in1 n0 n1 out", dict(in0="p", in1="p", n0=8, n1=8, out="p"), None),
    "ctd_proj_nn_f32": ("xyz0 xyz1 K B H W patch_size out", dict(_IMG, xyz0="p", xyz1="p", K="p", patch_size=3, out="p"), None),
    "ctd_proj_nn_f64": ("xyz0 xyz1 K B H W patch_size out", dict(_IMG, xyz0="p", xyz1="p", K="p", patch_size=3, out="p"), None),
    "ctd_hyperdepth_eval_f32": ("tables ims N H W row_from row_to n_disp_bins out",
                                dict(tables=_TABLES, ims="p", N=2, H=16, W=32, row_from=0, row_to=16, n_disp_bins=4, out="p"), None),
    "ctd_hyperdepth_train_count_f32": ("disps N H W row_from row_to n_disp_bins counts",
                                       dict(disps="p", N=2, H=16, W=32, row_from=0, row_to=4, n_disp_bins=4, counts="p"), None),
    "ctd_hyperdepth_train_workspace_bytes": ("params n_rows row_counts cap_leaves",
                                             dict(params=_PARAMS, n_rows=4, row_counts=[40, 0, 17, 64], cap_leaves=64), None),
    "ctd_hyperdepth_train_f32": ("params X n_x ims disps N H W row_from row_to row_counts ws ws_bytes out",
                                 dict(params=_PARAMS, X="p", n_x=17, ims="p", disps="p", N=2, H=16, W=32, row_from=0, row_to=4,
                                      row_counts=[40, 0, 17, 64], ws="p", ws_bytes=BIG, out=_OUT),
                                 ("ctd_hyperdepth_train_workspace_bytes", "params 4 row_counts out.cap_leaves")),
}
for _sfx in ("f32", "f64", "fast_f32"):
    FUNCS["ctd_photometric_fwd_" + _sfx] = ("es ta out B C H W bs type eps",
                                            dict(es="p", ta="p", out="p", B=2, C=1, H=16, W=32, bs=9, type=3, eps=0.5), None)
    FUNCS["ctd_photometric_bwd_" + _sfx] = ("es ta grad_out grad_es B C H W bs type eps",
                                            dict(es="p", ta="p", grad_out="p", grad_es="p", B=2, C=1, H=16, W=32, bs=9, type=3,
                                                 eps=0.5), None)
for _n in ("ctd_lcn_f32", "ctd_lcn_fast_f32"):
    FUNCS[_n] = ("x y std_out N H W radius eps", dict(x="p", y="p", std_out="p", N=2, H=16, W=32, radius=7, eps=0.05), None)
FUNCS["ctd_lcn_datagen_f32"] = ("img out out_std N H W kernel_size eps",
                                dict(img="p", out="p", out_std="p", N=2, H=16, W=32, kernel_size=11, eps=0.05), None)

QUERIES = sorted(n for n in FUNCS if _lib.SIGNATURES[n][0] is not _lib._c_int or n.endswith(("_supported", "_layout")))

ROWS = []


def rows(func, kind, *overrides):
    ROWS.extend((func, o, kind) for o in overrides)


def nulls(func, *names):
    rows(func, "rejected", *[{n: None} for n in names])


# sizes that fail every volume call: each size non-positive, D * H * W at the reference's int limit
_BAD_VOL1 = [dict(frames=-1), dict(H=0), dict(W=0), dict(D=0), dict(bs=0), dict(H=-3), dict(D=128, H=4096, W=4096)]
_BAD_VOL = _BAD_VOL1 + [dict(C=0), dict(C=-1)]
_BELOW_2_31 = dict(D=128, H=4096, W=4095)          # the largest volume below the limit: not an invalid argument
_BAD_TYPE = [dict(type=-1), dict(type=4)]
_BAD_IMG = [dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(B=65536), dict(B=1, H=32768, W=65536)]

# ---- query functions: good and bad shapes alike
for _n in ("ctd_xcorrvol_workspace_bytes", "ctd_xcorrvol_argmax_workspace_bytes", "ctd_xcorrvol_validity_workspace_bytes"):
    rows(_n, "query", {}, dict(algo=0), dict(algo=1), dict(algo=2), dict(algo=-1), dict(frames=0), dict(frames=16, H=432, W=512, D=128),
         dict(C=2), dict(C=2, algo=0), dict(bs=7), dict(bs=8), dict(bs=2), dict(bs=11), dict(bs=11, algo=0), dict(W=30), dict(D=512),
         dict(D=513), dict(D=513, algo=0), dict(frames=65535), dict(frames=65536, H=1, W=4), dict(H=65536, frames=1),
         dict(frames=1, H=65535, W=65540), dict(frames=5, H=32768, W=32767, D=1), dict(frames=4, H=32768, W=32768, D=1),
         dict(frames=4, H=32768, W=32767, D=1), _BELOW_2_31, dict(_BELOW_2_31, frames=1), dict(algo=0x101), *_BAD_VOL)
rows("ctd_xcorrvol_rank_supported", "query", {}, dict(C=2), dict(W=30), dict(D=512), dict(D=513), dict(bs=7), dict(bs=2), dict(bs=4),
     dict(bs=11), dict(H=0), dict(W=0), dict(D=0), dict(C=0), dict(bs=0), dict(D=128, H=4096, W=4096), _BELOW_2_31)
rows("ctd_xcorrvol_rank_layout", "query", {}, dict(per_frame=1), dict(frames=16, H=432, W=512, D=128), dict(frames=1, H=1024, W=1024, D=256),
     dict(frames=1, H=9, W=4, D=1), dict(offsets=None), dict(frames=0), dict(frames=-1), dict(H=0), dict(W=0), dict(D=0),
     dict(D=128, H=4096, W=4096), dict(frames=0, offsets=None))
rows("ctd_lcn_xcorrvol_supported", "query", {}, dict(radius=4), dict(radius=6), dict(bs=7), dict(W=30), dict(W=12), dict(W=16), dict(H=10),
     dict(H=11), dict(D=512), dict(D=513), dict(H=0), dict(D=0), dict(bs=0), dict(H=32768, W=32768, D=1), dict(H=32768, W=32764, D=1))
for _n in ("ctd_costvol_workspace_bytes", "ctd_costvol_argmin_workspace_bytes"):
    rows(_n, "query", {}, dict(per_frame=1), dict(type=0), dict(type=2), dict(type=3), dict(bs=7), dict(bs=8), dict(bs=2), dict(bs=4),
         dict(bs=11), dict(W=30), dict(W=4), dict(W=8), dict(D=512), dict(D=513), dict(frames=0), dict(frames=65535, D=1),
         dict(frames=65536, D=1, H=1, W=4), dict(frames=255, D=8193, H=1, W=4), dict(H=1048576, W=4, D=1, frames=1), _BELOW_2_31,
         *(_BAD_VOL1 + _BAD_TYPE))
rows("ctd_xcorrvol_subpixel_workspace_bytes", "query", {}, dict(per_frame=1), dict(bs=7), dict(bs=8), dict(bs=2), dict(bs=11), dict(frames=0),
     dict(W=30), _BELOW_2_31, *_BAD_VOL1)
rows("ctd_costvol_validity_workspace_bytes", "query", {}, dict(algo=0), dict(algo=2), dict(algo=-1), dict(per_frame=1), dict(type=0),
     dict(type=3), dict(bs=7), dict(bs=2), dict(bs=4), dict(bs=11), dict(bs=11, algo=0), dict(frames=0), dict(frames=8191, D=8, algo=0, H=1, W=4),
     dict(frames=8192, D=8, algo=0, H=1, W=4), dict(frames=8192, D=8, H=1, W=4), dict(frames=65536, D=1, H=1, W=4), dict(H=65536, frames=1, W=4),
     dict(frames=1, H=65535, W=65540, D=1), dict(frames=5, H=32768, W=32767, D=1), dict(frames=4, H=32768, W=32768, D=1),
     dict(frames=4, H=32768, W=32767, D=1), dict(W=30), dict(D=513), *(_BAD_VOL1 + _BAD_TYPE))
rows("ctd_sgm_workspace_bytes", "query", {}, dict(paths=4), dict(paths=6), dict(paths=0), dict(want_volume=1), dict(D=256), dict(D=257),
     dict(frames=0), dict(frames=-1), dict(D=0), dict(H=0), dict(W=0), dict(frames=1, D=128, H=4096, W=4096),
     dict(frames=1, D=128, H=4096, W=4095), dict(frames=2, D=64, H=4096, W=4096))
rows("ctd_disp_components_workspace_bytes", "query", {}, dict(frames=1, H=1, W=1), dict(frames=3, H=5, W=7), dict(frames=0), dict(frames=-1),
     dict(H=0), dict(W=0), dict(frames=1, H=32768, W=65536), dict(frames=1, H=32768, W=65535), dict(frames=2, H=32768, W=32768))
rows("ctd_depth_fuse_workspace_bytes", "query", {}, dict(B=1, V=64, H=1, W=1), dict(V=65), dict(V=64), dict(B=0), dict(B=-1), dict(V=0),
     dict(H=0), dict(W=0), dict(H=P24, B=1, V=1, W=1), dict(H=P24 + 1, B=1, V=1, W=1), dict(W=P24 + 1, B=1, V=1, H=1),
     dict(B=1 << 12, V=64, H=1 << 7, W=1 << 6), dict(B=1 << 18, V=64, H=1, W=1), dict(B=(1 << 18) - 1, V=64, H=1, W=1))
for _n in ("ctd_disparity_loss_workspace_bytes", "ctd_geometric_workspace_bytes", "ctd_pattern_loss_workspace_bytes"):
    rows(_n, "query", {}, dict(B=1, H=1, W=1), dict(B=3, H=33, W=130), dict(B=65535, H=1, W=1), dict(B=1, H=32768, W=65535), *_BAD_IMG)
rows("ctd_pattern_loss_multi_workspace_bytes", "query", {}, dict(n_levels=1), dict(n_levels=0), dict(n_levels=-1), dict(n_levels=9),
     dict(levels=None), {"levels.B": 0}, {"levels.H": 1}, {"levels.W": 1}, {"levels.disp": 0}, {"levels.im": 0}, {"levels.pattern": 0},
     {"levels.pattern_proj": 0}, {"levels.B": 1 << 20, "levels.H": 4096, "levels.W": 2048}, dict(n_levels=8, levels=[_LEVEL] * 8),
     dict(n_levels=9, levels=[_LEVEL] * 9))
for _n in ("ctd_mesh_bvh_bytes", "ctd_mesh_bvh_workspace_bytes"):
    rows(_n, "query", {}, dict(n_faces=0), dict(n_faces=1), dict(n_faces=-1), dict(n_faces=100000), dict(n_faces=1 << 28),
         dict(n_faces=(1 << 28) + 1))
rows("ctd_hyperdepth_train_workspace_bytes", "query", {}, dict(cap_leaves=0), dict(cap_leaves=-1), dict(params=None), dict(row_counts=None),
     dict(n_rows=0), dict(n_rows=1), dict(row_counts=[40, -1, 17, 64]), {"params.n_trees": 0}, {"params.n_trees": 16}, {"params.n_trees": 17},
     {"params.max_tree_depth": -1}, {"params.max_tree_depth": 24}, {"params.max_tree_depth": 25}, {"params.n_test_split_functions": -1},
     {"params.n_test_split_functions": 1 << 20}, {"params.n_test_thresholds": -1}, {"params.n_test_thresholds": 1 << 16},
     {"params.n_test_samples": 0}, {"params.n_test_samples": 8192}, {"params.n_test_samples": 8193}, {"params.min_samples_to_split": -1},
     {"params.min_samples_for_leaf": 0}, {"params.n_disp_bins": 0})

# ---- NCC volumes and their argmax
for _n in ("ctd_xcorrvol_f32", "ctd_xcorrvol_f64", "ctd_xcorrvol_argmax_f32", "ctd_xcorrvol_pattern_prepare_f32"):
    rows(_n, "rejected", dict(stride=-1), dict(_BELOW_2_31, frames=1, ws=None), *[b for b in _BAD_VOL])
    rows(_n, "rejected", dict(frames=0, H=0), dict(frames=0, stride=-1))                                     # sizes before emptiness
for _n in ("ctd_xcorrvol_f32", "ctd_xcorrvol_f64", "ctd_xcorrvol_argmax_f32"):
    rows(_n, "empty", dict(frames=0), dict(frames=0, in0=None, ws=None, ws_bytes=0))
rows("ctd_xcorrvol_pattern_prepare_f32", "rejected", dict(frames=0), dict(in1=None), dict(D=513), dict(D=513, ws=None), dict(bs=34),
     dict(bs=1), dict(H=1 << 20, W=4, D=1), dict(stride=5), dict(stride=5, ws=None), dict(ws=None), dict(ws_bytes=0), dict(ws=None, in1=None))
nulls("ctd_xcorrvol_f32", "in0", "in1", "out")
rows("ctd_xcorrvol_f32", "rejected", dict(algo=2), dict(algo=-1), dict(algo=0x100), dict(algo=0x100, H=0), dict(algo=0x102), dict(algo=2, in0=None),
     dict(algo=2, ws=None), dict(ws=None), dict(ws_bytes=0), dict(stride=512, ws_bytes="@need-1"), dict(bs=7, ws=None), dict(C=2, ws=None),
     dict(algo=1, ws=None), dict(algo=1, ws_bytes=0), dict(algo=0x101, ws=None), dict(algo=1, D=513), dict(algo=1, D=513, ws=None),
     dict(algo=1, bs=34), dict(algo=1, bs=1), dict(algo=1, frames=P24, H=1, W=4, D=1), dict(algo=1, W=(1 << 19) - 8, H=1, frames=1),
     dict(algo=1, out=None), dict(frames=0, algo=0x100))
rows("ctd_xcorrvol_f32", "empty", dict(frames=0, algo=1), dict(frames=0, algo=0x101), dict(frames=0, algo=2))
nulls("ctd_xcorrvol_f64", "in0", "in1", "out")
nulls("ctd_argmax_disp_f32", "vol", "idx")
rows("ctd_argmax_disp_f32", "rejected", dict(frames=-1), dict(D=0), dict(H=0), dict(W=0), dict(frames=0, D=0))
rows("ctd_argmax_disp_f32", "empty", dict(frames=0), dict(frames=0, vol=None, idx=None))
nulls("ctd_xcorrvol_argmax_f32", "in0", "in1", "idx")
rows("ctd_xcorrvol_argmax_f32", "rejected", dict(C=2), dict(C=2, frames=0), dict(C=2, in0=None), dict(C=2, H=0), dict(C=2, algo=0x100),
     dict(algo=2), dict(algo=-1), dict(algo=0x100), dict(algo=2, ws=None), dict(rerank_eps=NAN),
     dict(rerank_eps=NAN, ws=None), dict(rerank_eps=NAN, algo=0, ws=None), dict(ws=None), dict(ws_bytes=0), dict(ws_bytes="@need-1", stride=512),
     dict(rerank_eps=-1.0, ws=None), dict(rerank_eps=-1.0, vol_out=None, ws=None), dict(vol_out=None, ws=None), dict(vol_out="@vol_out+4", ws=None),
     dict(vol_out=None, bs=7), dict(vol_out=None, W=30), dict(vol_out=None, W=30, rerank_eps=NAN), dict(bs=7, ws=None), dict(W=30, ws=None),
     dict(D=513), dict(D=513, vol_out=None), dict(algo=0, ws=None), dict(algo=0, ws_bytes=0), dict(algo=0, bs=11), dict(algo=0, bs=11, ws=None),
     dict(algo=0, vol_out=None, ws=None), dict(algo=0, stride=512, ws_bytes="@need-1"), dict(frames=0, algo=0x100))
rows("ctd_xcorrvol_argmax_f32", "empty", dict(frames=0, algo=2), dict(frames=0, rerank_eps=NAN))

# ---- fused LCN + matcher
nulls("ctd_lcn_xcorrvol_argmax_f32", "raw", "lcn_out", "std_out", "in1", "idx")
rows("ctd_lcn_xcorrvol_argmax_f32", "rejected", dict(algo=0), dict(algo=0x100), dict(algo=2), dict(lcn_algo=2), dict(lcn_algo=-1), dict(stride=-1),
     dict(radius=-1), dict(rerank_eps=NAN), dict(radius=4), dict(radius=6), dict(bs=7), dict(W=30), dict(W=12), dict(H=10), dict(D=513),
     dict(vol_out="@vol_out+4"), dict(vol_out="@vol_out+8"), dict(radius=4, raw=None), dict(radius=4, frames=0, H=0), dict(radius=4, algo=0),
     dict(ws=None), dict(ws_bytes=0), dict(ws=None, vol_out=None), dict(ws=None, algo=0x101), dict(ws=None, lcn_algo=1), dict(stride=5, ws=None),
     dict(frames=0, rerank_eps=NAN), *_BAD_VOL1)
rows("ctd_lcn_xcorrvol_argmax_f32", "empty", dict(frames=0), dict(frames=0, radius=4), dict(frames=0, raw=None, idx=None))

# ---- LCN
for _n in ("ctd_lcn_f32", "ctd_lcn_fast_f32"):
    nulls(_n, "x", "y", "std_out")
    rows(_n, "rejected", dict(N=-1), dict(H=0), dict(W=0), dict(radius=-1), dict(radius=16), dict(radius=32), dict(H=32768, W=65536),
         dict(N=0, radius=16), dict(N=-1, x=None))
    rows(_n, "empty", dict(N=0), dict(N=0, x=None), dict(N=0, radius=15))
nulls("ctd_lcn_datagen_f32", "img", "out", "out_std")
rows("ctd_lcn_datagen_f32", "rejected", dict(N=-1), dict(H=0), dict(W=0), dict(kernel_size=-1), dict(N=65536), dict(N=65536, img=None))
rows("ctd_lcn_datagen_f32", "empty", dict(N=0), dict(N=0, img=None))

# ---- photometric loss and the cost volumes
for _sfx in ("f32", "f64", "fast_f32"):
    nulls("ctd_photometric_fwd_" + _sfx, "es", "ta", "out")
    nulls("ctd_photometric_bwd_" + _sfx, "es", "ta", "grad_out", "grad_es")
    for _n in ("ctd_photometric_fwd_" + _sfx, "ctd_photometric_bwd_" + _sfx):
        rows(_n, "rejected", dict(B=-1), dict(C=0), dict(H=0), dict(W=0), dict(bs=0), dict(type=7), dict(B=2, C=1, H=32768, W=32768),
             dict(B=0, type=4), dict(B=0, bs=0), dict(es=None, type=4), *_BAD_TYPE)
        rows(_n, "empty", dict(B=0), dict(B=0, es=None))
nulls("ctd_costvol_f32", "im", "pattern", "cost")
rows("ctd_costvol_f32", "rejected", dict(stride=-1), dict(frames=8192), dict(frames=8192, im=None), dict(frames=1, D=65536, H=1, W=4),
     dict(frames=0, type=4), dict(frames=0, stride=-1), *(_BAD_VOL1 + _BAD_TYPE))
rows("ctd_costvol_f32", "empty", dict(frames=0), dict(frames=0, im=None))
nulls("ctd_costvol_fast_f32", "im", "pattern", "cost")
rows("ctd_costvol_fast_f32", "rejected", dict(stride=-1), dict(stride=5), dict(stride=511), dict(stride=5, im=None), dict(frames=0, type=-1),
     *(_BAD_VOL1 + _BAD_TYPE))
rows("ctd_costvol_fast_f32", "empty", dict(frames=0), dict(frames=0, stride=5), dict(frames=0, im=None))
nulls("ctd_costvol_argmin_f32", "im", "pattern", "idx")
rows("ctd_costvol_argmin_f32", "rejected", dict(bs=8), dict(bs=2), dict(bs=4), dict(bs=11), dict(bs=1), dict(bs=11, im=None), dict(bs=11, stride=5),
     dict(bs=11, frames=0, H=0), dict(stride=-1), dict(stride=5), dict(stride=5, frames=0), dict(rerank_rel=NAN), dict(rerank_rel=NAN, frames=0),
     dict(frames=255, D=8193, H=1, W=4, ws=None), dict(H=1048576, W=4, D=1, frames=1, ws=None), dict(ws=None), dict(ws_bytes=0),
     dict(ws="@ws+128"), dict(frames=0, type=4), *(_BAD_VOL1 + _BAD_TYPE))
rows("ctd_costvol_argmin_f32", "empty", dict(frames=0), dict(frames=0, bs=11), dict(frames=0, im=None))

# ---- sub-pixel refinement
nulls("ctd_xcorrvol_subpixel_f32", "in0", "in1", "idx", "disp")
rows("ctd_xcorrvol_subpixel_f32", "rejected", dict(bs=8), dict(bs=2), dict(bs=4), dict(mode=2), dict(mode=-1), dict(mode=0x102), dict(stride=5),
     dict(stride=-1), dict(stride=5, frames=0), dict(ws=None), dict(ws="@ws+128"), dict(ws="@ws+16"), dict(ws_bytes=0), dict(ws_bytes="@need-1"),
     dict(ws_bytes="@need-1", stride=512), dict(ws_bytes="@need-1", mode=0x101), dict(ws=None, in0=None), dict(frames=0, mode=2), *_BAD_VOL1)
rows("ctd_xcorrvol_subpixel_f32", "empty", dict(frames=0), dict(frames=0, ws=None, in0=None), dict(frames=0, mode=0x101))
nulls("ctd_costvol_subpixel_f32", "im", "pattern", "idx", "disp")
rows("ctd_costvol_subpixel_f32", "rejected", dict(bs=8), dict(bs=2), dict(bs=4), dict(mode=2), dict(mode=-1), dict(mode=0x100), dict(stride=5),
     dict(stride=-1), dict(stride=5, frames=0), dict(frames=0, mode=2), *(_BAD_VOL1 + _BAD_TYPE))
rows("ctd_costvol_subpixel_f32", "empty", dict(frames=0), dict(frames=0, im=None))

# ---- match validity
_BAD_VALIDITY = [dict(lr_tol=-1), dict(min_gap=-0.5), dict(min_gap=NAN), dict(frames=0, lr_tol=-1), dict(frames=0, min_gap=NAN)]
# frames > 65535, H > 65535, a volume past the int limit (an invalid argument first), and frames * H * W at 2^32 and more
# under a volume below that limit (and the largest pixel count below 2^32, which passes: no workspace then)
_UNSUPPORTED_PIXELS = [dict(frames=65536, H=1, W=4, D=1), dict(H=65536, W=4, D=1, frames=1), dict(frames=1, H=65535, W=65540, D=1),
                       dict(frames=5, H=32768, W=32767, D=1), dict(frames=4, H=32768, W=32768, D=1)]
nulls("ctd_match_validity_f32", "vol", "idx", "flags", "idx_r", "gap")
rows("ctd_match_validity_f32", "rejected", dict(frames=-1), dict(D=0), dict(H=0), dict(W=0), dict(D=128, H=4096, W=4096),
     dict(H=65536, W=4, D=1, frames=1, vol=None), dict(H=65536, W=4, D=1, frames=1, lr_tol=-1), *(_BAD_VALIDITY + _UNSUPPORTED_PIXELS))
rows("ctd_match_validity_f32", "empty", dict(frames=0), dict(frames=0, vol=None))
for _n in ("ctd_xcorrvol_validity_f32", "ctd_costvol_validity_f32"):
    nulls(_n, "idx", "flags", "idx_r", "gap")
    rows(_n, "rejected", dict(algo=2), dict(algo=-1), dict(algo=0x101), dict(stride=5), dict(stride=-1), dict(stride=5, frames=0),
         dict(bs=7, ws=None), dict(bs=2), dict(bs=4), dict(bs=11), dict(bs=11, idx=None), dict(bs=11, ws=None), dict(bs=11, stride=5),
         dict(bs=11, algo=0, ws=None), dict(ws=None), dict(ws_bytes=0), dict(ws_bytes="@need-1"), dict(ws_bytes="@need-1", algo=0),
         dict(ws_bytes="@need-1", stride=512), dict(ws="@ws+128"), dict(ws="@ws+16", ws_bytes="@need"), dict(ws=None, idx=None),
         dict(H=65536, W=4, D=1, frames=1, ws=None), dict(H=65536, W=4, D=1, frames=1, idx=None),
         dict(frames=5, H=32768, W=32767, D=1, ws=None), dict(frames=5, H=32768, W=32767, D=1, idx=None),
         dict(frames=4, H=32768, W=32767, D=1, ws=None), *(_BAD_VALIDITY + _UNSUPPORTED_PIXELS + _BAD_VOL1))
    rows(_n, "empty", dict(frames=0), dict(frames=0, ws=None, idx=None), dict(frames=0, bs=11))
nulls("ctd_xcorrvol_validity_f32", "in0", "in1")
rows("ctd_xcorrvol_validity_f32", "rejected", dict(C=0), dict(C=2), dict(C=2, algo=0, ws=None), dict(C=2, stride=512), dict(C=2, algo=0, stride=512),
     dict(D=512, ws=None), dict(D=513), dict(D=513, algo=0, ws=None), dict(D=513, ws=None), dict(D=513, in0=None))
nulls("ctd_costvol_validity_f32", "im", "pattern")
rows("ctd_costvol_validity_f32", "rejected", dict(frames=8191, H=1, W=4, algo=0, ws=None), dict(frames=8192, H=1, W=4, algo=0),
     dict(frames=8192, H=1, W=4, ws=None), dict(D=513, ws=None), dict(type=0, ws_bytes="@need-1"), dict(type=3, ws_bytes="@need-1"),
     dict(frames=8192, H=1, W=4, algo=0, ws=None), *_BAD_TYPE)

# ---- semi-global aggregation
nulls("ctd_sgm_aggregate_f32", "vol", "idx", "best", "ws")
rows("ctd_sgm_aggregate_f32", "rejected", dict(frames=0), dict(frames=-1), dict(D=0), dict(H=0), dict(W=0), dict(paths=6), dict(paths=0),
     dict(p1=-1.0), dict(p1=NAN), dict(p2=NAN), dict(p1=9.0), dict(p2=INF), dict(p1=INF, p2=INF), dict(frames=1, D=128, H=4096, W=4096),
     dict(frames=1, D=128, H=4096, W=4095, ws=None), dict(D=257), dict(D=257, vol=None), dict(D=257, paths=6), dict(D=257, ws=None),
     dict(D=256, ws=None), dict(ws_bytes=0), dict(ws_bytes="@need-1"), dict(ws="@ws+8"), dict(ws="@ws+4", ws_bytes="@need"),
     dict(frames=0, vol=None), dict(ws=None, idx=None), dict(S_out="@vol+64", D=257), dict(S_out="@vol+64", p1=9.0), dict(S_out="@vol+64", best=None))

# ---- disparity post-filters
_BAD_DISP = [dict(frames=-1), dict(H=0), dict(W=0), dict(H=32768, W=65536, frames=1), dict(frames=2, H=32768, W=32768)]
_BAD_LINK = [dict(max_diff=-1.0), dict(max_diff=NAN), dict(connectivity=6), dict(connectivity=0), dict(frames=0, connectivity=6)]
_BAD_WS = [dict(ws=None), dict(ws_bytes=0), dict(ws_bytes="@need-1"), dict(ws="@ws+8"), dict(ws="@ws+4", ws_bytes="@need")]
nulls("ctd_disp_components_f32", "disp", "label", "size")
rows("ctd_disp_components_f32", "rejected", dict(frames=0, disp=None), dict(ws=None, disp=None), dict(ws=None, connectivity=6),
     *(_BAD_DISP + _BAD_LINK + _BAD_WS))
rows("ctd_disp_components_f32", "empty", dict(frames=0), dict(frames=0, ws=None), dict(frames=0, valid=None))
nulls("ctd_disp_speckle_f32", "disp", "keep")
rows("ctd_disp_speckle_f32", "rejected", dict(max_size=-1), dict(frames=0, max_size=-1), dict(frames=0, keep=None), dict(ws=None, keep=None),
     *(_BAD_DISP + _BAD_LINK + _BAD_WS))
rows("ctd_disp_speckle_f32", "empty", dict(frames=0), dict(frames=0, ws=None, size=None))
nulls("ctd_disp_median_f32", "disp", "out", "valid_out")
rows("ctd_disp_median_f32", "rejected", dict(window=4), dict(window=1), dict(window=9), dict(fill_min=-1), dict(out="@disp+0"), dict(valid_out="@valid+0"),
     dict(frames=0, out="@disp+0"), dict(frames=0, window=4), dict(frames=0, disp=None), dict(window=4, disp=None), *_BAD_DISP)
rows("ctd_disp_median_f32", "empty", dict(frames=0), dict(frames=0, valid=None))

# ---- multi-view depth consistency and fusion (buffers 16 MiB apart; n = B V H W = 768)
_BAD_FUSION = [dict(max_px=-1.0), dict(max_px=INF), dict(max_px=NAN), dict(max_rel=-0.5), dict(max_rel=INF), dict(max_rel=NAN),
               dict(min_views=-1), dict(min_views=256), dict(B=-1), dict(V=0), dict(V=-3), dict(H=0), dict(W=0),
               dict(H=P24 + 1, B=1, V=1, W=1), dict(W=P24 + 1, B=1, V=1, H=1), dict(B=1 << 12, V=64, H=1 << 7, W=1 << 6),
               dict(B=0, max_px=-1.0), dict(B=0, depth=None), dict(V=65, H=0), dict(V=65, depth=None),
               # a written buffer on an input, on another written buffer, and one byte into / past each neighbour
               dict(fused="@depth+0"), dict(keep="@valid+0"), dict(keep="@depth+3071"), dict(count="@keep+0"), dict(count="@keep+767"),
               dict(keep="@count+767"), dict(fused="@R+8"), dict(count="@K+0"), dict(count="@K+35"), dict(keep="@t+71"), dict(fused="@ray+1535"),
               dict(count="@fused+3071")]
_UNSUPPORTED_FUSION = [dict(V=65), dict(V=65, fused="@depth+0"), dict(B=1 << 18, V=64, H=1, W=1), dict(H=P24, B=1, V=1, W=1, fused="@depth+0")]
nulls("ctd_depth_consistency_f32", "depth", "ray", "K", "R", "t", "count", "keep", "fused")
rows("ctd_depth_consistency_f32", "rejected", *(_BAD_FUSION + _UNSUPPORTED_FUSION))
rows("ctd_depth_consistency_f32", "empty", dict(B=0), dict(B=0, valid=None), dict(B=0, fused="@depth+0"))          # (empty spans are absent)
nulls("ctd_depth_fuse_points_f32", "depth", "ray", "K", "R", "t", "points", "src", "n_per_track")
rows("ctd_depth_fuse_points_f32", "rejected", dict(points="@fused+0"), dict(src="@points+0"), dict(src="@points+9215"), dict(n_per_track="@src+8"),
     dict(n_per_track="@src+6143"), dict(ws="@depth+0"), dict(ws="@points+256"), dict(ws="@count-256"), dict(points="@ws+0"), dict(ws=None),
     dict(ws_bytes=0), dict(ws_bytes="@need-1"), dict(ws="@ws+64"), dict(ws="@ws+128", ws_bytes="@need"), dict(ws=None, points=None),
     dict(ws=None, V=65), dict(ws=None, src="@points+0"), *(_BAD_FUSION + _UNSUPPORTED_FUSION))
rows("ctd_depth_fuse_points_f32", "empty", dict(B=0), dict(B=0, ws=None, ws_bytes=0), dict(B=0, count=None, keep=None, fused=None))

# ---- losses
for _n, _p in (("ctd_disp_to_depth_fwd_f32", ("disp", "depth")), ("ctd_idx_to_depth_f32", ("idx", "depth")),
               ("ctd_disp_to_depth_bwd_f32", ("disp", "grad_depth", "grad_disp"))):
    nulls(_n, *_p)
    rows(_n, "rejected", dict(n=-1), {"n": -1, _p[0]: None})
    rows(_n, "empty", dict(n=0), {"n": 0, _p[0]: None})
nulls("ctd_disparity_loss_fwd_f32", "disp", "loss")
nulls("ctd_disparity_loss_bwd_f32", "disp", "grad_loss", "grad_disp")
for _n in ("ctd_disparity_loss_fwd_f32", "ctd_disparity_loss_bwd_f32"):
    rows(_n, "rejected", *_BAD_IMG)
for _n, _p in (("ctd_geometric_fwd_f32", ("loss",)), ("ctd_geometric_sym_fwd_f32", ("loss", "ticket")),
               ("ctd_geometric_bwd_f32", ("grad_loss", "grad_depth0", "grad_depth1"))):
    nulls(_n, "depth0", "depth1", "ray", "K", "R0", "t0", "R1", "t1", *_p)
    rows(_n, "rejected", dict(H=1), dict(W=1), *_BAD_IMG)
nulls("ctd_pattern_loss_fwd_f32", "disp", "im", "pattern", "pattern_proj", "terms", "ws")
nulls("ctd_pattern_loss_bwd_f32", "disp", "im", "pattern", "terms", "grad_val", "grad_disp")
for _n in ("ctd_pattern_loss_fwd_f32", "ctd_pattern_loss_bwd_f32"):
    rows(_n, "rejected", dict(H=1), dict(W=1), dict(type=4, disp=None), *(_BAD_IMG + _BAD_TYPE))
rows("ctd_pattern_loss_fwd_f32", "rejected", dict(ws_bytes=0), dict(ws_bytes="@need-1"), dict(ws=None, type=4), dict(ws=None, terms=None))
_BAD_LEVELS = [dict(n_levels=0), dict(n_levels=-1), dict(n_levels=9), dict(levels=None), {"levels.B": 0}, {"levels.H": 1}, {"levels.W": 1},
               {"levels.disp": 0}, {"levels.im": 0}, {"levels.pattern": 0}, {"levels.B": 1 << 20, "levels.H": 4096, "levels.W": 2048},
               dict(terms=None), dict(terms=None, n_levels=0), dict(type=4, n_levels=0), *_BAD_TYPE]
rows("ctd_pattern_loss_multi_fwd_f32", "rejected", {"levels.pattern_proj": 0}, {"levels.pattern_proj": 0, "ws": None}, dict(ws=None), dict(ws_bytes=0),
     dict(ws_bytes="@need-1"), dict(ws=None, n_levels=0), *_BAD_LEVELS)
rows("ctd_pattern_loss_multi_bwd_f32", "rejected", {"levels.grad_disp": 0}, dict(grad_vals=None), dict(grad_vals=None, n_levels=0), *_BAD_LEVELS)

# ---- nearest neighbours
for _n in ("ctd_nn_f32", "ctd_nn_f64", "ctd_crosscheck"):
    nulls(_n, "in0", "in1", "out")
    rows(_n, "rejected", dict(n0=-1), dict(n1=-1), dict(n0=0, n1=-1), dict(n0=-1, in0=None))
    rows(_n, "empty", dict(n0=0), dict(n0=0, in0=None, out=None), dict(n0=0, n1=0, in1=None))
rows("ctd_nn_f32", "rejected", dict(n1=0, in0=None), dict(n1=0, in1=None, out=None))
for _n in ("ctd_proj_nn_f32", "ctd_proj_nn_f64"):
    nulls(_n, "xyz0", "xyz1", "K", "out")
    rows(_n, "rejected", dict(B=-1), dict(H=0), dict(W=0), dict(patch_size=-1), dict(B=0, H=0), dict(B=-1, K=None))
    rows(_n, "empty", dict(B=0), dict(B=0, K=None))

# ---- rendering
_BAD_CAM = [dict(n_verts=-1), dict(n_faces=-1), dict(cam_w=0), dict(cam_h=0), dict(cam_w=32768, cam_h=21846), dict(cam=None), dict(shader=None),
            dict(verts=None), dict(faces=None), dict(n_faces=-1, cam=None)]
_BAD_PROJ = _BAD_CAM + [dict(proj_w=0), dict(proj_h=0), dict(proj=None), dict(pattern=None), dict(color=None), dict(colors=None),
                        dict(n_faces=0, color=None), dict(n_faces=0, cam_w=0)]
_BAD_PLAIN = _BAD_CAM + [dict(colors=None), dict(normals=None), dict(normals=None, color=None), dict(n_faces=0, cam=None)]
_BAD_BVH = [dict(bvh=None), dict(bvh="@bvh+8"), dict(bvh="@bvh+4"), dict(n_faces=(1 << 28) + 1), dict(n_faces=(1 << 28) + 1, bvh=None),
            dict(bvh=None, cam_w=0), dict(n_faces=0, bvh=None)]
rows("ctd_render_mesh_proj_f32", "rejected", *_BAD_PROJ)
rows("ctd_render_mesh_f32", "rejected", *_BAD_PLAIN)
rows("ctd_render_mesh_proj_bvh_f32", "rejected", *(_BAD_PROJ + _BAD_BVH))
rows("ctd_render_mesh_bvh_f32", "rejected", *(_BAD_PLAIN + _BAD_BVH))
nulls("ctd_mesh_bvh_build_f32", "bvh", "verts", "faces", "ws")
rows("ctd_mesh_bvh_build_f32", "rejected", dict(n_verts=-1), dict(n_faces=-1), dict(n_faces=(1 << 28) + 1), dict(n_verts=0), dict(bvh="@bvh+8"),
     dict(ws="@ws+8"), dict(bvh_bytes=0), dict(bvh_bytes=0, ws_bytes=0), dict(ws_bytes=0), dict(ws_bytes="@need-1"), dict(n_faces=0, bvh=None),
     dict(n_faces=0, bvh_bytes=0, ws=None), dict(n_faces=0, bvh="@bvh+8", ws=None), dict(bvh=None, n_verts=-1), dict(ws=None, bvh_bytes=0),
     dict(bvh="@bvh+8", bvh_bytes=0), dict(ws="@ws+8", ws_bytes=0))

# ---- synthesis
_BAD_SYN = [dict(N=-1), dict(N=65536), dict(H=0), dict(W=0), dict(H=32768, W=21846)]
nulls("ctd_syn_finish_f32", "depth", "color", "normal", "blend", "im", "ambient", "grad")
rows("ctd_syn_finish_f32", "rejected", dict(lcn_radius=-1), dict(N=0, lcn_radius=-1), dict(N=-1, depth=None), *_BAD_SYN)
rows("ctd_syn_finish_f32", "empty", dict(N=0), dict(N=0, depth=None))
nulls("ctd_augment_f32", "img", "params", "out", "minmax")
rows("ctd_augment_f32", "rejected", dict(noise_f64=2), dict(noise_f64=-1), dict(N=0, noise_f64=2), *_BAD_SYN)
rows("ctd_augment_f32", "empty", dict(N=0), dict(N=0, img=None))
nulls("ctd_salt_pepper_f32", "img", "minmax", "counts", "salt", "pepper")
rows("ctd_salt_pepper_f32", "rejected", dict(kmax=-1), dict(N=0, kmax=-1), *_BAD_SYN)
rows("ctd_salt_pepper_f32", "empty", dict(N=0), dict(kmax=0), dict(kmax=0, img=None))

# ---- HyperDepth evaluation and training
nulls("ctd_hyperdepth_eval_f32", "tables", "ims", "out")
rows("ctd_hyperdepth_eval_f32", "rejected", dict(N=-1), dict(H=0), dict(W=0), dict(H=P24, row_to=16), dict(W=P24), dict(row_from=-1), dict(row_from=17),
     dict(row_to=17), dict(n_disp_bins=0), {"tables.n_trees": 0}, {"tables.n_trees": 17}, {"tables.n_classes": 1}, {"tables.n_nodes": -1},
     {"tables.n_leaves": -1}, {"tables.n_entries": -1}, {"tables.max_depth": -1}, {"tables.n_rows": -1}, {"tables.row0": 1}, {"tables.n_rows": 15},
     {"tables.row0": 4, "row_from": 3, "row_to": 10}, {"tables.roots": 0}, {"tables.leaf_off": 0}, {"tables.leaf_sum": 0}, {"tables.nodes": 0},
     {"tables.entries": 0}, {"tables.nodes": (1 << 24) + 8}, {"tables.entries": (5 << 24) + 4}, {"tables.leaf_off": (3 << 24) + 4},
     {"tables.roots": (2 << 24) + 2}, {"tables.leaf_sum": (4 << 24) + 2}, dict(out="@out+2"), {"tables.n_trees": 16, "tables.n_classes": 12289},
     {"tables.n_classes": 15873}, {"tables.n_classes": 15873, "N": 0}, {"tables.n_classes": 15873, "out": "@out+2"}, {"tables.n_classes": 15873, "ims": None},
     dict(N=1 << 20, H=1 << 12, W=32, row_to=16), dict(N=0, H=0), dict(N=0, ims=None), {"N": 0, "tables.n_trees": 0})
rows("ctd_hyperdepth_eval_f32", "empty", dict(N=0), dict(N=0, row_from=16), {"N": 0, "tables.n_nodes": 0, "tables.nodes": 0})
_BAD_HD_SHAPE = [dict(N=0), dict(H=0), dict(W=0), dict(H=P24), dict(W=P24), dict(N=1 << 12, H=1 << 10, W=1 << 9), dict(row_from=-1), dict(row_from=4),
                 dict(row_from=5), dict(row_to=17)]
nulls("ctd_hyperdepth_train_count_f32", "disps", "counts")
rows("ctd_hyperdepth_train_count_f32", "rejected", dict(n_disp_bins=0), dict(W=1 << 16, n_disp_bins=1 << 15, N=1, H=4), *_BAD_HD_SHAPE)
nulls("ctd_hyperdepth_train_f32", "params", "X", "ims", "disps", "row_counts", "ws", "out")
rows("ctd_hyperdepth_train_f32", "rejected", {"params.n_trees": 0}, {"params.n_trees": 17}, {"params.max_tree_depth": 25}, {"params.n_test_samples": 0},
     {"params.n_test_samples": 8193}, {"params.min_samples_for_leaf": 0}, {"params.n_disp_bins": 0}, {"params.n_test_split_functions": 1 << 20},
     {"params.n_test_thresholds": 1 << 16}, {"params.min_samples_to_split": -1}, dict(n_x=16), {"out.roots": 0}, {"out.leaf_off": 0}, {"out.leaf_sum": 0},
     {"out.used": 0}, {"out.cap_nodes": -1}, {"out.cap_leaves": -1}, {"out.cap_entries": -1}, {"out.nodes": 0}, {"out.entries": 0},
     {"out.entries": (5 << 24) + 4}, {"out.leaf_off": (3 << 24) + 4}, {"out.used": (6 << 24) + 4}, dict(X="@X+4"), dict(ws="@ws+128"),
     dict(row_counts=[40, -1, 17, 64]), dict(ws_bytes=0), dict(ws_bytes="@need-1"), dict(ws_bytes=0, n_x=16), dict(ws_bytes=0, row_counts=[40, -1, 17, 64]),
     {"ws_bytes": 0, "out.used": (6 << 24) + 4}, {"ws_bytes": 0, "params.n_trees": 17}, *_BAD_HD_SHAPE)


def _short(v):
    return "[_LEVEL]*%d" % len(v) if isinstance(v, list) and v and all(x == _LEVEL for x in v) else repr(v)


def row_id(func, overrides):
    return "%s(%s)" % (func, ", ".join("%s=%s" % (k, _short(overrides[k])) for k in sorted(overrides)))


_STRUCTS = {"tables": _lib.HdTables, "params": _lib.HdTrainParams, "out": _lib.HdTrainOut, "levels": _lib.PatternLevel}


def _resolved(func, overrides):
    """name -> Python value of one call: base, overrides, made-up addresses, "@name+offset" references"""
    names, base, _ = FUNCS[func]
    names = names.split()
    vals = {}
    for n in names:
        v = base[n]
        vals[n] = [dict(x) for x in v] if isinstance(v, list) and v and isinstance(v[0], dict) else (dict(v) if isinstance(v, dict) else v)
    for k, v in overrides.items():
        if "." in k:
            obj, field = k.split(".")
            for d in (vals[obj] if isinstance(vals[obj], list) else [vals[obj]]):
                assert field in d, k
                d[field] = v
        else:
            assert k in vals, (func, k)
            vals[k] = [dict(x) for x in v] if isinstance(v, list) and v and isinstance(v[0], dict) else v
    addr = {n: (i + 1) << 24 for i, n in enumerate(names)}
    for n in names:
        v = vals[n]
        if v == "p":
            vals[n] = addr[n]
        elif isinstance(v, str) and v.startswith("@") and not v.startswith("@need"):
            other, sign, off = v[1:].partition("+") if "+" in v else v[1:].partition("-")
            vals[n] = addr[other] + int(sign + off)
    return names, vals


def _c_args(names, vals, keep):
    """ctypes arguments of a call (`keep` holds the objects the pointers refer to until the call has returned)"""
    args = []
    for n in names:
        v = vals[n]
        if n in _STRUCTS and isinstance(v, dict):
            v = _STRUCTS[n](**v)
            keep.append(v)
            v = ctypes.byref(v)
        elif n == "levels" and isinstance(v, list):
            v = (_lib.PatternLevel * len(v))(*[_lib.PatternLevel(**d) for d in v])
            keep.append(v)
        elif n == "row_counts" and isinstance(v, list):
            v = (ctypes.c_int64 * len(v))(*v)
            keep.append(v)
        args.append(v)
    return args


def _need(lib, func, vals):
    query, spec = FUNCS[func][2]
    args = []
    for s in spec.split():
        if s == "stride":
            args.append(1 if vals["stride"] else 0)                  # per_frame_pattern of the query
        elif "." in s:
            args.append(vals[s.split(".")[0]][s.split(".")[1]])
        else:
            args.append(vals[s] if s in vals else int(s))
    keep = []
    qnames = FUNCS[query][0].split()
    return getattr(lib, query)(*_c_args(qnames, dict(zip(qnames, args)), keep))


def run(lib):
    """[[row id, answer], ...] of every row of the table; an answer is the returned integer (ctd_xcorrvol_rank_layout: the status
    followed by the five offsets it wrote)"""
    out = []
    for func, overrides, kind in ROWS:
        assert kind in ("query", "rejected", "empty") and (kind == "query") == (func in QUERIES), (func, kind)
        assert kind == "query" or overrides, "the base call of %s would pass validation" % func
        names, vals = _resolved(func, overrides)
        for n in names:
            if isinstance(vals[n], str) and vals[n].startswith("@need"):
                vals[n] = _need(lib, func, vals) + int(vals[n][5:] or 0)
        keep = []
        args = _c_args(names, vals, keep)
        if func == "ctd_xcorrvol_rank_layout":
            off = (ctypes.c_size_t * 5)(*([0] * 5)) if vals["offsets"] == "out5" else None
            args[-1] = off
            answer = [lib.ctd_xcorrvol_rank_layout(*args)] + (list(off) if off is not None else [])
        elif kind == "query":
            answer = getattr(lib, func)(*args)
        else:
            answer = getattr(lib, func)(*(args + [-1, None]))         # device -1: no device switch; no stream
        out.append([row_id(func, overrides), answer])
    return out


if __name__ == "__main__":
    # python -m tests.abi_rejections LIBRARY > tests/golden/abi_rejections.json   (LIBRARY: the libctd_hip.so that defines
    # the contract, i.e. one built from the commit whose answers are to be pinned -- not the code under test)
    import json
    import sys
    lib_ = ctypes.CDLL(sys.argv[1])
    for name_, (res_, args_) in _lib.SIGNATURES.items():
        getattr(lib_, name_).restype, getattr(lib_, name_).argtypes = res_, args_
    print("[\n" + ",\n".join(json.dumps(r) for r in run(lib_)) + "\n]")
