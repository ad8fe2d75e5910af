"""CPU-only checks: the C-ABI library loads and exports every symbol that a header under include/ declares, every
ctypes table matches its header in names and in types, host-side argument validation works without a GPU, the Python
surface mirrors the reference's torchext names."""
import ctypes
import glob
import os
import re

import pytest
import torch

from tests.abi_headers import parse_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "ctd_hip.h")


def declared_symbols(header=HEADER):
    src = open(header).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ctd_[a-z0-9_]+)\s*\(", src)))


# ---------------------------------------------------------------------------------------------------------------------
# The whole C interface: every header under include/ against its table of _lib.TABLES and the built library.
# A new entry point needs its prototype in the header, its entry in _lib.TABLES["<header>"] and its name below.
# ---------------------------------------------------------------------------------------------------------------------
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, "*.h")))

EXPECTED = {
    "ctd_hip.h": [
        "ctd_argmax_disp_f32", "ctd_augment_f32", "ctd_costvol_argmin_f32", "ctd_costvol_argmin_workspace_bytes",
        "ctd_costvol_f32", "ctd_costvol_fast_f32", "ctd_costvol_subpixel_f32", "ctd_costvol_validity_f32",
        "ctd_costvol_validity_workspace_bytes", "ctd_costvol_workspace_bytes", "ctd_crosscheck",
        "ctd_depth_consistency_f32", "ctd_depth_fuse_points_f32", "ctd_depth_fuse_workspace_bytes",
        "ctd_disp_components_f32", "ctd_disp_components_workspace_bytes", "ctd_disp_median_f32", "ctd_disp_speckle_f32",
        "ctd_disp_to_depth_bwd_f32", "ctd_disp_to_depth_fwd_f32", "ctd_disparity_loss_bwd_f32",
        "ctd_disparity_loss_fwd_f32", "ctd_disparity_loss_workspace_bytes", "ctd_geometric_bwd_f32",
        "ctd_geometric_fwd_f32", "ctd_geometric_sym_fwd_f32", "ctd_geometric_workspace_bytes", "ctd_hyperdepth_eval_f32",
        "ctd_hyperdepth_train_count_f32", "ctd_hyperdepth_train_f32", "ctd_hyperdepth_train_workspace_bytes",
        "ctd_idx_to_depth_f32", "ctd_lcn_datagen_f32", "ctd_lcn_f32", "ctd_lcn_fast_f32", "ctd_lcn_xcorrvol_argmax_f32",
        "ctd_lcn_xcorrvol_supported", "ctd_match_validity_f32", "ctd_mesh_bvh_build_f32", "ctd_mesh_bvh_bytes",
        "ctd_mesh_bvh_workspace_bytes", "ctd_nn_f32", "ctd_nn_f64", "ctd_pattern_loss_bwd_f32", "ctd_pattern_loss_fwd_f32",
        "ctd_pattern_loss_multi_bwd_f32", "ctd_pattern_loss_multi_fwd_f32", "ctd_pattern_loss_multi_workspace_bytes",
        "ctd_pattern_loss_workspace_bytes", "ctd_photometric_bwd_f32", "ctd_photometric_bwd_f64",
        "ctd_photometric_bwd_fast_f32", "ctd_photometric_fwd_f32", "ctd_photometric_fwd_f64",
        "ctd_photometric_fwd_fast_f32", "ctd_proj_nn_f32", "ctd_proj_nn_f64", "ctd_render_mesh_bvh_f32",
        "ctd_render_mesh_f32", "ctd_render_mesh_proj_bvh_f32", "ctd_render_mesh_proj_f32", "ctd_salt_pepper_f32",
        "ctd_sgm_aggregate_f32", "ctd_sgm_workspace_bytes", "ctd_status_string", "ctd_syn_finish_f32", "ctd_version",
        "ctd_xcorrvol_argmax_f32", "ctd_xcorrvol_argmax_workspace_bytes", "ctd_xcorrvol_f32", "ctd_xcorrvol_f64",
        "ctd_xcorrvol_pattern_prepare_f32", "ctd_xcorrvol_rank_layout", "ctd_xcorrvol_rank_supported",
        "ctd_xcorrvol_subpixel_f32", "ctd_xcorrvol_subpixel_workspace_bytes", "ctd_xcorrvol_validity_f32",
        "ctd_xcorrvol_validity_workspace_bytes", "ctd_xcorrvol_workspace_bytes"],
    "ctd_hip_bench.h": ["ctd_kernel_timing_collect", "ctd_kernel_timing_enable"],
    "ctd_hip_band.h": ["ctd_costvol_argmin_band_f32", "ctd_xcorrvol_argmax_band_f32",
                       "ctd_xcorrvol_argmax_band_workspace_bytes"],
    "ctd_hip_warp.h": ["ctd_depth_warp_f32", "ctd_depth_warp_workspace_bytes", "ctd_disparity_band_window_f32"],
    "ctd_hip_band_validity.h": ["ctd_costvol_band_validity_f32", "ctd_xcorrvol_band_validity_f32"],
    "ctd_hip_icp.h": ["ctd_depth_icp_system_f32", "ctd_depth_icp_update_f32", "ctd_depth_icp_workspace_bytes",
                      "ctd_depth_normals_f32"],
    "ctd_hip_tsdf.h": ["ctd_tsdf_integrate_f32", "ctd_tsdf_raycast_f32", "ctd_tsdf_surface_points_f32",
                       "ctd_tsdf_surface_workspace_bytes"],
    "ctd_hip_mesh.h": ["ctd_tsdf_mesh_case", "ctd_tsdf_mesh_faces_i32", "ctd_tsdf_mesh_workspace_bytes"],
    "ctd_hip_mesh_clean.h": ["ctd_mesh_clean_i32", "ctd_mesh_clean_workspace_bytes", "ctd_mesh_components_i32"],
    "ctd_hip_mesh_dist.h": ["ctd_point_mesh_distance_f32"],
    "ctd_hip_mesh_color.h": ["ctd_mesh_view_colors_f32"],
    "ctd_hip_mesh_smooth.h": ["ctd_mesh_adjacency_i32", "ctd_mesh_adjacency_workspace_bytes", "ctd_mesh_smooth_f32",
                              "ctd_mesh_smooth_workspace_bytes", "ctd_mesh_vertex_normals_f32"],
    "ctd_hip_mesh_simplify.h": ["ctd_mesh_simplify_f32", "ctd_mesh_simplify_workspace_bytes"],
    "ctd_hip_mesh_sdf.h": ["ctd_point_mesh_signed_f32"],
}

C_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
             "size_t": ctypes.c_size_t, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64}
# struct of ctd_hip.h -> (its mirror in _lib, the size that the header's comment states)
MIRRORS = {"ctd_pattern_level": ("PatternLevel", None), "ctd_hd_tables": ("HdTables", 88),
           "ctd_hd_train_params": ("HdTrainParams", 48), "ctd_hd_train_out": ("HdTrainOut", 72)}

# What belongs to a header besides its file name and its functions: prefixes of its names and of its macros.  No header
# that came before it may hold one of these, in its prose either (test_a_header_names_only_what_came_before_it).
OWN_WORDS = {
    "ctd_hip_band.h": ["ctd_band"],
    "ctd_hip_warp.h": ["ctd_depth_warp"],
    "ctd_hip_icp.h": ["ctd_icp"],
    "ctd_hip_tsdf.h": ["ctd_tsdf"],
    "ctd_hip_mesh.h": ["ctd_tsdf_mesh"],
    "ctd_hip_mesh_clean.h": ["ctd_mesh_clean", "ctd_mesh_components"],
    "ctd_hip_mesh_dist.h": ["ctd_point_mesh"],
    "ctd_hip_mesh_color.h": ["ctd_mesh_view_colors"],
    "ctd_hip_mesh_smooth.h": ["ctd_mesh_adjacency", "ctd_mesh_smooth", "ctd_mesh_vertex_normals",
                              "CTD_MESH_ADJ_MAX_INCIDENT", "CTD_MESH_VERT_"],
    "ctd_hip_mesh_simplify.h": ["CTD_MESH_SIMPLIFY_"],
    "ctd_hip_mesh_sdf.h": ["ctd_point_mesh_signed"],
}


def _matches(ctype, declared, mirrors):
    """whether the table's ctypes type passes what the header declares ('int', 'float*', 'ctd_hd_tables*', ...)"""
    if not declared.endswith("*"):
        return ctype is C_SCALARS[declared]
    if ctype in (ctypes.c_void_p, ctypes.c_char_p):
        return True
    if not (isinstance(ctype, type) and issubclass(ctype, ctypes._Pointer)):
        return False
    pointee = declared[:-1]
    return ctype._type_ is (mirrors[pointee] if pointee in mirrors else C_SCALARS.get(pointee))


@pytest.mark.parametrize("header", HEADERS)
def test_header_matches_table_and_library(header):
    """Names, return types and every parameter of the header's prototypes against _lib.TABLES[header], position by
    position; the structs that _lib mirrors; the library's exports; what lib() bound."""
    from connecting_the_dots_amd import _lib
    from connecting_the_dots_amd import build
    build.build()
    assert HEADERS == sorted(_lib.TABLES) == sorted(EXPECTED)          # no header without a table, no table without one
    table = _lib.TABLES[header]
    functions, structs = parse_header(os.path.join(INCLUDE, header))
    assert sorted(functions) == sorted(table) == EXPECTED[header] == declared_symbols(os.path.join(INCLUDE, header))
    mirrors = {c: getattr(_lib, py) for c, (py, _) in MIRRORS.items()}
    exported, bound = ctypes.CDLL(_lib.LIB_PATH), _lib.lib()
    for name, (ret, params) in functions.items():
        res, args = table[name]
        assert res is dict(C_SCALARS, **{"void": None, "char*": ctypes.c_char_p})[ret], "%s returns %s, the table has %s" % (name, ret, res)
        assert len(args) == len(params), "%s takes %d parameters, the table has %d" % (name, len(params), len(args))
        for i, (ctype, declared) in enumerate(zip(args, params)):
            assert _matches(ctype, declared, mirrors), "%s, parameter %d: %s in the header, %s in the table" % (
                name, i, declared, ctype)
        assert hasattr(exported, name), "libctd_hip.so does not export %s" % name
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype == res, name
    text = open(os.path.join(INCLUDE, header)).read()
    for cname in sorted(set(structs) & set(MIRRORS)):
        mirror, size = mirrors[cname], MIRRORS[cname][1]
        fields = [(f, ctypes.c_void_p if t.endswith("*") else C_SCALARS[t]) for f, t in structs[cname]]
        assert fields == list(mirror._fields_), "%s: fields of %s against %s" % (cname, header, mirror.__name__)
        stated = re.search(r"\}\s*%s;\s*/\*\s*(\d+) bytes" % cname, text)
        assert (int(stated.group(1)) if stated else None) == size and size in (None, ctypes.sizeof(mirror)), cname
    if header == "ctd_hip.h":
        assert set(MIRRORS) <= set(structs)
        assert not any("timing" in n for n in functions)               # the measurement hooks are in ctd_hip_bench.h
        assert bound.ctd_version() == 5
        assert bound.ctd_status_string(1) == b"invalid argument"


def test_every_function_has_one_header_and_one_table():
    from connecting_the_dots_amd import _lib
    declared = [n for h in HEADERS for n in parse_header(os.path.join(INCLUDE, h))[0]]
    tabled = [n for table in _lib.TABLES.values() for n in table]
    assert len(declared) == len(set(declared)) and len(tabled) == len(set(tabled)) and sorted(declared) == sorted(tabled)
    for h in HEADERS:                                                 # of the project's headers only ctd_hip.h is included
        included = re.findall(r'#\s*include\s*"([^"]+)"', open(os.path.join(INCLUDE, h)).read())
        assert set(included) <= ({"ctd_hip.h"} if h != "ctd_hip.h" else set()), (h, included)


def test_a_header_names_only_what_came_before_it():
    """Each header was added beside the ones that existed and left them alone: no header holds, in code or in prose, the
    file name, a function or an own word (OWN_WORDS) of a header that follows it in _lib.TABLES.  ctd_hip.h says where
    its measurement hooks went, and ctd_hip_mesh_simplify.h names nothing but ctd_hip.h."""
    from connecting_the_dots_amd import _lib
    order = list(_lib.TABLES)
    may_name = {h: set(order[:i]) for i, h in enumerate(order)}
    may_name["ctd_hip.h"] = {"ctd_hip_bench.h"}
    may_name["ctd_hip_mesh_simplify.h"] = {"ctd_hip.h"}
    for h in order:
        text = open(os.path.join(INCLUDE, h)).read()
        for other in set(order) - may_name[h] - {h}:
            for word in [other] + sorted(_lib.TABLES[other]) + OWN_WORDS.get(other, []):
                assert word not in text, "%s holds %s of %s" % (h, word, other)


def test_workspace_query_and_validation_need_no_gpu():
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    assert L.ctd_xcorrvol_workspace_bytes(16, 1, 432, 512, 128, 9, 0) > 0
    assert L.ctd_xcorrvol_workspace_bytes(16, 1, 432, 512, 128, 9, 1) >= L.ctd_xcorrvol_workspace_bytes(16, 1, 432, 512, 128, 9, 0)
    assert L.ctd_xcorrvol_workspace_bytes(1, 1, 0, 512, 128, 9, 0) == 0
    # invalid sizes are rejected before any HIP call
    assert L.ctd_xcorrvol_f32(None, None, 0, None, 1, 1, -4, 8, 8, 9, 0, None, 0, -1, None) == 1
    assert L.ctd_lcn_f32(None, None, None, 1, 8, 8, 8, 0.05, -1, None) == 1          # radius >= H
    assert L.ctd_photometric_fwd_f32(None, None, None, 1, 1, 8, 8, 9, 7, 0.5, -1, None) == 1   # bad type
    # 2^31 outputs exceed the reference's int indexing (common_cuda.h:65-66)
    assert L.ctd_xcorrvol_f32(None, None, 0, None, 1, 1, 4096, 4096, 128, 9, 0, None, 0, -1, None) == 1


def test_python_surface_mirrors_reference_names():
    from connecting_the_dots_amd import torchext as te
    for name in ("nn", "NNFunction", "crosscheck", "CrossCheckFunction", "proj_nn", "ProjNNFunction", "xcorrvol",
                 "XCorrVolFunction", "photometric_loss", "PhotometricLossFunction", "photometric_loss_pytorch",
                 "CoordConv2d"):
        assert hasattr(te, name), name
    for name in ("xcorrvol_batch", "xcorrvol_argmax", "argmax_disp", "lcn", "LCN", "costvol", "disp_to_depth",
                 "disparity_loss", "geometric_loss", "DispToDepth", "DisparityLoss", "ProjectionDepthSimilarityLoss",
                 "RectifiedPatternSimilarityLoss"):
        assert hasattr(te, name), name


def test_cpu_tensors_are_rejected_loudly():
    from connecting_the_dots_amd import torchext as te
    x = torch.rand(1, 8, 8)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        te.xcorrvol(x, x, 4, 9)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        te.photometric_loss(x[None], x[None], 9)
    with pytest.raises(Exception, match="invalid loss type"):
        te.photometric_loss(x[None], x[None], 9, "nope")


def test_photometric_pytorch_formulation_matches_oracle(oracle):
    """photometric_loss_pytorch runs on CPU tensors (stock ops) and agrees with the oracle."""
    import numpy as np
    from connecting_the_dots_amd import torchext as te
    from tests.util import assert_close
    rs = np.random.RandomState(3)
    es, ta = rs.rand(1, 2, 12, 14), rs.rand(1, 2, 12, 14)
    for ty, name in enumerate(("mse", "sad", "census_mse", "census_sad")):
        got = te.photometric_loss_pytorch(torch.from_numpy(es), torch.from_numpy(ta), 9, name, 0.5).numpy()
        assert_close(got, oracle.photometric_fwd(es, ta, 9, ty, 0.5), rtol=1e-10, atol=1e-12, what=name)


def test_coordconv_grid():
    from connecting_the_dots_amd import torchext as te
    m = te.CoordConv2d(1, 2, 3, 1, 1)
    y = m(torch.zeros(2, 1, 5, 7))
    assert y.shape == (2, 2, 5, 7)
    assert m.uv.shape == (1, 2, 5, 7)
    assert float(m.uv[0, 0, 0, 0]) == -1 and float(m.uv[0, 0, 0, -1]) == 1       # u spans [-1, 1] (modules.py:19)
    assert float(m.uv[0, 1, 0, 0]) == -1 and float(m.uv[0, 1, -1, 0]) == 1


def test_all_d_plan_of_the_benchmark_shapes():
    """Host logic of the ranked argmax (no GPU work): how the all-D kernel cuts the BASELINE shapes -- band height and
    passes over the disparities (ctd_xcorrvol_rank_layout offsets[0] / [4]) -- and that its workspace query covers it."""
    import ctypes
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    off = (ctypes.c_size_t * 5)()
    assert L.ctd_xcorrvol_rank_layout(16, 432, 512, 128, 0, off) == 0
    assert (off[0], off[4]) == (54, 5)             # config 2: one round of 256 workgroups, 5 passes of 26 disparities
    assert L.ctd_xcorrvol_rank_layout(1, 1024, 1024, 256, 0, off) == 0
    assert (off[0], off[4]) == (16, 9)             # config 4: 64 bands x 4 tiles = 256 workgroups, 9 passes
    assert L.ctd_xcorrvol_rank_layout(1, 9, 4, 1, 0, off) == 0 and 1 <= off[0] <= 9 and off[4] == 1
    assert L.ctd_xcorrvol_rank_supported(1, 432, 512, 128, 9) == 1
    assert L.ctd_xcorrvol_rank_supported(1, 432, 510, 128, 9) == 0      # W % 4
    assert L.ctd_xcorrvol_rank_supported(1, 432, 512, 600, 9) == 0      # D > 512
    need = L.ctd_xcorrvol_argmax_workspace_bytes(16, 1, 432, 512, 128, 9, 1)
    assert need >= L.ctd_xcorrvol_workspace_bytes(16, 1, 432, 512, 128, 9, 1) > 0


def test_ticket_words_are_cleared_when_a_launch_returns_an_error():
    """A launch that takes its ticket words at zero and fails must not leave them dirty for the next call."""
    from connecting_the_dots_amd.torchext import _common as F
    ticket = torch.zeros(128, dtype=torch.int32)

    def failing(tk):
        tk[3] = 7                                            # what an aborted launch may leave behind
        return 2                                             # CTD_ERR_WORKSPACE
    with pytest.raises(RuntimeError, match="workspace"):
        F._call_with_ticket(failing, ticket, "geometric_loss")
    assert int(ticket.abs().sum()) == 0
    F._call_with_ticket(lambda tk: 0, ticket, "geometric_loss")   # a good call passes straight through


def test_kernel_timing_state_is_per_thread():
    """The measurement hooks keep their state per calling thread: enabling them in one thread does not instrument (or
    race with) launches of another.  Without a GPU: collect() in a thread that never enabled them reports nothing."""
    import threading
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    seen = {}

    def other():
        seen["n"] = L.ctd_kernel_timing_collect(None, None)
    t = threading.Thread(target=other)
    t.start()
    t.join()
    assert seen["n"] == 0
