"""Mirror of the reference's `torchext/functions.py` on top of libctd_hip.so.

Same names, argument meaning, autograd contract and error behaviour as the reference
(torchext/functions.py:1-147); every op takes CUDA(=HIP) tensors that are contiguous and
launches on the caller's current stream and the tensor's device.  There is no CPU path in
this package: CPU tensors raise (the reference's CPU path is `ext_cpu`, which lives on as
the test oracle only).

Additive API (no reference counterpart): `xcorrvol_batch`, `argmax_disp`,
`xcorrvol_argmax`, `lcn`, ... and the keyword `algo` of the ops that have two kernel families:
    'fast'  (default) tolerance-level kernels, |a-b| <= 1e-5*|b| + 1e-6 against the reference (LDS-tiled, HBM- or
            issue-bound; f32 and odd block sizes up to 9 -- anything else runs the reference-order kernels); the NCC
            volume of C > 1 channels is within the sum of that bound over its per-channel NCCs, 1e-5 * sum_c |b_c| +
            C * 1e-6 (include/ctd_hip.h);
    'exact' the reference's operation order, bit-identical to its CPU build (the parity anchor).
The default can be changed with the environment variables CTD_NCC_ALGO (xcorrvol family) and CTD_PHOTO_ALGO
(photometric loss, cost volumes, pattern similarity loss).
"""
from .nn_ops import CrossCheckFunction, NNFunction, ProjNNFunction, crosscheck, nn, proj_nn
from .ncc import (PreparedPattern, XCorrVolFunction, argmax_disp, prepare_pattern, xcorrvol, xcorrvol_argmax,
                  xcorrvol_batch)
from .lcn_ops import lcn, lcn_normalize, lcn_xcorrvol_argmax
from .photometric import (PatternLossFunction, PatternLossMultiFunction, PhotometricLossFunction, pattern_loss,
                          pattern_loss_multi, photometric_loss, photometric_loss_pytorch)
from .costvol_ops import costvol, costvol_argmin
from .subpixel import costvol_subpixel, xcorrvol_subpixel
from .validity import VALID_IN_PATTERN, VALID_LR_OK, VALID_UNIQUE, costvol_validity, match_validity, xcorrvol_validity
from .band import (costvol_argmin_band, costvol_band_validity, disparity_band, xcorrvol_argmax_band,
                   xcorrvol_band_validity)
from .sgm import costvol_sgm, sgm_aggregate, xcorrvol_sgm
from .disp_filter import disp_components, disp_median, disp_speckle, disparity_filter
from .multiview import (depth_consistency, depth_fuse_points, depth_icp, depth_icp_system, depth_icp_update,
                        depth_normals, depth_to_disp, depth_warp, disparity_band_window)
from .tsdf import tsdf_integrate, tsdf_raycast, tsdf_surface_points, tsdf_volume
from .losses import (DispToDepthFunction, DisparityLossFunction, GeometricLossFunction, disp_to_depth, disparity_loss,
                     geometric_loss, idx_to_depth)

__all__ = [
    "CrossCheckFunction", "NNFunction", "ProjNNFunction", "crosscheck", "nn", "proj_nn", "PreparedPattern",
    "XCorrVolFunction", "argmax_disp", "prepare_pattern", "xcorrvol", "xcorrvol_argmax", "xcorrvol_batch", "lcn",
    "lcn_normalize", "lcn_xcorrvol_argmax", "PatternLossFunction", "PatternLossMultiFunction",
    "PhotometricLossFunction", "pattern_loss", "pattern_loss_multi", "photometric_loss", "photometric_loss_pytorch",
    "costvol", "costvol_argmin", "costvol_subpixel", "xcorrvol_subpixel", "VALID_IN_PATTERN", "VALID_LR_OK",
    "VALID_UNIQUE", "costvol_validity", "match_validity", "xcorrvol_validity", "costvol_argmin_band",
    "costvol_band_validity", "disparity_band", "xcorrvol_argmax_band", "xcorrvol_band_validity", "costvol_sgm",
    "sgm_aggregate", "xcorrvol_sgm", "disp_components", "disp_median", "disp_speckle", "disparity_filter",
    "depth_consistency", "depth_fuse_points", "depth_icp", "depth_icp_system", "depth_icp_update", "depth_normals",
    "depth_to_disp", "depth_warp", "disparity_band_window", "tsdf_integrate", "tsdf_raycast", "tsdf_surface_points",
    "tsdf_volume", "DispToDepthFunction", "DisparityLossFunction", "GeometricLossFunction", "disp_to_depth",
    "disparity_loss", "geometric_loss", "idx_to_depth",
]
