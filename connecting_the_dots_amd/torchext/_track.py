# The checks of a track of posed views, for the wrappers of ctd_hip.h (fusion), ctd_hip_warp.h, _icp.h and _tsdf.h.
import torch

from ._common import _check, _f32, _same_device


def _max_views(V, who):
    if V > 64:
        raise RuntimeError("%s: at most 64 views" % who)


def _depth_views(depth, who):
    """depth [B,V,H,W] with 1 <= V <= 64 -> (B, V, H, W)"""
    if depth.dim() != 4 or min(depth.shape[1:]) == 0:
        raise RuntimeError("%s expects depth [B,V,H,W] with V, H, W >= 1" % who)
    _max_views(depth.shape[1], who)
    return tuple(depth.shape)


def _valid_mask(valid, depth, who):
    """valid (bool or uint8, shaped as depth, or None) as uint8 or None"""
    if valid is None:
        return None
    _check(valid, "valid", (torch.bool, torch.uint8))
    if valid.shape != depth.shape:
        raise RuntimeError("%s: valid must have the shape of depth" % who)
    _same_device(depth, valid)
    return valid.view(torch.uint8)


def _depth_ray_inputs(depth, ray, valid, who):
    """the tensors of a track of views without poses -> (device, valid as uint8 or None)"""
    dev = _same_device(_f32(depth, "depth"), _f32(ray, "ray"))
    B, V, H, W = _depth_views(depth, who)
    if ray.numel() != H * W * 3:
        raise RuntimeError("%s: ray [H*W,3] expected" % who)
    return dev, _valid_mask(valid, depth, who)


def _track_inputs(depth, ray, K, R, t, valid, who):
    """the tensors of a track of posed views -> (device, valid as uint8 or None)"""
    ts = [_f32(x, n) for x, n in ((depth, "depth"), (ray, "ray"), (K, "K"), (R, "R"), (t, "t"))]
    dev = _same_device(*ts)
    B, V, H, W = _depth_views(depth, who)
    if ray.numel() != H * W * 3 or K.numel() != 9 or R.numel() != B * V * 9 or t.numel() != B * V * 3:
        raise RuntimeError("%s: ray [H*W,3], K [3,3], R [B,V,3,3], t [B,V,3] expected" % who)
    return dev, _valid_mask(valid, depth, who)


def _pose_shapes(R, t, who, B=None, V=None, tail=""):
    """R [B,V,3,3] and t [B,V,3] exactly, for the ops that size a launch or an output by them (the other track ops take
    poses by element count) -> (B, V).  B, V: what they must be; V=None: any 1 <= V <= 64.  `tail` ends the message."""
    if not isinstance(R, torch.Tensor) or not isinstance(t, torch.Tensor) or R.dim() != 4 or \
            tuple(R.shape[2:]) != (3, 3) or (B is not None and R.shape[0] != B) or \
            (R.shape[1] == 0 if V is None else R.shape[1] != V) or tuple(t.shape) != tuple(R.shape[:2]) + (3,):
        raise RuntimeError("%s: R must be shaped [B,V,3,3] and t [B,V,3]%s" % (who, tail))
    if V is None:
        _max_views(R.shape[1], who)
    return R.shape[0], R.shape[1]
