"""The definition of band-limited matching (include/ctd_hip_band.h) restated with torch on the CPU: given the
reference-order volume, the masked first-index argmax / argmin of every pixel over its own range [lo, hi]."""
import torch


def band_ref(vol, lo, hi, maximise):
    """vol f32 [N,D,H,W], lo / hi integer [N,H,W] (inclusive, clipped here to [0, D-1]) ->
    (idx int64 [N,H,W], best f32 [N,H,W]): the first index of the best vol[n,d,h,w] over d in [lo', hi'] and its value;
    -1 and NaN where the clipped band is empty.  A running best in ascending d with a strict compare."""
    vol = vol.detach().cpu()
    N, D, H, W = vol.shape
    lo = lo.detach().cpu().to(torch.int64).clamp(min=0)
    hi = hi.detach().cpu().to(torch.int64).clamp(max=D - 1)
    assert lo.shape == (N, H, W) and hi.shape == (N, H, W)
    idx = torch.full((N, H, W), -1, dtype=torch.int64)
    best = torch.full((N, H, W), float("nan"), dtype=torch.float32)
    for d in range(D):
        v = vol[:, d]
        better = (v > best) if maximise else (v < best)
        take = (lo <= d) & (d <= hi) & ((idx < 0) | better)
        idx = torch.where(take, torch.full_like(idx, d), idx)
        best = torch.where(take, v, best)
    return idx, best
