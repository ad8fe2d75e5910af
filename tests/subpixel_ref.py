"""The sub-pixel rule of include/ctd_hip.h restated with torch on the CPU (a module, not a test), shared by
tests/test_subpixel_gpu.py and the chain tests.  In float32 (the default) it is the rule bit for bit; dtype=float64
evaluates the same expressions on float64 scores."""
import torch


def fit_reference(vol, idx, maximum, mode, dtype=torch.float32):
    """vol [N,D,H,W], idx [N,H,W] -> (disp, refined u8)"""
    vol, idx = vol.detach().cpu().to(dtype), idx.detach().cpu()
    D = vol.shape[1]
    valid = (idx >= 0) & (idx < D)
    inner = valid & (idx > 0) & (idx < D - 1)
    ic = idx.clamp(0, D - 1)

    def at(k):
        return vol.gather(1, (ic + k).clamp(0, D - 1).unsqueeze(1)).squeeze(1)

    m, z, p = at(-1), at(0), at(1)
    half = torch.tensor(0.5, dtype=dtype)
    if maximum:
        if mode == "parabola":
            den = (m - z) + (p - z)
            ok = den < 0
            delta = half * ((m - p) / den)
        else:
            q = torch.where(p > m, z - m, z - p)
            ok = q > 0
            delta = half * ((p - m) / q)
    else:
        if mode == "parabola":
            den = (m - z) + (p - z)
            ok = den > 0
            delta = half * ((m - p) / den)
        else:
            q = torch.where(p < m, m - z, p - z)
            ok = q > 0
            delta = half * ((m - p) / q)
    ok = ok & inner
    d = ic.to(dtype)
    disp = torch.where(ok, d + delta.clamp(-0.5, 0.5), d)
    disp = torch.where(valid, disp, torch.tensor(float("nan"), dtype=dtype))
    return disp, ok.to(torch.uint8)
