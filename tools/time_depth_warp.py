"""Times forward depth warping and the windowed band (csrc/depth_warp.hip) and writes profiles/depth_warp.txt:
  - depth_warp at 4 tracks x 4 views x 432 x 512 (the clean scene of tests/fusion_ref.py), splat 0 and 1, into every
    view and into one view (views 0..2 into view 3), with each call's compulsory bytes;
  - disparity_band_window at 16 x 432 x 512 on the warped disparity, windows 1, 3 and 7, and beside it, as context, the
    same band built in torch from max_pool2d on +-prior (checked equal before it is timed);
  - the chain warp -> depth_to_disp -> disparity_band_window -> xcorrvol_argmax_band (radius 1, prepared pattern) at
    BASELINE config 2 (16 x 432 x 512, D 128, block 9), step by step and as one (holes "full"; the matcher also on the
    holes "empty" band), beside xcorrvol_argmax (fast, prepared), the full search that profiles/band_match.txt records.
    python tools/time_depth_warp.py [--reps 30] [--out profiles/depth_warp.txt]
Device time from HIP events around each call, after warm-up calls; median / min / max over the repetitions."""
import argparse
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import fusion_ref, workloads  # noqa: E402

SHAPE = (4, 4, 432, 512)                                       # B, V, H, W: 16 views = the 16 frames of config 2
BF, D, BS = 100.0, 128, 9                                      # depths 1.8 .. 2.7 -> disparities 37 .. 56


def median_ms(fn, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times)), float(np.max(times))


def band_from_max_pool(prior, radius, n_disps, window, holes):
    """disparity_band_window in stock torch: max_pool2d pads with -inf, which is what a hole is on both signs"""
    finite = torch.isfinite(prior)
    ninf = torch.full_like(prior, float("-inf"))
    k = window // 2
    M = torch.nn.functional.max_pool2d(torch.where(finite, prior, ninf)[:, None], window, 1, k)[:, 0]
    m = -torch.nn.functional.max_pool2d(torch.where(finite, -prior, ninf)[:, None], window, 1, k)[:, 0]
    some = M > float("-inf")
    lo = torch.ceil(torch.where(some, m, torch.zeros_like(m)) - radius).clamp(0, n_disps)
    hi = torch.floor(torch.where(some, M, torch.zeros_like(M)) + radius).clamp(-1, n_disps - 1)
    full = holes == "full"
    lo = torch.where(some, lo, torch.full_like(lo, 0 if full else n_disps)).to(torch.int32)
    hi = torch.where(some, hi, torch.full_like(hi, n_disps - 1 if full else -1)).to(torch.int32)
    return lo, hi


def recorded_full_search():
    """the full search's median as profiles/band_match.txt holds it (tools/time_band_match.py wrote the line)"""
    path = os.path.join(ROOT, "profiles", "band_match.txt")
    try:
        m = re.search(r"^xcorrvol_argmax fast, prepared\s+([0-9.]+) /", open(path).read(), re.M)
    except OSError:
        m = None
    return "profiles/band_match.txt has it at %s ms" % m.group(1) if m else "profiles/band_match.txt does not have it"


def report(shape, reps, warmup=10, n_disps=D, block=BS):
    """the text of profiles/depth_warp.txt for one shape"""
    B, V, H, W = shape
    n, N = B * V * H * W, B * V
    sc = fusion_ref.make_scene("clean", B, V, H, W, 1)
    t_in = [torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "ray", "K", "R", "t", "valid")]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s.rstrip())

    say("forward depth warping and the windowed band: %d tracks x %d views x %dx%d (clean scene of tests/fusion_ref.py)"
        % (B, V, W, H))
    say("device %s; median / min / max of %d calls (device time, HIP events), after %d warm-up calls"
        % (torch.cuda.get_device_name(0), reps, warmup))
    say()
    say("depth_warp (memset of the keys + warp_scatter_kernel + warp_resolve_kernel), z and src returned")
    say("compulsory bytes: 8 B key set + per source pixel 5 B depth / valid (+ 12 B ray per plane pixel) + per candidate 8 B "
        "key read and up to 8 B atomic + per output pixel 8 B key read, 12 B z and src written")
    fmt = "%-52s %8.4f / %8.4f / %8.4f ms   %s"
    one_s = torch.zeros(B, V, dtype=torch.bool, device="cuda")
    one_s[:, :V - 1] = True
    one_t = torch.zeros(B, V, dtype=torch.bool, device="cuda")
    one_t[:, V - 1] = True
    for splat in (0, 1):
        for what, kw, pairs in (("into every view", {}, V * (V - 1)), ("views 0..%d into view %d" % (V - 2, V - 1),
                                                                        dict(sources=one_s, targets=one_t), V - 1)):
            z = te.depth_warp(*t_in, splat=splat, **kw)
            tgt = z if not kw else z[:, V - 1]
            cand = B * pairs * H * W * (2 * splat + 1) ** 2
            nbytes = 8 * n + 5 * n + 12 * H * W + 16 * cand + 20 * n
            note = "%5.1f %% holes in the targets, <= %.0f MB (%d candidates at most)" % (
                100.0 * float(torch.isnan(tgt).float().mean()), nbytes / 1e6, cand)
            t = median_ms(lambda: te.depth_warp(*t_in, splat=splat, return_src=True, **kw), reps, warmup)
            say(fmt % (("depth_warp splat %d, %s" % (splat, what),) + t + (note,)))
    say()

    z = te.depth_warp(*t_in, splat=1)
    prior = te.depth_to_disp(z, BF).view(N, H, W)
    say("disparity_band_window on the warped disparity (splat 1), %d x %dx%d, radius 1, D %d, holes full; 12 B / pixel compulsory "
        "= %.1f MB" % (N, W, H, n_disps, 12 * n / 1e6))
    for window in (1, 3, 7):
        lo, hi = te.disparity_band_window(prior, 1.0, n_disps, window, "full")
        rlo, rhi = band_from_max_pool(prior, 1.0, n_disps, window, "full")
        same = bool(torch.equal(lo, rlo)) and bool(torch.equal(hi, rhi))
        t = median_ms(lambda: te.disparity_band_window(prior, 1.0, n_disps, window, "full"), reps, warmup)
        say(fmt % (("disparity_band_window window %d" % window,) + t + ("mean width %.2f" % float((hi - lo + 1).float().mean()),)))
        t = median_ms(lambda: band_from_max_pool(prior, 1.0, n_disps, window, "full"), reps, warmup)
        say(fmt % (("  torch, max_pool2d on +-prior, window %d" % window,) + t + ("== the kernel: %s" % ("yes" if same else "NO"),)))
    say()

    say("the chain at config 2 (%d x %dx%d, D %d, block %d, shared pattern; the bench's LCN'd synthetic frames): every view from "
        "the other views of its track, splat 1, window 3, radius 1" % (N, W, H, n_disps, block))
    rs = np.random.RandomState(2)
    pat = workloads.syn_dot_pattern(H, W, seed=42)
    raw = torch.from_numpy(np.stack([workloads.synth_ir(pat, rs, n_disps)[0] for _ in range(N)])[:, None]).cuda()
    x = te.lcn(raw, 5, 0.05)[0]
    p = te.lcn(torch.from_numpy(pat[None, None]).cuda(), 5, 0.05)[0][0].contiguous()
    h = te.prepare_pattern(p, N, n_disps, block)
    lo, hi = te.disparity_band_window(prior, 1.0, n_disps, 3, "full")
    te.xcorrvol_argmax_band(x, p, lo, hi, n_disps, block, prepared=h)

    def chain():
        zz = te.depth_warp(*t_in, splat=1)
        l, u = te.disparity_band_window(te.depth_to_disp(zz, BF).view(N, H, W), 1.0, n_disps, 3, "full")
        return te.xcorrvol_argmax_band(x, p, l, u, n_disps, block, prepared=h)

    width = "mean width %.2f, %.2f %% of the pixels search everything" % (
        float((hi - lo + 1).float().mean()), 100.0 * float(((lo == 0) & (hi == n_disps - 1)).float().mean()))
    say(fmt % (("depth_warp splat 1 (z only)",) + median_ms(lambda: te.depth_warp(*t_in, splat=1), reps, warmup) + ("",)))
    say(fmt % (("depth_to_disp (torch)",) + median_ms(lambda: te.depth_to_disp(z, BF), reps, warmup) + ("",)))
    say(fmt % (("disparity_band_window window 3",) + median_ms(
        lambda: te.disparity_band_window(prior, 1.0, n_disps, 3, "full"), reps, warmup) + (width,)))
    say(fmt % (("xcorrvol_argmax_band on that band, prepared",) + median_ms(
        lambda: te.xcorrvol_argmax_band(x, p, lo, hi, n_disps, block, prepared=h), reps, warmup) + ("",)))
    lo_e, hi_e = te.disparity_band_window(prior, 1.0, n_disps, 3, "empty")
    some = lo_e <= hi_e
    say(fmt % (("  the same with holes=\"empty\"",) + median_ms(
        lambda: te.xcorrvol_argmax_band(x, p, lo_e, hi_e, n_disps, block, prepared=h), reps, warmup) + (
            "mean width %.2f where not empty, %.2f %% of the pixels search nothing" % (
                float((hi_e - lo_e + 1)[some].float().mean()), 100.0 * float((~some).float().mean())),)))
    t_chain = median_ms(chain, reps, warmup)
    say(fmt % (("the four as one chain",) + t_chain + ("",)))
    t_full = median_ms(lambda: te.xcorrvol_argmax(x, p, n_disps, block, prepared=h), reps, warmup)
    say(fmt % (("xcorrvol_argmax fast, prepared (the full search)",) + t_full + (recorded_full_search(),)))
    say("chain / full search = %.2f" % (t_chain[0] / t_full[0]))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_warp.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_depth_warp.py needs a GPU"
    text = report(SHAPE, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
