"""Times band-limited matching against the full search at BASELINE config 2 (16 x 432 x 512, D 128, block 9, shared
pattern; the bench's LCN'd synthetic frames against the LCN'd dot pattern) and writes profiles/band_match.txt:
  - xcorrvol_argmax_band (prepared pattern) with prior = the full matcher's own indices + seeded integer noise in
    [-r, r] and band = disparity_band(prior, r), r = 1, 2, 4, 8, 16, beside xcorrvol_argmax (fast, prepared);
  - costvol_argmin_band(sad) on the same bands beside costvol_argmin(sad);
  - each kernel's compulsory bytes (inputs read once, outputs written once) beside its time;
  - frame 0 of every band result checked against the masked argmax of the exact volume (tests/band_ref.py).
    python tools/time_band_match.py [--reps 30] [--out profiles/band_match.txt]
Device time from HIP events around each call, after warm-up launches; median / min / max over the repetitions."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import workloads  # noqa: E402
from tests.band_ref import band_ref  # noqa: E402

RADII = (1, 2, 4, 8, 16)


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


def bands_around(idx, r, D, seed):
    g = torch.Generator().manual_seed(seed)
    noise = torch.randint(-r, r + 1, idx.shape, generator=g).to(idx.device)
    return te.disparity_band((idx + noise).float(), float(r), D)


def frame0_ok(out, vol0, lo, hi, maximise):
    ridx, rbest = band_ref(vol0, lo[:1], hi[:1], maximise)
    return bool(torch.equal(out[0][:1].cpu(), ridx)) and bool(torch.equal(out[1][:1].cpu().view(torch.int32),
                                                                          rbest.view(torch.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_match.txt"))
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    N, H, W, D, BS = 16, 432, 512, 128, 9
    rs = np.random.RandomState(2)
    pat = workloads.syn_dot_pattern(H, W, seed=42)
    raw = torch.from_numpy(np.stack([workloads.synth_ir(pat, rs, D)[0] for _ in range(N)])[:, None]).cuda()
    x = te.lcn(raw, 5, 0.05)[0]
    p = te.lcn(torch.from_numpy(pat[None, None]).cuda(), 5, 0.05)[0][0].contiguous()
    px = N * H * W
    frames_b, pat_b = 4 * px, 4 * H * W
    full_bytes = frames_b + pat_b + 12 * px                           # + idx i64 + best f32
    band_bytes = full_bytes + 8 * px                                  # + lo, hi i32
    ncc_band_bytes = band_bytes + 8 * H * (W + D - 1)                 # + the (mu1, s1) table of the prepared pattern
    fmt = "%-44s %8.4f / %8.4f / %8.4f ms   %7.1f MB compulsory   %s"

    say("band-limited matching, config 2: %d x %dx%d, D %d, block %d, shared pattern" % (N, W, H, D, BS))
    say("device %s; median / min / max of %d calls (device time, HIP events), after 10 warm-up calls"
        % (torch.cuda.get_device_name(0), args.reps))
    say("prior = the full matcher's indices + uniform integer noise in [-r, r]; band = disparity_band(prior, r)")
    say()

    say("NCC (xcorrvol_argmax_band, prepared pattern) against xcorrvol_argmax (fast, prepared)")
    h = te.prepare_pattern(p, N, D, BS)
    idx_full = te.xcorrvol_argmax(x, p, D, BS, prepared=h)[0]
    t_full = median_ms(lambda: te.xcorrvol_argmax(x, p, D, BS, prepared=h), args.reps)
    say(fmt % (("xcorrvol_argmax fast, prepared",) + t_full + (full_bytes / 1e6, "")))
    vol0 = te.xcorrvol_batch(x[:1], p, D, BS, algo="exact").cpu()
    ncc_ms = {}
    for r in RADII:
        lo, hi = bands_around(idx_full, r, D, r)
        out = te.xcorrvol_argmax_band(x, p, lo, hi, D, BS, prepared=h)
        note = "mean width %.1f, frame 0 == band_ref: %s, == full search on %.2f %% of pixels" % (
            float((hi - lo + 1).float().mean()), "yes" if frame0_ok(out, vol0, lo, hi, True) else "NO",
            100.0 * float((out[0] == idx_full).float().mean()))
        t = median_ms(lambda: te.xcorrvol_argmax_band(x, p, lo, hi, D, BS, prepared=h), args.reps)
        ncc_ms[r] = t[0]
        say(fmt % (("xcorrvol_argmax_band r = %d" % r,) + t + (ncc_band_bytes / 1e6, note)))
    lo, hi = bands_around(idx_full, 4, D, 4)
    t = median_ms(lambda: te.xcorrvol_argmax_band(x, p, lo, hi, D, BS), args.reps)
    say(fmt % (("xcorrvol_argmax_band r = 4, pattern not prepared",) + t + (ncc_band_bytes / 1e6, "")))
    faster = [r for r in RADII if ncc_ms[r] < t_full[0]]
    say("break-even: the band call is faster than the full search at r = %s" % (faster if faster else "no measured radius"))
    say()
    del vol0

    say("SAD (costvol_argmin_band) against costvol_argmin, eps 0.1")
    im, pp = x[:, 0].contiguous(), p[0].contiguous()
    cidx_full = te.costvol_argmin(im, pp, D, BS, "sad")[0]
    t_cfull = median_ms(lambda: te.costvol_argmin(im, pp, D, BS, "sad"), args.reps)
    say(fmt % (("costvol_argmin sad",) + t_cfull + (full_bytes / 1e6, "")))
    cvol0 = te.costvol(im[:1], pp, D, BS, "sad", 0.1, algo="exact").cpu()
    sad_ms = {}
    for r in RADII:
        lo, hi = bands_around(cidx_full, r, D, 100 + r)
        out = te.costvol_argmin_band(im, pp, lo, hi, D, BS, "sad")
        note = "mean width %.1f, frame 0 == band_ref: %s, == full search on %.2f %% of pixels" % (
            float((hi - lo + 1).float().mean()), "yes" if frame0_ok(out, cvol0, lo, hi, False) else "NO",
            100.0 * float((out[0] == cidx_full).float().mean()))
        t = median_ms(lambda: te.costvol_argmin_band(im, pp, lo, hi, D, BS, "sad"), args.reps)
        sad_ms[r] = t[0]
        say(fmt % (("costvol_argmin_band sad r = %d" % r,) + t + (band_bytes / 1e6, note)))
    faster = [r for r in RADII if sad_ms[r] < t_cfull[0]]
    say("break-even: the band call is faster than the full search at r = %s" % (faster if faster else "no measured radius"))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
