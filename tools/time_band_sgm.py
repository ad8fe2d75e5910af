"""Times band-limited semi-global matching (csrc/band_sgm.hip) at BASELINE config 2 (16 x 432 x 512, D 128, block 9,
shared pattern; the bench's LCN'd synthetic frames against the LCN'd dot pattern) and writes profiles/band_sgm.txt:
  - the yardstick: costvol_sgm(sad) and xcorrvol_sgm on the full volume (csrc/sgm.hip and its wrappers, which this
    feature leaves untouched), 4 and 8 paths, with the volume call and sgm_aggregate timed apart as well;
  - the bands of tools/time_band_match.py (prior = the full matcher's indices + uniform integer noise in [-r, r], band =
    disparity_band(prior, r)) at r = 1 / 2 / 4 / 8, i.e. slots = 3 / 5 / 9 / 17: the band volume call
    (costvol_band_volume sad, xcorrvol_band_volume with a prepared pattern) and band_sgm_aggregate at 4 and 8 paths,
    apart and as their sum beside the full route;
  - the bytes the aggregation moves by the algorithm (3 Vb + P per direction, less one Vb for the first, plus Vb + P
    for the argmin; Vb = the band volume, P = lo and hi) and the implied share of the 6.29 TB/s copy rate;
  - frame 0 of the r = 2 results against tests/band_sgm_ref.py.
    python tools/time_band_sgm.py [--reps 20] [--out profiles/band_sgm.txt]
Device time from HIP events around each call, after warm-up launches; median / min / max over the repetitions."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import bandsgm  # noqa: E402
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import band_sgm_ref, workloads  # noqa: E402

COPY_RATE = 6.29e12                    # bytes / s, float4 copy on an MI355X
P1, P2 = 0.02, 0.16
RADII = (1, 2, 4, 8)
FMT = "%-52s %8.3f / %8.3f / %8.3f ms   %s"


def median_ms(fn, reps, warmup=5):
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


def frame0_ok(vb, lo, hi, D, paths, maximise, out):
    S, idx, best = band_sgm_ref.band_sgm_ref(vb[:1].cpu().numpy(), lo[:1].cpu().numpy(), hi[:1].cpu().numpy(), D, P1, P2,
                                             paths, maximise)
    return bool(np.array_equal(out[0][:1].cpu().numpy(), idx)) and \
        bool(np.array_equal(out[1][:1].cpu().numpy().view(np.int32), best.view(np.int32)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_sgm.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_band_sgm.py needs a GPU"
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
    im, pp = x[:, 0].contiguous(), p[0].contiguous()
    px = N * H * W

    say("band-limited SGM, config 2: %d x %dx%d, D %d, block %d, shared pattern, P1 %g, P2 %g" % (N, W, H, D, BS, P1, P2))
    say("device %s; median / min / max of %d calls (device time, HIP events), after 5 warm-up calls"
        % (torch.cuda.get_device_name(0), args.reps))
    say("prior = the full matcher's indices + uniform integer noise in [-r, r]; band = disparity_band(prior, r)")

    for fam in ("sad", "ncc"):
        say()
        maximise = fam == "ncc"
        if fam == "sad":
            say("SAD: costvol_band_volume + band_sgm_aggregate against costvol_sgm (full volume, default algo), eps 0.1")
            full_vol = lambda: te.costvol(im, pp, D, BS, "sad", 0.1)                              # noqa: E731
            full_sgm = lambda paths: te.costvol_sgm(im, pp, D, BS, "sad", 0.1, P1, P2, paths)     # noqa: E731
            idx_full = te.costvol_argmin(im, pp, D, BS, "sad")[0]
            band_vol = lambda lo, hi, s: bandsgm.costvol_band_volume(im, pp, lo, hi, D, BS, "sad", 0.1, s)   # noqa: E731
        else:
            say("NCC: xcorrvol_band_volume (prepared pattern) + band_sgm_aggregate against xcorrvol_sgm (full volume, "
                "default algo)")
            h = te.prepare_pattern(p, N, D, BS)
            full_vol = lambda: te.xcorrvol_batch(x, p, D, BS)                                     # noqa: E731
            full_sgm = lambda paths: te.xcorrvol_sgm(x, p, D, BS, P1, P2, paths)                  # noqa: E731
            idx_full = te.xcorrvol_argmax(x, p, D, BS, prepared=h)[0]
            band_vol = lambda lo, hi, s: bandsgm.xcorrvol_band_volume(x, p, lo, hi, D, BS, s, prepared=h)    # noqa: E731
        t_vol = median_ms(full_vol, args.reps)
        say(FMT % (("full volume call",) + t_vol + ("V = %.3f GB" % (4.0 * px * D / 1e9),)))
        vol = full_vol()
        t_full = {}
        for paths in (4, 8):
            t = median_ms(lambda: te.sgm_aggregate(vol, P1, P2, paths, maximise), args.reps)
            say(FMT % (("sgm_aggregate paths=%d" % paths,) + t + ("%d V" % (3 * paths),)))
        del vol
        for paths in (4, 8):
            t_full[paths] = median_ms(lambda: full_sgm(paths), args.reps)
            say(FMT % (("%s paths=%d (the yardstick)" % ("costvol_sgm" if fam == "sad" else "xcorrvol_sgm", paths),) +
                       t_full[paths] + ("",)))
        for r in RADII:
            slots = 2 * r + 1
            lo, hi = bands_around(idx_full, r, D, r if fam == "ncc" else 100 + r)
            width = float((hi - lo + 1).clamp(min=0).float().mean())
            vb = band_vol(lo, hi, slots)
            Vb, P = 4.0 * px * slots, 8.0 * px
            t_bv = median_ms(lambda: band_vol(lo, hi, slots), args.reps)
            say(FMT % (("r = %d, slots %d: band volume call" % (r, slots),) + t_bv +
                       ("mean width %.2f, Vb = %.1f MB" % (width, Vb / 1e6),)))
            for paths in (4, 8):
                t = median_ms(lambda: bandsgm.band_sgm_aggregate(vb, lo, hi, D, P1, P2, paths, maximise), args.reps)
                moved = (3 * paths) * Vb + (paths + 1) * P
                note = "%.2f GB moved -> %.2f TB/s = %.1f %% of the copy rate; band route %.3f ms = %.1f %% of the full one" % (
                    moved / 1e9, moved / t[0] / 1e9, 100.0 * moved / (t[0] * 1e-3) / COPY_RATE, t_bv[0] + t[0],
                    100.0 * (t_bv[0] + t[0]) / t_full[paths][0])
                if r == 2:
                    out = bandsgm.band_sgm_aggregate(vb, lo, hi, D, P1, P2, paths, maximise)
                    note += "; frame 0 == band_sgm_ref: %s" % ("yes" if frame0_ok(vb, lo, hi, D, paths, maximise, out) else "NO")
                say(FMT % (("r = %d, slots %d: band_sgm_aggregate paths=%d" % (r, slots, paths),) + t + (note,)))
            del vb

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
