"""Times the band matchers' validity at BASELINE config 2 (16 x 432 x 512, D 128, block 9, shared prepared pattern; the
bench's LCN'd synthetic frames against the LCN'd dot pattern) and writes profiles/band_validity.txt.  Bands are those of
tools/time_band_match.py (prior = the full matcher's indices + seeded integer noise in [-r, r], band =
disparity_band(prior, r)) at r = 1, 2, 4.  Per radius, for NCC and for SAD:
  (a) the new call: xcorrvol_band_validity / costvol_band_validity;
  (b) the band matcher alone: xcorrvol_argmax_band / costvol_argmin_band -- and, with --parent-lib, the same C entry
      point of a library built from the parent commit's band_match.hip (tools/build_variant.sh), called through the
      same ctypes path as this tree's, to show that moving the scorers into a header did not change the kernel;
  (c) the only alternative before this op: the band matcher followed by xcorrvol_validity / costvol_validity
      (algo="fast") on its idx, which materialises and scans all D disparities.
(a) and (c) are timed at min_gap 0 and 0.05: the old op re-scores exactly every pixel whose fast gap lies within the
fast volume's error bound of min_gap (at 0: every exact tie), so its time depends on min_gap -- the count of re-scored
pixels and pattern columns is printed beside it -- and the new call's does not.
(a) - (b) is the price of the flags; the claim to check is (a) < (c).  Frame 0 of every (a) result is compared with
tests/band_validity_ref.py on the exact volume, bit for bit.
    python tools/time_band_validity.py [--reps 30] [--parent-lib tools/variants/libctd_NAME.so] [--out FILE]
Device time from HIP events around each call, after 10 warm-up calls; median / min / max over the repetitions."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import _lib  # noqa: E402
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import band_validity_ref as bvr  # noqa: E402
from tests import workloads  # noqa: E402
from tools.time_band_match import bands_around, median_ms  # noqa: E402

RADII = (1, 2, 4)
MIN_GAPS = (0.0, 0.05)
PREPARED = 0x100


def bind(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in _lib.TABLES["ctd_hip_band.h"].items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def frame0_ok(out, vol0, lo, hi, maximise):
    ref = bvr.band_validity_ref(vol0.numpy(), lo[:1].cpu().numpy(), hi[:1].cpu().numpy(), maximise)
    for o, r in zip(out, ref):
        o, r = o[:1].cpu(), torch.from_numpy(np.ascontiguousarray(r))
        if o.dtype == torch.float32:
            if not torch.equal(torch.isnan(o), torch.isnan(r)):
                return False
            o, r = torch.nan_to_num(o, nan=0.0).view(torch.int32), torch.nan_to_num(r, nan=0.0).view(torch.int32)
        if not torch.equal(o, r):
            return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "band_validity.txt"))
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
    im, pp = x[:, 0].contiguous(), p[0].contiguous()
    dev = x.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    here = bind(_lib.LIB_PATH)
    parent = bind(args.parent_lib) if args.parent_lib else None
    fmt = "  %-70s %8.4f / %8.4f / %8.4f ms   %s"

    say("validity of the band matchers, config 2: %d x %dx%d, D %d, block %d, shared pattern" % (N, W, H, D, BS))
    say("device %s; median / min / max of %d calls (device time, HIP events), after 10 warm-up calls"
        % (torch.cuda.get_device_name(0), args.reps))
    say("prior = the full matcher's indices + uniform integer noise in [-r, r]; band = disparity_band(prior, r)")
    say("lr_tol 1;  (a) the new call, (b) the band matcher alone, (c) band matcher + *_validity(algo=\"fast\")")
    say()

    h = te.prepare_pattern(p, N, D, BS)
    idx_full = te.xcorrvol_argmax(x, p, D, BS, prepared=h)[0]
    cidx_full = te.costvol_argmin(im, pp, D, BS, "sad")[0]
    vol0 = te.xcorrvol_batch(x[:1], p, D, BS, algo="exact").cpu()
    cvol0 = te.costvol(im[:1], pp, D, BS, "sad", 0.1, algo="exact").cpu()
    te.xcorrvol_argmax_band(x, p, *bands_around(idx_full, 1, D, 1), D, BS, prepared=h)      # fills the handle's planes
    ws = h.subpixel[(H, W, D, BS)]
    idx_o = torch.empty((N, H, W), dtype=torch.int64, device=dev)
    best_o = torch.empty((N, H, W), dtype=torch.float32, device=dev)

    def raw_ncc(lib, lo, hi):
        st = lib.ctd_xcorrvol_argmax_band_f32(x.data_ptr(), p.data_ptr(), 0, lo.data_ptr(), hi.data_ptr(), idx_o.data_ptr(),
                                              best_o.data_ptr(), N, H, W, D, BS, PREPARED, ws.data_ptr(), ws.numel(),
                                              dev.index, stream)
        assert st == 0, st

    def raw_sad(lib, lo, hi):
        st = lib.ctd_costvol_argmin_band_f32(im.data_ptr(), pp.data_ptr(), 0, lo.data_ptr(), hi.data_ptr(),
                                             idx_o.data_ptr(), best_o.data_ptr(), N, H, W, D, BS, 1, 0.1, dev.index, stream)
        assert st == 0, st

    summary = []
    for fam in ("NCC", "SAD"):
        ncc = fam == "NCC"
        say("%s (%s)" % (fam, "xcorrvol_band_validity, prepared pattern" if ncc else "costvol_band_validity, eps 0.1"))
        for r in RADII:
            lo, hi = bands_around(idx_full if ncc else cidx_full, r, D, r if ncc else 100 + r)
            if ncc:
                fa = lambda g=0.0: te.xcorrvol_band_validity(x, p, lo, hi, D, BS, 1, g, prepared=h)         # noqa: E731
                fb = lambda: te.xcorrvol_argmax_band(x, p, lo, hi, D, BS, prepared=h)                       # noqa: E731
                fv = lambda g, **kw: te.xcorrvol_validity(x, p, fb()[0], D, BS, 1, g, algo="fast", **kw)    # noqa: E731
                raw = raw_ncc
            else:
                fa = lambda g=0.0: te.costvol_band_validity(im, pp, lo, hi, D, BS, "sad", 0.1, 1, g)        # noqa: E731
                fb = lambda: te.costvol_argmin_band(im, pp, lo, hi, D, BS, "sad")                           # noqa: E731
                fv = lambda g, **kw: te.costvol_validity(im, pp, fb()[0], D, BS, "sad", 0.1, 1, g, algo="fast", **kw)  # noqa: E731
                raw = raw_sad
            out = fa()
            ok = frame0_ok(out, vol0 if ncc else cvol0, lo, hi, ncc)
            valid = float((out[2] == 7).float().mean())
            again = fa()
            same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                   b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(out, again))
            say(" r = %d: mean width %.1f; frame 0 == band_validity_ref: %s; two runs equal: %s; flags == 7 on %.1f %% of pixels"
                % (r, float((hi - lo + 1).float().mean()), "yes" if ok else "NO", "yes" if same else "NO", 100 * valid))
            tb = median_ms(fb, args.reps)
            say(fmt % (("(b) band matcher alone",) + tb + ("",)))
            tb_here = median_ms(lambda: raw(here, lo, hi), args.reps)
            say(fmt % (("(b) the C entry point, this tree's library",) + tb_here + ("",)))
            if parent is not None:                                  # this tree, the parent, this tree again: no order bias
                tb_par = median_ms(lambda: raw(parent, lo, hi), args.reps)
                tb_again = median_ms(lambda: raw(here, lo, hi), args.reps)
                say(fmt % (("(b) the C entry point, the parent commit's band_match.hip",) + tb_par + ("",)))
                say(fmt % (("(b) the C entry point, this tree's library, again",) + tb_again +
                           ("this tree (mean of both) / parent = %.3f" % (0.5 * (tb_here[0] + tb_again[0]) / tb_par[0]),)))
            # the old op settles near-decisions (|gap - min_gap| within the fast volume's error bound, exact ties above
            # all) by exact re-scoring, one wavefront per pixel: its time depends on min_gap; the new call's does not
            for g in MIN_GAPS:
                ta = median_ms(lambda: fa(g), args.reps)
                tc = median_ms(lambda: fv(g), args.reps)
                n_pix, n_col = (int(t.numel()) for t in fv(g, return_rescored=True)[3:])
                say(fmt % (("(a) band validity, min_gap %g" % g,) + ta + ("",)))
                say(fmt % (("(c) band matcher + validity of the whole volume (fast), min_gap %g" % g,) + tc +
                           ("re-scored: %d pixels (%.2f %%), %d pattern columns of %d" % (n_pix, 100.0 * n_pix / (N * H * W), n_col,
                                                                                       N * H * W),)))
                say("      (a) - (b) = %.4f ms (the price of the flags);  (c) / (a) = %.2f: (a) is %s" %
                    (ta[0] - tb[0], tc[0] / ta[0], "the faster route" if ta[0] < tc[0] else "NOT the faster route"))
                summary.append((fam, r, g, ta[0], tb[0], tc[0], n_pix))
        say()
    say("summary, medians in ms:  family r min_gap  (a)      (b)      (c)      (a)-(b)  (c)/(a)  pixels re-scored by (c)")
    for fam, r, g, a, b, c, n_pix in summary:
        say("                         %-6s %d %-7g  %-8.4f %-8.4f %-8.4f %-8.4f %-7.2f  %d" % (fam, r, g, a, b, c, a - b, c / a, n_pix))

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
