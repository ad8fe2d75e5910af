"""Times the training-sample finishing kernels of connecting_the_dots_amd.synth against the bytes they must move:
  - finish_render (ctd_syn_finish_f32) on N frames of 480 x 640: 48 B / pixel (depth 4, colour 12, ambient-normal 12 in;
    im, ambient, grad, disp, mask 20 out);
  - the augmentation kernel (ctd_augment_f32, device-generator noise, f32 plane): 12 B / pixel (image, noise in; image
    out), and the whole augment() call (draws with torch, blur / noise / clip, salt and pepper);
  - beside them, the CPU restatement of the finishing in the reference's order (numpy f32 Sobel + the C oracle's
    Cython-order LCN) on one frame.
    python tools/time_synth.py [--frames 16] [--reps 50] [--out FILE]
Device time from HIP events around each call after warm-up launches; median / min / max over the repetitions; the
achieved rate is the algorithmic bytes over the median time.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from connecting_the_dots_amd import _lib, synth  # noqa: E402


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


def cpu_finish(depth, color, normal, b, bf):
    """one frame in the reference's order on the host (numpy f32 + the C oracle's datagen LCN)"""
    from oracle import oracle
    kd = np.array([-1, -2, 0, 2, 1], np.float32)
    ks = np.array([1, 4, 6, 4, 1], np.float32)

    def sep(a, kr, kc):
        H, W = a.shape
        ap = np.pad(a, 2, mode="reflect")
        h = np.zeros((H + 4, W), np.float32)
        for j in range(5):
            h = h + kr[j] * ap[:, j:j + W]
        v = np.zeros((H, W), np.float32)
        for j in range(5):
            v = v + kc[j] * h[j:j + H]
        return v
    c, n = color, normal
    amb = ((n[..., 0] + n[..., 1]) + n[..., 2]) / np.float32(3)
    im = np.float32(b) * (((c[..., 0] + c[..., 1]) + c[..., 2]) / np.float32(3)) + np.float32(1 - b) * amb
    disp = np.float32(bf) / depth
    gx, gy = sep(amb, kd, ks), sep(amb, ks, kd)
    pre = np.maximum(np.sqrt(gx * gx + gy * gy) - np.float32(0.8), np.float32(0))
    return im, disp, np.clip(oracle.lcn_datagen(pre, 5, 0.1)[0], 0, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, H, W = args.frames, args.height, args.width
    rs = np.random.RandomState(0)
    depth = rs.uniform(0.5, 4, size=(N, H, W)).astype(np.float32)
    color = rs.uniform(0, 1, size=(N, H, W, 3)).astype(np.float32)
    normal = rs.uniform(0, 1, size=(N, H, W, 3)).astype(np.float32)
    d, c, n = (torch.from_numpy(a).cuda() for a in (depth, color, normal))
    px = N * H * W
    res = {"frames": N, "H": H, "W": W}
    fmt = "%-48s %.4f / %.4f / %.4f ms   %.0f GB/s"

    t = median_ms(lambda: synth.finish_render(d, c, n, 0.6, 0.075, 567.6), args.reps)
    res["finish_ms"], res["finish_GBps"] = t[0], 48.0 * px / t[0] / 1e6
    print(fmt % (("finish_render %dx%dx%d (48 B/px)" % (N, H, W),) + t + (res["finish_GBps"],)))

    img = torch.from_numpy(rs.uniform(0, 1, size=(N, 1, H, W)).astype(np.float32)).cuda()
    noise = torch.randn((N, H, W), device="cuda")
    for blur in (0, 1):
        p = np.zeros(N, synth.AUGMENT_PARAMS)
        p["blur"], p["taps"], p["noise_scale"] = blur, synth.gaussian_taps(0.35), 3.0 / 255
        params = torch.from_numpy(p.view(np.uint8)).cuda()
        out = torch.empty_like(img)
        mm = torch.empty((N, 2), dtype=torch.int32, device="cuda")
        L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream

        def run():
            _lib.check(L.ctd_augment_f32(img.data_ptr(), noise.data_ptr(), 0, params.data_ptr(), out.data_ptr(),
                                         mm.data_ptr(), N, H, W, 0, st), "augment")
        t = median_ms(run, args.reps)
        key = "augment_blur%d" % blur
        res[key + "_ms"], res[key + "_GBps"] = t[0], 12.0 * px / t[0] / 1e6
        print(fmt % (("augment kernel, blur %s (12 B/px, incl. minmax memset)" % ("on" if blur else "off"),) + t +
                     (res[key + "_GBps"],)))
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    t = median_ms(lambda: synth.augment(img, generator=g), args.reps)
    res["augment_call_ms"] = t[0]
    print("%-48s %.4f / %.4f / %.4f ms" % (("augment() with device draws",) + t))

    t0 = time.perf_counter()
    cpu_finish(depth[0], color[0], normal[0], 0.6, 0.075 * 567.6)
    res["cpu_finish_one_frame_ms"] = (time.perf_counter() - t0) * 1e3
    print("%-48s %.1f ms (one frame, one host thread)" % ("CPU restatement, numpy f32 + C LCN", res["cpu_finish_one_frame_ms"]))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
