"""Times HyperDepth forest evaluation (ctd_hyperdepth_eval_f32) at 480 x 640, 6 trees of depth 8, C = 6400
(640 columns x 10 disparity bins), N in {1, 8}, synthetic leaf lists of exactly L entries, L in {16, 256, 2048}.

    python tools/time_hyperdepth.py [--reps 20] [--out FILE]

The device tables are built directly in the C layout of ctd_hd_tables (include/ctd_hip.h), on the device: P distinct
forests of full binary trees (random offsets in the 32 x 32 patch, integer thresholds), leaf lists of L distinct
classes (an arithmetic progression mod C with a random start and a step coprime to C, sorted), counts 1..20.  Row r
uses forest r % P, P = min(480, 2^27.5 / (6 * 256 * L)) so the entries stay near 1.5 GB (every row distinct up to
L = 256).  Device time from HIP events around each call, after warm-up; median / min / max.  "entry bytes / s" counts
the 8-byte (class, count) entries of the 6 reached lists per pixel once; the kernel reads each twice when a pixel's
lists exceed 512 entries (registers hold the first 512 between its two passes).
The CPU line is the numpy restatement of tests/hyperdepth_ref.py on 8 rows of one image (checked bit for bit against
the kernel there), scaled to a frame; the reference module's time comes from the fixture generator
(tests/golden/make_golden_hyperdepth.py) and was measured on the machine that generated the fixture."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import _lib  # noqa: E402
from tests import hyperdepth_ref as R  # noqa: E402

H, W, BINS, T, DEPTH = 480, 640, 10, 6, 8
C = W * BINS
NS, NL = 2 ** DEPTH - 1, 2 ** DEPTH          # splits and leaves per tree


def build_tables(L, P, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = "cuda"
    ri = lambda lo, hi, shape: torch.randint(lo, hi, shape, device=dev, generator=g, dtype=torch.int64)  # noqa: E731
    ntree = P * T
    i = torch.arange(NS, device=dev)
    tree_base_n = (torch.arange(ntree, device=dev) * NS)[:, None]
    tree_base_l = (torch.arange(ntree, device=dev) * NL)[:, None]

    def child(c):                                                    # heap layout, leaves are children >= NS
        return torch.where(c < NS, tree_base_n + c, -(tree_base_l + (c - NS)) - 1)

    thr = torch.round(torch.randn((ntree, NS), device=dev, generator=g) * 64).float().view(torch.int32).long()
    nodes = torch.stack([thr, ri(0, 32, (ntree, NS)), ri(0, 32, (ntree, NS)), ri(0, 32, (ntree, NS)),
                         ri(0, 32, (ntree, NS)), child(2 * i + 1), child(2 * i + 2),
                         torch.zeros((ntree, NS), device=dev, dtype=torch.long)], 2).reshape(-1, 8).int()
    roots = ((torch.arange(H, device=dev) % P)[:, None] * T + torch.arange(T, device=dev)[None]) * NS
    roots = roots.int().contiguous()
    nleaf = ntree * NL
    a = ri(0, C, (nleaf, 1))
    s = 2 * ri(0, C // 2, (nleaf, 1)) + 1
    s = torch.where(s % 5 == 0, s + 2, s)                            # odd, not a multiple of 5: coprime to 6400
    cls = torch.empty((nleaf, L), device=dev, dtype=torch.int32)
    cnt = torch.empty((nleaf, L), device=dev, dtype=torch.int32)
    k = torch.arange(L, device=dev)[None]
    for b in range(0, nleaf, 4096):
        cls[b:b + 4096] = torch.sort((a[b:b + 4096] + k * s[b:b + 4096]) % C, 1).values.int()
        cnt[b:b + 4096] = ri(1, 21, (min(4096, nleaf - b), L)).int()
    entries = torch.stack([cls, cnt], 2).reshape(-1, 2).contiguous()
    leaf_off = torch.arange(nleaf + 1, device=dev, dtype=torch.int64) * L
    leaf_sum = cnt.sum(1, dtype=torch.int64).int().contiguous()
    t = dict(nodes=nodes.contiguous(), roots=roots, leaf_off=leaf_off, leaf_sum=leaf_sum, entries=entries)
    st = _lib.HdTables(t["nodes"].data_ptr(), roots.data_ptr(), leaf_off.data_ptr(), leaf_sum.data_ptr(),
                       entries.data_ptr(), nodes.shape[0], nleaf, entries.shape[0], 0, H, T, C, DEPTH, 0)
    return t, st


def host_flat(t, f, L):
    """forest f of the tables as tests/hyperdepth_ref.py's flattened dict (forest-local indices)"""
    nb, lb = f * T * NS, f * T * NL
    nodes = t["nodes"][nb:nb + T * NS].cpu().numpy().astype(np.int64)
    for c in (5, 6):
        v = nodes[:, c]
        nodes[:, c] = np.where(v >= 0, v - nb, ~(~v - lb))
    lens = np.full(T * NL, L, np.int64)
    return dict(nodes=nodes.astype(np.int32), roots=np.arange(T, dtype=np.int32) * NS, lens=lens,
                sums=t["leaf_sum"][lb:lb + T * NL].cpu().numpy(),
                entries=t["entries"][lb * L:(lb + T * NL) * L].cpu().numpy())


def time_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return np.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["HyperDepth forest evaluation, ctd_hyperdepth_eval_f32, %s" % torch.cuda.get_device_name(0),
             "shape %d x %d, %d trees of depth %d, C = %d (%d bins), reps %d, HIP-event median (min / max)"
             % (H, W, T, DEPTH, C, BINS, args.reps), ""]
    print("\n".join(lines), flush=True)
    L_ = _lib.lib()
    rs = np.random.RandomState(0)
    ims_all = torch.from_numpy(rs.randint(0, 256, (8, H, W)).astype(np.uint8)).cuda()
    for L in (16, 256, 2048):
        P = int(min(H, 2 ** 27.5 // (T * NL * L)))
        t, st = build_tables(L, P)
        torch.cuda.synchronize()
        tb = t["entries"].numel() * 4
        for N in (1, 8):
            ims = ims_all[:N].contiguous()
            out = torch.empty((N, H, W, 3), device="cuda")
            stream = torch.cuda.current_stream().cuda_stream

            def run():
                _lib.check(L_.ctd_hyperdepth_eval_f32(ctypes.byref(st), ims.data_ptr(), N, H, W, 0, H, BINS,
                                                      out.data_ptr(), 0, stream), "hyperdepth eval")
            med, lo, hi = time_ms(run, args.reps)
            px = N * H * W
            eb = px * T * L * 8
            line = ("L %5d  N %d  distinct row forests %3d (entries %6.0f MB)  %8.3f ms (%.3f / %.3f)  %7.1f Mpix/s  "
                    "entry bytes %7.2f GB -> %6.2f TB/s" % (L, N, P, tb / 1e6, med, lo, hi, px / med / 1e3, eb / 1e9,
                                                          eb / med / 1e9))
            lines.append(line)
            print(line, flush=True)
        if L <= 256:                                               # CPU restatement, 8 rows of image 0, checked
            im0 = ims_all[:1].cpu().numpy()
            out1 = torch.empty((1, H, W, 3), device="cuda")
            _lib.check(L_.ctd_hyperdepth_eval_f32(ctypes.byref(st), ims_all.data_ptr(), 1, H, W, 0, H, BINS,
                                                  out1.data_ptr(), 0, torch.cuda.current_stream().cuda_stream), "eval")
            gpu = out1.cpu().numpy()
            t0 = time.time()
            rows = range(100, 108)
            ok = True
            for r in rows:
                ref = R.eval_row_flat(host_flat(t, r % P, L), C, im0, r, BINS)
                ok &= np.array_equal(ref.view(np.int32), gpu[:, r].view(np.int32))
            dt = (time.time() - t0) / len(rows) * H
            line = ("L %5d  CPU numpy restatement (1 image, 8 rows timed, x60): %8.0f ms per frame; bit-exact vs the "
                    "kernel on those rows: %s" % (L, dt * 1e3, ok))
            lines.append(line)
            print(line, flush=True)
            if not ok:
                sys.exit("kernel and restatement differ")
        del t, st
        torch.cuda.empty_cache()
    g = os.path.join(ROOT, "tests", "golden", "hyperdepth.npz")
    secs, px = np.load(g)["ref_seconds_realistic"]
    lines.append("")
    lines.append("reference hyperdepth module (Cython + OpenMP, 4 threads), fixture case 'realistic' (6 trees, depth 8, "
                 "C = 960, lists 100..300), measured by make_golden_hyperdepth.py on the fixture machine's CPU, file "
                 "loading included: %.3f s for %d pixels = %.1f us / pixel" % (secs, px, secs / px * 1e6))
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
