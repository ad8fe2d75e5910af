#!/usr/bin/env python3
"""Benchmark of the disparity hot path on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--algo fast|exact] [--frames 16] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

At EVERY N the headline `value` / `ms_per_step` time one step of BASELINE config 2 per rank: 16 synthetic 512x432 frames
resident in HBM -> LCN (r=5, eps=0.05) -> zero-mean NCC block-matching volume against the LCN'd pattern over 128
disparities (materialised, [16,128,432,512] f32) -> argmax over disparity with reference (bit-exact) indices.  Frames
shard across ranks (weak scaling: 128 frames on 8 GPUs) and this step has no collective.

A SECOND timed region, reported at every N under `config3`, times BASELINE config 3's step: the same 16 frames per GPU
plus disparity -> depth and the two-view geometric loss on frame pairs, and the path's one exchange -- a non-blocking
all-gather of the per-rank loss scalar (RCCL over xGMI) once a process group exists.  value(N) / value(1) and
config3.value(N) / config3.value(1) are both like-for-like scaling ratios.

`python bench.py --gpus N` without a launcher starts the N ranks itself (one child process per GPU; the parent never
touches a GPU and relays rank 0's line).  Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement").
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

H, W, D, BS = 432, 512, 128, 9
LCN_RADIUS, LCN_EPS = 5, 0.05
BYTES_PER_PIXDISP = 4.0 + 8.0 / D          # 4*D*H*W volume write + both inputs read once
HBM_PEAK_GBS = 8000.0                      # MI355X_MICROARCH.md: 8 TB/s HBM3E spec peak
FOCAL, BASELINE_M = 567.6, 0.075           # camera of the reference's data (create_syn_data.py:228-230)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=16, help="frames per GPU per step (BASELINE config 2 / 3: 16)")
    ap.add_argument("--algo", default="fast", choices=["fast", "exact"])
    ap.add_argument("--lcn-algo", default="fused", choices=["fused", "fused_exact", "fast", "exact"],
                    help="LCN of the frames inside the step: 'fused' (default) = ONE call, ctd_lcn_xcorrvol_argmax_f32: the "
                         "streaming kernel that writes the LCN outputs and the matcher's window statistics from the raw frames "
                         "(f32 box sums: tolerance level); 'fused_exact' = the same with f64 box sums (the oracle's bits); "
                         "'fast' / 'exact' = the LCN as a call of its own (tiled f32 / f64 kernel) before xcorrvol_argmax")
    ap.add_argument("--workload", default=None, choices=["config2", "config3", "config4"],
                    help="default: the config-2 headline region AND the config-3 region (`config3` block); config2 / config3 = "
                         "that region only (the profiling scripts: per-kernel statistics of one step kind); "
                         "config4 = BASELINE configs[3]: 1024x1024 frames, 256 disparities, NCC volume + argmax and the "
                         "soft-census cost volume (one frame per step unless --frames says otherwise)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise torch.distributed even with ONE rank and run the N > 1 code path (config 3, the "
                         "scalar all-gather, the f64 all-reduce of the elapsed time) on it: RCCL on a one-GPU box")
    ap.add_argument("--headline-only", action="store_true",
                    help="only the timed steps: no parity probe, no CPU baseline, no also_measured legs (what the profiling "
                         "scripts run, so that per-kernel statistics hold the step's own launches only)")
    ap.add_argument("--no-parity-probe", action="store_true",
                    help="skip the untimed 1-frame parity probe (the profiling scripts do: its launches would be averaged "
                         "into the per-kernel statistics)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the headline region's last step returned as DIR/<name>.npy "
                         "(float32, at most 60 MiB in all; larger arrays as a fixed, seeded sample, see dump_outputs); "
                         "rank 0's frames")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def check_gpu_count(n_ranks, backend, n_devices):
    """--gpus N over RCCL needs N devices (connecting_the_dots_amd.sharding.check_gpu_count)."""
    from connecting_the_dots_amd import sharding
    err = sharding.check_gpu_count(n_ranks, backend, n_devices, what="--gpus")
    return ("bench.py: " + err) if err else None


def self_launch(args, deadline_s=None):
    """--gpus N without a launcher: start N ranks (fresh interpreters; this parent has not touched a GPU), relay
    rank 0's output, exit non-zero if any rank failed or the deadline passed (sharding.launch_ranks)."""
    from connecting_the_dots_amd import sharding
    return sharding.launch_ranks(os.path.abspath(__file__), sys.argv[1:], args.gpus, deadline_s)


def make_inputs(frames, rank, device):
    """Synthetic data of BASELINE.md section 3: RandomState(1234 + global frame index) uniform [0,1) frames,
    the reference's seeded synthetic dot pattern (data/commons.py:8-11) as the pattern."""
    import numpy as np
    import torch
    from tests import workloads
    a = np.stack([workloads.uniform_frame(1234 + rank * frames + i, H, W) for i in range(frames)])
    pat = workloads.syn_dot_pattern(H, W, seed=42)[None, None]
    return torch.from_numpy(a).to(device), torch.from_numpy(pat).to(device)


def make_poses(frames, rank, device):
    """small seeded rigid motions per frame"""
    import numpy as np
    import torch
    rs = np.random.RandomState(777 + rank)
    Rs, ts = [], []
    for _ in range(frames):
        ax = rs.randn(3) * 0.01
        th = np.linalg.norm(ax)
        k = ax / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        Rs.append(np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx)
        ts.append(rs.randn(3) * 0.02)
    return (torch.from_numpy(np.stack(Rs).astype(np.float32)).to(device),
            torch.from_numpy(np.stack(ts).astype(np.float32)).to(device))


def _ref_xcorrvol_worker(job):
    """one frame through the reference's own xcorrvol_cpu (child process of the all-cores leg)"""
    import torch
    from oracle import build_ref
    ref = build_ref.load()
    torch.set_num_threads(1)
    a, b = job
    t0 = time.perf_counter()
    ref.xcorrvol_cpu(a, b, D, BS)
    return time.perf_counter() - t0


def cpu_baseline(pattern_lcn_cpu, frames_lcn_cpu):
    """The reference CPU path on a bounded sample of the same workload: (a) one frame through the
    reference's own xcorrvol_cpu (oracle/_ref, built from /root/reference by oracle/build_ref.py; else the C port) on
    one core -- what one reference call does, its loop is serial (ext_cpu.cpp:7-12) -- and (b) one frame per host core
    in `cores` independent processes, the fair all-cores number."""
    import torch
    try:
        from oracle import build_ref
        ref = build_ref.load()
    except Exception:
        ref = None
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    a = frames_lcn_cpu[0].contiguous()
    b = pattern_lcn_cpu.contiguous()
    t0 = time.perf_counter()
    if ref is not None:
        torch.set_num_threads(1)
        ref.xcorrvol_cpu(a, b, D, BS)
        kind = "reference"
    else:
        from oracle import oracle
        oracle.xcorrvol(a.numpy(), b.numpy(), D, BS, nthreads=1)
        kind = "port"
    dt = time.perf_counter() - t0
    out = {"value": H * W * D / dt / 1e6, "unit": "Mpix*disp/s", "cores": 1, "kind": kind, "cpu_model": model,
           "host_cores": ncpu,
           "sample": "1 of the 16 frames of one step, full 512x432x128 NCC volume (xcorrvol_cpu, serial loop), %.1f s" % dt}
    # (b) all host cores: one frame per process, at most 16 processes (about the same wall time as leg (a))
    try:
        import multiprocessing as mp
        workers = max(1, min(ncpu, 16))
        jobs = [(frames_lcn_cpu[i % frames_lcn_cpu.shape[0]].contiguous(), b) for i in range(workers)]
        ctx = mp.get_context("spawn")
        t0 = time.perf_counter()
        with ctx.Pool(workers) as pool:
            if ref is not None:
                times = pool.map(_ref_xcorrvol_worker, jobs)
            else:
                times = None
        wall = time.perf_counter() - t0
        if times:
            busy = max(times)                                  # processes run side by side: the slowest one bounds the rate
            out["all_cores"] = {"value": workers * H * W * D / busy / 1e6, "unit": "Mpix*disp/s", "cores": workers,
                                "sample": "%d processes x 1 frame each, slowest %.1f s (pool wall %.1f s incl. start-up)"
                                          % (workers, busy, wall)}
    except Exception as e:                                     # the single-core leg stands on its own
        out["all_cores"] = {"error": repr(e)}
    return out


def measured_traffic(kernel_substr, pattern="*_pmc_hbm_traffic.json", exclude="config4"):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC summary (separate --pmc
    passes of tools/profile_round.sh; FETCH_SIZE doubled as MI355X_MICROARCH.md prescribes for gfx950,
    WRITE_SIZE as is, both in KiB) and the file it was read from.  (None, None) when no profile of this build has
    been committed: the counters are NOT collected in this run."""
    import glob
    files = sorted(f for f in glob.glob(os.path.join(ROOT, "profiles", pattern)) if not exclude or exclude not in os.path.basename(f))
    for f in reversed(files):
        for name, c in json.load(open(f)).items():
            if kernel_substr in name and "FETCH_SIZE" in c and "WRITE_SIZE" in c:
                return (2.0 * c["FETCH_SIZE"] + c["WRITE_SIZE"]) * 1024.0, "profiles/" + os.path.basename(f)
    return None, None


def committed_number(fname, key):
    """A number recorded by a committed profile (profiles/<fname>, a `key = value` line): read, not measured here."""
    try:
        for line in open(os.path.join(ROOT, "profiles", fname)):
            if line.strip().startswith(key):
                return float(line.split("=", 1)[1].split()[0])
    except (OSError, ValueError, IndexError):
        pass
    return None


def parity_probe(te, device):
    """disparity MAE vs the reference on the committed full-size golden (seeds 1234 / 42); runs BEFORE the warm-up.
    Any failure (fixture missing, call failing) propagates: a bench that cannot check its indices exits non-zero."""
    import numpy as np
    import torch
    from tests import workloads
    from tests.util import golden
    g = golden("xcorrvol_cfg1")
    a = torch.from_numpy(workloads.uniform_frame(1234, H, W)).to(device)
    b = torch.from_numpy(workloads.uniform_frame(42, H, W)).to(device)
    idx, _, _ = te.xcorrvol_argmax(a, b, D, BS, return_volume=True)
    return float(np.abs(idx.cpu().numpy().astype(np.int64) - g["uni_argmax"].astype(np.int64)).mean())


def timed_workload_probe(te, x, idx, pat_lcn):
    """disparity MAE of the TIMED workload: frame 0 of the last timed step's indices against the reference-order kernel
    (algo='exact', bit-identical to the reference: tests/test_xcorrvol_gpu.py) on the same LCN'd frame, first index on
    ties.  One ~3 ms call after the timed region.  Failures propagate."""
    import torch
    ref_vol = te.xcorrvol_batch(x[:1].contiguous(), pat_lcn, D, BS, algo="exact")
    ref_idx, _ = te.argmax_disp(ref_vol)
    return float((idx[:1].to(torch.int64) - ref_idx).abs().to(torch.float64).mean().item())


def exact_lcn_pipeline_probe(te, frames, idx, pat_lcn):
    """End-to-end index parity of the timed step whatever LCN kernel it ran: frame 0 RAW -> lcn(algo='exact') (the oracle's
    bits) -> reference-order NCC volume -> argmax, against the step's indices of frame 0.  With a tolerance-level LCN a few
    near-tie pixels may legitimately move (the reference's own LCN is a tolerance: ATen's conv2d summation order is
    unspecified, networks.py:523-533); tests/test_lcn_stream_gpu.py asserts every such pixel IS a near-tie of the exact
    volume.  Returns (mean |d idx|, pixels differing, pixels)."""
    import torch
    y, _ = te.lcn(frames[:1].contiguous(), LCN_RADIUS, LCN_EPS, algo="exact")
    ref_idx, _ = te.argmax_disp(te.xcorrvol_batch(y, pat_lcn, D, BS, algo="exact"))
    diff = (idx[:1].to(torch.int64) - ref_idx).abs()
    return float(diff.to(torch.float64).mean().item()), int((diff != 0).sum().item()), int(diff.numel())


def lcn_and_match(te, frames, pat_lcn, n_disp, lcn_algo, prepared, return_volume=True):
    """LCN + NCC volume + argmax of one batch the way --lcn-algo says; returns what the caller receives, by name:
    lcn, lcn_std, disparity_index, best_score and cost_volume (None without return_volume)."""
    if lcn_algo.startswith("fused"):
        out = te.lcn_xcorrvol_argmax(frames, pat_lcn, n_disp, BS, LCN_RADIUS, LCN_EPS, return_volume=return_volume,
                                     lcn_algo="exact" if lcn_algo == "fused_exact" else "fast", prepared=prepared)
        x, std, idx, best = out[:4]
        vol = out[4] if return_volume else None
    else:
        x, std = te.lcn(frames, LCN_RADIUS, LCN_EPS, algo=lcn_algo)
        out = te.xcorrvol_argmax(x, pat_lcn, n_disp, BS, return_volume=return_volume, prepared=prepared)
        idx, best = out[:2]
        vol = out[2] if return_volume else None
    return {"lcn": x, "lcn_std": std, "disparity_index": idx, "best_score": best, "cost_volume": vol}


DUMP_BYTES = 60 << 20                      # --dump-outputs: under 64 MB in all
DUMP_MIN_SAMPLE = 1 << 20                  # elements kept back for every array still to come
DUMP_SEED = 20240611


def dump_outputs(outdir, arrays):
    """--dump-outputs: write each (name, tensor) of `arrays` as outdir/<name>.npy, float32 (float64 stays float64;
    integer indices are exact in float32).  Smallest first, an array is written whole while it fits the budget
    left after DUMP_MIN_SAMPLE elements kept back for each array still to come; the arrays that do not share what
    remains as fixed samples: the flat (C-order) elements at the sorted indices
    np.random.RandomState(DUMP_SEED).randint(0, numel, k), the same in every run of the same shape.
    Returns name -> {"shape", "written", "sampled"} for the JSON line."""
    import numpy as np
    import torch
    os.makedirs(outdir, exist_ok=True)
    items = sorted(((n, t.detach()) for n, t in arrays if t is not None), key=lambda item: item[1].numel())
    size = [8 if t.dtype == torch.float64 else 4 for _, t in items]
    whole, left = [], DUMP_BYTES
    for i, (_, t) in enumerate(items):
        keep = DUMP_MIN_SAMPLE * sum(size[i + 1:])
        fits = t.numel() * size[i] <= left - keep
        whole.append(fits)
        if fits:
            left -= t.numel() * size[i]
    n_sampled = sum(size[i] for i in range(len(items)) if not whole[i])
    per = left // n_sampled if n_sampled else 0            # elements per sampled array
    manifest = {}
    for i, (name, t) in enumerate(items):
        t = t if t.dtype == torch.float64 else t.float()
        if whole[i] or per >= t.numel():
            a = t.contiguous().cpu().numpy()
        else:
            ix = np.sort(np.random.RandomState(DUMP_SEED).randint(0, t.numel(), size=per, dtype=np.int64))
            a = torch.take(t, torch.from_numpy(ix).to(t.device)).cpu().numpy()
        np.save(os.path.join(outdir, name + ".npy"), a)
        manifest[name] = {"shape": list(t.shape), "written": int(a.size), "sampled": int(a.size) < t.numel()}
    return manifest


def also_measured(te, L, frames, pat_lcn, args):
    """SURVEY 8d asks for two more numbers next to the step: (i) the volume-materialising kernel alone (no ranking in
    its epilogue: what ctd_xcorrvol_f32 launches), priced against the same roofline, and (ii) the fused, volume-free
    LCN -> NCC -> argmax (nothing materialised; bytes are inputs + indices only, so no HBM roofline applies).  Timed
    after the headline region, 20 repetitions each after 80 untimed ones, same inputs."""
    import ctypes
    import torch
    x, _ = te.lcn(frames, LCN_RADIUS, LCN_EPS, algo="exact" if args.lcn_algo in ("exact", "fused_exact") else "fast")
    L.ctd_kernel_timing_enable(1)
    for _ in range(80):                            # ~30 ms of the same work first: clocks (see the settle loop in main)
        te.xcorrvol_batch(x, pat_lcn, D, BS, algo="fast")
    torch.cuda.synchronize()
    L.ctd_kernel_timing_collect(None, None)
    for _ in range(20):
        te.xcorrvol_batch(x, pat_lcn, D, BS, algo="fast")
    torch.cuda.synchronize()
    L.ctd_kernel_timing_enable(0)
    ms, cols = ctypes.c_double(0), ctypes.c_int(0)
    n = L.ctd_kernel_timing_collect(ctypes.byref(ms), ctypes.byref(cols))
    units = args.frames * H * cols.value * D
    plain = {"kernel": "ncc_fast_alld_kernel without the ranking (volume only, what ctd_xcorrvol_f32 launches)", "avg_launch_ms": ms.value, "launches": n,
             "achieved_GBs": units * BYTES_PER_PIXDISP / (ms.value * 1e-3) / 1e9 if n else None,
             "frac_of_hbm_peak": units * BYTES_PER_PIXDISP / (ms.value * 1e-3) / 1e9 / HBM_PEAK_GBS if n else None}
    for _ in range(80):
        lcn_and_match(te, frames, pat_lcn, D, args.lcn_algo, None, return_volume=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        held = lcn_and_match(te, frames, pat_lcn, D, args.lcn_algo, None, return_volume=False)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 20
    fused = {"what": "LCN -> NCC -> argmax with reference indices, no volume materialised", "ms_per_step": dt * 1e3,
             "value": args.frames * H * W * D / dt / 1e6, "unit": "Mpix*disp/s",
             "valu_busy": committed_number("round4_sq_counters_alld.txt", "valu_busy"),
             "valu_busy_source": "profiles/round4_sq_counters_alld.txt (SQ pass of tools/pmc.sh on the no-store all-D kernel with the round-4 roles, committed)"}
    return {"volume_kernel_alone": plain, "fused_volume_free": fused}


def run_config4(args):
    """BASELINE configs[3], the HBM-bound stress: 1024x1024 frames, 256 disparities.  One step = LCN -> NCC volume
    (materialised, 1 GiB per frame) + argmax with reference indices -> soft-census (census_sad, eps 0.5) cost volume of
    the same frame by the census-transform kernel (another GiB).  `value` counts the pix*disp of BOTH volumes per step
    time; `roofline` prices the NCC volume kernel at 4.03125 B per pix*disp, `census` the census kernel at 4 B + inputs."""
    import ctypes
    import numpy as np
    import torch
    H4, W4, D4 = 1024, 1024, 256
    frames_n = args.frames if args.frames != 16 else 1
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    from connecting_the_dots_amd import _lib, torchext as te
    from tests import workloads
    L = _lib.lib()
    fr = torch.from_numpy(np.stack([workloads.uniform_frame(1234 + i, H4, W4) for i in range(frames_n)])).to(device)
    fr = fr.reshape(frames_n, 1, H4, W4).contiguous()
    pat = torch.from_numpy(workloads.syn_dot_pattern(H4, W4, seed=42)).to(device).reshape(1, 1, H4, W4)
    pat_lcn = te.lcn(pat.contiguous(), LCN_RADIUS, LCN_EPS)[0][0].contiguous()            # [1, H, W]
    bpp = 4.0 + 8.0 / D4
    prepared = te.prepare_pattern(pat_lcn, frames_n, D4, BS)     # the pattern half of the matcher's pre-pass, once per run

    def step():
        out = lcn_and_match(te, fr, pat_lcn, D4, args.lcn_algo, prepared)
        out["census_cost_volume"] = te.costvol(out["lcn"][:, 0], pat_lcn[0], D4, BS, "census_sad", 0.5, algo="fast")
        return out

    import gc
    gc.collect()
    gc.disable()
    L.ctd_kernel_timing_enable(2 * (args.steps + args.warmup) + 16)
    t_settle, settle_steps = time.perf_counter(), 0
    while time.perf_counter() - t_settle < 0.3 and settle_steps < 400:      # clocks (see the settle loop in main)
        held = step()
        settle_steps += 1
        if settle_steps % 10 == 0:
            torch.cuda.synchronize()
            L.ctd_kernel_timing_collect(None, None)
    for _ in range(args.warmup):
        held = step()
    torch.cuda.synchronize()
    L.ctd_kernel_timing_collect(None, None)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        held = step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    gc.enable()
    L.ctd_kernel_timing_enable(0)
    avg_ms, cols = ctypes.c_double(0), ctypes.c_int(0)
    n_launch = L.ctd_kernel_timing_collect(ctypes.byref(avg_ms), ctypes.byref(cols))
    dumped = dump_outputs(args.dump_outputs, list(held.items())) if args.dump_outputs else None
    x = held["lcn"]
    # the census kernel alone, device time (our kernels launch on torch's current stream, so torch events bracket them)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        te.costvol(x[:, 0], pat_lcn[0], D4, BS, "census_sad", 0.5, algo="fast")
    e0.record()
    for _ in range(args.steps):
        cen = te.costvol(x[:, 0], pat_lcn[0], D4, BS, "census_sad", 0.5, algo="fast")
    e1.record()
    torch.cuda.synchronize()
    cen_ms = e0.elapsed_time(e1) / args.steps
    units = frames_n * H4 * W4 * D4
    kernel_units = frames_n * H4 * cols.value * D4
    achieved = kernel_units * bpp / (avg_ms.value * 1e-3) / 1e9 if n_launch else None
    cen_bytes = units * 4.0 + frames_n * H4 * W4 * 8.0
    out = {
        "metric": "Mpix*disparities/s on 1024x1024x256 cost volumes (NCC + soft census, BOTH counted); config-4 line, not "
                  "comparable with the 512x432x128 headline",
        "value": 2 * units * args.steps / elapsed / 1e6, "unit": "Mpix*disp/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "settle_steps": settle_steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "BASELINE config 4 (configs[3]): %d frame(s) of 1024x1024, 256 disparities, block 9: LCN + NCC "
                               "cost volume (materialised) + argmax, then the soft-census (census_sad, eps 0.5) cost volume "
                               "of the same frame; value counts both volumes" % frames_n,
                   "frames_per_gpu": frames_n, "H": H4, "W": W4, "D": D4, "block_size": BS,
                   "device": torch.cuda.get_device_name(device)},
        "roofline": {"bound": "hbm", "kernel": "ncc_fast_alld_kernel (volume + ranking over every disparity in one workgroup)",
                     "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBS if achieved else None, "avg_launch_ms": avg_ms.value,
                     "launches": n_launch, "algorithmic_bytes_per_launch": kernel_units * bpp},
        "census": {"kernel": "costvol_census_kernel<3, 9> (census transform staged per tap, v_sad_u32 accumulation)",
                   "avg_launch_ms": cen_ms, "value": units / (cen_ms * 1e-3) / 1e6, "unit": "Mpix*disp/s",
                   "bound": "valu (81 v_sad_u32 per output) -- priced against the volume's bytes anyway",
                   "achieved_GBs": cen_bytes / (cen_ms * 1e-3) / 1e9, "frac_of_hbm_peak": cen_bytes / (cen_ms * 1e-3) / 1e9 / HBM_PEAK_GBS},
    }
    traffic, traffic_src = (measured_traffic("alld", "*_config4_pmc_hbm_traffic.json", None) if frames_n == 1 else (None, None))
    out["roofline"]["traffic"] = traffic
    out["roofline"]["traffic_source"] = (traffic_src + " (rocprofv3 --pmc passes of `bench.py --workload config4`, committed; not "
                                         "collected in this run)") if traffic_src else None
    # the separable SAD volume of the same frame (another GiB), device time
    for _ in range(10):
        te.costvol(x[:, 0], pat_lcn[0], D4, BS, "sad", 0.5, algo="fast")
    e0.record()
    for _ in range(args.steps):
        sad = te.costvol(x[:, 0], pat_lcn[0], D4, BS, "sad", 0.5, algo="fast")
    e1.record()
    torch.cuda.synchronize()
    sad_ms = e0.elapsed_time(e1) / args.steps
    del sad
    out["sad"] = {"kernel": "ncc_fast_alld_kernel in its SAD mode (box filter of |P[r][c-d] - I[r][c]|, one subtract per output) + "
                            "operand-plane copy", "avg_call_ms": sad_ms, "value": units / (sad_ms * 1e-3) / 1e6, "unit": "Mpix*disp/s",
                  "achieved_GBs": cen_bytes / (sad_ms * 1e-3) / 1e9, "frac_of_hbm_peak": cen_bytes / (sad_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
    # One frame is the hardest shape for the all-D kernel (4 column tiles: 256 workgroups means 16-row bands with 8 warm-up
    # rows each, nine passes).  The same kernel on a call of TWO such frames (32-row bands), priced the same way:
    if frames_n == 1:
        fr2 = torch.cat([fr, torch.from_numpy(workloads.uniform_frame(4321, H4, W4)).to(device).reshape(1, 1, H4, W4)])
        x2, _ = te.lcn(fr2, LCN_RADIUS, LCN_EPS, algo="exact" if args.lcn_algo in ("exact", "fused_exact") else "fast")
        prep2 = te.prepare_pattern(pat_lcn, 2, D4, BS)
        idx_timed = held["disparity_index"][:1].clone()  # (the one-frame step's volumes make room for the two-frame call's)
        del held
        L.ctd_kernel_timing_enable(2 * args.steps + 64)
        for _ in range(20):
            h2 = te.xcorrvol_argmax(x2, pat_lcn, D4, BS, return_volume=True, prepared=prep2)
        torch.cuda.synchronize()
        L.ctd_kernel_timing_collect(None, None)
        for _ in range(args.steps):
            h2 = te.xcorrvol_argmax(x2, pat_lcn, D4, BS, return_volume=True, prepared=prep2)
        torch.cuda.synchronize()
        L.ctd_kernel_timing_enable(0)
        ms2, c2 = ctypes.c_double(0), ctypes.c_int(0)
        n2 = L.ctd_kernel_timing_collect(ctypes.byref(ms2), ctypes.byref(c2))
        ach2 = 2 * H4 * c2.value * D4 * bpp / (ms2.value * 1e-3) / 1e9 if n2 else None
        out["ncc_two_frames_per_call"] = {"avg_launch_ms": ms2.value, "launches": n2, "achieved_GBs": ach2,
                                          "frac_of_hbm_peak": ach2 / HBM_PEAK_GBS if ach2 else None}
        del h2, x2, prep2, fr2
        held = {"lcn": x, "disparity_index": idx_timed}
    # indices of the timed step's frame 0 against the reference-order kernel on the same LCN'd frame (first index on ties)
    ref_vol = te.xcorrvol_batch(x[:1].contiguous(), pat_lcn, D4, BS, algo="exact")
    ref_idx, _ = te.argmax_disp(ref_vol)
    out["disparity_mae_vs_ref"] = float((held["disparity_index"][:1].to(torch.int64) - ref_idx).abs().to(torch.float64).mean().item())
    del ref_vol
    if not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_config4(pat_lcn.cpu(), x[0].cpu(), H4, W4, D4)
    if dumped is not None:
        out["dump_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
    emit(json.dumps(out))


def cpu_baseline_config4(pat_lcn_cpu, frame_lcn_cpu, H4, W4, D4):
    """The reference's CPU path on a bounded sample of config 4: (a) its xcorrvol_cpu on the full frame over the first
    16 of the 256 disparities, (b) its photometric_loss_forward (census_sad) composed into the cost volume
    over the first 8 disparities -- one core each (both loops are serial, ext_cpu.cpp:7-12)."""
    import numpy as np
    import torch
    try:
        from oracle import build_ref
        ref = build_ref.load()
    except Exception:
        ref = None
    torch.set_num_threads(1)
    a, b = frame_lcn_cpu.contiguous(), pat_lcn_cpu.contiguous()         # [1, H, W]
    dn, dc = 16, 8
    t0 = time.perf_counter()
    if ref is not None:
        ref.xcorrvol_cpu(a, b, dn, BS)
        kind = "reference"
    else:
        from oracle import oracle
        oracle.xcorrvol(a.numpy(), b.numpy(), dn, BS, nthreads=1)
        kind = "port"
    t_ncc = time.perf_counter() - t0
    cols = torch.arange(W4)
    t0 = time.perf_counter()
    for d in range(dc):
        pd = b[:, :, (cols - d).clamp(0, W4 - 1)].reshape(1, 1, H4, W4).contiguous()
        if ref is not None:
            ref.photometric_loss_forward(pd, a.reshape(1, 1, H4, W4), BS, 3, 0.5)
        else:
            from oracle import oracle
            oracle.photometric_fwd(pd.numpy(), a.reshape(1, 1, H4, W4).numpy(), BS, 3, 0.5)
    t_cen = time.perf_counter() - t0
    return {"value": H4 * W4 * dn / t_ncc / 1e6, "unit": "Mpix*disp/s", "cores": 1, "kind": kind,
            "sample": "NCC: the full 1024x1024 frame over the first %d of %d disparities (xcorrvol_cpu), %.1f s" % (dn, D4, t_ncc),
            "census": {"value": H4 * W4 * dc / t_cen / 1e6, "unit": "Mpix*disp/s", "cores": 1,
                       "sample": "photometric_loss_forward(census_sad) on the pattern shifted by d = 0..%d, %.1f s" % (dc - 1, t_cen)}}


_JSON_OUT = None


def protect_stdout():
    """The contract is ONE JSON line on stdout.  Libraries print there too (RCCL's version banner at communicator
    creation, for one): keep a private handle on the real stdout for the line and point fd 1 at stderr for everything
    else, C libraries included."""
    global _JSON_OUT
    if _JSON_OUT is None:
        sys.stdout.flush()
        _JSON_OUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)
    return _JSON_OUT


def emit(line):
    out = protect_stdout()
    out.write(line + "\n")
    out.flush()


def main():
    args = parse_args()
    if args.headline_only:
        args.no_parity_probe = args.no_cpu_baseline = True
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    protect_stdout()
    if args.workload == "config4":
        if args.gpus != 1:
            raise SystemExit("bench.py: --workload config4 is a one-GPU line")
        return run_config4(args)

    import numpy as np
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    backend = os.environ.get("CTD_DIST_BACKEND", "nccl")     # "nccl" is RCCL on ROCm; "gloo" for rehearsals
    err = check_gpu_count(world, backend, torch.cuda.device_count())
    if err:
        raise SystemExit(err)
    # one rank per GPU; the modulo only matters for the gloo rehearsal of the N > 1 path on a box with fewer GPUs
    dev_index = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    dist = None
    if world > 1 or args.force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:                      # --force-dist without a launcher: a free port of our own
            import socket
            sk = socket.socket()
            sk.bind(("127.0.0.1", 0))
            os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
            sk.close()
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    os.environ["CTD_NCC_ALGO"] = args.algo
    from connecting_the_dots_amd import _lib, sharding, torchext as te
    L = _lib.lib()

    frames, pattern = make_inputs(args.frames, rank, device)
    pat_lcn, _ = te.lcn(pattern, LCN_RADIUS, LCN_EPS)        # once per run, as exp_synph.py:64-71 does
    pat_lcn = pat_lcn[0].contiguous()
    # ... and so is the pattern half of the matcher's pre-pass (window statistics, fix-up lists of the pattern)
    prepared = te.prepare_pattern(pat_lcn, args.frames, D, BS) if args.algo == "fast" else None
    mae = None if args.no_parity_probe or rank != 0 else parity_probe(te, device)

    want2 = args.workload in (None, "config2")                   # the headline region (config 2)
    want3 = args.workload in (None, "config3")                   # the config-3 region
    K = torch.tensor([[FOCAL, 0, 324.7], [0, 570.2, 250.1], [0, 0, 1]], device=device)
    Ki = torch.linalg.inv(K.double()).float()
    geo = te.ProjectionDepthSimilarityLoss(K, Ki, H, W, clamp=0.1) if want3 else None
    if want3:
        R, t = make_poses(args.frames, rank, device)
        half = args.frames // 2                                 # pairs (i, i + half): both halves are contiguous slices
        Ra, ta, Rb, tb = R[:half].contiguous(), t[:half].contiguous(), R[half:2 * half].contiguous(), t[half:2 * half].contiguous()
    # the loss exchange of config 3 is queued without stalling the compute stream (sharding.gather_scalars_async): a
    # ring of four result buffers, each waited for (stream-level) when its slot comes round again and at the end
    ring = [None] * 4
    n_exchanged = [0]

    def step2():
        """config 2: LCN -> NCC volume (materialised) -> argmax with reference indices"""
        return lcn_and_match(te, frames, pat_lcn, D, args.lcn_algo, prepared)

    def step3(exchange=True):
        """config 3: the same, then disparity -> depth (+1: disparity 0 would be depth 1e12), the symmetric geometric loss
        of the frame pairs (i, i + frames/2) and the path's only exchange: every rank's loss scalar to every rank"""
        out = lcn_and_match(te, frames, pat_lcn, D, args.lcn_algo, prepared)
        depth = te.idx_to_depth(out["disparity_index"], FOCAL * BASELINE_M, 1.0).view(-1, 1, H, W)
        loss = geo(depth[:half], depth[half:2 * half], Ra, ta, Rb, tb)
        if exchange:
            k = n_exchanged[0] % len(ring)
            if ring[k] is not None and ring[k][1] is not None:
                ring[k][1].wait()
            src = loss if backend == "nccl" or dist is None else loss.cpu()
            buf, work = sharding.gather_scalars_async(src, out=None if ring[k] is None or dist is None else ring[k][0],
                                                      force=args.force_dist)
            ring[k] = (buf, work, src)
            n_exchanged[0] += 1
        out["geometric_loss"] = loss
        return out

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_region(step):
        """W untimed warm-up steps, then EXACTLY K steps between barrier + synchronize on both sides; returns (seconds,
        dominant kernel's average launch ms, its launches, columns it covers, the last step's outputs)."""
        for _ in range(args.warmup):
            held = step()
        barrier()
        L.ctd_kernel_timing_collect(None, None)   # (discard the warm-up's kernel timings)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            held = step()
        barrier()
        dt = time.perf_counter() - t0
        avg_ms, cols = ctypes.c_double(0), ctypes.c_int(0)
        n = L.ctd_kernel_timing_collect(ctypes.byref(avg_ms), ctypes.byref(cols))
        return dt, avg_ms.value, n, cols.value, held

    def max_over_ranks(seconds):
        if dist is None:
            return seconds
        tt = torch.tensor([seconds], device=device if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        return float(tt.item())

    # Settle first (not part of the W warm-up steps the contract asks for, and just as untimed).  Two things need it:
    # on a freshly booted box the first passes through the Python / allocator / code-object paths take several ms of
    # HOST time per step while the image pages in, and the card's power management needs some tens of ms of
    # continuous work before the clocks stop rising (measured: 0.70 -> 0.62 -> 0.60 ms per step over the first three
    # regions of 20 steps).  Run chunks of 10 synchronised steps until at least 0.25 s have gone by and two
    # consecutive chunks agree within 3 %, at most 100 chunks; `settle_steps` in the JSON line says how many ran.
    # (No collective in here: the number of settle steps differs from rank to rank.)
    # Everything slow on the host (the collector's full pass, ~50 ms) happens before it: the card drops its clocks
    # when it idles that long and then needs some 25 steps to get them back (measured: with the collector run between
    # the settle loop and 5 warm-up steps the 14 ms timed region came out 13 % slower, its dominant kernel 0.46
    # instead of 0.40 ms; with 25 warm-up steps it did not).
    # The cold number first: W warm-up steps and K timed steps straight after start-up, before any settling -- what a
    # caller sees who runs the contract's command on an idle card (clocks still ramping, code objects and allocator
    # pools freshly touched).  Reported as `cold_ms_per_step` next to the steady-state `ms_per_step`.
    import ctypes
    head = step2 if want2 else (lambda: step3(exchange=False))
    L.ctd_kernel_timing_enable(2 * (args.steps + args.warmup) + 16)   # (the argument also sizes the event pool)
    for _ in range(args.warmup):
        head()
    torch.cuda.synchronize()
    t_c = time.perf_counter()
    for _ in range(args.steps):
        held = head()
    torch.cuda.synchronize()
    cold_ms = (time.perf_counter() - t_c) / args.steps * 1e3
    L.ctd_kernel_timing_collect(None, None)
    import gc
    gc.collect()
    gc.disable()                                  # no collector pauses from here to the end of the timed regions
    prev, settle_steps, t_settle, burst_ms = None, 0, time.perf_counter(), None
    for _ in range(100):
        t_s = time.perf_counter()
        for _ in range(10):
            spare, held = held, head()            # outputs held like in the timed loop, plus the set this function
                                                  # holds while it runs that loop: the caching allocator ends up owning
                                                  # all three sets, so no timed step allocates (with --warmup 1 the first
                                                  # timed step used to; a 4-step region once came out at 13 ms per step)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t_s
        L.ctd_kernel_timing_collect(None, None)
        settle_steps += 10
        burst_ms = dt * 100 if burst_ms is None else min(burst_ms, dt * 100)
        if prev is not None and abs(dt - prev) <= 0.03 * min(dt, prev) and time.perf_counter() - t_settle >= 0.25:
            break
        prev = dt
    spare = None
    # ---- headline region: config 2 (config 3 when --workload config3 asks for that region alone)
    elapsed, avg_launch_ms, n_launch, cols, head_out = timed_region(head if want2 else step3)
    held = None                                   # from here on head_out is the one set held between regions
    x, idx = head_out["lcn"], head_out["disparity_index"]
    # run-to-run spread: two more regions of the same K steps (reported next to the headline one, never instead of it)
    repeats = []
    if not args.headline_only:
        for _ in range(2):
            repeats.append(timed_region(head if want2 else step3)[0] / args.steps * 1e3)
    # ---- second region: config 3, straight behind (clocks stay up), same K / W, its own barriers
    c3 = None
    if want2 and want3:
        for _ in range(10):
            step3(exchange=False)                 # the geometric kernels' first launches (code objects, workspaces): untimed
        c3_elapsed, _, _, _, c3_out = timed_region(step3)
        c3 = max_over_ranks(c3_elapsed)
        head_out["config3_geometric_loss"] = c3_out["geometric_loss"]
        del c3_out
    gc.enable()
    L.ctd_kernel_timing_enable(0)
    L.ctd_kernel_timing_collect(None, None)
    dumped = dump_outputs(args.dump_outputs, list(head_out.items())) if args.dump_outputs and rank == 0 else None
    elapsed = max_over_ranks(elapsed)
    ranks_seen = dist.get_world_size() if dist is not None else 1

    mae_timed = mae_e2e = None
    if rank == 0 and mae is not None and args.algo == "fast":
        mae_timed = timed_workload_probe(te, x, idx, pat_lcn)
        mae_e2e = exact_lcn_pipeline_probe(te, frames, idx, pat_lcn)
    elif mae is not None:
        mae_timed = mae
    if rank == 0:
        units_per_step = world * args.frames * H * W * D
        value = units_per_step * args.steps / elapsed / 1e6
        kernel_units = args.frames * H * cols * D
        achieved = kernel_units * BYTES_PER_PIXDISP / (avg_launch_ms * 1e-3) / 1e9 if n_launch else None
        kernel = "ncc_fast_alld_kernel" if args.algo == "fast" else "ncc_exact_kernel"
        lcn_text = {"fused": "frame LCN + window statistics fused into one streaming kernel (f32 box sums)",
                    "fused_exact": "frame LCN + window statistics fused into one streaming kernel (f64 box sums: the oracle's bits)",
                    "fast": "frame LCN as its own call (tiled kernel, f32 box sums)",
                    "exact": "frame LCN as its own call (tiled kernel, f64 box sums: the oracle's bits)"}[args.lcn_algo]
        what2 = ("BASELINE config 2: batch=16 512x432 frames per GPU, 128 disparities, block 9, LCN(r=5,eps=0.05) + NCC "
                 "cost volume (materialised) + argmax; pattern LCN'd and prepared once per run; " + lcn_text)
        what3 = ("BASELINE config 3: 16 frames per GPU (%d in all), LCN + NCC cost volume (materialised) + argmax + "
                 "disparity->depth + two-view geometric loss on frame pairs + all-gather of the loss scalar" % (world * args.frames))
        par = "frames sharded over %d GPU(s), one process per GPU, no collective in this step" % world
        par3 = "frames sharded over %d GPU(s), one process per GPU%s" % (
            world, "" if dist is None else ", one non-blocking all-gather of a scalar per step (%s)" % ("RCCL" if backend == "nccl" else backend))
        out = {
            "metric": "Mpix*disparities/s on 512x432x128 cost volume; disparity MAE vs ref",
            "value": value,
            "unit": "Mpix*disp/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "cold_ms_per_step": cold_ms,
            "fastest_settle_chunk_ms_per_step": burst_ms,     # 10 steps, clocks up and the card not yet power-limited: NOT the headline
            "repeat_ms_per_step": repeats,
            "settle_steps": settle_steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": (what2 if want2 else what3) + ", algo=%s" % args.algo,
                       "frames_per_gpu": args.frames, "H": H, "W": W, "D": D, "block_size": BS,
                       "parallelism": par if want2 else par3,
                       "ranks_seen": ranks_seen, "device": torch.cuda.get_device_name(device)},
            # the worst of: the reference's committed golden (one raw frame pair, before the warm-up), frame 0 of the timed
            # workload against the reference-order kernel on the step's own LCN output, and -- detail only, see there -- the
            # whole pipeline from the RAW frame through the exact LCN
            "disparity_mae_vs_ref": None if mae is None else max(mae, mae_timed),
            "disparity_mae_detail": None if mae is None else {
                "golden_cfg1_frame_pair": mae, "timed_workload_frame0_vs_reference_order_kernel": mae_timed,
                "timed_workload_frame0_vs_exact_lcn_pipeline": None if mae_e2e is None else {
                    "mae": mae_e2e[0], "pixels_differing": mae_e2e[1], "pixels": mae_e2e[2],
                    "note": "raw frame -> lcn(algo='exact') -> reference-order volume -> argmax against the step's indices; 0 "
                            "differing pixels when the step's LCN carries the oracle's bits, near-tie pixels only otherwise "
                            "(tests/test_lcn_stream_gpu.py)"}},
            "roofline": {
                "bound": "hbm",
                "kernel": kernel + (" (volume + ranking over every disparity in one workgroup)" if args.algo == "fast" else ""),
                "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS if achieved else None,
                "avg_launch_ms": avg_launch_ms, "launches": n_launch,
                "algorithmic_bytes_per_launch": kernel_units * BYTES_PER_PIXDISP,
            },
        }
        if c3 is not None:
            out["config3"] = {"workload": what3, "parallelism": par3, "steps": args.steps, "warmup": args.warmup,
                              "ms_per_step": c3 / args.steps * 1e3, "value": units_per_step * args.steps / c3 / 1e6,
                              "unit": "Mpix*disp/s"}
        traffic, traffic_src = measured_traffic(kernel)
        out["roofline"]["traffic"] = traffic
        out["roofline"]["traffic_source"] = (traffic_src + " (rocprofv3 --pmc passes of this build, committed; not collected in this run)") if traffic_src else None
        # second denominator: what a kernel that does NOTHING but this kernel's stores (same grid, same wave-instructions,
        # same LDS-limited residency, non-temporal) reaches on THIS card, measured now by the microbenchmark
        # tools/bin/ctd_store_ceiling (tools/ubench_src/store_ceiling.hip, built by __graft_entry__.build()); cards differ by
        # more than 10 % here (profiles/round3_store_ceiling.txt), so a committed number would not do.  NOT a ceiling of the
        # kernel: the paced kernel has been seen a few per cent above its bare pattern (round-4 verdict) -- hence the name.
        ceil_tbs, ceil_src, ceil_burst, card_tbs, card_pat = None, None, None, None, None
        exe = os.path.join(ROOT, "tools", "bin", "ctd_store_ceiling")
        if want2 and world == 1 and os.path.exists(exe) and not args.headline_only:
            try:
                import ctypes as _ct
                off = (_ct.c_size_t * 5)()
                L.ctd_xcorrvol_rank_layout(args.frames, H, W, D, 0, off)          # off[0]: the kernel's band height
                # (a plain child process, started after the timed regions: never an exec from this GPU-initialised parent)
                txt = subprocess.run([exe, "pattern", str(int(off[0]))], capture_output=True, timeout=120).stdout.decode()
                for line in txt.splitlines():
                    if line.startswith("all_d_pattern_store_only_TBs"):
                        ceil_tbs = float(line.split("=")[1])
                        ceil_src = ("measured in this run after 0.6 s of continuous launches, like the timed region "
                                    "(tools/bin/ctd_store_ceiling pattern %d)" % int(off[0]))
                    if line.startswith("all_d_pattern_store_only_burst_TBs"):
                        ceil_burst = float(line.split("=")[1])
                    if line.startswith("card_best_store_only_TBs"):
                        card_tbs = float(line.split("=")[1])
                    if line.startswith("card_best_pattern"):
                        card_pat = line.split("=", 1)[1].strip()
            except Exception:                                  # noqa: BLE001
                pass
        if ceil_tbs is None:
            ceil_tbs = committed_number("round3_store_ceiling_summary.txt", "all_d_pattern_store_only_TBs")
            ceil_src = "profiles/round3_store_ceiling_summary.txt (another card: indicative only)" if ceil_tbs else None
        if ceil_tbs and achieved:
            # two store-only rates measured on THIS card at the same 1.81 GB: the kernel's own pattern (26 planes per
            # workgroup, 13 storing wavefronts per CU) and the best pattern known for the card (few wavefronts per CU writing
            # interleaved contiguous pieces in step) -- the layout [N, D, H, W] does not let a workgroup that owns every
            # disparity of its pixels write that way (profiles/round4_store_streams.txt)
            out["roofline"]["pattern_store_only_rate"] = {"GBs": ceil_tbs * 1e3, "frac_of_peak": ceil_tbs * 1e3 / HBM_PEAK_GBS,
                                                          "kernel_frac_of_it": achieved / (ceil_tbs * 1e3), "source": ceil_src}
            if ceil_burst:        # the same launches right after start-up: the card is not yet power-limited
                out["roofline"]["pattern_store_only_rate"]["burst_GBs"] = ceil_burst * 1e3
            if card_tbs:
                out["roofline"]["pattern_store_only_rate"].update({
                    "card_best_GBs": card_tbs * 1e3, "card_best_frac_of_peak": card_tbs * 1e3 / HBM_PEAK_GBS,
                    "card_best_pattern": card_pat, "kernel_frac_of_card_best": achieved / (card_tbs * 1e3)})
        if want3 and n_exchanged[0]:
            last = ring[(n_exchanged[0] - 1) % len(ring)]
            if last[1] is not None:
                last[1].wait()
            gathered = [float(v) for v in last[0].flatten().tolist()]
            (out["config3"] if c3 is not None else out["config"])["loss_allgather"] = gathered
        if dist is None and args.algo == "fast" and not args.headline_only and want2:
            out["also_measured"] = also_measured(te, L, frames, pat_lcn, args)
        if not args.no_cpu_baseline and dist is None:          # rank 0 at N = 1 only
            out["cpu_baseline"] = cpu_baseline(pat_lcn.cpu(), x[:min(args.frames, 32)].cpu())
        if dumped is not None:
            out["dump_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        emit(json.dumps(out))
    if dist is not None:
        for slot in ring:                                          # no exchange left in flight at tear-down
            if slot is not None and slot[1] is not None:
                slot[1].wait()
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
