"""Times the mesh extraction (csrc/tsdf_mesh.hip) and writes profiles/tsdf_mesh.txt: the count call and the fill call of
ctd_tsdf_mesh_faces_i32 and the whole mesh.tsdf_mesh (surface points, count, one synchronisation, fill), each beside
torchext.tsdf_surface_points of the same volume, on two volumes: the corner model of tests/tsdf_ref.make_corner_model
with the constants of tests/test_tsdf_host.py (72 x 48 x 32 voxels, what the reference-scene test meshes) and a sphere
in 256^3 voxels, B = 1.
    python tools/time_tsdf_mesh.py [--reps 30] [--grid 256] [--out profiles/tsdf_mesh.txt]
Device time from HIP events around each call, after warm-up calls; median / min / max over the repetitions.  The
compulsory bytes of a call (every array it has to read or write once; the gathers of neighbours fall on arrays already
counted) come from the shape and from what the volume holds."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import _lib, mesh  # noqa: E402
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import test_tsdf_host as th  # noqa: E402

HBM_PEAK = 8.0e12                                              # bytes / s


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


def corner_volume():
    sc = th.corner_model()
    vw = sc["views"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    T, w = te.tsdf_volume(1, *th.CORNER_DIMS)
    origin = up(sc["origin"])
    te.tsdf_integrate(T, w, origin, sc["voxel"], up(vw["depth"]), up(sc["ray"]), up(sc["K"]), up(vw["R"]), up(vw["t"]))
    return T, w, origin, sc["voxel"]


def sphere_volume(n):
    """tsdf = clamp((|x - centre| - 0.37 n) / 4 voxels, -1, 1), weight 1 everywhere: the band |tsdf| < 1 is 8 voxels thick"""
    ax = torch.arange(n, dtype=torch.float32, device="cuda")
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    c = (n - 1) / 2.0
    d = torch.sqrt((x - (c + 0.13)) ** 2 + (y - (c - 0.21)) ** 2 + (z - (c + 0.07)) ** 2) - 0.37 * n
    T = torch.clamp(d / 4.0, -1.0, 1.0).unsqueeze(0).contiguous()
    return T, torch.ones_like(T), torch.zeros((1, 3), device="cuda"), 1.0


def section(say, name, T, w, origin, voxel, reps, warmup=10):
    B, nz, ny, nx = T.shape
    voxels = B * nx * ny * nz
    L = _lib.lib()
    m = mesh.tsdf_mesh(T, w, origin, voxel, return_normals=True)
    n_verts, n_faces = m.verts.shape[0], m.faces.shape[0]
    weighted, usable = int((w >= 1).sum()), int(((w >= 1) & (T.abs() < 1)).sum())
    say("%s: %d x %d x %d voxels, B = %d; %d weighted, %d usable; %d vertices, %d faces" % (name, nx, ny, nz, B, weighted, usable,
                                                                                        n_verts, n_faces))
    ws = torch.empty(L.ctd_tsdf_mesh_workspace_bytes(B, nx, ny, nz), dtype=torch.uint8, device="cuda")
    counts = torch.zeros(B, dtype=torch.int64, device="cuda")
    faces = torch.empty((max(n_faces, 1), 3), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def c_call(f, cap):
        st = L.ctd_tsdf_mesh_faces_i32(T.data_ptr(), w.data_ptr(), 1.0, f, counts.data_ptr(), cap, B, nx, ny, nz, ws.data_ptr(),
                                       ws.numel(), 0, stream)
        _lib.check(st, "ctd_tsdf_mesh_faces_i32")

    chunks = B * ((nx * ny * nz + 255) // 256)
    # flags pass: weight, tsdf behind it, flags out; case pass: flags in, weight + tsdf again, a case per voxel and a first
    # index per flagged voxel (at most one per vertex) out; the two scans: counts out and in
    b_count = (4 * voxels + 4 * weighted + voxels) + (voxels + 4 * voxels + 4 * weighted + voxels + 4 * n_verts) + 4 * 4 * chunks
    # the offsets again, per face 3 x (index + flags) gathered and 12 B out (the cases of the workgroups that have faces: not
    # counted)
    b_fill = b_count + 8 * chunks + n_faces * (15 + 12)
    fmt = "  %-34s %8.4f / %8.4f / %8.4f ms  %12d B  %6.3f TB/s = %5.1f %% of peak  (%s)"

    def line(what, tm, nbytes, note):
        rate = nbytes / (tm[0] * 1e-3)
        say(fmt % ((what,) + tm + (nbytes, rate / 1e12, 100.0 * rate / HBM_PEAK, note)))

    line("mesh faces: count call", median_ms(lambda: c_call(None, 0), reps, warmup), b_count,
         "flags, scan, first indices + cases, scan")
    line("mesh faces: fill call", median_ms(lambda: c_call(faces.data_ptr(), n_faces), reps, warmup), b_fill,
         "the count pass again, cases read, %d faces written" % n_faces)
    assert torch.equal(faces[:n_faces], m.faces)
    t_pts = median_ms(lambda: te.tsdf_surface_points(T, w, origin, voxel, return_normals=True), reps, warmup)
    t_all = median_ms(lambda: mesh.tsdf_mesh(T, w, origin, voxel, return_normals=True), reps, warmup)
    say("  %-34s %8.4f / %8.4f / %8.4f ms  (count, one synchronisation, allocation, fill + normals)" %
        (("tsdf_surface_points (wrapper)",) + t_pts))
    say("  %-34s %8.4f / %8.4f / %8.4f ms  (tsdf_surface_points, then faces: count, one synchronisation, fill)" %
        (("mesh.tsdf_mesh (wrapper)",) + t_all))
    say("  the faces on top of the points: %.4f ms = %.2f x tsdf_surface_points" % (t_all[0] - t_pts[0], (t_all[0] - t_pts[0]) / t_pts[0]))
    say()


def report(grid, reps, warmup=10):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s.rstrip())

    say("mesh extraction: marching cubes over a truncated signed distance volume, faces indexing the surface points")
    say("device %s; median / min / max of %d calls (device time, HIP events), after %d warm-up calls"
        % (torch.cuda.get_device_name(0), reps, warmup))
    say("compulsory bytes from the shape and the volume; rate = bytes / median; share of the %.1f TB/s HBM peak" % (HBM_PEAK / 1e12))
    say()
    section(say, "corner model (tests/test_tsdf_host.py)", *corner_volume(), reps, warmup)
    section(say, "sphere", *sphere_volume(grid), reps, warmup)
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_mesh.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_tsdf_mesh.py needs a GPU"
    text = report(args.grid, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
