"""Times the mesh clean-up (csrc/mesh_clean.hip) and writes profiles/mesh_clean.txt: ctd_mesh_components_i32, the count-only
call and the full call of ctd_mesh_clean_i32, and the wrappers meshops.mesh_clean and meshops.clean_tsdf_mesh, on the
meshes of the 4-track corner workload of profiles/tsdf.txt (tools/time_tsdf.py: 4 tracks x 4 views x 512 x 432 into
256^3 voxels per track, meshed by mesh.tsdf_mesh).
    python tools/time_mesh_clean.py [--reps 100] [--grid 256] [--min-faces 32] [--kernel-stats DIR] [--out profiles/mesh_clean.txt]
Device time from HIP events around each call, after warm-up calls; median / min / max over the repetitions.  The compulsory
bytes of a pass (every array it has to read or write once; gathers fall on arrays already counted, except the positions,
which count once per vertex; the traffic of the atomics is not counted) come from the sizes and from what is kept, and a
call's bytes are the sum over its passes.

The passes one by one come from the profiler, in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_mesh_clean.py --passes-of 0 --reps 200
runs nothing but the full ctd_mesh_clean_i32 call on track 0 (after building the mesh), and --kernel-stats DIR of a later
plain run appends the kernels' median times from DIR's kernel_trace.csv, each against its compulsory bytes.  The report
ends with what the clean-up buys on the fused scenes of tests/test_mesh_clean_host.py, computed on the host."""
import argparse
import csv
import glob
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import _lib, mesh, meshops  # noqa: E402
from connecting_the_dots_amd import torchext as te  # noqa: E402
from tests import icp_ref  # noqa: E402
from tools.time_tsdf import CENTRE, EXTENT, SHAPE, median_ms  # noqa: E402

HBM_PEAK = 8.0e12                                              # bytes / s


def corner_mesh(shape, n):
    B, V, H, W = shape
    sc = icp_ref.make_corner(B, V, H, W, 1)
    depth, ray, K, R, t = [torch.from_numpy(np.ascontiguousarray(sc[k])).cuda() for k in ("depth", "ray", "K", "R", "t")]
    voxel = EXTENT / n
    origin = torch.tensor([[c - 0.5 * voxel * (n - 1) for c in CENTRE]] * B, dtype=torch.float32, device="cuda")
    T, w = te.tsdf_volume(B, n, n, n)
    te.tsdf_integrate(T, w, origin, voxel, depth, ray, K, R, t)
    return mesh.tsdf_mesh(T, w, origin, voxel, return_normals=True)


def truth_section(say, min_faces):
    """what the clean-up buys on the fused scenes of tests/test_mesh_clean_host.py (host side, the restatement)"""
    from tests import mesh_ref, meshclean_ref, tsdf_ref
    from tests.test_mesh_clean_host import MEASURED_RATIO
    from tests.test_tsdf_host import fused_scene
    say("what it buys (host side, tests/meshclean_ref.py, min_faces = %d): the fused scenes of tests/test_tsdf_host.fused_scene, "
        "valid=keep, meshed by tests/mesh_ref.faces;" % min_faces)
    say("share of the vertices farther than a voxel from the true surfaces (tests/tsdf_ref.scene_surface_distance) and mean distance")
    for kind, seed in sorted(MEASURED_RATIO):
        sc = fused_scene(kind, seed, masked=True)
        faces, _ = mesh_ref.faces(sc["tsdf"], sc["weight"])
        d = tsdf_ref.scene_surface_distance(sc["points"])
        c = meshclean_ref.clean(faces, len(d), min_faces=min_faces)
        kept = c["vert_index"]
        far0, far1 = (d > sc["voxel"]).mean(), (d[kept] > sc["voxel"]).mean()
        say("  %-5s seed %d: %d vertices, %d faces, %d components -> %d vertices, %d faces, %d components; far share %.2f %% -> "
            "%.2f %% (ratio %.3f); mean distance %.2e -> %.2e" % (kind, seed, len(d), len(faces), c["counts"][2], c["counts"][0],
                                                               c["counts"][1], c["counts"][3], 100 * far0, 100 * far1,
                                                               far1 / far0, d.mean(), d[kept].mean()))
    say()


def pass_bytes(nv, nf, kv, kf):
    """compulsory bytes of each pass for a mesh of nv vertices and nf faces of which kv and kf are kept"""
    cf, cv = (nf + 255) // 256 + 1, (nv + 255) // 256 + 1
    return {
        "mc_init_kernel": (9 * nv, "parent, counter, kept byte written"),
        "mc_union_kernel": (12 * nf + 12 * nv + 4 * nf, "faces, positions once per vertex, root written"),
        "mc_flatten_kernel": (8 * nf, "root read and written"),
        "mc_roots_kernel": (8 * nv, "parent, counter"),
        "mc_sizes_kernel": (8 * nf, "root read, size written"),
        "mc_flag_kernel": (5 * nf + 12 * kf + kv, "root, flag written, kept faces' indices, their vertices' bytes"),
        "mc_vert_count_kernel": (nv, "kept bytes"),
        "fuse_scan_kernel": (8 * (cf + cv) // 2, "counts read, offsets written; average of the two scans"),
        "mc_vert_scatter_kernel": (5 * nv + 4 * kv, "kept bytes, new indices written, vert_index"),
        "mc_face_scatter_kernel": (nf + 28 * kf, "flags, kept faces read, faces_out and face_index written"),
    }


COMPONENTS = ("mc_init_kernel", "mc_union_kernel", "mc_flatten_kernel", "mc_roots_kernel", "mc_sizes_kernel")
COUNT_ONLY = ("mc_init_kernel", "mc_union_kernel", "mc_flatten_kernel", "mc_roots_kernel", "mc_flag_kernel",
              "mc_vert_count_kernel", "fuse_scan_kernel", "fuse_scan_kernel")
FULL = COUNT_ONLY + ("mc_vert_scatter_kernel", "mc_face_scatter_kernel")


def kernel_stats(path):
    """kernel name (without namespace and arguments) -> (calls, median, least, largest ns) over the dispatches of a rocprofv3
    kernel_trace.csv from the first mc_init_kernel on: what comes before it builds the mesh"""
    if os.path.isdir(path):
        path = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)[-1]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    times, started = {}, False
    for r in rows:
        name = re.search(r"(\w+)(?:<.*>)?\(", r["Kernel_Name"].replace("(anonymous namespace)", ""))
        name = name.group(1) if name else r["Kernel_Name"]
        started = started or name == "mc_init_kernel"
        if started:
            times.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    return {k: (len(v), float(np.median(v)), float(min(v)), float(max(v))) for k, v in times.items()}


def passes_only(shape, grid, min_faces, track, reps, warmup=10):
    """the full clean call on one track, reps times: what the profiler run traces"""
    m = corner_mesh(shape, grid)
    verts, faces, _ = m.track(track)
    nv, nf = verts.shape[0], faces.shape[0]
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(L.ctd_mesh_clean_workspace_bytes(nv, nf), dtype=torch.uint8, device="cuda")
    counts = torch.empty(4, dtype=torch.int64, device="cuda")
    fo = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
    fi, vi = torch.empty(nf, dtype=torch.int32, device="cuda"), torch.empty(nv, dtype=torch.int32, device="cuda")
    for _ in range(warmup + reps):
        _lib.check(L.ctd_mesh_clean_i32(faces.data_ptr(), verts.data_ptr(), nv, nf, 1, min_faces, 0, fo.data_ptr(), fi.data_ptr(),
                                        nf, vi.data_ptr(), nv, counts.data_ptr(), ws.data_ptr(), ws.numel(), 0, stream),
                   "ctd_mesh_clean_i32")
    torch.cuda.synchronize()
    print("track %d: %d vertices, %d faces; %d full calls; counts %s" % (track, nv, nf, warmup + reps, counts.tolist()))


def report(shape, grid, min_faces, reps, warmup=10, stats=None):
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s.rstrip())

    B = shape[0]
    m = corner_mesh(shape, grid)
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    say("mesh clean-up: components, removal of components of fewer than %d faces and of faces with coincident vertices, "
        "compaction" % min_faces)
    say("meshes of mesh.tsdf_mesh over the workload of profiles/tsdf.txt: %d tracks x %d views x %dx%d into %d^3 voxels per "
        "track (corner scene of tests/icp_ref.py)" % (B, shape[1], shape[3], shape[2], grid))
    say("device %s; median / min / max of %d calls (device time, HIP events), after %d warm-up calls"
        % (torch.cuda.get_device_name(0), reps, warmup))
    say("compulsory bytes from the sizes and from what is kept; rate = bytes / median; share of the %.1f TB/s HBM peak"
        % (HBM_PEAK / 1e12))
    say()
    fmt = "  %-34s %8.4f / %8.4f / %8.4f ms  %10d B  %6.4f TB/s = %5.2f %% of peak  (%s)"

    def line(what, tm, nbytes, note):
        rate = nbytes / (tm[0] * 1e-3)
        say(fmt % ((what,) + tm + (nbytes, rate / 1e12, 100.0 * rate / HBM_PEAK, note)))

    for b in range(B):
        verts, faces, normals = m.track(b)
        nv, nf = verts.shape[0], faces.shape[0]
        c = meshops.mesh_clean(verts, faces, min_faces=min_faces, normals=normals)
        kv, kf = c.verts.shape[0], c.faces.shape[0]
        _, size, _ = meshops.mesh_components(faces, nv)
        say("track %d: %d vertices, %d faces, %d components (the largest of %d faces); kept %d vertices, %d faces in %d components"
            % (b, nv, nf, c.n_components, int(size.max()) if nf else 0, kv, kf, c.n_components_kept))
        ws = torch.empty(L.ctd_mesh_clean_workspace_bytes(nv, nf), dtype=torch.uint8, device="cuda")
        label = torch.empty(nf, dtype=torch.int32, device="cuda")
        sizes = torch.empty(nf, dtype=torch.int32, device="cuda")
        counts = torch.empty(4, dtype=torch.int64, device="cuda")
        fo = torch.empty((nf, 3), dtype=torch.int32, device="cuda")
        fi = torch.empty(nf, dtype=torch.int32, device="cuda")
        vi = torch.empty(nv, dtype=torch.int32, device="cuda")

        def components():
            _lib.check(L.ctd_mesh_components_i32(faces.data_ptr(), verts.data_ptr(), nv, nf, 1, label.data_ptr(),
                                                 sizes.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), 0, stream),
                       "ctd_mesh_components_i32")

        def clean(outputs):
            p = (lambda x: x.data_ptr()) if outputs else (lambda x: None)
            _lib.check(L.ctd_mesh_clean_i32(faces.data_ptr(), verts.data_ptr(), nv, nf, 1, min_faces, 0, p(fo), p(fi), nf, p(vi),
                                            nv, counts.data_ptr(), ws.data_ptr(), ws.numel(), 0, stream), "ctd_mesh_clean_i32")

        pb = pass_bytes(nv, nf, kv, kf)
        b_comp, b_count, b_full = (sum(pb[k][0] for k in ks) for ks in (COMPONENTS, COUNT_ONLY, FULL))
        t_comp = median_ms(components, reps, warmup)
        t_count = median_ms(lambda: clean(False), reps, warmup)
        t_full = median_ms(lambda: clean(True), reps, warmup)
        line("components call", t_comp, b_comp, "init, union, flatten, roots, sizes")
        line("clean: count-only call", t_count, b_count, "init, union, flatten, roots, flag, vertex count, 2 scans")
        line("clean: full call", t_full, b_full, "the same + vertex scatter, face scatter with the remap")
        assert torch.equal(fo[:kf], c.faces) and torch.equal(vi[:kv], c.vert_index)
        t_wrap = median_ms(lambda: meshops.mesh_clean(verts, faces, min_faces=min_faces, normals=normals), reps, warmup)
        say("  %-34s %8.4f / %8.4f / %8.4f ms  (allocation, full call, one synchronisation, copies of the kept rows, gathers)"
            % (("meshops.mesh_clean (wrapper)",) + t_wrap))
        if stats is not None and b == 0:
            say("  the passes of the full call, kernel time from rocprofv3 --kernel-trace in a run of its own, median (least .. largest):")
            total = 0.0
            for k in dict.fromkeys(FULL):
                calls, avg, lo, hi = stats[k]                      # (avg: the median)
                total += avg * FULL.count(k)
                rate = pb[k][0] / (avg * 1e-9)
                say("    %-26s %5d calls  %8.2f us (%7.2f .. %7.2f)  %9d B  %6.4f TB/s = %5.2f %% of peak  (%s)"
                    % (k, calls, avg / 1e3, lo / 1e3, hi / 1e3, pb[k][0], rate / 1e12, 100.0 * rate / HBM_PEAK, pb[k][1]))
            say("    the ten kernels of a call together: %.2f us" % (total / 1e3))
        say()
    t_all = median_ms(lambda: meshops.clean_tsdf_mesh(m, min_faces=min_faces), reps, warmup)
    say("%-36s %8.4f / %8.4f / %8.4f ms  (%d tracks one after the other, one synchronisation each)"
        % (("meshops.clean_tsdf_mesh (wrapper)",) + t_all + (B,)))
    say()
    truth_section(say, min_faces)
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--passes-of", type=int, default=None, help="only the full clean call on this track (for the profiler)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 output directory or kernel_trace.csv of a --passes-of run")
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--min-faces", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_mesh_clean.py needs a GPU"
    if args.passes_of is not None:
        passes_only(SHAPE, args.grid, args.min_faces, args.passes_of, args.reps)
        return
    text = report(SHAPE, args.grid, args.min_faces, args.reps,
                  stats=kernel_stats(args.kernel_stats) if args.kernel_stats else None)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
