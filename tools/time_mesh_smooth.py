"""Times the mesh connectivity, smoothing and vertex normals (csrc/mesh_smooth.hip) and writes profiles/mesh_smooth.txt:
ctd_mesh_adjacency_i32, one and ten iterations of ctd_mesh_smooth_f32 and ctd_mesh_vertex_normals_f32, on the two scene
meshes of profiles/point_mesh.txt and profiles/render_bvh.txt (tests/bvh_scenes.get_mesh_like: about 71 K and 987 K faces).
    python tools/time_mesh_smooth.py [--faces 100000 1000000] [--reps 30] [--out profiles/mesh_smooth.txt]
Device time from HIP events around each call, after warm-up calls; median / min / max over the repetitions.  Each time
stands beside the compulsory bytes of the call (every array it has to read or write once; the gathers fall on arrays
already counted; the workspace traffic of the adjacency build and the atomics are not counted) and the share of the
device's copy rate that this comes to, the copy rate measured here by a device-to-device copy of 256 MiB (read + write).

Each time also stands beside the same result from stock torch ops on the device, which is what a user has without these
kernels: the half-edge list by torch.unique over the keys i * n + j (with counts: the multiplicities), a smoothing pass
by index_add_ over the half-edge list, the normals by index_add_ of the face cross products.  torch's index_add_ adds
with floating-point atomics, so its sums run in no fixed order; the results are compared within a tolerance, not bitwise.
The report ends with what the smoothing buys on the fused scenes of tests/test_mesh_smooth_host.py, computed on the host."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import _lib, meshsmooth  # noqa: E402
from tools.time_tsdf import median_ms  # noqa: E402

COPY_BYTES = 256 << 20


def copy_rate(reps):
    a = torch.empty(COPY_BYTES, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    t = median_ms(lambda: b.copy_(a), reps, 5)[0]
    return 2.0 * COPY_BYTES / (t * 1e-3)


def torch_adjacency(faces, n):
    """the one-rings by stock ops: unique half-edges (sorted by i, then j) with their multiplicities, row starts"""
    f = faces.long()
    ok = ((f >= 0) & (f < n)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])
    v = f[ok]
    src = v[:, [0, 0, 1, 1, 2, 2]].reshape(-1)
    dst = v[:, [1, 2, 0, 2, 0, 1]].reshape(-1)
    key, mult = torch.unique(src * n + dst, return_counts=True)
    i, j = torch.div(key, n, rounding_mode="floor"), key % n
    deg = torch.bincount(i, minlength=n)
    offsets = torch.cat([deg.new_zeros(1), torch.cumsum(deg, 0)])
    boundary = torch.zeros(n, dtype=torch.bool, device=faces.device)
    boundary[i[mult == 1]] = True
    return i, j, deg, offsets, boundary


def torch_pass(x, i, j, deg, hold, f):
    s = torch.zeros_like(x).index_add_(0, i, x.index_select(0, j))
    m = s / deg.clamp(min=1).to(x.dtype)[:, None]
    return torch.where(hold[:, None], x, x + f * (m - x))


def torch_smooth(x, i, j, deg, boundary, iters, lam, mu):
    hold = boundary | (deg == 0)
    for _ in range(iters):
        x = torch_pass(x, i, j, deg, hold, lam)
        x = torch_pass(x, i, j, deg, hold, mu)
    return x


def torch_normals(x, faces):
    f = faces.long()
    v0, v1, v2 = x[f[:, 0]], x[f[:, 1]], x[f[:, 2]]
    c = torch.cross(v1 - v0, v2 - v0, dim=1)
    acc = torch.zeros_like(x)
    for k in range(3):
        acc.index_add_(0, f[:, k], c)
    return acc / acc.norm(dim=1, keepdim=True)


def truth_section(say):
    """what the smoothing buys on the fused scenes of tests/test_mesh_smooth_host.py (host side, the restatement)"""
    from tests import mesh_ref, meshclean_ref, meshsmooth_ref, tsdf_ref
    from tests.test_mesh_smooth_host import MEASURED_MEDIAN_RATIO
    from tests.test_tsdf_host import fused_scene
    say("what it buys (host side, tests/meshsmooth_ref.py, 10 x (lambda 0.5 | mu -0.53), boundary held): the fused scenes of "
        "tests/test_tsdf_host.fused_scene,")
    say("meshed by tests/mesh_ref.faces and cleaned with min_faces = 32; distance of the vertices to the true surfaces "
        "(tests/tsdf_ref.scene_surface_distance)")
    for kind, seed in sorted(MEASURED_MEDIAN_RATIO):
        sc = fused_scene(kind, seed, masked=True)
        faces, _ = mesh_ref.faces(sc["tsdf"], sc["weight"])
        c = meshclean_ref.clean(faces, len(sc["points"]), min_faces=32)
        verts = sc["points"][c["vert_index"]]
        adj = meshsmooth_ref.adjacency(c["faces"], len(verts))
        out = meshsmooth_ref.smooth(verts, adj["offsets"], adj["neighbors"], adj["vflags"])
        d0, d1 = tsdf_ref.scene_surface_distance(verts), tsdf_ref.scene_surface_distance(out)
        say("  %-5s seed %d: %d vertices, %d faces, %d boundary edges; median %.3e -> %.3e (ratio %.3f); mean %.3e -> %.3e (ratio %.3f)"
            % (kind, seed, len(verts), len(c["faces"]), adj["counts"][2], np.median(d0), np.median(d1), np.median(d1) / np.median(d0),
               d0.mean(), d1.mean(), d1.mean() / d0.mean()))
    say()


def report(targets, reps, warmup=10):
    from tests import bvh_scenes
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s.rstrip())

    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rate = copy_rate(reps)
    say("mesh connectivity by vertex, Taubin smoothing (lambda 0.5 | mu -0.53, boundary held) and area-weighted vertex normals")
    say("scene meshes of tests/bvh_scenes.get_mesh_like (the meshes of profiles/point_mesh.txt and profiles/render_bvh.txt)")
    say("device %s; median / min / max of %d calls (device time, HIP events), after %d warm-up calls"
        % (torch.cuda.get_device_name(0), reps, warmup))
    say("copy rate measured here: %.3f TB/s (device-to-device copy of %d MiB, read + write); compulsory bytes from the sizes; "
        "share = bytes / median / copy rate" % (rate / 1e12, COPY_BYTES >> 20))
    say("torch: the same result from stock torch ops on the device (torch.unique over the half-edge keys; index_add_ over the "
        "half-edge list)")
    say()
    fmt = "  %-30s %8.4f / %8.4f / %8.4f ms  %10d B  %6.4f TB/s = %5.1f %% of the copy rate | torch %9.4f ms = x %6.2f  (%s)"

    def line(what, tm, nbytes, t_torch, note):
        r = nbytes / (tm[0] * 1e-3)
        say(fmt % ((what,) + tm + (nbytes, r / 1e12, 100.0 * r / rate, t_torch, t_torch / tm[0], note)))

    for target in targets:
        v, _, f = bvh_scenes.get_mesh_like(target, 0)
        verts, faces = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
        n, m = verts.shape[0], faces.shape[0]
        adj = meshsmooth.MeshAdjacency(faces, n)
        nnz, n_inc = adj.neighbors.shape[0], adj.face_ids.shape[0]
        say("%d faces, %d vertices: %d edges (%d boundary, %d non-manifold), at most %d faces at a vertex, euler %d%s"
            % (m, n, adj.n_edges, adj.n_boundary_edges, adj.n_nonmanifold_edges, adj.max_incident, adj.euler,
               ", closed" if adj.closed else ""))
        ws = torch.empty(L.ctd_mesh_adjacency_workspace_bytes(n, m), dtype=torch.uint8, device="cuda")
        offsets, face_offsets = torch.empty(n + 1, dtype=torch.int32, device="cuda"), torch.empty(n + 1, dtype=torch.int32, device="cuda")
        neighbors, face_ids = torch.empty(6 * m, dtype=torch.int32, device="cuda"), torch.empty(3 * m, dtype=torch.int32, device="cuda")
        vflags, counts = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(6, dtype=torch.int64, device="cuda")

        def build():
            _lib.check(L.ctd_mesh_adjacency_i32(faces.data_ptr(), n, m, offsets.data_ptr(), neighbors.data_ptr(), 6 * m,
                                                face_offsets.data_ptr(), face_ids.data_ptr(), 3 * m, vflags.data_ptr(),
                                                counts.data_ptr(), ws.data_ptr(), ws.numel(), 0, stream), "ctd_mesh_adjacency_i32")

        sws = torch.empty(max(L.ctd_mesh_smooth_workspace_bytes(n), 256), dtype=torch.uint8, device="cuda")
        out = torch.empty_like(verts)

        def smooth(iters):
            _lib.check(L.ctd_mesh_smooth_f32(verts.data_ptr(), n, adj.offsets.data_ptr(), adj.neighbors.data_ptr(), nnz,
                                             adj.vflags.data_ptr(), iters, 0.5, -0.53, 1, out.data_ptr(), sws.data_ptr(),
                                             sws.numel(), 0, stream), "ctd_mesh_smooth_f32")

        normals = torch.empty_like(verts)

        def normal():
            _lib.check(L.ctd_mesh_vertex_normals_f32(verts.data_ptr(), n, faces.data_ptr(), m, adj.face_offsets.data_ptr(),
                                                     adj.face_ids.data_ptr(), n_inc, normals.data_ptr(), 0, stream),
                       "ctd_mesh_vertex_normals_f32")

        i, j, deg, _, boundary = torch_adjacency(faces, n)
        b_build = 12 * m + 8 * (n + 1) + 4 * nnz + 4 * n_inc + n
        b_pass = 12 * n + 4 * (n + 1) + 4 * nnz + n + 12 * n
        b_normals = 12 * n + 12 * m + 4 * (n + 1) + 4 * n_inc + 12 * n
        t = median_ms(build, reps, warmup)
        assert torch.equal(offsets, adj.offsets) and torch.equal(neighbors[:nnz], adj.neighbors) and torch.equal(vflags, adj.vflags)
        assert torch.equal(j.int(), adj.neighbors) and torch.equal(boundary, (adj.vflags & 2) != 0)
        line("adjacency build", t, b_build, median_ms(lambda: torch_adjacency(faces, n), reps, warmup)[0],
             "faces read; offsets, neighbors, face_offsets, face_ids, vflags written")
        for iters in (1, 10):
            t = median_ms(lambda: smooth(iters), reps, warmup)
            want = torch_smooth(verts, i, j, deg, boundary, iters, 0.5, -0.53)
            err = float((out - want).abs().max())
            line("smoothing, %2d iteration%s" % (iters, "" if iters == 1 else "s"), t, 2 * iters * b_pass,
                 median_ms(lambda: torch_smooth(verts, i, j, deg, boundary, iters, 0.5, -0.53), reps, warmup)[0],
                 "%d passes: positions read and written, offsets, neighbors, vflags; largest difference to torch %.1e" % (2 * iters, err))
        t = median_ms(normal, reps, warmup)
        want = torch_normals(verts, faces)
        both = torch.isfinite(want).all(1) & torch.isfinite(normals).all(1)
        line("vertex normals", t, b_normals, median_ms(lambda: torch_normals(verts, faces), reps, warmup)[0],
             "positions, faces, face_offsets, face_ids read, normals written; largest difference to torch %.1e"
             % float((normals - want)[both].abs().max()))
        t = median_ms(lambda: meshsmooth.MeshAdjacency(faces, n), reps, warmup)
        say("  %-30s %8.4f / %8.4f / %8.4f ms  (allocation, the build, one synchronisation, copies of the two lists)"
            % (("meshsmooth.MeshAdjacency",) + t))
        t = median_ms(lambda: meshsmooth.mesh_smooth(verts, faces, adjacency=adj), reps, warmup)
        say("  %-30s %8.4f / %8.4f / %8.4f ms  (allocation and the ten iterations, no synchronisation)"
            % (("meshsmooth.mesh_smooth",) + t))
        say()
    truth_section(say)
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[100000, 1000000], help="targets of tests/bvh_scenes.get_mesh_like")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_mesh_smooth.py needs a GPU"
    text = report(args.faces, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
