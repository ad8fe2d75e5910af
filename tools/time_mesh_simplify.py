"""Times the mesh simplification (csrc/mesh_simplify.hip) and writes profiles/mesh_simplify.txt: ctd_mesh_simplify_f32 at cells
of 2, 4 and 8 mean edge lengths on the two scene meshes of profiles/point_mesh.txt and profiles/mesh_smooth.txt
(tests/bvh_scenes.get_mesh_like: about 71 K and 987 K faces).
    python tools/time_mesh_simplify.py [--faces 100000 1000000] [--reps 30] [--out profiles/mesh_simplify.txt]
Device time from HIP events around each call, after warm-up calls; median / min / max over the repetitions.  Each time
stands beside the compulsory bytes of the call (every input and output array once; the gathers fall on arrays already
counted; the workspace traffic, the two tables among it, and the atomics are not counted) and the share of the device's
copy rate that this comes to, the copy rate measured here by a device-to-device copy of 256 MiB (read + write).
The call reads the incident-face rows of a meshsmooth.MeshAdjacency, which the torch route does not need: its build is
NOT in the times of the call; it is timed on a line of its own, and the last line of a mesh is the whole of
meshsimplify.mesh_simplify with the adjacency built inside, which is what simplify_tsdf_mesh pays per track.

Each time also stands beside the stock-torch route on the device, which is what a user has without these kernels:
torch.unique over the cell keys, index_add_ for the clusters' means (mean placement only: there is no quadric solve in
it), torch.unique over the sorted cluster triples.  Its cluster and face counts are compared with the kernels'; its
positions are not (index_add_ adds with floating-point atomics in no fixed order, and they are means).  Where the kernels
lose to that route, the line says so."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from connecting_the_dots_amd import _lib, meshsimplify, meshsmooth  # noqa: E402
from tools.time_mesh_smooth import copy_rate  # noqa: E402
from tools.time_tsdf import median_ms  # noqa: E402

COPY_BYTES = 256 << 20


def torch_simplify(verts, faces, origin, cell):
    """clustering by stock ops, mean placement -> (means [c,3], cluster of every vertex or -1, kept faces [k,3], clusters)"""
    n = verts.shape[0]
    f = faces.long()
    ok = ((f >= 0) & (f < n)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])
    t = torch.floor((verts - origin) / torch.full_like(verts[:1], cell))   # (a tensor: a true division, as in the rule)
    used = torch.zeros(n, dtype=torch.bool, device=verts.device)
    used[f[ok].reshape(-1)] = True
    cl = used & ((t >= 0) & (t < meshsimplify.MAX_CELLS_PER_AXIS)).all(1)
    i = t[cl].long()
    uk, inv, cnt = torch.unique((i[:, 0] << 40) | (i[:, 1] << 20) | i[:, 2], return_inverse=True, return_counts=True)
    cid = torch.full((n,), -1, dtype=torch.long, device=verts.device)
    cid[cl] = inv
    mean = torch.zeros((uk.shape[0], 3), dtype=verts.dtype, device=verts.device).index_add_(0, inv, verts[cl])
    mean = mean / cnt.to(verts.dtype)[:, None]
    tri = cid[f[ok]]
    tri = tri[(tri >= 0).all(1)]
    tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 0] != tri[:, 2]) & (tri[:, 1] != tri[:, 2])]
    _, first = torch.unique(torch.sort(tri, 1)[0], dim=0, return_inverse=True)
    keep = torch.zeros(tri.shape[0], dtype=torch.bool, device=verts.device)
    at = torch.full((int(first.max()) + 1 if first.numel() else 0,), tri.shape[0], dtype=torch.long, device=verts.device)
    at.scatter_reduce_(0, first, torch.arange(tri.shape[0], device=verts.device), "amin")
    keep[at] = True
    return mean, cid, tri[keep], uk.shape[0]


def report(targets, reps, warmup=10):
    from tests import bvh_scenes
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s.rstrip())

    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    rate = copy_rate(reps)
    say("mesh simplification: uniform-grid vertex clustering with quadric placement (reg 1e-3, drop_duplicates)")
    say("scene meshes of tests/bvh_scenes.get_mesh_like (the meshes of profiles/point_mesh.txt and profiles/mesh_smooth.txt)")
    say("device %s; median / min / max of %d calls (device time, HIP events), after %d warm-up calls"
        % (torch.cuda.get_device_name(0), reps, warmup))
    say("copy rate measured here: %.3f TB/s (device-to-device copy of %d MiB, read + write); compulsory bytes from the sizes; "
        "share = bytes / median / copy rate" % (rate / 1e12, COPY_BYTES >> 20))
    say("torch: clustering with mean placement by stock torch ops on the device (torch.unique over the cell keys, index_add_ "
        "means, torch.unique over the sorted triples)")
    say("the call reads the face_offsets / face_ids of a meshsmooth.MeshAdjacency, which the torch route does not need: that "
        "build is NOT in the times of the cell lines; it has a line of its own below them")
    say()
    fmt = "  %-22s %8.4f / %8.4f / %8.4f ms  %10d B  %6.4f TB/s = %5.1f %% of the copy rate | torch %9.4f ms = x %6.2f  (%s)"
    for target in targets:
        v, _, f = bvh_scenes.get_mesh_like(target, 0)
        verts, faces = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
        n, m = verts.shape[0], faces.shape[0]
        adj = meshsmooth.MeshAdjacency(faces, n)
        n_inc = adj.face_ids.shape[0]
        fl = faces.long()
        edge = torch.cat([(verts[fl[:, a]] - verts[fl[:, b]]).norm(dim=1) for a, b in ((0, 1), (1, 2), (2, 0))])
        mean_edge, median_edge = float(edge.mean()), float(edge.median())
        origin = verts.amin(0)
        o = [float(x) for x in origin.cpu()]
        say("%d faces, %d vertices; edge length: mean %.5f, median %.5f (the board's two faces are 1000 wide); origin = the "
            "smallest coordinates" % (m, n, mean_edge, median_edge))
        ws = torch.empty(L.ctd_mesh_simplify_workspace_bytes(n, m), dtype=torch.uint8, device="cuda")
        say("  workspace %d B = %.1f B per vertex + face" % (ws.numel(), ws.numel() / (n + m)))
        verts_out, leader = torch.empty((n, 3), device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        vert_cluster = torch.empty(n, dtype=torch.int32, device="cuda")
        faces_out, face_index = torch.empty((m, 3), dtype=torch.int32, device="cuda"), torch.empty(m, dtype=torch.int32, device="cuda")
        counts = torch.empty(8, dtype=torch.int64, device="cuda")
        for k in (2, 4, 8):
            cell = float(torch.tensor(k * mean_edge, dtype=torch.float32))

            def call():
                _lib.check(L.ctd_mesh_simplify_f32(verts.data_ptr(), n, faces.data_ptr(), m, adj.face_offsets.data_ptr(),
                                                   adj.face_ids.data_ptr(), n_inc, o[0], o[1], o[2], cell, 1e-3, 1,
                                                   verts_out.data_ptr(), leader.data_ptr(), n, vert_cluster.data_ptr(),
                                                   faces_out.data_ptr(), face_index.data_ptr(), m, counts.data_ptr(), ws.data_ptr(),
                                                   ws.numel(), 0, stream), "ctd_mesh_simplify_f32")

            tm = median_ms(call, reps, warmup)
            c = counts.cpu().tolist()
            _, _, tri, n_clusters = torch_simplify(verts, faces, origin, cell)
            same = n_clusters == c[2] and tri.shape[0] == c[1]
            t_torch = median_ms(lambda: torch_simplify(verts, faces, origin, cell), reps, warmup)[0]
            nbytes = 12 * n + 12 * m + 4 * (n + 1) + 4 * n_inc + 16 * c[0] + 4 * n + 16 * c[1] + 64
            r = nbytes / (tm[0] * 1e-3)
            note = "%d -> %d faces, %d -> %d vertices; %d collapsed, %d duplicates, %d unclusterable, %d mean fall-backs, largest " \
                   "cluster %d; torch %s%s" % (m, c[1], n, c[0], c[4], c[5], c[3], c[6], c[7],
                                               "counts the same clusters and faces" if same else
                                               "counts %d clusters and %d faces" % (n_clusters, tri.shape[0]),
                                               "; the kernels LOSE to the torch route here" if t_torch < tm[0] else "")
            say(fmt % (("cell = %d mean edges" % k,) + tm + (nbytes, r / 1e12, 100.0 * r / rate, t_torch, t_torch / tm[0], note)))
        cell = float(torch.tensor(4 * mean_edge, dtype=torch.float32))
        t = median_ms(lambda: meshsimplify.mesh_simplify(verts, faces, cell, origin=o, adjacency=adj), reps, warmup)
        say("  %-22s %8.4f / %8.4f / %8.4f ms  (cell = 4 mean edges, a ready adjacency: allocation, the call, one "
            "synchronisation, copies of the outputs)" % (("meshsimplify.mesh_simplify",) + t))
        t_adj = median_ms(lambda: meshsmooth.MeshAdjacency(faces, n), reps, warmup)
        say("  %-22s %8.4f / %8.4f / %8.4f ms  (what the cell lines leave out: allocation, the build, one synchronisation, "
            "copies of the two lists)" % (("meshsmooth.MeshAdjacency",) + t_adj))
        t_all = median_ms(lambda: meshsimplify.mesh_simplify(verts, faces, cell, origin=o), reps, warmup)
        say("  %-22s %8.4f / %8.4f / %8.4f ms  (cell = 4 mean edges, the adjacency built inside: what simplify_tsdf_mesh pays "
            "per track, without normals)" % (("mesh_simplify, all of it",) + t_all))
        say()
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[100000, 1000000], help="targets of tests/bvh_scenes.get_mesh_like")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_simplify.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_mesh_simplify.py needs a GPU"
    text = report(args.faces, args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
