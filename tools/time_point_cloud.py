"""Time of the point-cloud family (pointcloud: PointGrid, knn, the three consumers) next to the only stock equivalent,
chunked torch.cdist + topk, and next to one unhinted point_mesh_distance query of as many points.

The scenes are those of the mesh profiles (tests/bvh_scenes.get_mesh_like at 10^5 and 10^6 target faces, without the
board's two triangles): area-weighted surface samples (mesheval.sample_surface, seeded), 10^5 of them and as many as the
scene has faces.  Per scene and count:
  grid       PointGrid(points) with the default cell, and the cell the rule chose
  knn        knn(grid, k) for k = 8, 16, 32, 64, the points querying themselves, with the compulsory bytes (12 q in,
             8 q k out) and what they come to per second
  cells      with --cells: knn at k = 16 for cells of 0.25 .. 8 times the default one (how the default rule was tuned)
  consumers  neighbor_mean_distance, estimate_normals (both include their knn at k = 16), voxel_downsample at the
             default cell (includes its grid)
  cdist      at 10^5 points only: torch.cdist of chunks of --chunk queries against all points, topk(k + 1) of each
             (the point itself is among them), k = 16; a fraction --cdist-fraction of the chunks is run and the time scaled
  mesh       the unhinted point_mesh_distance of the same points through a prebuilt tree: one traversal per point
Device-event times, the minimum and the median over --reps after a warm-up of each.  No counters are collected here.

    python tools/time_point_cloud.py [--faces 100000 1000000] [--reps 10] [--cells] [--out profiles/point_cloud.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--faces", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--cdist-fraction", type=float, default=1.0)
    ap.add_argument("--cells", action="store_true", help="sweep the cell size at k = 16")
    ap.add_argument("--out", default=None, help="append the table to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from connecting_the_dots_amd import mesheval, renderer
    from connecting_the_dots_amd import pointcloud as pc
    from tests import bvh_scenes

    if not torch.cuda.is_available():
        raise SystemExit("time_point_cloud.py measures on the GPU; there is none here")
    dev = torch.device("cuda", 0)

    def timed(fn, reps):
        """-> (last result, min ms, median ms)"""
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return out, min(ts), float(np.median(ts))

    def cdist_topk(p, k, fraction):
        chunks = list(range(0, p.shape[0], args.chunk))
        run = chunks[:max(1, int(round(len(chunks) * fraction)))]
        for a in run:
            d = torch.cdist(p[a:a + args.chunk], p)
            d.topk(k + 1, dim=1, largest=False)
        return len(chunks) / len(run)

    lines = ["surface samples of the mesh-profile scenes; reps %d; times in ms, min / median; default-cell rule: fill %g, "
             "at most %d doublings" % (args.reps, pc.DEFAULT_CELL_FILL, pc.DEFAULT_CELL_DOUBLINGS)]
    for nf in args.faces:
        v, _, f = bvh_scenes.get_mesh_like(nf, 0)
        f = np.ascontiguousarray(f[2:])                                   # without the board
        vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        tree = renderer.MeshBVH(vt, ft)
        gen = torch.Generator(device=dev)
        for n in sorted({args.points, len(f)}):
            gen.manual_seed(1)
            p = mesheval.sample_surface(vt, ft, n, gen)[0].contiguous()
            grid, g_lo, g_md = timed(lambda: pc.PointGrid(p), args.reps)
            lines.append("scene %d faces, %d points: PointGrid %8.3f / %8.3f   cell %.5g, dims %s, %d cells (%.2f points each), "
                         "%.1f MB" % (len(f), n, g_lo, g_md, grid.cell, grid.dims, grid.n_cells, n / grid.n_cells, grid.nbytes / 1e6))
            base16 = None
            for k in (8, 16, 32, 64):
                (idx, d2), lo, md = timed(lambda: pc.knn(grid, k), args.reps)
                byt = 12 * n + 8 * n * k
                base16 = md if k == 16 else base16
                lines.append("    knn k = %2d  %9.3f / %9.3f   %.1f M queries/s   compulsory %.1f MB = %.1f GB/s" % (
                    k, lo, md, n / md * 1e-3, byt / 1e6, byt / md * 1e-6))
            if args.cells:
                for scale in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0):
                    g2 = pc.PointGrid(p, grid.cell * scale)
                    _, lo, md = timed(lambda: pc.knn(g2, 16), max(3, args.reps // 2))
                    lines.append("    cell x %-5g (%.2f points a cell): knn k = 16 %9.3f / %9.3f" % (scale, n / g2.n_cells, lo, md))
            _, lo, md = timed(lambda: pc.neighbor_mean_distance(grid, 16), args.reps)
            lines.append("    neighbor_mean_distance k = 16 (with its knn) %9.3f / %9.3f" % (lo, md))
            _, lo, md = timed(lambda: pc.estimate_normals(grid, 16), args.reps)
            lines.append("    estimate_normals k = 16 (with its knn)       %9.3f / %9.3f" % (lo, md))
            vd, lo, md = timed(lambda: pc.voxel_downsample(p, grid.cell), args.reps)
            lines.append("    voxel_downsample at that cell (with its grid) %9.3f / %9.3f -> %d points" % (lo, md, vd.points.shape[0]))
            _, lo, md = timed(lambda: mesheval.point_mesh_distance(p, vt, ft, bvh=tree), max(3, args.reps // 2))
            lines.append("    point_mesh_distance, unhinted, through the tree %9.3f / %9.3f" % (lo, md))
            if n == args.points:
                scale, lo, md = timed(lambda: cdist_topk(p, 16, args.cdist_fraction), max(2, args.reps // 3))
                lines.append("    chunked cdist + topk(17), chunks of %d%s %9.3f / %9.3f   knn k = 16 takes %.4f of it (%.0f times faster)" % (
                    args.chunk, "" if scale == 1 else " (measured on 1 / %.1f of the chunks and scaled)" % scale, lo * scale,
                    md * scale, base16 / (md * scale), md * scale / base16))
            print("\n".join(lines), flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write("\n".join(lines) + "\n")
            lines = []


if __name__ == "__main__":
    main()
