"""Point clouds without a mesh (include/ext/ctd_hip_point_cloud.h, csrc/point_cloud.hip): exact k-nearest-neighbours
among bare points over a sorted grid of cells, and what rests on it: a statistical outlier mask, covariance normals and a
voxel-mean down-sample.  For the `points [M,3]` that `depth_fuse_points` and `tsdf_surface_points` end in, or points from
anywhere else.

    grid = pointcloud.PointGrid(points)                        # built once, like renderer.MeshBVH
    idx, d2 = pointcloud.knn(grid, 16)                         # int32 [n,16], f32 [n,16]: exact, ascending (d2, index)
    idx, d2 = pointcloud.knn(grid, 8, queries=other, max_dist=0.05)
    keep, mean_dist, info = pointcloud.statistical_outlier_mask(grid, k=16, std_ratio=2.0)
    normals, variation, ok = pointcloud.estimate_normals(grid, k=16, toward=pointcloud.view_centers(src, R, t, (V, H, W)))
    thin = pointcloud.voxel_downsample(points, 0.01)           # .points, .count, .cell_of_point, .first, .attributes

The chain for fused points: `depth_fuse_points` -> `PointGrid` -> `statistical_outlier_mask` -> `PointGrid(points[keep])`
-> `estimate_normals(toward=view_centers(...))` -> `meshrobust.robust_mesh_icp(normals=, min_cos=)`.

One track per call: slice a batch by its `n_per_track`.  What this does not do: no batching across tracks, no radius
queries (all points within a distance), no k above 64, nothing differentiable, and no consistent orientation of normals
without viewpoints.

The header's prototypes are bound here, onto the library handle of `_lib.lib()` at first use; this table is not one of
`_lib.TABLES`.  No fallback to torch: a missing kernel is an error.
"""
import ctypes
import math

import torch

from . import _lib
from ._meshargs import _flag, _nx3
from .torchext._common import _call, _check, _integer, _number, _ptr, _same_device, _stream

_c_int, _c_float, _vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p

HEADER = "ext/ctd_hip_point_cloud.h"

# mirrors include/ext/ctd_hip_point_cloud.h one to one, in the header's order (tests/test_point_cloud_host.py)
TABLE = {
    "ctd_point_cell_keys_f32": (_c_int, [_vp, _c_int, _c_float, _c_float, _c_float, _c_float, _vp]),
    "ctd_point_knn_f32": (_c_int, [_vp, _vp, _c_int, _vp, _vp, _c_int, _c_int, _c_int, _c_int, _c_float, _c_float, _c_float,
                                   _c_float, _vp, _c_int, _c_int, _c_float, _vp, _vp]),
    "ctd_point_mean_dist_f32": (_c_int, [_vp, _c_int, _c_int, _vp]),
    "ctd_point_normals_f32": (_c_int, [_vp, _c_int, _vp, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp]),
    "ctd_point_voxel_mean_f32": (_c_int, [_vp, _c_int, _c_int, _vp, _vp, _c_int, _vp]),
}
for _sig in TABLE.values():
    _sig[1].extend([_c_int, _vp])                             # every call ends in (device, stream)

MAX_K = 64
MAX_DIM = 1 << 21                                             # cells per axis: three coordinates in one int64 key
MAX_ATTRIBUTES = 64
NO_CELL = 2 ** 63 - 1                                         # the key of a point of no cell
# the default-cell rule (profiles/point_cloud.txt has the timings that chose them)
DEFAULT_CELL_FILL = 4.0                                       # double until the occupied cells hold this many points on average
DEFAULT_CELL_DOUBLINGS = 8

_bound = None


def lib():
    """the handle of `_lib.lib()` with this module's prototypes bound"""
    global _bound
    if _bound is None:
        l = _lib.lib()
        for name, (res, args) in TABLE.items():
            fn = getattr(l, name)           # AttributeError here means header / library mismatch
            fn.restype = res
            fn.argtypes = args
        _bound = l
    return _bound


_RULE = """
    The rule (include/ext/ctd_hip_point_cloud.h).  For a finite query q and a finite point p with the original index i:
    d2 = ((dx * dx) + (dy * dy)) + (dz * dz) with dx = p_0 - q_0 and so on, in f32 in this association.  p is a candidate
    when d2 <= max_dist^2 (squared once on the host, as f32; None: no limit) and d2 < +inf.  The neighbours are the k
    candidates that come first in ascending (d2, i) order: the lower index wins a tie.  With queries=None the points query
    themselves and a point is excluded from its own list by index: a coincident other point stays, with d2 = 0.  Where
    fewer than k candidates exist the rest are idx = -1, d2 = +inf; a query that is not finite gets only those.  The
    result is the exact answer, bit-equal to brute force under this rule for every `cell`."""


def _f32(x):
    return ctypes.c_float(x).value


def _cell_keys(points, origin, cell, who):
    n = points.shape[0]
    keys = torch.empty((n,), dtype=torch.int64, device=points.device)
    _call(lib().ctd_point_cell_keys_f32, who, _ptr(points) or None, n, origin[0], origin[1], origin[2], cell,
          _ptr(keys) or None, points.device.index, _stream(points.device))
    return keys


class PointGrid:
    """The sorted grid of cells over points f32 [n,3] (a CUDA tensor), built once and reused by `knn`, the consumers and
    `voxel_downsample`.  A point p lies in the cell g_c = floorf((p_c - origin_c) / cell), in f32, with origin the minimum
    of the finite points; a point with a NaN or an infinity belongs to no cell: it is never a neighbour, and as a query it
    gets empty results.  At most 2^21 cells per axis (the three coordinates share one int64 key, x in the lowest bits);
    a smaller `cell` than that allows is an error.  The keys are sorted with `torch.sort(stable=True)`; there is no hash
    table and nothing depends on the order the points came in.

    cell=None picks one deterministically: (the longest side of the finite points' box) / sqrt(n_finite), doubled until
    the occupied cells hold at least DEFAULT_CELL_FILL = 4 points on average, at most DEFAULT_CELL_DOUBLINGS = 8 times
    (1 when the box is a single point).  On surface samples that ends near 8 or 9 points a cell, the fastest of the
    sizes tried at k = 16 (profiles/point_cloud.txt).  No result depends on `cell`, only the time.

    Attributes: `points` (the tensor it was built from, which must not change), `cell` (float, as f32), `origin` (three
    floats), `dims` (nx, ny, nz), `n_cells` (occupied ones), `n_finite`, `order` int32 [n] (the original indices in
    sorted order, the points of no cell last), `keys` int64 [n_cells] ascending, `start` int32 [n_cells + 1],
    `sorted_points` f32 [n_finite,3], `nbytes`.  Building synchronises (the origin and the dims come to the host)."""

    def __init__(self, points, cell=None):
        who = "PointGrid"
        _nx3(points, who, "points", torch.float32)
        if cell is not None:
            cell = _f32(_number(cell, "cell", who, lo_open=True))
            if not 0 < cell < float("inf"):
                raise RuntimeError("%s: cell must be a positive finite f32, got %r" % (who, cell))
        n = points.shape[0]
        self.points, self.n = points, n
        finite = torch.isfinite(points).all(dim=1)
        self.n_finite = int(finite.sum()) if n else 0
        dev = points.device
        if self.n_finite == 0:
            self.cell, self.origin, self.dims, self.n_cells = (1.0 if cell is None else cell), (0.0, 0.0, 0.0), (1, 1, 1), 0
            self.order = torch.arange(n, dtype=torch.int32, device=dev)
            self.keys = torch.zeros((0,), dtype=torch.int64, device=dev)
            self.start = torch.zeros((1,), dtype=torch.int32, device=dev)
            self.sorted_points = points[:0].contiguous()
            return
        inf = torch.full_like(points, float("inf"))
        lo = torch.where(finite[:, None], points, inf).amin(dim=0)
        hi = torch.where(finite[:, None], points, -inf).amax(dim=0)
        self.origin = tuple(lo.tolist())
        side = max(h - l for h, l in zip(hi.tolist(), self.origin))
        if cell is None:
            keys, cell = self._default_cell(side, who)
        else:
            self._check_extent(side, cell, who)
            keys = _cell_keys(points, self.origin, cell, who)
        self.cell = cell
        sorted_keys, perm = torch.sort(keys, stable=True)
        self.order = perm.to(torch.int32)
        live = sorted_keys[:self.n_finite]
        self.keys, counts = torch.unique_consecutive(live, return_counts=True)
        self.n_cells = self.keys.shape[0]
        self.start = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).to(torch.int32)
        self.sorted_points = points[perm[:self.n_finite]].contiguous()
        mask = MAX_DIM - 1
        top = torch.stack([(self.keys & mask).amax(), ((self.keys >> 21) & mask).amax(), (self.keys >> 42).amax()])
        last = sorted_keys[self.n_finite - 1:self.n_finite]
        top, last = top.tolist(), int(last)
        if last == NO_CELL:
            raise RuntimeError("%s: a finite point fell outside the 2^21 cells of an axis (cell %g is too small)" % (who, cell))
        self.dims = tuple(int(v) + 1 for v in top)

    @staticmethod
    def _check_extent(side, cell, who):
        if not side / cell + 2 <= MAX_DIM:
            raise RuntimeError("%s: at most 2^21 = %d cells per axis: the longest side %g needs a cell above %g, got %g" % (
                who, MAX_DIM, side, side / (MAX_DIM - 2), cell))

    def _default_cell(self, side, who):
        """-> (keys, cell) by the documented rule; each trial is one key launch and one count of the occupied cells"""
        if not side > 0:
            return _cell_keys(self.points, self.origin, 1.0, who), 1.0
        cell = _f32(side / math.sqrt(self.n_finite))
        cell = max(cell, _f32(side / (MAX_DIM - 2) * 1.000001))
        for doubling in range(DEFAULT_CELL_DOUBLINGS + 1):
            keys = _cell_keys(self.points, self.origin, cell, who)
            occupied = int(torch.unique(keys).shape[0]) - (1 if self.n_finite < self.n else 0)
            if doubling == DEFAULT_CELL_DOUBLINGS or self.n_finite >= DEFAULT_CELL_FILL * occupied:
                return keys, cell
            cell = _f32(cell * 2.0)

    @property
    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (self.order, self.keys, self.start, self.sorted_points))


def _grid(grid, who):
    if not isinstance(grid, PointGrid):
        raise RuntimeError("%s: grid must be a pointcloud.PointGrid" % who)
    return grid


def knn(grid, k, queries=None, max_dist=None):
    """The k nearest points of `grid` (a PointGrid) to every query -> (idx int32 [q,k], d2 f32 [q,k]), 1 <= k <= 64.
    queries: None (the points query themselves, q = n, rows in the points' own order) or f32 [q,3] on the grid's device;
    max_dist: None or a finite number >= 0.  One launch on the current stream, no synchronisation, no workspace.

    Cost.  A thread per query scans the cells around it ring by ring and stops when no unsearched cell can hold a point
    that enters its list.  Without max_dist that is at the latest when the rings cover the whole grid: a query far from
    every point (an isolated outlier in a large empty box, or a point set smaller than k + 1) walks many empty rows of
    cells, one binary search each.  With max_dist the search ends at the ring that max_dist reaches.  Queries that are
    neighbours in memory should be neighbours in space (the points' own queries are taken in cell order)."""
    who = "knn"
    _grid(grid, who)
    k = _integer(k, "k", who, 1, MAX_K, "an integer in [1, %d]" % MAX_K)
    limit = float("inf")
    if max_dist is not None:
        m = _f32(_number(max_dist, "max_dist", who))
        limit = _f32(m * m)                                   # (the product of two f32 is exact in f64: one rounding)
    dev = grid.points.device
    if queries is not None:
        _nx3(queries, who, "queries", torch.float32, letter="q")
        _same_device(grid.points, queries)
    q = grid.n if queries is None else queries.shape[0]
    if q * k >= 2 ** 31:
        raise RuntimeError("%s: q * k must stay below 2^31, got q = %d, k = %d" % (who, q, k))
    idx = torch.empty((q, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((q, k), dtype=torch.float32, device=dev)
    ox, oy, oz = grid.origin
    _call(lib().ctd_point_knn_f32, who, _ptr(grid.sorted_points) or None, _ptr(grid.order) or None, grid.n_finite,
          _ptr(grid.keys) or None, _ptr(grid.start), grid.n_cells, grid.dims[0], grid.dims[1], grid.dims[2], ox, oy, oz,
          grid.cell, None if queries is None else (_ptr(queries) or _ptr(grid.start)), q, k, limit, _ptr(idx) or None,
          _ptr(d2) or None, dev.index, _stream(dev))
    return idx, d2


def _mean_dist(d2, who):
    n, k = d2.shape
    mean = torch.empty((n,), dtype=torch.float32, device=d2.device)
    _call(lib().ctd_point_mean_dist_f32, who, _ptr(d2) or None, n, k, _ptr(mean) or None, d2.device.index, _stream(d2.device))
    return mean


def neighbor_mean_distance(grid, k):
    """Per point of `grid`, the mean distance to its k nearest neighbours (`knn(grid, k)`) -> f32 [n]: the sum of
    sqrt((double) d2) over the neighbours that exist, in f64 in list order, divided by their number and rounded to f32.
    NaN for a point without a neighbour (a single point, or one that is not finite).  Two launches."""
    who = "neighbor_mean_distance"
    _grid(grid, who)
    return _mean_dist(knn(grid, k)[1], who)


def statistical_outlier_mask(grid, k=16, std_ratio=2.0):
    """The statistical outlier filter -> (keep bool [n], mean_dist f32 [n], info): keep = mean_dist <= threshold with
    mean_dist = `neighbor_mean_distance(grid, k)` and threshold = mean + std_ratio * std of its finite entries (the
    population std), computed in f64 by torch; a point with a NaN mean_dist is not kept.  info = {"threshold", "mean",
    "std"}: float64 tensors on the device (no synchronisation).  mean + 2 std is a meaningful threshold only while the
    inliers outnumber the outliers clearly (5 : 1 in the tests)."""
    who = "statistical_outlier_mask"
    _grid(grid, who)
    std_ratio = _number(std_ratio, "std_ratio", who)
    md = _mean_dist(knn(grid, k)[1], who)
    live = torch.isfinite(md)
    v = md.double()
    count = live.sum()
    mean = torch.where(live, v, torch.zeros_like(v)).sum() / count
    std = torch.sqrt(torch.where(live, (v - mean) ** 2, torch.zeros_like(v)).sum() / count)
    threshold = mean + std_ratio * std
    return live & (v <= threshold), md, {"threshold": threshold, "mean": mean, "std": std}


def estimate_normals(grid, k=16, toward=None, return_cov=False):
    """Normals of the points of `grid` from the covariance of each point with its k nearest neighbours ->
    (normals f32 [n,3], variation f32 [n], ok uint8 [n]), plus cov f64 [n,9] with return_cov=True (the centroid, then the
    sums xx, xy, xz, yy, yz, zz about it).  Per point the members are the point itself, then its neighbours in list order;
    the centroid and then the six sums are f64 sums in that order; the unit eigenvector of the smallest eigenvalue (a
    fixed-sweep f64 Jacobi) is rounded to f32; variation = l0 / (l0 + l1 + l2), the surface variation.  ok = 0, with NaN
    normal and variation, for fewer than 3 members or l1 - l0 <= 1e-9 * l2: a line, a single point, an isotropic blob.
    toward: None (the sign is arbitrary), f32 [3] (one viewpoint) or f32 [n,3] (one per point, `view_centers`): the
    normal is negated where dot(normal, toward - p) < 0.  Two launches, no synchronisation."""
    who = "estimate_normals"
    _grid(grid, who)
    _flag(return_cov, "return_cov", who)
    n, dev = grid.n, grid.points.device
    stride = 0
    if toward is not None:
        _check(toward, "%s: toward" % who, (torch.float32,))
        _same_device(grid.points, toward)
        if tuple(toward.shape) not in ((3,), (n, 3)):
            raise RuntimeError("%s: toward must be shaped [3] or [%d,3], got %s" % (who, n, tuple(toward.shape)))
        stride = 3 if toward.dim() == 2 else 0
    idx = knn(grid, k)[0]
    normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
    variation = torch.empty((n,), dtype=torch.float32, device=dev)
    ok = torch.empty((n,), dtype=torch.uint8, device=dev)
    cov = torch.empty((n, 9), dtype=torch.float64, device=dev) if return_cov else None
    _call(lib().ctd_point_normals_f32, who, _ptr(grid.points) or None, n, _ptr(idx) or None, idx.shape[1],
          (_ptr(toward) or None) if n else None, stride, _ptr(normals) or None, _ptr(variation) or None, _ptr(ok) or None,
          (_ptr(cov) or None) if return_cov else None, dev.index, _stream(dev))
    return (normals, variation, ok, cov) if return_cov else (normals, variation, ok)


def view_centers(src, R, t, shape):
    """The camera centre of the view each fused point came from -> f32 [M,3], for `estimate_normals(toward=)`.  src int64
    [M] as `depth_fuse_points` returns it (the flat index into [B,V,H,W]), R f32 [B,V,3,3] and t f32 [B,V,3] the track's
    poses (x_cam = R x_world + t), shape = (V, H, W).  The centre of view (b, r) is -t_r @ R_r, and
    r = (src // (H * W)) % V, b = src // (V * H * W).  Torch ops only."""
    who = "view_centers"
    if not isinstance(src, torch.Tensor) or src.dtype != torch.int64 or src.dim() != 1:
        raise RuntimeError("%s: src must be an int64 tensor shaped [M]" % who)
    if len(shape) != 3:
        raise RuntimeError("%s: shape must be (V, H, W)" % who)
    V, H, W = (_integer(s, "shape", who, 1) for s in shape)
    if R.dim() != 4 or tuple(R.shape[1:]) != (V, 3, 3) or tuple(t.shape) != (R.shape[0], V, 3):
        raise RuntimeError("%s: R must be shaped [B,%d,3,3] and t [B,%d,3]" % (who, V, V))
    _same_device(src, R, t)
    centers = -(t.unsqueeze(-2) @ R).squeeze(-2)                # [B,V,3]: -t @ R = -R^T t
    view = torch.div(src, H * W, rounding_mode="floor")         # b * V + r
    return centers.reshape(-1, 3)[view].to(torch.float32).contiguous()


class VoxelDownsample:
    """What `voxel_downsample` returns: `points` f32 [m,3], `count` int32 [m], `cell_of_point` int32 [n] (-1 for a point
    that is not finite), `first` int32 [m] (the lowest original index of each cell), `attributes` f32 [m,C] or None, and
    the `grid` it was made from."""

    def __init__(self, points, count, cell_of_point, first, attributes, grid):
        self.points, self.count, self.cell_of_point, self.first = points, count, cell_of_point, first
        self.attributes, self.grid = attributes, grid


def _voxel_mean(values, grid, who):
    n, C = values.shape
    out = torch.empty((grid.n_cells, C), dtype=torch.float32, device=values.device)
    _call(lib().ctd_point_voxel_mean_f32, who, _ptr(values) or None, n, C, _ptr(grid.order) or None, _ptr(grid.start),
          grid.n_cells, _ptr(out) or None, values.device.index, _stream(values.device))
    return out


def voxel_downsample(points, cell=None, attributes=None):
    """One point per occupied cell of a grid of edge `cell`: the mean of the cell's members -> a `VoxelDownsample`, its
    rows in ascending key order (x fastest, then y, then z).  points: f32 [n,3] (a CUDA tensor), or a `PointGrid`, whose
    cell then holds (`cell` must be None or equal to it).  attributes: None or f32 [n,C], C <= 64, averaged alike.  Each
    mean is an f64 sum over the members in ascending original index, divided by the count and rounded to f32 once.  An
    even sub-sample: `global_mesh_icp(voxel_downsample(points, c).points, ...)` scores points from all over the set where
    `points[:2048]` of fused points is one corner of the first view."""
    who = "voxel_downsample"
    if isinstance(points, PointGrid):
        grid = points
        if cell is not None and _f32(_number(cell, "cell", who, lo_open=True)) != grid.cell:
            raise RuntimeError("%s: cell %r is not the grid's %r" % (who, cell, grid.cell))
    else:
        _nx3(points, who, "points", torch.float32)
        if cell is None:
            raise RuntimeError("%s: give a cell (or a PointGrid)" % who)
        grid = PointGrid(points, cell)
    pts, n, dev = grid.points, grid.n, grid.points.device
    if attributes is not None:
        _check(attributes, "%s: attributes" % who, (torch.float32,))
        _same_device(pts, attributes)
        if attributes.dim() != 2 or attributes.shape[0] != n or not 1 <= attributes.shape[1] <= MAX_ATTRIBUTES:
            raise RuntimeError("%s: attributes must be shaped [%d,C], 1 <= C <= %d, got %s" % (who, n, MAX_ATTRIBUTES,
                                                                                              tuple(attributes.shape)))
    m = grid.n_cells
    count = (grid.start[1:] - grid.start[:-1]).contiguous()
    cell_of_point = torch.full((n,), -1, dtype=torch.int32, device=dev)
    members = grid.order[:grid.n_finite].long()
    cell_of_point[members] = torch.repeat_interleave(torch.arange(m, dtype=torch.int32, device=dev), count.long())
    first = grid.order[grid.start[:-1].long()].contiguous()     # (a stable sort: a cell's lowest index comes first)
    return VoxelDownsample(_voxel_mean(pts, grid, who), count, cell_of_point, first,
                           None if attributes is None else _voxel_mean(attributes, grid, who), grid)


knn.__doc__ += _RULE
