"""The point-cloud family (include/ext/ctd_hip_point_cloud.h, connecting_the_dots_amd/pointcloud.py) restated in numpy: the
yardstick of tests/test_point_cloud_host.py and tests/test_point_cloud_gpu.py, not the code under test.  There is no grid
here: `knn` is brute force over all points under the header's rule, with d2 in f32 in the header's association and the
(d2, index) order; the f64 sums of the consumers run in the header's order, one member at a time (numpy's own sums are
pairwise and would differ in the last bit); the normals come from numpy.linalg.eigh."""
import numpy as np

F = np.float32
INF = F(np.inf)


def _f32(a, cols=3):
    return np.ascontiguousarray(np.asarray(a, F).reshape(-1, cols))


def max_d2(max_dist):
    """max_dist squared once, as f32; None is no limit"""
    return INF if max_dist is None else F(max_dist) * F(max_dist)


def knn(points, k, queries=None, max_dist=None, chunk=512):
    """-> idx int32 [q,k], d2 f32 [q,k].  queries=None: the points query themselves, each excluded from its own list by
    index.  A candidate is a finite point with d2 <= max_d2 and d2 < +inf; a query that is not finite has none."""
    P = _f32(points)
    Q = P if queries is None else _f32(queries)
    n, q = len(P), len(Q)
    limit = max_d2(max_dist)
    finite = np.isfinite(P).all(1)
    idx = np.full((q, k), -1, np.int32)
    out = np.full((q, k), INF, F)
    if n == 0:
        return idx, out
    with np.errstate(all="ignore"):
        for a in range(0, q, chunk):
            Qc = Q[a:a + chunk]
            dx, dy, dz = (P[None, :, c] - Qc[:, None, c] for c in range(3))
            d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
            assert d2.dtype == F
            good = finite[None, :] & np.isfinite(Qc).all(1)[:, None] & (d2 <= limit) & (d2 < INF)
            if queries is None:
                rows = np.arange(len(Qc))
                good[rows, a + rows] = False
            d2 = np.where(good, d2, INF)
            by = np.argsort(d2, axis=1, kind="stable")[:, :k]          # ascending d2, the lower index first among equals
            got = np.take_along_axis(d2, by, 1)
            m = by.shape[1]
            out[a:a + chunk, :m] = got
            idx[a:a + chunk, :m] = np.where(got < INF, by, -1)
    return idx, out


def mean_dist(d2):
    """per row the f64 sum of sqrt(d2) over the entries below +inf in list order / their number -> f32, NaN for none"""
    d2 = np.asarray(d2, F)
    s, c = np.zeros(len(d2)), np.zeros(len(d2), np.int64)
    for j in range(d2.shape[1]):
        live = d2[:, j] < INF
        s = np.where(live, s + np.sqrt(np.where(live, d2[:, j], 0).astype(np.float64)), s)
        c += live
    with np.errstate(all="ignore"):
        return np.where(c > 0, s / c, np.nan).astype(F)


def outlier_mask(points, k=16, std_ratio=2.0):
    """-> keep bool [n], mean_dist f32 [n], threshold (f64): keep = mean_dist <= mean + std_ratio * std over the finite
    entries (the population std), in f64; a NaN mean is not kept"""
    md = mean_dist(knn(points, k)[1])
    live = np.isfinite(md)
    v = md[live].astype(np.float64)
    threshold = v.mean() + std_ratio * v.std() if len(v) else np.nan
    with np.errstate(all="ignore"):
        return live & (md.astype(np.float64) <= threshold), md, threshold


def covariance(points, idx):
    """-> cov f64 [n,9] (the centroid, then the sums xx, xy, xz, yy, yz, zz about it) and count int [n]: the members are
    the point, then its neighbours idx >= 0 in list order; every sum one member at a time in f64"""
    P = _f32(points).astype(np.float64)
    n = len(P)
    idx = np.asarray(idx).reshape(n, -1)
    with np.errstate(all="ignore"):
        s, count = P.copy(), np.ones(n, np.int64)
        for j in range(idx.shape[1]):
            live = idx[:, j] >= 0
            s = np.where(live[:, None], s + P[np.where(live, idx[:, j], 0)], s)
            count += live
        c = s / count[:, None]
        d = P - c
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        sums = np.stack([d[:, a] * d[:, b] for a, b in pairs], 1)
        for j in range(idx.shape[1]):
            live = idx[:, j] >= 0
            d = P[np.where(live, idx[:, j], 0)] - c
            sums = np.where(live[:, None], sums + np.stack([d[:, a] * d[:, b] for a, b in pairs], 1), sums)
    return np.concatenate([c, sums], 1), count


def normals(points, idx, toward=None):
    """-> dict(normal f64 [n,3] (unit, unrounded; NaN where ok = 0), variation f64 [n], ok uint8 [n], gap f64 [n] =
    (l1 - l0) / l2, cov f64 [n,9]) by numpy.linalg.eigh; toward [3] or [n,3]: negated where dot(normal, toward - p) < 0"""
    P = _f32(points).astype(np.float64)
    cov, count = covariance(points, idx)
    xx, xy, xz, yy, yz, zz = cov[:, 3:].T
    A = np.stack([xx, xy, xz, xy, yy, yz, xz, yz, zz], 1).reshape(-1, 3, 3)
    usable = np.isfinite(A).all((1, 2))
    lam, vec = np.linalg.eigh(np.where(usable[:, None, None], A, np.eye(3)))
    with np.errstate(all="ignore"):
        ok = usable & (count >= 3) & (lam[:, 1] - lam[:, 0] > 1e-9 * lam[:, 2])
        nrm = vec[:, :, 0]
        if toward is not None:
            v = np.asarray(toward, F).astype(np.float64).reshape(-1, 3) - P
            flip = ((nrm[:, 0] * v[:, 0]) + (nrm[:, 1] * v[:, 1])) + (nrm[:, 2] * v[:, 2]) < 0
            nrm = np.where(flip[:, None], -nrm, nrm)
        var = lam[:, 0] / ((lam[:, 0] + lam[:, 1]) + lam[:, 2])
        gap = np.where(ok, (lam[:, 1] - lam[:, 0]) / lam[:, 2], 0.0)
    return {"normal": np.where(ok[:, None], nrm, np.nan), "variation": np.where(ok, var, np.nan), "ok": ok.astype(np.uint8),
            "gap": gap, "cov": cov}


def cell_coords(points, origin, cell):
    """g = floorf((p - origin) / cell) in f32 -> (g int64 [n,3], finite bool [n])"""
    P = _f32(points)
    finite = np.isfinite(P).all(1)
    with np.errstate(all="ignore"):
        g = np.floor((np.where(finite[:, None], P, 0) - np.asarray(origin, F)) / F(cell))
    assert g.dtype == F
    return g.astype(np.int64), finite


def voxel_downsample(points, cell, attributes=None):
    """-> dict(points f32 [m,3], count int32 [m], cell_of_point int32 [n], first int32 [m], attributes f32 [m,C] | None,
    keys int64 [m]): one row per occupied cell, keys ascending (x lowest, then y, then z, 21 bits each); origin = the
    minimum of the finite points; the means are f64 sums in ascending original index, divided and rounded to f32 once"""
    P = _f32(points)
    n = len(P)
    finite = np.isfinite(P).all(1)
    cell_of_point = np.full(n, -1, np.int32)
    if not finite.any():
        return {"points": np.zeros((0, 3), F), "count": np.zeros(0, np.int32), "cell_of_point": cell_of_point,
                "first": np.zeros(0, np.int32), "attributes": None if attributes is None else np.zeros((0, np.shape(attributes)[1]), F),
                "keys": np.zeros(0, np.int64)}
    origin = P[finite].min(0)
    g, _ = cell_coords(P, origin, cell)
    key = g[:, 0] + (g[:, 1] << 21) + (g[:, 2] << 42)
    keys, inverse = np.unique(key[finite], return_inverse=True)
    members = np.nonzero(finite)[0]
    cell_of_point[members] = inverse
    m = len(keys)
    count = np.bincount(inverse, minlength=m).astype(np.int32)
    first = np.full(m, n, np.int64)
    np.minimum.at(first, inverse, members)

    def means(values):
        s = np.zeros((m, values.shape[1]))
        np.add.at(s, inverse, values[members].astype(np.float64))      # unbuffered: one member at a time, ascending index
        return (s / count[:, None]).astype(F)
    return {"points": means(P), "count": count, "cell_of_point": cell_of_point, "first": first.astype(np.int32),
            "attributes": None if attributes is None else means(np.asarray(attributes, F).reshape(n, -1)), "keys": keys}


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
PLANE_N = np.array([0.10, -0.05, 1.0]) / np.linalg.norm([0.10, -0.05, 1.0])    # the background plane of tests/fusion_ref.py
PLANE_C = 2.5
CAMERA = np.zeros(3)


def noisy_plane(n_in, n_out, seed, sigma=0.005):
    """n_in points of the plane PLANE_N . X = PLANE_C over a 1 x 1 patch seen from CAMERA = 0, with Gaussian noise of
    sigma (0.2 % of the depth 2.5, as the noisy scene of tests/fusion_ref.py) along the normal, then n_out gross outliers
    uniform in the slab from 0.5 to 1.5 times the depth -> points f32 [n_in + n_out,3] (shuffled), is_outlier bool"""
    rs = np.random.RandomState(seed)
    u = np.cross(PLANE_N, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(PLANE_N, u)
    ab = rs.uniform(-0.5, 0.5, (n_in, 2))
    inl = PLANE_N * PLANE_C + ab[:, :1] * u + ab[:, 1:] * v + rs.normal(0, sigma, (n_in, 1)) * PLANE_N
    ab = rs.uniform(-0.5, 0.5, (n_out, 2))
    out = PLANE_N * PLANE_C * rs.uniform(0.5, 1.5, (n_out, 1)) + ab[:, :1] * u + ab[:, 1:] * v
    pts = np.concatenate([inl, out]).astype(F)
    is_out = np.arange(n_in + n_out) >= n_in
    perm = rs.permutation(n_in + n_out)
    return np.ascontiguousarray(pts[perm]), is_out[perm]


def sphere(n, seed, radius=1.0, centre=(0.3, -0.2, 2.0)):
    """n points uniform on a sphere -> points f32 [n,3], the outward unit normals f64 [n,3], the centre"""
    rs = np.random.RandomState(seed)
    d = rs.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = (np.asarray(centre) + radius * d).astype(F)
    return pts, d, np.asarray(centre, np.float64)


def angle(a, b):
    """the angle in radians between unit vectors, up to sign, by atan2 (accurate near 0)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs((a * b).sum(-1)))
