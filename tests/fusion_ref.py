"""Numpy restatement of the multi-view depth consistency check and the point fusion (include/ctd_hip.h,
ctd_depth_consistency_f32 / ctd_depth_fuse_points_f32), and a small analytic scene generator for their tests.

Everything the definitions compute is np.float32, in exactly the written association (Python evaluates a + b + c from
the left, as C does), vectorised over the pixels of a view with Python loops over the views.  Pixels that a step fails
are carried along (their values may be NaN or inf) and masked at the end, which changes nothing for the others.

The scenes: a pinhole camera with focal length 1.2 * max(H, W) and the principal point at the image centre; per view a
small rotation and translation of it (X_cam = R X_world + t); a slanted world plane rendered to per-view depth in
float64 and cast to f32, and a nearer, bounded plane patch in front of it that occludes part of it in some views.
"""
import numpy as np

F = np.float32
NAN = F(np.nan)


# ---------------------------------------------------------------------------------------------------------------------
# the definitions
# ---------------------------------------------------------------------------------------------------------------------
def live_mask(depth, valid=None):
    """valid nonzero (None: everywhere) and depth finite and > 0"""
    with np.errstate(invalid="ignore"):
        live = np.isfinite(depth) & (depth > 0)
    return live if valid is None else live & (np.asarray(valid) != 0)


def transform(d, rays, Ra, ta, Rb, tb, K):
    """depth d [n] along rays [n,3] of view a -> (uvd0, uvd1, uvd2) in view b, all f32"""
    P = [d * rays[:, i] - ta[i] for i in range(3)]
    Q = [P[0] * Ra[0, j] + P[1] * Ra[1, j] + P[2] * Ra[2, j] for j in range(3)]
    S = [Q[0] * Rb[j, 0] + Q[1] * Rb[j, 1] + Q[2] * Rb[j, 2] + tb[j] for j in range(3)]
    return [S[0] * K[j, 0] + S[1] * K[j, 1] + S[2] * K[j, 2] for j in range(3)]


def match(depth_t, live_t, ray, K, R_t, t_t, r, s, max_px, max_rel):
    """Steps a, b, c for every pixel of view r against view s of one track (depth_t, live_t [V,H,W]; R_t [V,3,3];
    t_t [V,3]).  -> dict of [H*W] arrays: `landed` (step a passed: inside the image, on a live source pixel), `q` (the
    source pixel's in-view index, 0 where step a failed before it was known), `z` (z' of step b), `consistent`."""
    V, H, W = depth_t.shape
    assert depth_t.dtype == F and ray.dtype == F and K.dtype == F and R_t.dtype == F and t_t.dtype == F
    d_r = depth_t[r].reshape(-1)
    live_r = live_t[r].reshape(-1)
    ys_, xs_ = np.divmod(np.arange(H * W), W)
    with np.errstate(all="ignore"):
        uvd = transform(d_r, ray, R_t[r], t_t[r], R_t[s], t_t[s], K)
        ok = live_r & (uvd[2] > 0)
        xs = np.floor(uvd[0] / uvd[2] + F(0.5))
        ys = np.floor(uvd[1] / uvd[2] + F(0.5))
        assert xs.dtype == F and ys.dtype == F
        ok &= (xs >= F(0)) & (xs <= F(W - 1)) & (ys >= F(0)) & (ys <= F(H - 1))
        q = np.where(ok, ys, F(0)).astype(np.int64) * W + np.where(ok, xs, F(0)).astype(np.int64)
        landed = ok & live_t[s].reshape(-1)[q]
        d_s = depth_t[s].reshape(-1)[q]
        back = transform(d_s, ray[q], R_t[s], t_t[s], R_t[r], t_t[r], K)
        z = back[2]
        ok = landed & (z > 0)
        du = back[0] / z - xs_.astype(F)
        dv = back[1] / z - ys_.astype(F)
        near = (du * du + dv * dv <= F(max_px) * F(max_px)) & (np.abs(z - d_r) <= F(max_rel) * d_r)
        assert du.dtype == F and z.dtype == F
    return {"landed": landed, "q": q, "z": z, "consistent": ok & near}


def all_matches(depth, valid, ray, K, R, t, max_px, max_rel):
    """{(b, r, s): match(...)} for every ordered pair of different views of every track"""
    B, V, H, W = depth.shape
    live = live_mask(depth, valid)
    return {(b, r, s): match(depth[b], live[b], ray, K, R[b], t[b], r, s, max_px, max_rel)
            for b in range(B) for r in range(V) for s in range(V) if s != r}


def consistency(depth, ray, K, R, t, valid=None, max_px=1.0, max_rel=0.01, min_views=1, matches=None):
    """-> count uint8, keep uint8, fused f32 (NaN where keep == 0), each [B,V,H,W]"""
    B, V, H, W = depth.shape
    assert 1 <= V <= 64 and 0 <= min_views <= 255
    if matches is None:
        matches = all_matches(depth, valid, ray, K, R, t, max_px, max_rel)
    live = live_mask(depth, valid)
    count = np.zeros((B, V, H * W), np.uint8)
    fused = np.empty((B, V, H * W), F)
    for b in range(B):
        for r in range(V):
            acc = depth[b, r].reshape(-1).copy()
            for s in range(V):                                    # ascending: the order of the sum
                if s == r:
                    continue
                m = matches[b, r, s]
                with np.errstate(all="ignore"):
                    acc = np.where(m["consistent"], acc + m["z"], acc)
                count[b, r] += m["consistent"].astype(np.uint8)
            with np.errstate(all="ignore"):
                fused[b, r] = acc / (1 + count[b, r].astype(np.int32)).astype(F)
    count = count.reshape(B, V, H, W)
    keep = live & (count >= min_views)
    fused = np.where(keep, fused.reshape(B, V, H, W), NAN)
    assert fused.dtype == F
    return count, keep.astype(np.uint8), fused


def fuse_points(depth, ray, K, R, t, valid=None, max_px=1.0, max_rel=0.01, min_views=1, dedupe=True, matches=None):
    """-> points [M,3] f32, src [M] int64 (ascending), n_per_track [B] int64, (count, keep, fused)"""
    B, V, H, W = depth.shape
    if matches is None:
        matches = all_matches(depth, valid, ray, K, R, t, max_px, max_rel)
    count, keep, fused = consistency(depth, ray, K, R, t, valid, max_px, max_rel, min_views, matches)
    emit = keep.reshape(B, V, H * W) != 0
    if dedupe:
        emit = emit.copy()
        for b in range(B):
            for r in range(V):
                for s in range(r):                                # first view wins
                    m = matches[b, r, s]
                    emit[b, r] &= ~(m["consistent"] & (keep[b, s].reshape(-1)[m["q"]] != 0))
    src = np.nonzero(emit.reshape(-1))[0].astype(np.int64)
    view, p = np.divmod(src, H * W)
    Rv, tv = R.reshape(B * V, 3, 3)[view], t.reshape(B * V, 3)[view]
    f = fused.reshape(-1)[src]
    P = [f * ray[p, i] - tv[:, i] for i in range(3)]
    points = np.stack([P[0] * Rv[:, 0, j] + P[1] * Rv[:, 1, j] + P[2] * Rv[:, 2, j] for j in range(3)], 1)
    points = points.reshape(-1, 3)
    assert points.dtype == F
    n_per_track = emit.reshape(B, -1).sum(1).astype(np.int64)
    return points, src, n_per_track, (count, keep, fused)


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def camera(H, W):
    """-> K [3,3] f32, ray [H*W,3] f32 = [u v 1] @ Ki^T.  The focal length is rounded to f32 first and the principal
    point is a half-integer, so K is the same matrix in f32 and f64."""
    f = float(F(1.2 * max(H, W)))
    K = np.array([[f, 0, (W - 1) / 2], [0, f, (H - 1) / 2], [0, 0, 1]], np.float64)
    v, u = np.divmod(np.arange(H * W), W)
    ray = np.stack([u, v, np.ones(H * W)], 1) @ np.linalg.inv(K).T
    return K.astype(F), np.ascontiguousarray(ray.astype(F))


def _rot(axis_angle):
    a = np.linalg.norm(axis_angle)
    if a == 0:
        return np.eye(3)
    k = axis_angle / a
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


def overlapping_poses(rs, B, V, max_deg=3.0, max_t=0.05):
    """a base camera at the origin looking down +z, plus per view a rotation of up to max_deg degrees about a random
    axis and a translation of up to max_t per component (the scene is 1.8 .. 2.7 away) -> R [B,V,3,3], t [B,V,3] f32"""
    R = np.empty((B, V, 3, 3))
    t = np.empty((B, V, 3))
    for b in range(B):
        for v in range(V):
            axis = rs.normal(size=3)
            R[b, v] = _rot(axis / np.linalg.norm(axis) * np.deg2rad(rs.uniform(0, max_deg)))
            t[b, v] = rs.uniform(-max_t, max_t, 3)
    return R.astype(F), t.astype(F)


def facing_away_poses(rs, B, V):
    """V cameras at (almost) one place, turned about the y axis in steps of 360 / V degrees.  The half field of view is
    atan(0.5 / 1.2) = 22.6 degrees at most and the steps are at least 72 (V <= 5), so nothing one view sees at a depth
    >= 1 projects into the image of another: it is behind it or far off to the side."""
    assert V <= 5
    R = np.empty((B, V, 3, 3))
    for v in range(V):
        R[:, v] = _rot(np.array([0.0, 2 * np.pi * v / V, 0.0]))
    t = rs.uniform(-0.01, 0.01, (B, V, 3))
    return R.astype(F), t.astype(F)


PLANE = (np.array([0.10, -0.05, 1.0]), 2.5)                      # n . X = c, the background
PATCH = (np.array([0.0, 0.0, 1.0]), 1.8, (-0.15, 0.35), (-0.2, 0.2))   # a nearer plane, bounded in world x and y


def render_planes(ray, R, t, H, W, patch=True):
    """per-view depth of PLANE (and of PATCH in front of it) in float64 from the f32 poses, cast to f32 -> [B,V,H,W]"""
    B, V = R.shape[:2]
    ray64 = ray.astype(np.float64)
    depth = np.empty((B, V, H * W))
    for b in range(B):
        for v in range(V):
            Rm, tv = R[b, v].astype(np.float64), t[b, v].astype(np.float64)
            o, dirs = -Rm.T @ tv, ray64 @ Rm                       # X_world = R^T (d ray - t) = o + d (R^T ray)
            n, c = PLANE
            d = (c - n @ o) / (dirs @ n)
            if patch:
                n2, c2, xr, yr = PATCH
                d2 = (c2 - n2 @ o) / (dirs @ n2)
                X = o + d2[:, None] * dirs
                hit = (d2 > 0) & (d2 < d) & (X[:, 0] > xr[0]) & (X[:, 0] < xr[1]) & (X[:, 1] > yr[0]) & (X[:, 1] < yr[1])
                d = np.where(hit, d2, d)
            depth[b, v] = d
    return depth.reshape(B, V, H, W).astype(F)


SCENE_KINDS = ("clean", "noisy", "away")


def make_scene(kind, B, V, H, W, seed):
    """-> dict(depth f32 [B,V,H,W], valid uint8 [B,V,H,W], ray, K, R, t).
    clean: both planes, no noise, valid all ones.  plane: the same without the patch (no occlusion anywhere).
    noisy: Gaussian depth noise (sigma = 0.2 % of the depth), gross outliers on about 10 % of the pixels (the depth
      scaled by 0.5 .. 0.9 or 1.1 .. 1.5), holes of every kind: NaN (3 %), 0 (2 %), negative (2 %), +inf (1 %),
      valid == 0 (5 %, among them pixels whose depth is fine).
    away: the facing-away poses with depths between 1 and 3; every pixel is live and no projection lands."""
    rs = np.random.RandomState(seed)
    K, ray = camera(H, W)
    if kind == "away":
        R, t = facing_away_poses(rs, B, V)
        depth = rs.uniform(1.0, 3.0, (B, V, H, W)).astype(F)
        valid = np.ones((B, V, H, W), np.uint8)
    else:
        R, t = overlapping_poses(rs, B, V)
        depth = render_planes(ray, R, t, H, W, patch=kind != "plane")
        valid = np.ones((B, V, H, W), np.uint8)
        if kind == "noisy":
            depth = (depth * (1 + rs.normal(0, 0.002, depth.shape))).astype(F)
            out = rs.rand(*depth.shape) < 0.10
            scale = np.where(rs.rand(*depth.shape) < 0.5, rs.uniform(0.5, 0.9, depth.shape), rs.uniform(1.1, 1.5, depth.shape))
            depth = np.where(out, depth * scale, depth).astype(F)
            u = rs.rand(*depth.shape)
            depth[u < 0.03] = np.nan
            depth[(u >= 0.03) & (u < 0.05)] = 0
            depth[(u >= 0.05) & (u < 0.07)] *= -1
            depth[(u >= 0.07) & (u < 0.08)] = np.inf
            valid[rs.rand(*depth.shape) < 0.05] = 0
        else:
            assert kind in ("clean", "plane")
    return {"depth": np.ascontiguousarray(depth), "valid": valid, "ray": ray, "K": K, "R": R, "t": t}
