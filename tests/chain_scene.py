"""The scene of the chain tests (tests/test_chain_truth_host.py, tests/test_chain_truth_gpu.py) and its ground truth in
float64 -- numpy only, and independent of the renderer (csrc/ctd_render.h) and of its restatement in oracle/.

Two tracks of V = 4 views each.  Track 0 is workloads.render_scene's slanted wall with three boxes in front of it, track
1 another seed's three boxes without the wall, so some of its rays miss.  The views of a track are posed by
synth.sample_track_poses(RandomState(seed)), the production poses: X_cam = R X_world + t, the projector has the
camera's rotation and t_proj = t + [-baseline, 0, 0], i.e. it sits at +baseline on the camera's x axis, and pixel w of
the camera sees pattern column w - d, d = f * baseline / z.  Image 64 x 256, f = 0.9 W, principal point at the centre
of the pixel grid (pixel centres are the integers), baseline 0.075, block 9, LCN radius 5 / eps 0.05, D = 32.

The truth is a float64 Moeller-Trumbore ray caster over the f32 mesh and poses cast to float64 (`cast`), vectorised
over pixels and faces.  Every mask comes from that truth alone, never from comparing it with what is tested:

  interior   every pixel of the (block + 2 * LCN radius)^2 = 19 x 19 window around the pixel lies in the image and hits
             the same face.  The two triangles of a quad of the mesh are one face here (surface = triangle // 2, the
             way workloads.render_scene emits them): they are coplanar, so depth and disparity are linear across their
             shared diagonal.
  good       interior & lit64 & (w - d64 >= block // 2)
  shadow     interior & hit & ~lit64
  visible    `visibility(r, s)`: the point of pixel p of view r, projected into view s and rounded to the nearest pixel q,
             lies in s's image on a hit pixel whose float64 depth z64_s[q] is the depth z' of the point in s:
             |z64_s[q] / z' - 1| <= SAME_REL.  It is occluded, or q sees another surface, when that difference is
             >= OTHER_REL (or q is outside the image or a miss).  Between the two lies the grey zone, `unsure`.

The grey zone.  The consistency rule of include/ctd_hip.h compares, at max_rel = MAX_REL = 0.002, the depth of q's own
point seen from r with the depth of p; the truth compares depths in s.  Both differences are those of one plane sampled
half a pixel apart when p and q see the same face, and the two views see that face under slightly different slopes
(the cameras of a track are at most 0.2 * sqrt(3) apart, 3 away from what they look at), so a pixel pair the rule
accepts at 0.002 may differ by somewhat more or less than 0.002 in s.  SAME_REL = MAX_REL / 2 and OTHER_REL = 2 * MAX_REL
bracket the rule's tolerance by a factor of two on either side; `unsure` is asserted to stay below 5 % of the pixels
of every ordered view pair (measured: tests/test_chain_truth_host.py).

The second half of the chain (tests/test_chain_recon_host.py, tests/test_chain_recon_gpu.py) adds, again from the truth
alone:

  normal     per pixel the unit normal of the hit face in the camera's frame, R n, turned so that it faces the camera
             (normal . X_cam < 0); NaN at a miss.
  recon_grid one volume per track around the truth points of all its views, padded by 4 voxels (the truncation), with
             one `dims` for both tracks.
  field      an analytic scalar of the world position with values in [0, 1] and periods of metres; `field_images` holds
             it at the truth points of every pixel (0 at a miss), so a vertex coloured from the views must come out as
             `field(vertex)` up to the field's change over the vertex's distance to the truth and over a pixel.
  occluded64 `occluded64(b, s, points, margin)` casts the ray from the centre of camera s of track b to each point
             against the true mesh.  With `length` the distance from the centre to the point and `first` the distance
             to the first hit: occluded when first < length - 2 margin, visible when first >= length - margin / 2
             (or nothing is hit), grey in between.  The silhouette rule: a point is grey as well when its ray passes
             within `reach` voxels (a voxel is margin / 2, the README's margin being 2 voxels) of a silhouette of view s
             that lies in front of it.  A silhouette pixel is a pixel of the view's truth whose 3 x 3 neighbourhood
             holds two surfaces (surface = triangle // 2) or a miss; z_near is the nearest depth of that neighbourhood,
             and a voxel there spans f * voxel / z_near pixels.  The ray is near the silhouette when the point's
             projection (not rounded) lies within reach * f * voxel / z_near pixels of the silhouette pixel's centre,
             and the silhouette lies in front of the point when z_near < z - 2 margin, z being the point's depth in s:
             only a surface that far in front makes a point occluded, and an edge nearer to the point's own depth is
             the rim of the point's own surface or of a neighbour that cannot hide it.  Near an edge in front, a
             reconstruction eroded or dilated there decides differently from the true mesh without being wrong.
             Points outside the image are grey.  REACH = 0.5: at a reach of one voxel no truly occluded candidate of the
             reference chain is used, but 14.7 % of track 0's candidates are grey (its boxes stand a metre from the
             cameras, where a voxel spans 6 pixels, in front of a wall full of vertices); at half a voxel grey is 9.2 %
             and 43 of 268 truly occluded candidates are used (tests/test_chain_recon_host.py measures both).
"""
import functools

import numpy as np

from tests import workloads

H, W = 64, 256
B, V = 2, 4
D = 32
BLOCK = 9
LCN_RADIUS, LCN_EPS = 5, 0.05
BASELINE = 0.075
SHADER = (0.5, 1.5, 0.0, 10.0)                    # create_syn_data.py:155, as synth.render_track_sample
D_ALPHA, D_BETA = 0.0, 0.35
SCENE_SEEDS = (3, 11)                             # workloads.render_scene seeds of the two tracks' meshes
POSE_SEEDS = (101, 202)                           # RandomState seeds of synth.sample_track_poses
MAX_PX, MAX_REL = 1.0, 0.002                      # the multi-view tolerance the chain tests use
SAME_REL, OTHER_REL = MAX_REL / 2, 2 * MAX_REL    # the grey zone of `visibility`
WINDOW = BLOCK + 2 * LCN_RADIUS


def intrinsics():
    """K f32 [3,3]: workloads.render_scene's camera for this image size"""
    f = 0.9 * W
    return np.array([[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]], np.float32)


def rays(K):
    """ray f32 [H*W,3] = [u v 1] K^-T, formed in float64"""
    v, u = np.divmod(np.arange(H * W), W)
    r = np.stack([u, v, np.ones(H * W)], 1) @ np.linalg.inv(K.astype(np.float64)).T
    return np.ascontiguousarray(r.astype(np.float32))


def pattern01():
    return workloads.syn_dot_pattern(H, W)


def meshes():
    """one dict(verts, colors, faces) per track"""
    out = []
    for b, seed in enumerate(SCENE_SEEDS):
        sc = workloads.render_scene(seed, H=H, W=W, n_boxes=3, wall=(b == 0))
        out.append({k: sc[k] for k in ("verts", "colors", "faces")})
    return out


def poses():
    """one synth.sample_track_poses dict per track (R, t, R_proj, t_proj [V,...] f32, blend_im)"""
    from connecting_the_dots_amd import synth
    return [synth.sample_track_poses(np.random.RandomState(s), track_length=V, baseline=BASELINE) for s in POSE_SEEDS]


# ---------------------------------------------------------------------------------------------------------------------
# the float64 ray caster
# ---------------------------------------------------------------------------------------------------------------------
def ray_mesh(orig, dirs, verts, faces, chunk=4096):
    """Moeller-Trumbore, float64.  orig [3] | [n,3], dirs [n,3], verts [m,3], faces [k,3] -> (t [n] (inf: no hit), face
    [n] (-1)): the smallest ray parameter t > 0 over the faces; the first face keeps a tie."""
    verts = np.asarray(verts, np.float64)
    v0, v1, v2 = (verts[faces[:, i]] for i in range(3))
    e1, e2 = v1 - v0, v2 - v0                                           # [k,3]
    dirs = np.asarray(dirs, np.float64)
    orig = np.broadcast_to(np.asarray(orig, np.float64), dirs.shape)
    n = dirs.shape[0]
    t_out = np.full(n, np.inf)
    f_out = np.full(n, -1, np.int64)
    for a in range(0, n, chunk):
        d = dirs[a:a + chunk, None, :]                                  # [c,1,3]
        o = orig[a:a + chunk, None, :]
        pvec = np.cross(d, e2[None])                                    # [c,k,3]
        det = (e1[None] * pvec).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            tvec = o - v0[None]
            u = (tvec * pvec).sum(-1) * inv
            qvec = np.cross(tvec, e1[None])
            v = (d * qvec).sum(-1) * inv
            t = (e2[None] * qvec).sum(-1) * inv
        ok = (np.abs(det) > 1e-14) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0)
        t = np.where(ok, t, np.inf)
        f = t.argmin(1)
        tm = t[np.arange(t.shape[0]), f]
        t_out[a:a + chunk] = tm
        f_out[a:a + chunk] = np.where(np.isfinite(tm), f, -1)
    return t_out, f_out


def cast(mesh, K, R, t, t_proj):
    """One view in float64 from the f32 inputs -> dict of [H,W] arrays: z64 (z-depth, inf where nothing is hit), hit,
    face (triangle id, -1), lit64 (the projector, at the camera's rotation and t_proj, sees the hit point: the first hit
    of the ray from the projector's centre through the point is the point itself), d64 = f * baseline / z64 (0 where
    nothing is hit), and X [H,W,3], the world points."""
    K, R, t, tp = (np.asarray(a, np.float64) for a in (K, R, t, t_proj))
    v, u = np.divmod(np.arange(H * W), W)
    cam = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones(H * W)], 1)     # [u v 1] K^-T, z = 1
    C = -R.T @ t
    dirs = cam @ R                                                      # R^T cam: world direction with camera z = 1,
    z, face = ray_mesh(C, dirs, mesh["verts"], mesh["faces"])           # so the ray parameter is the z-depth
    hit = face >= 0
    X = C + np.where(hit, z, 0.0)[:, None] * dirs
    Cp = -R.T @ tp
    tl, _ = ray_mesh(Cp, X - Cp, mesh["verts"], mesh["faces"])          # the point itself is at parameter 1
    lit = hit & (tl >= 1.0 - 1e-9)
    baseline = np.linalg.norm(Cp - C)
    with np.errstate(divide="ignore"):
        d = np.where(hit, K[0, 0] * baseline / z, 0.0)
    sh = (H, W)
    return dict(z64=z.reshape(sh), hit=hit.reshape(sh), face=face.reshape(sh), lit64=lit.reshape(sh), d64=d.reshape(sh),
                X=X.reshape(H, W, 3))


def interior_mask(face):
    """face [H,W] triangle ids -> bool [H,W]: the WINDOW x WINDOW window lies in the image and on one surface"""
    k = WINDOW // 2
    surf = np.where(face >= 0, face // 2, -1)
    pad = np.full((H + 2 * k, W + 2 * k), -2, np.int64)                 # outside the image: equal to nothing
    pad[k:k + H, k:k + W] = surf
    same = surf >= 0
    for dy in range(WINDOW):
        for dx in range(WINDOW):
            same &= pad[dy:dy + H, dx:dx + W] == surf
    return same


# ---------------------------------------------------------------------------------------------------------------------
# the scene
# ---------------------------------------------------------------------------------------------------------------------
class Scene:
    """meshes, poses [B,V], K, ray, pattern, and per (b, v) the float64 truth with its masks"""

    def __init__(self):
        self.K = intrinsics()
        self.ray = rays(self.K)
        self.f = float(self.K[0, 0])
        self.bf = BASELINE * self.f                                     # baseline * focal, formed in double
        self.pattern = pattern01()
        self.pattern3 = np.ascontiguousarray(np.repeat(self.pattern[:, :, None], 3, 2))
        self.meshes = meshes()
        self.poses = poses()
        self.R = np.stack([p["R"] for p in self.poses])                 # [B,V,3,3] f32
        self.t = np.stack([p["t"] for p in self.poses])                 # [B,V,3]
        self.t_proj = np.stack([p["t_proj"] for p in self.poses])
        self.truth = [[cast(self.meshes[b], self.K, self.R[b, v], self.t[b, v], self.t_proj[b, v]) for v in range(V)]
                      for b in range(B)]
        cols = np.arange(W)[None, :]
        for b in range(B):
            for v in range(V):
                T = self.truth[b][v]
                T["interior"] = interior_mask(T["face"])
                T["good"] = T["interior"] & T["lit64"] & (cols - T["d64"] >= BLOCK // 2)
                T["shadow"] = T["interior"] & T["hit"] & ~T["lit64"]

    def stack(self, key):
        """[B*V,H,W] in the frame order b * V + v"""
        return np.stack([self.truth[b][v][key] for b in range(B) for v in range(V)])

    def visibility(self, b, r, s):
        """-> (visible, unsure) bool [H,W] for the pixels of view r of track b against view s (module docstring)"""
        Tr, Ts = self.truth[b][r], self.truth[b][s]
        K, Rs, ts = (np.asarray(a, np.float64) for a in (self.K, self.R[b, s], self.t[b, s]))
        Xs = Tr["X"].reshape(-1, 3) @ Rs.T + ts
        zp = Xs[:, 2]
        hit = Tr["hit"].reshape(-1)
        with np.errstate(all="ignore"):
            xs = np.floor(K[0, 0] * Xs[:, 0] / zp + K[0, 2] + 0.5)
            ys = np.floor(K[1, 1] * Xs[:, 1] / zp + K[1, 2] + 0.5)
        inside = hit & (zp > 0) & (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        q = np.where(inside, ys, 0).astype(np.int64) * W + np.where(inside, xs, 0).astype(np.int64)
        landed = inside & Ts["hit"].reshape(-1)[q]
        with np.errstate(all="ignore"):
            rel = np.abs(Ts["z64"].reshape(-1)[q] / zp - 1.0)
        visible = landed & (rel <= SAME_REL)
        unsure = landed & (rel > SAME_REL) & (rel < OTHER_REL)
        return visible.reshape(H, W), unsure.reshape(H, W)

    def mesh_distance(self, b, points, chunk=8192):
        """float64 distance of points [n,3] to the nearest triangle of track b's mesh -> [n]"""
        m = self.meshes[b]
        return mesh_distance(points, m["verts"], m["faces"], chunk)


def mesh_distance(points, verts, faces, chunk=8192):
    """Point-to-triangle distance (the closest point is the projection onto the plane when that lies inside the
    triangle, otherwise the closest point of the three edge segments), minimised over the faces; float64."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    verts = np.asarray(verts, np.float64)
    a, b, c = (verts[faces[:, i]] for i in range(3))                    # [k,3]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    out = np.empty(P.shape[0])

    def seg(p, u, w):                                                   # distance^2 of p [m,1,3] to segments u-w [k,3]
        e = (w - u)[None]
        s = np.clip(((p - u[None]) * e).sum(-1) / (e * e).sum(-1), 0.0, 1.0)
        d = p - (u[None] + s[..., None] * e)
        return (d * d).sum(-1)

    for i in range(0, P.shape[0], chunk):
        p = P[i:i + chunk, None, :]
        h = ((p - a[None]) * n[None]).sum(-1)                           # signed height over each plane [m,k]
        foot = p - h[..., None] * n[None]
        inside = np.ones(h.shape, bool)
        for u, w in ((a, b), (b, c), (c, a)):
            inside &= (np.cross((w - u)[None], foot - u[None]) * n[None]).sum(-1) >= 0
        d2 = np.minimum(np.minimum(seg(p, a, b), seg(p, b, c)), seg(p, c, a))
        d2 = np.where(inside, h * h, d2)
        out[i:i + chunk] = np.sqrt(d2.min(1))
    return out


def mesh_distance_near(points, verts, faces, k=24, chunk=2048):
    """`mesh_distance` over the k faces whose centroids lie nearest to each point only: an upper bound of the distance,
    and the distance itself when the nearest face is among them (a mesh of small triangles, such as a TSDF mesh, seen
    from nearby); float64.  Faces without area count by their edges."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    tri = np.asarray(verts, np.float64)[faces]                          # [f,3,3]
    cen = tri.mean(1)
    k = min(k, len(tri))
    out = np.empty(P.shape[0])

    def seg(p, u, w):
        e = w - u
        ee = (e * e).sum(-1)
        s = np.clip(((p - u) * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
        d = p - (u + s[..., None] * e)
        return (d * d).sum(-1)

    for i in range(0, P.shape[0], chunk):
        p = P[i:i + chunk]
        d2c = ((p[:, None, :] - cen[None]) ** 2).sum(-1)
        idx = np.argpartition(d2c, k - 1, axis=1)[:, :k]                # [m,k]
        a, b, c = (tri[idx, j] for j in range(3))                       # [m,k,3]
        p = p[:, None, :]
        n = np.cross(b - a, c - a)
        nn = (n * n).sum(-1)
        flat = nn > 0
        n = n / np.sqrt(np.where(flat, nn, 1.0))[..., None]
        h = ((p - a) * n).sum(-1)
        foot = p - h[..., None] * n
        inside = flat.copy()
        for u, w in ((a, b), (b, c), (c, a)):
            inside &= (np.cross(w - u, foot - u) * n).sum(-1) >= 0
        d2 = np.minimum(np.minimum(seg(p, a, b), seg(p, b, c)), seg(p, c, a))
        out[i:i + chunk] = np.sqrt(np.where(inside, h * h, d2).min(1))
    return out


def face_normals(mesh):
    """unit normals [k,3] float64 of a mesh's triangles, (v1 - v0) x (v2 - v0)"""
    v = np.asarray(mesh["verts"], np.float64)
    f = mesh["faces"]
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def truth_normals(sc, b, v):
    """-> [H,W,3] float64: the normal of the hit face in the frame of camera v of track b, facing the camera; NaN at a miss"""
    T = sc.truth[b][v]
    R, t = np.asarray(sc.R[b, v], np.float64), np.asarray(sc.t[b, v], np.float64)
    n = face_normals(sc.meshes[b])[np.maximum(T["face"], 0)] @ R.T
    Xc = T["X"] @ R.T + t
    n = np.where((n * Xc).sum(-1, keepdims=True) > 0, -n, n)
    return np.where(T["hit"][..., None], n, np.nan)


def truth_points(sc, b, mask_key="hit"):
    """the truth points of the pixels of all views of track b under a mask -> [n,3] float64"""
    return np.concatenate([sc.truth[b][v]["X"][sc.truth[b][v][mask_key]] for v in range(V)])


def recon_grid(voxel, pad=4):
    """-> (origin f32 [B,3], dims = (nx, ny, nz)): per track the bounding box of its truth points padded by `pad` voxels;
    dims is the larger of the two tracks' on every axis"""
    sc = scene()
    lo = np.stack([truth_points(sc, b).min(0) - pad * voxel for b in range(B)])
    hi = np.stack([truth_points(sc, b).max(0) + pad * voxel for b in range(B)])
    dims = tuple(int(n) for n in (np.ceil((hi - lo) / voxel).astype(np.int64) + 1).max(0))
    return np.ascontiguousarray(lo.astype(np.float32)), dims


FIELD_PERIODS = (2.3, 1.7, 3.1)                                   # metres
FIELD_PHASES = (0.0, 1.0, 2.0)


def field(X):
    """[...,3] world points -> [...] float64 in [0, 1]: 1/2 + the mean of three sines, one per coordinate, / 2"""
    X = np.asarray(X, np.float64)
    s = sum(np.sin(2 * np.pi * X[..., c] / FIELD_PERIODS[c] + FIELD_PHASES[c]) for c in range(3))
    return 0.5 + s / 6.0


def field_images(b):
    """-> f32 [V,1,H,W]: the field at the truth points of track b's views, 0 at a miss"""
    sc = scene()
    return np.stack([np.where(T["hit"], field(T["X"]), 0.0)[None] for T in sc.truth[b]]).astype(np.float32)


def silhouette_mask(face):
    """face [H,W] triangle ids -> bool [H,W]: the 3 x 3 neighbourhood (inside the image) holds two surfaces or a miss"""
    surf = np.where(face >= 0, face // 2, -1)
    pad = np.pad(surf, 1, mode="edge")
    out = surf < 0
    for dy in range(3):
        for dx in range(3):
            n = pad[dy:dy + H, dx:dx + W]
            out |= (n != surf) | (n < 0)
    return out


REACH = 0.5                                                       # of the silhouette rule, in voxels


def near_silhouette(T, f_reach, us, vs, z_limit):
    """the truth T of a view, f_reach = focal length * the reach as a length, projections (us, vs) [n] in pixels and depths
    z_limit [n] -> bool [n]: the centre of a silhouette pixel whose z_near is below z_limit lies within f_reach / z_near
    pixels of (us, vs)"""
    sil = silhouette_mask(T["face"])
    pad = np.pad(T["z64"], 1, mode="edge")
    z_near = np.min([pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], 0)
    with np.errstate(all="ignore"):
        radius = np.where(sil & np.isfinite(z_near), f_reach / z_near, -1.0)
    out = np.zeros(len(us), bool)
    xs, ys = np.floor(us + 0.5).astype(np.int64), np.floor(vs + 0.5).astype(np.int64)
    r_max = int(np.ceil(radius.max())) + 1
    for dy in range(-r_max, r_max + 1):
        for dx in range(-r_max, r_max + 1):
            y, x = ys + dy, xs + dx
            ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            y, x = np.where(ok, y, 0), np.where(ok, x, 0)
            out |= ok & (radius[y, x] >= np.hypot(x - us, y - vs)) & (z_near[y, x] < z_limit)
    return out


def occluded64(b, s, points, margin, reach=REACH):
    """-> (occluded, visible, grey) bool [n] for points [n,3] seen from camera s of track b (module docstring)"""
    sc = scene()
    T = sc.truth[b][s]
    K, R, t = (np.asarray(a, np.float64) for a in (sc.K, sc.R[b, s], sc.t[b, s]))
    P = np.asarray(points, np.float64).reshape(-1, 3)
    C = -R.T @ t
    e = P - C
    length = np.linalg.norm(e, axis=1)
    first, _ = ray_mesh(C, e / length[:, None], sc.meshes[b]["verts"], sc.meshes[b]["faces"])
    occluded = first < length - 2 * margin
    visible = first >= length - margin / 2
    Xc = P @ R.T + t
    with np.errstate(all="ignore"):
        us = K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2]
        vs = K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]
        inside = (Xc[:, 2] > 0) & (us >= -0.5) & (us < W - 0.5) & (vs >= -0.5) & (vs < H - 0.5)
    near = near_silhouette(T, K[0, 0] * reach * (margin / 2), np.where(inside, us, 0.0), np.where(inside, vs, 0.0),
                           Xc[:, 2] - 2 * margin)
    grey = ~inside | near | ~(occluded | visible)
    return occluded & ~grey, visible & ~grey, grey


@functools.lru_cache(maxsize=1)
def scene():
    """the one Scene every chain test shares (read only)"""
    return Scene()
