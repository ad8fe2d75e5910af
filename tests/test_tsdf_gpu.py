"""GPU parity of the truncated signed distance volumes (torchext.tsdf_integrate, tsdf_surface_points, tsdf_raycast;
include/ctd_hip_tsdf.h) against tests/tsdf_ref.py.

Every output equals the numpy restatement bit for bit (the rules use IEEE add, sub, mul, div, sqrt, floor, min and
compares only, so a mismatch is an ordering bug on one of the two sides), NaN patterns included, and every call runs
twice from equal inputs with equal bits.  The volumes start from a sentinel pattern in tsdf (random values and NaNs
where weight == 0, which no call may read or, untouched, overwrite).  The chain test runs depth_consistency ->
tsdf_integrate(valid=keep) -> tsdf_raycast -> depth_icp on the corner scene and meets the pins of
tests/test_tsdf_host.py."""
import numpy as np
import pytest
import torch

from tests import fusion_ref as fr
from tests import icp_ref as ir
from tests import tsdf_ref as tr
from tests.test_tsdf_mesh_gpu import SCAN_GRIDS
from tests.test_tsdf_host import (CAST, CORNER_DIMS, CORNER_SHAPE, F2M_ITERS, MAX_F2M_ROT_ERR_DEG, MAX_F2M_T_ERR, corner_model,
                                  model_track)

pytestmark = pytest.mark.gpu

F = np.float32
# (nx, ny, nz): 33 x 18 is one ragged 64 x 4 tile row and five tile rows, 12474 voxels are 49 chunks of 256 with a ragged last
# one; 64 x 5 fills a tile row exactly and leaves a one-row tile; 2 x 2 x 2 is less than a wavefront and one cell
GRIDS = [(33, 18, 21), (64, 5, 7), (2, 2, 2)]
# SCAN_GRIDS, for the surface points alone (tests/test_tsdf_mesh_gpu.py says why): more workgroup counts than one round of
# the scan takes, a last chunk of one voxel, a track of exactly one chunk
IMAGES = [(24, 40), (17, 29)]
B = 2


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s vs %s %s" % (what, got.dtype, got.shape, want.dtype,
                                                                                      want.shape)
    view = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
    a, b = np.ascontiguousarray(got).view(view), np.ascontiguousarray(want).view(view)
    if got.dtype == F:                                             # any NaN is as good as another; the values are bits
        nan_a, nan_b = np.isnan(got), np.isnan(want)
        assert np.array_equal(nan_a, nan_b), "%s: the NaN positions differ at %d elements" % (what, int((nan_a != nan_b).sum()))
        a, b = np.where(nan_a, 0, a), np.where(nan_b, 0, b)
    assert np.array_equal(a, b), "%s: %d of %d elements differ" % (what, int((a != b).sum()), a.size)


def grid(kind, dims):
    """tests/tsdf_ref.grid_for; the 2 x 2 x 2 grid has voxels of 3 with one column on the optical axis, so that the voxel
    (0, 0, 1) of a track lies at z = 2.6, just behind the plane, and is seen"""
    return tr.grid_for(kind, B, dims, 3.0, (-0.2, -0.1)) if dims == (2, 2, 2) else tr.grid_for(kind, B, dims)


def sentinel_volume(dims, seed):
    """a fresh volume whose tsdf holds what no call may read: random values, NaNs and infs; weight 0 everywhere"""
    nx, ny, nz = dims
    rs = np.random.RandomState(seed)
    tsdf = rs.uniform(-3, 3, (B, nz, ny, nx)).astype(F)
    tsdf.reshape(-1)[::7] = np.nan
    tsdf.reshape(-1)[3::11] = np.inf
    return tsdf, np.zeros((B, nz, ny, nx), F)


def random_volume(dims, seed, empty_track=None):
    """a volume nothing integrated: tsdf in [-1.2, 1.2] with exact +-1, zeros and ties, weight in {0, 1, 2, 3}; the tsdf of
    a voxel of weight 0 is NaN"""
    nx, ny, nz = dims
    rs = np.random.RandomState(seed)
    tsdf = np.round(rs.uniform(-1.2, 1.2, (B, nz, ny, nx)) * 8) / 8                # multiples of 1/8: ties of |T| are common
    weight = rs.randint(0, 4, (B, nz, ny, nx)) * (rs.rand(B, nz, ny, nx) < 0.9)
    if empty_track is not None:
        weight[empty_track] = 0
    tsdf = np.where(weight == 0, np.nan, tsdf)
    return tsdf.astype(F), weight.astype(F)


def integrate_on_gpu(te, T0, w0, origin, voxel, sc, valid, views=None, **kw):
    """tsdf_integrate from clones of T0, w0 over some views of the scene -> the volume as numpy; the inputs stay"""
    sel = slice(None) if views is None else views
    t_in = [dev(sc["depth"][:, sel]), dev(sc["ray"]), dev(sc["K"]), dev(sc["R"][:, sel]), dev(sc["t"][:, sel]),
            dev(None if valid is None else valid[:, sel])]
    before = [None if x is None else x.clone() for x in t_in]
    T, w, o = dev(T0), dev(w0), dev(origin)
    out = te.tsdf_integrate(T, w, o, voxel, *t_in[:5], valid=t_in[5], **kw)
    assert out[0] is T and out[1] is w
    for x, x0 in zip(t_in + [o], before + [dev(origin)]):
        assert x is None or torch.equal(x.view(torch.uint8).reshape(-1), x0.view(torch.uint8).reshape(-1)), "an input was written"
    return host(T), host(w)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", GRIDS)
def test_integrate_equals_the_restatement(te, dims):
    touched = 0
    for (H, W) in IMAGES:
        for V in (1, 3, 4):
            for kind in fr.SCENE_KINDS:
                seed = 100 * V + H + dims[0]
                sc = fr.make_scene(kind, B, V, H, W, seed)
                origin, voxel = grid(kind, dims)
                T0, w0 = sentinel_volume(dims, seed)
                for with_valid in (True, False):
                    what = "%s %s %dx%d V=%d valid %d" % (kind, dims, H, W, V, with_valid)
                    valid = sc["valid"] if with_valid else None
                    want = tr.integrate(T0, w0, origin, voxel, sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], valid)
                    got = integrate_on_gpu(te, T0, w0, origin, voxel, sc, valid)
                    again = integrate_on_gpu(te, T0, w0, origin, voxel, sc, valid)
                    same_bits(got[0], again[0], what + ": two runs, tsdf")
                    same_bits(got[1], again[1], what + ": two runs, weight")
                    same_bits(got[1], want[1], what + " weight")
                    same_bits(got[0], want[0], what + " tsdf")
                    assert np.array_equal(got[0].view(np.int32)[want[1] == 0], T0.view(np.int32)[want[1] == 0]), what
                    if kind == "away":                              # no projection lands: untouched bit for bit
                        assert np.array_equal(got[0].view(np.int32), T0.view(np.int32)) and not got[1].any(), what
                        continue
                    touched += int((want[1] > 0).sum())
                    # a second integration on top of the first, capped at 2: the weights are not 0 now
                    want2 = tr.integrate(want[0], want[1], origin, voxel, sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], valid,
                                         trunc=1.7 * voxel, max_weight=2.0)
                    got2 = integrate_on_gpu(te, got[0], got[1], origin, voxel, sc, valid, trunc=1.7 * voxel, max_weight=2.0)
                    same_bits(got2[1], want2[1], what + " second pass, weight")
                    same_bits(got2[0], want2[0], what + " second pass, tsdf")
                    assert not np.array_equal(want2[0].view(np.int32), want[0].view(np.int32))   # (it did something)
                    if V == 4:                                      # views {0,1} and then {2,3}: the bits of one call
                        half = integrate_on_gpu(te, T0, w0, origin, voxel, sc, valid, views=slice(0, 2))
                        both = integrate_on_gpu(te, half[0], half[1], origin, voxel, sc, valid, views=slice(2, 4))
                        same_bits(both[0], got[0], what + " split, tsdf")
                        same_bits(both[1], got[1], what + " split, weight")
    print("%s: %d voxel updates compared" % (dims, touched))
    assert touched > (0 if dims == (2, 2, 2) else 1000)             # the cases are not vacuous


def test_the_parity_grid_reaches_behind_the_cameras_and_outside_every_frustum():
    """what tests/tsdf_ref.grid_for promises for the big grid: voxels behind the cameras, voxels in front that no view
    sees, and voxels of every weight up to V"""
    dims, (H, W), V = GRIDS[0], IMAGES[0], 4
    sc = fr.make_scene("clean", B, V, H, W, 1)
    origin, voxel = tr.grid_for("clean", B, dims)
    T, w = tr.integrate(*tr.volume(B, *dims), origin, voxel, sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], sc["valid"])
    z = tr.centres(origin[0], voxel, *dims)[2].reshape(w[0].shape)
    assert (z < -0.1).any() and not w[0][z < -0.1].any()            # behind every camera
    assert (w[0][(z > 0.5) & (z < 1.5)] == 0).any()                 # in front, beside every frustum
    assert set(np.unique(w)) == {0, 1, 2, 3, 4}
    assert tr.usable_mask(T, w).sum() > 500 and (T[w > 0] < 0).any()


# ---------------------------------------------------------------------------------------------------------------------
def surface_c_call(T, w, o, voxel, min_weight, points, normals, src, capacity):
    """ctd_tsdf_surface_points_f32 on device tensors (points None: count only) -> n_per_track"""
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    Bb, nz, ny, nx = T.shape
    n_per_track = torch.full((Bb,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(L.ctd_tsdf_surface_workspace_bytes(Bb, nx, ny, nz), dtype=torch.uint8, device="cuda")
    ptr = lambda x: None if x is None else x.data_ptr()           # noqa: E731
    st = L.ctd_tsdf_surface_points_f32(ptr(T), ptr(w), ptr(o), voxel, min_weight, ptr(points), ptr(normals), ptr(src),
                                       ptr(n_per_track), capacity, Bb, nx, ny, nz, ptr(ws), ws.numel(), 0,
                                       torch.cuda.current_stream().cuda_stream)
    _lib.check(st, "ctd_tsdf_surface_points_f32")
    return n_per_track


def check_surface(te, T, w, origin, voxel, min_weight, what):
    want_p, want_n, want_src, want_count = tr.surface_points(T, w, origin, voxel, min_weight)
    t_in = [dev(T), dev(w), dev(origin)]
    before = [x.clone() for x in t_in]
    got = te.tsdf_surface_points(*t_in, voxel, min_weight=min_weight, return_normals=True)
    again = te.tsdf_surface_points(*t_in, voxel, min_weight=min_weight, return_normals=True)
    for x, y in zip(got, again):
        same_bits(host(x), host(y), what + ": two runs")
    for x, x0 in zip(t_in, before):
        assert torch.equal(x.view(torch.int32), x0.view(torch.int32)), what + ": an input was written"
    points, src, n_per_track, normals = (host(x) for x in got)
    assert np.array_equal(n_per_track, want_count), "%s: counts %s vs %s" % (what, n_per_track, want_count)
    same_bits(src, want_src, what + " src")
    same_bits(points, want_p, what + " points")
    same_bits(normals, want_n, what + " normals")
    alone = te.tsdf_surface_points(*t_in, voxel, min_weight=min_weight)
    assert len(alone) == 3
    same_bits(host(alone[0]), want_p, what + " without normals")
    # the count-only call
    assert np.array_equal(host(surface_c_call(*t_in, voxel, min_weight, None, None, None, 0)), want_count), what
    # capacity = half the total: exactly the first half, the rest of the buffers untouched; the counts stay the true ones
    m = len(want_src)
    half = m // 2
    p = torch.full((m + 1, 3), -7.0, device="cuda")
    n = torch.full((m + 1, 3), -7.0, device="cuda")
    s = torch.full((m + 1,), -7, dtype=torch.int64, device="cuda")
    assert np.array_equal(host(surface_c_call(*t_in, voxel, min_weight, p, n, s, half)), want_count), what
    same_bits(host(p)[:half], want_p[:half], what + " capacity, points")
    same_bits(host(n)[:half], want_n[:half], what + " capacity, normals")
    same_bits(host(s)[:half], want_src[:half], what + " capacity, src")
    assert (host(p)[half:] == -7).all() and (host(n)[half:] == -7).all() and (host(s)[half:] == -7).all(), what
    return m, int(np.isfinite(want_n).all(1).sum())


@pytest.mark.parametrize("dims", GRIDS + SCAN_GRIDS)
def test_surface_points_equal_the_restatement(te, dims):
    H, W = IMAGES[0]
    n_points = n_normals = 0
    for kind in ("clean", "noisy") if dims in GRIDS else ():         # (the scan grids: random volumes only)
        sc = fr.make_scene(kind, B, 4, H, W, 7)
        origin, voxel = grid(kind, dims)
        T, w = tr.integrate(*sentinel_volume(dims, 7), origin, voxel, sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], sc["valid"])
        for min_weight in (1.0, 2.0):
            m, k = check_surface(te, T, w, origin, voxel, min_weight, "%s %s min_weight %g" % (kind, dims, min_weight))
            n_points, n_normals = n_points + m, n_normals + k
    if dims == GRIDS[0]:
        assert n_points > 1000 and n_normals > 100                  # the cases are not vacuous
    # a volume of random values: crossings along every axis, ties of |T|, |T| == 1, neighbours of weight 0 and outside
    # the grid; track 1 is empty
    origin, voxel = tr.grid_for("clean", B, dims)
    T, w = random_volume(dims, 11, empty_track=1)
    for min_weight in (1.0, 2.0):
        want = tr.surface_points(T, w, origin, voxel, min_weight)
        assert want[3][1] == 0 and (dims == (2, 2, 2) or want[3][0] > 0)
        if dims in SCAN_GRIDS and min_weight == 2.0:
            continue
        m, k = check_surface(te, T, w, origin, voxel, min_weight, "random %s min_weight %g" % (dims, min_weight))
        if dims == GRIDS[0]:
            assert m > 1000 and 0 < k < m and len(set((want[2] % 3).tolist())) == 3
    T, w = random_volume(dims, 12, empty_track=0)                   # the empty track first: its offsets are all 0
    check_surface(te, T, w, origin, voxel, 1.0, "random %s, track 0 empty" % (dims,))
    if dims in SCAN_GRIDS:                                          # both tracks full: track 1 starts from track 0's total
        m, _ = check_surface(te, *random_volume(dims, 13), origin, voxel, 1.0, "random %s, both tracks" % (dims,))
        assert m > (100000 if dims[2] > 1 else 0)                   # the cases are not vacuous


# ---------------------------------------------------------------------------------------------------------------------
def cast_poses(rs):
    """R [B,3,3,3], t [B,3,3]: a view that looks into the grid, one turned 25 degrees about y (partly past it) and one
    turned 180 degrees (away from it)"""
    R, t = fr.overlapping_poses(rs, B, 3)
    for b in range(B):
        R[b, 1] = (fr._rot(np.array([0.0, np.deg2rad(25.0), 0.0])) @ R[b, 1].astype(np.float64)).astype(F)
        R[b, 2] = (fr._rot(np.array([0.0, np.pi, 0.0])) @ R[b, 2].astype(np.float64)).astype(F)
    return np.ascontiguousarray(R), np.ascontiguousarray(t)


def check_cast(te, T, w, origin, voxel, ray, R, t, H, W, d_min, step, n_steps, min_weight, what):
    want = tr.raycast(T, w, origin, voxel, ray, R, t, H, W, d_min, step, n_steps, min_weight)
    t_in = [dev(T), dev(w), dev(origin)]
    p_in = [dev(ray), dev(R), dev(t)]
    before = [x.clone() for x in t_in + p_in]
    got = te.tsdf_raycast(*t_in, voxel, *p_in, H, W, d_min, step, n_steps, min_weight=min_weight)
    again = te.tsdf_raycast(*t_in, voxel, *p_in, H, W, d_min, step, n_steps, min_weight=min_weight)
    same_bits(host(got), host(again), what + ": two runs")
    for x, x0 in zip(t_in + p_in, before):
        assert torch.equal(x.view(torch.int32), x0.view(torch.int32)), what + ": an input was written"
    same_bits(host(got), want, what)
    return np.isfinite(want).reshape(want.shape[0], want.shape[1], -1).sum(-1)


@pytest.mark.parametrize("dims", GRIDS)
def test_raycast_equals_the_restatement(te, dims):
    hits = np.zeros(3, np.int64)
    for (H, W) in IMAGES:
        K, ray = fr.camera(H, W)
        R, t = cast_poses(np.random.RandomState(H))
        sc = fr.make_scene("noisy", B, 4, H, W, 9)
        origin, voxel = grid("noisy", dims)
        T, w = tr.integrate(*sentinel_volume(dims, 9), origin, voxel, sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], sc["valid"])
        for min_weight in (1.0, 2.0):
            for d_min, step, n_steps in ((0.5, 0.07, 48), (0.0, 0.1, 32), (1.9, 0.02, 64)):
                what = "integrated %s %dx%d min_weight %g from %g by %g x %d" % (dims, H, W, min_weight, d_min, step, n_steps)
                hits += check_cast(te, T, w, origin, voxel, ray, R, t, H, W, d_min, step, n_steps, min_weight, what).sum(0)
        Tr, wr = random_volume(dims, 13, empty_track=None)
        for min_weight in (1.0, 2.0):
            what = "random %s %dx%d min_weight %g" % (dims, H, W, min_weight)
            check_cast(te, Tr, wr, origin, voxel, ray, R, t, H, W, 0.3, 0.06, 56, min_weight, what)
    if dims == GRIDS[0]:
        assert hits[0] > 1000 and hits[1] > 100 and hits[2] == 0, hits   # into the grid, partly past it, away from it


def test_single_steps_single_views_and_empty_batches(te):
    dims, (H, W) = GRIDS[0], IMAGES[1]
    sc = fr.make_scene("clean", B, 1, H, W, 3)
    origin, voxel = tr.grid_for("clean", B, dims)
    T, w = tr.integrate(*tr.volume(B, *dims), origin, voxel, sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"])
    check_cast(te, T, w, origin, voxel, sc["ray"], sc["R"], sc["t"], H, W, 2.0, 0.05, 1, 1.0, "one step")    # never a hit
    check_cast(te, T, w, origin, voxel, sc["ray"], sc["R"], sc["t"], H, W, 2.0, 0.5, 2, 1.0, "two steps")
    # tsdf_volume: ones and zeros of the right shape
    Tv, wv = te.tsdf_volume(B, *dims)
    assert Tv.shape == wv.shape == (B, dims[2], dims[1], dims[0]) and Tv.is_cuda and bool((Tv == 1).all()) and not bool(wv.any())
    # B == 0: empty outputs of the right shapes, nothing launched
    T0, w0 = te.tsdf_volume(0, 4, 5, 6)
    o0 = torch.empty((0, 3), device="cuda")
    d0 = torch.empty((0, 2, H, W), device="cuda")
    R0, t0 = torch.empty((0, 2, 3, 3), device="cuda"), torch.empty((0, 2, 3), device="cuda")
    ray, K = dev(sc["ray"]), dev(sc["K"])
    assert te.tsdf_integrate(T0, w0, o0, 0.1, d0, ray, K, R0, t0)[0] is T0
    p, s, n_per_track, nrm = te.tsdf_surface_points(T0, w0, o0, 0.1, return_normals=True)
    assert p.shape == (0, 3) and s.shape == (0,) and n_per_track.shape == (0,) and nrm.shape == (0, 3) and s.dtype == torch.int64
    assert te.tsdf_raycast(T0, w0, o0, 0.1, ray, R0, t0, H, W, 0.5, 0.1, 4).shape == (0, 2, H, W)
    # a volume without a crossing: no points, the right dtypes
    p, s, n_per_track = te.tsdf_surface_points(*te.tsdf_volume(B, *dims), dev(origin), voxel)
    assert p.shape == (0, 3) and s.shape == (0,) and host(n_per_track).tolist() == [0, 0]


def test_bad_inputs_are_rejected_loudly(te):
    dims, (H, W) = (6, 5, 4), (5, 7)
    sc = fr.make_scene("clean", B, 2, H, W, 1)
    depth, ray, K, R, t, valid = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t", "valid")]
    T, w = te.tsdf_volume(B, *dims)
    origin = dev(tr.grid_for("clean", B, dims)[0])
    wide = torch.zeros((B, 4, 5, 12), device="cuda")[..., ::2]              # the right shape, not contiguous
    assert wide.shape == T.shape and not wide.is_contiguous()
    for call in (lambda: te.tsdf_integrate(wide, w, origin, 0.1, depth, ray, K, R, t),
                 lambda: te.tsdf_integrate(T, w, origin, 0.1, depth, ray, K, R.transpose(2, 3), t),
                 lambda: te.tsdf_surface_points(T, wide, origin, 0.1),
                 lambda: te.tsdf_raycast(T, w, origin, 0.1, ray, R.transpose(2, 3), t, H, W, 0.5, 0.1, 4)):
        with pytest.raises(RuntimeError, match="contiguous"):
            call()
    # wrong device: any one tensor left on the host
    for k in range(8):
        args = [T, w, origin, depth, ray, K, R, t]
        args[k] = args[k].cpu()
        with pytest.raises(RuntimeError):
            te.tsdf_integrate(*args[:3], 0.1, *args[3:])
    with pytest.raises(RuntimeError):
        te.tsdf_integrate(T, w, origin, 0.1, depth, ray, K, R, t, valid=valid.cpu())
    for k in range(3):
        args = [T, w, origin]
        args[k] = args[k].cpu()
        with pytest.raises(RuntimeError):
            te.tsdf_surface_points(*args, 0.1)
    for k in range(6):
        args = [T, w, origin, ray, R, t]
        args[k] = args[k].cpu()
        with pytest.raises(RuntimeError):
            te.tsdf_raycast(*args[:3], 0.1, *args[3:], H, W, 0.5, 0.1, 4)
    # shapes
    with pytest.raises(RuntimeError, match=r"tsdf and weight \[B,nz,ny,nx\]"):
        te.tsdf_integrate(T, w[:, :3].contiguous(), origin, 0.1, depth, ray, K, R, t)
    with pytest.raises(RuntimeError, match=r"tsdf and weight \[B,nz,ny,nx\]"):
        te.tsdf_surface_points(T[0], w[0], origin, 0.1)
    with pytest.raises(RuntimeError, match=r"origin must be shaped \[B,3\]"):
        te.tsdf_surface_points(T, w, origin[:1].contiguous(), 0.1)
    with pytest.raises(RuntimeError, match="must have the B of tsdf"):
        te.tsdf_integrate(T, w, origin, 0.1, depth[:1].contiguous(), ray, K, R[:1].contiguous(), t[:1].contiguous())
    with pytest.raises(RuntimeError, match=r"R must be shaped \[B,V,3,3\] and t \[B,V,3\]"):
        te.tsdf_raycast(T, w, origin, 0.1, ray, R.reshape(4, 3, 3), t, H, W, 0.5, 0.1, 4)
    with pytest.raises(RuntimeError, match=r"ray \[H\*W,3\] expected"):
        te.tsdf_raycast(T, w, origin, 0.1, ray, R, t, H, W + 1, 0.5, 0.1, 4)
    # an output over an input: the library refuses
    with pytest.raises(RuntimeError, match="invalid argument"):
        te.tsdf_integrate(T, T, origin, 0.1, depth, ray, K, R, t)


# ---------------------------------------------------------------------------------------------------------------------
def test_the_chain_from_consistency_to_frame_to_model_alignment(te):
    """depth_consistency -> tsdf_integrate(valid=keep) -> tsdf_raycast -> depth_icp with the model as view 0, on the
    corner scene: the pins of tests/test_tsdf_host.py"""
    sc = corner_model()
    vw = sc["views"]
    ray, K = dev(sc["ray"]), dev(sc["K"])
    depth, R, t = dev(vw["depth"]), dev(vw["R"]), dev(vw["t"])
    keep = te.depth_consistency(depth, ray, K, R, t, max_px=1.0, max_rel=0.01, min_views=1)[1]
    assert np.array_equal(host(keep), vw["keep"])
    T, w = te.tsdf_volume(1, *CORNER_DIMS)
    origin = dev(sc["origin"])
    te.tsdf_integrate(T, w, origin, sc["voxel"], depth, ray, K, R, t, valid=keep)
    cast = te.tsdf_raycast(T, w, origin, sc["voxel"], ray, dev(sc["R_cast"]), dev(sc["t_cast"]), *CORNER_SHAPE[2:], CAST["d_min"],
                           CAST["step"], CAST["n_steps"])
    want_T, want_w = tr.integrate(*tr.volume(1, *CORNER_DIMS), sc["origin"], sc["voxel"], vw["depth"], sc["ray"], sc["K"],
                                  vw["R"], vw["t"], vw["keep"])
    same_bits(host(T), want_T, "corner tsdf")
    same_bits(host(w), want_w, "corner weight")
    same_bits(host(cast), tr.raycast(want_T, want_w, sc["origin"], sc["voxel"], sc["ray"], sc["R_cast"], sc["t_cast"],
                                     *CORNER_SHAPE[2:], **CAST), "corner cast")
    track, R0, t0, R_true, t_true = model_track(sc, host(cast))
    Rg, tg, info = te.depth_icp(dev(track), ray, K, dev(R0), dev(t0), iters=F2M_ITERS)
    rot0, tr0 = ir.pose_errors(R0, t0, R_true, t_true)
    rot1, tr1 = ir.pose_errors(host(Rg), host(tg), R_true, t_true)
    print("frame to model: translation error %.3e -> %.3e, rotation error %.4f -> %.3e degrees, hit share %.4f" % (
        tr0[0, 1], tr1[0, 1], rot0[0, 1], rot1[0, 1], float(np.isfinite(host(cast)).mean())))
    assert host(info["ok"]).tolist() == [[0, 1]]
    assert tr1[0, 1] <= MAX_F2M_T_ERR and rot1[0, 1] <= MAX_F2M_ROT_ERR_DEG
    # and the model as a band prior: the cast, as disparities, has a band at every pixel that hit
    disp = te.depth_to_disp(cast[:, 0].contiguous(), 60.0)        # 60 / 2.1 .. 2.7: disparities of 22 .. 29 of 64
    lo, hi = te.disparity_band_window(disp, 2, 64)
    hit = torch.isfinite(cast[:, 0])
    assert bool(hit.any()) and bool((hi >= lo)[hit].all()) and bool(((hi - lo)[hit] < 63).all())
