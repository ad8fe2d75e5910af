"""GPU parity of the depth-map normals and the point-to-plane ICP (torchext.depth_normals, depth_icp_system,
depth_icp_update, depth_icp; include/ctd_hip_icp.h) against tests/icp_ref.py.

Normals, residual and assoc equal the numpy restatement at every element (np.array_equal on the values and the NaN masks;
the rules use IEEE add, sub, mul, div, sqrt, floor and compares only, so a mismatch is an ordering bug on one of the two
sides).  The count of a system is equal; every other entry is a sum of exact f64 products in an order the header fixes,
compared with math.fsum over the same products: any order lies within (count - 1) * 2^-53 * sum |term| of it.  Every
call runs twice and the two results must be equal bit for bit.  The update is fed the GPU's own systems and compared with
the restatement on the same numbers: ok equal, |dR_ij| <= 2^-23 (one f32 ulp below 1), |dt_i| <= 2^-23 * max(1, max |t|),
views left unchanged bit for bit.  depth_icp on the corner scene meets the truth predicates and pinned thresholds of
tests/test_depth_icp_host.py; its difference from the restatement's trajectory is printed, not asserted (an association
may flip on a last-bit pose difference)."""
import numpy as np
import pytest
import torch

from tests import fusion_ref as fr
from tests import icp_ref as ir
from tests.test_depth_icp_host import (CORNER_ITERS, CORNER_SEED, CORNER_SHAPE, MAX_FINAL_ROT_ERR_DEG, MAX_FINAL_T_ERR,
                                       MAX_NORMAL_ANGLE_DEG, normal_angles_deg, stencils_on_one_plane)

pytestmark = pytest.mark.gpu

# (B, V, H, W): W no multiple of 64, H * W no multiple of the 1024-pixel chunk of the system kernel; 5 x 7 is less than a
# wavefront, 48 x 80 = 3840 pixels are 4 workgroups a view with a ragged last one, 33 x 130 = 4290 are 5
SHAPES = [(1, 2, 5, 7), (2, 3, 48, 80), (1, 4, 33, 130)]
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(t):
    """a float tensor as integers, so that NaN entries compare equal to themselves"""
    return t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def same_float(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: the NaN positions differ at %d elements" % (
        what, int((np.isnan(got) != np.isnan(want)).sum()))
    a, b = np.nan_to_num(got, nan=0.0), np.nan_to_num(want, nan=0.0)
    assert np.array_equal(a, b), "%s: %d of %d values differ" % (what, int((a != b).sum()), a.size)


def equal_runs(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)), "%s: two runs differ" % what


def unchanged(t_in, before, what):
    for x, x0 in zip(t_in, before):
        assert x is None or torch.equal(bits(x), bits(x0)), "%s: an input was written" % what


def targets_for(B, V):
    """None (every view to view 0) and a table with -1, the view itself, out-of-range entries and, where there are more
    than two views, a target other than view 0: (1,2): [-1 0]; (2,3): [-1 1 0] [-2^31 2 2^31-1]; (1,4): [-1 1 3 4]"""
    tab = np.zeros((B, V), np.int32)
    for b in range(B):
        for s in range(V):
            tab[b, s] = (s + 1) % V                                     # a ring: V == 1 gives the view itself
    tab[0, 0] = -1
    if V > 2:
        tab[0, 1] = 1                                                   # itself
        tab[0, V - 1] = V if V > 3 else 0                               # one past the last view
    if B > 1:
        tab[1, 0] = -2 ** 31
        tab[1, V - 1] = 2 ** 31 - 1
    return [None, tab]


def check_normals(te, sc, with_valid, max_rel, what):
    valid = sc["valid"] if with_valid else None
    want = ir.normals(sc["depth"], sc["ray"], valid, max_rel)
    t_in = [dev(sc["depth"]), dev(sc["ray"]), dev(valid)]
    before = [None if x is None else x.clone() for x in t_in]
    got = te.depth_normals(*t_in, max_rel=max_rel)
    equal_runs((got,), (te.depth_normals(*t_in, max_rel=max_rel),), what)
    same_float(host(got), want, what)
    unchanged(t_in, before, what)
    return want


def check_system(te, sc, normal, with_valid, target, max_dist, what, R=None, t=None):
    """depth_icp_system at one setting, twice, with and without the maps, against the restatement -> the GPU's system"""
    valid = sc["valid"] if with_valid else None
    R, t = (sc["R"] if R is None else R), (sc["t"] if t is None else t)
    want, want_res, want_assoc, abs_sum = ir.icp_system(sc["depth"], normal, sc["ray"], sc["K"], R, t, valid, target,
                                                        max_dist, with_abs=True)
    t_in = [dev(sc["depth"]), dev(normal), dev(sc["ray"]), dev(sc["K"]), dev(R), dev(t), dev(valid), dev(target)]
    before = [None if x is None else x.clone() for x in t_in]
    got = te.depth_icp_system(*t_in, max_dist=max_dist, return_maps=True)
    equal_runs(got, te.depth_icp_system(*t_in, max_dist=max_dist, return_maps=True), what)
    alone = te.depth_icp_system(*t_in, max_dist=max_dist)
    assert isinstance(alone, torch.Tensor)
    equal_runs((alone,), got[:1], what + " without the maps")
    unchanged(t_in, before, what)
    system, residual, assoc = (host(x) for x in got)
    assert system.dtype == np.float64 and system.shape == want.shape and assoc.dtype == np.int64
    same_float(residual, want_res, what + " residual")
    assert np.array_equal(assoc, want_assoc), "%s: %d assoc differ" % (what, int((assoc != want_assoc).sum()))
    assert np.array_equal(system[..., 28], want[..., 28]), "%s: counts %s vs %s" % (what, system[..., 28], want[..., 28])
    bound = np.maximum(want[..., 28:29] - 1, 0) * 2.0 ** -53 * abs_sum
    err = np.abs(system - want)
    worst = np.max(err / np.where(bound > 0, bound, 1.0) * (bound > 0))
    print("%s: largest |system - fsum| = %.3e, largest share of its bound %.3e, counts %s" % (
        what, err.max(), worst, want[..., 28].astype(int).ravel().tolist()))
    assert (err <= bound).all(), "%s: %d entries outside (count - 1) * 2^-53 * sum|term|" % (what, int((err > bound).sum()))
    B, V = R.shape[:2]
    for b in range(B):
        for s in range(V):
            if ir.target_of(target, b, s, V) < 0:
                assert (system[b, s] == 0).all() and np.isnan(residual[b, s]).all() and (assoc[b, s] == -1).all()
    return got[0]


def check_update(te, system, R, t, target, what, **kw):
    """depth_icp_update on the GPU's own system against the restatement on the same numbers"""
    want_R, want_t, want_ok = ir.icp_update(host(system), R, t, target, **kw)
    t_in = [system, dev(R), dev(t), dev(target)]
    before = [None if x is None else x.clone() for x in t_in]
    got = te.depth_icp_update(*t_in, **kw)
    equal_runs(got, te.depth_icp_update(*t_in, **kw), what)
    unchanged(t_in, before, what)
    got_R, got_t, got_ok = (host(x) for x in got)
    assert got_R.dtype == np.float32 and got_t.dtype == np.float32 and got_ok.dtype == np.uint8
    assert got_R.shape == R.shape and got_t.shape == t.shape and got_ok.shape == R.shape[:2]
    assert np.array_equal(got_ok, want_ok), "%s: ok %s vs %s" % (what, got_ok.tolist(), want_ok.tolist())
    dR = np.abs(got_R.astype(np.float64) - want_R).max() if R.size else 0.0
    dt = np.abs(got_t.astype(np.float64) - want_t).max() if t.size else 0.0
    t_tol = ULP * max(1.0, float(np.abs(want_t).max())) if t.size else 0.0
    print("%s: ok %s, largest |dR| %.3e (bound %.3e), largest |dt| %.3e (bound %.3e)" % (what, got_ok.ravel().tolist(), dR,
                                                                                        ULP, dt, t_tol))
    assert dR <= ULP and dt <= t_tol
    still = got_ok == 0
    assert np.array_equal(got_R[still].view(np.int32), R[still].view(np.int32)), what
    assert np.array_equal(got_t[still].view(np.int32), t[still].view(np.int32)), what
    return got_ok


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_normals_equal_the_restatement(te, shape):
    B, V, H, W = shape
    seed = 1000 * B + 100 * V + H + W
    for kind in fr.SCENE_KINDS:
        sc = fr.make_scene(kind, B, V, H, W, seed)
        for with_valid in (True, False):
            for max_rel in (0.02, 0.5, 0.0):
                want = check_normals(te, sc, with_valid, max_rel, "%s %s valid %d max_rel %g" % (kind, shape, with_valid, max_rel))
                if max_rel == 0.5 and kind != "away":
                    assert np.isfinite(want).all(-1).any()               # the case is not vacuous
    sc = ir.make_corner(B, V, H, W, seed)
    want = check_normals(te, sc, True, 0.02, "corner %s" % (shape,))
    has = int(np.isfinite(want).all(-1).sum())
    assert has == B * V * (H - 2) * (W - 2) if min(H, W) >= 33 else has > 0   # (a 5 x 7 image has pixels 7 degrees wide)


def test_normals_of_the_corner_scene_against_the_truth(te):
    sc = ir.make_corner(*CORNER_SHAPE, CORNER_SEED)
    normal = host(te.depth_normals(dev(sc["depth"]), dev(sc["ray"])))
    same = stencils_on_one_plane(sc["plane"])
    assert np.isfinite(normal[same]).all()
    ang = normal_angles_deg(normal, sc["normal_true"])[same]
    print("largest angle to the true normal: %.3e degrees" % ang.max())
    assert ang.max() <= MAX_NORMAL_ANGLE_DEG


@pytest.mark.parametrize("shape", SHAPES)
def test_system_equals_the_restatement(te, shape):
    B, V, H, W = shape
    seed = 1000 * B + 100 * V + H + W
    # a 5 x 7 image has pixels 7 degrees wide: neighbouring depths differ by tens of per cent and a pixel of another view
    # is decimetres away, so the small shape takes wider tolerances to have anything land
    big = min(H, W) >= 33
    normal_rel, max_dists = (0.05, (0.1, 0.004)) if big else (0.5, (1.0, 0.1))
    landed = 0
    for kind in ("noisy", "clean", "away"):
        sc = fr.make_scene(kind, B, V, H, W, seed)
        for with_valid in ((True, False) if kind == "noisy" else (True,)):
            normal = ir.normals(sc["depth"], sc["ray"], sc["valid"] if with_valid else None, 10.0 if kind == "away" else normal_rel)
            assert np.isfinite(normal).all(-1).any()
            for target in targets_for(B, V):
                for max_dist in max_dists:
                    what = "%s %s valid %d target %s max_dist %g" % (kind, shape, with_valid, "ring" if target is not None else None,
                                                                    max_dist)
                    system = check_system(te, sc, normal, with_valid, target, max_dist, what)
                    count = host(system)[..., 28]
                    if kind == "away":
                        assert (count == 0).all()
                    elif target is None and max_dist == max_dists[0]:
                        landed += 1
                        assert (count[:, 1:] > 0).all(), what                # the case is not vacuous
    assert landed == 3
    # at perturbed poses the residuals are large and of both signs
    sc = ir.make_corner(B, V, H, W, seed)
    normal = ir.normals(sc["depth"], sc["ray"], None, normal_rel)
    system = check_system(te, sc, normal, True, None, max_dists[0], "corner %s perturbed" % (shape,), R=sc["R0"], t=sc["t0"])
    assert host(system)[:, 1:, 28].min() > 0


def test_update_on_the_gpus_own_systems(te):
    sc = ir.make_corner(*CORNER_SHAPE, CORNER_SEED)
    B, V = CORNER_SHAPE[:2]
    normal = ir.normals(sc["depth"], sc["ray"])
    t_in = [dev(sc["depth"]), dev(normal), dev(sc["ray"]), dev(sc["K"])]
    for target in targets_for(B, V):
        name = "corner target %s" % ("ring" if target is not None else None)
        system = te.depth_icp_system(*t_in, dev(sc["R0"]), dev(sc["t0"]), target=dev(target))
        ok = check_update(te, system, sc["R0"], sc["t0"], target, name)
        skipped = np.array([[ir.target_of(target, b, s, V) < 0 for s in range(V)] for b in range(B)])
        assert np.array_equal(ok == 0, skipped)                           # every view that has a target moves
        assert not check_update(te, system, sc["R0"], sc["t0"], target, name + " min_count", min_count=10 ** 6).any()
        assert not check_update(te, system, sc["R0"], sc["t0"], target, name + " min_pivot", min_pivot=0.9).any()
        check_update(te, system, sc["R0"], sc["t0"], target, name + " damped", damping=0.5, min_count=0)
    # a single plane: the pivots refuse; with the pivot test off the update goes through
    sp = fr.make_scene("plane", *CORNER_SHAPE, CORNER_SEED)
    R0, t0 = ir.perturb_poses(sp["R"], sp["t"], np.random.RandomState(CORNER_SEED), {1: (1.0, 0.01), 2: (2.0, 0.03)})
    normal = te.depth_normals(dev(sp["depth"]), dev(sp["ray"]))
    system = te.depth_icp_system(dev(sp["depth"]), normal, dev(sp["ray"]), dev(sp["K"]), dev(R0), dev(t0))
    assert not check_update(te, system, R0, t0, None, "plane").any()
    # a zero system (views that see nothing of each other), also at min_count = 0
    sa = fr.make_scene("away", 2, 3, 17, 65, 3)
    normal = te.depth_normals(dev(sa["depth"]), dev(sa["ray"]), max_rel=10.0)
    system = te.depth_icp_system(dev(sa["depth"]), normal, dev(sa["ray"]), dev(sa["K"]), dev(sa["R"]), dev(sa["t"]))
    assert (host(system) == 0).all()
    assert not check_update(te, system, sa["R"], sa["t"], None, "away", min_count=0).any()


def test_depth_icp_refines_the_corner_scene(te):
    """the truth predicates and pinned thresholds of tests/test_depth_icp_host.py, on the GPU"""
    sc = ir.make_corner(*CORNER_SHAPE, CORNER_SEED)
    t_in = [dev(sc[k]) for k in ("depth", "ray", "K", "R0", "t0", "valid")]
    before = [x.clone() for x in t_in]
    R, t, info = te.depth_icp(*t_in, iters=CORNER_ITERS)
    again = te.depth_icp(*t_in, iters=CORNER_ITERS)
    equal_runs((R, t, info["count"], info["rmse"], info["ok"]), again[:2] + tuple(again[2][k] for k in ("count", "rmse", "ok")),
               "depth_icp")
    unchanged(t_in, before, "depth_icp")
    assert info["count"].shape == info["rmse"].shape == (CORNER_ITERS,) + CORNER_SHAPE[:2] and info["count"].is_cuda
    assert info["count"].dtype == torch.float64 and info["ok"].dtype == torch.uint8
    Rg, tg = host(R), host(t)
    rot0, tr0 = ir.pose_errors(sc["R0"], sc["t0"], sc["R"], sc["t"])
    rot1, tr1 = ir.pose_errors(Rg, tg, sc["R"], sc["t"])
    print("translation error %s -> %s, rotation error (degrees) %s -> %s" % (tr0[:, 1:].ravel(), tr1[:, 1:].ravel(),
                                                                              rot0[:, 1:].ravel(), rot1[:, 1:].ravel()))
    assert host(info["ok"]).tolist() == [[0, 1, 1], [0, 1, 1]]
    assert np.array_equal(Rg[:, 0], sc["R0"][:, 0]) and np.array_equal(tg[:, 0], sc["t0"][:, 0])
    assert (tr1[:, 1:] <= tr0[:, 1:] / 20).all()
    assert tr1.max() <= MAX_FINAL_T_ERR and rot1.max() <= MAX_FINAL_ROT_ERR_DEG
    # against the restatement's trajectory: printed, not asserted
    Rr, tref, iref = ir.depth_icp(sc["depth"], sc["ray"], sc["K"], sc["R0"], sc["t0"], sc["valid"], iters=CORNER_ITERS)
    print("difference from the restatement: |dR| %.3e, |dt| %.3e, counts differ by at most %d, rmse by %.3e" % (
        np.abs(Rg.astype(np.float64) - Rr).max(), np.abs(tg.astype(np.float64) - tref).max(),
        int(np.abs(host(info["count"]) - iref["count"]).max()),
        np.nanmax(np.abs(host(info["rmse"])[:, :, 1:] - iref["rmse"][:, :, 1:]))))
    # what the consistency check says before and after
    shares = []
    for Rx, tx in ((sc["R"], sc["t"]), (sc["R0"], sc["t0"]), (Rg, tg)):
        keep = te.depth_consistency(t_in[0], t_in[1], t_in[2], dev(Rx), dev(tx), max_px=1.0, max_rel=0.002)[1]
        shares.append(float(keep.float().mean()))
    print("keep share: true poses %.4f, perturbed %.4f, refined %.4f" % tuple(shares))
    assert shares[2] >= 0.9 * shares[0]


def test_targets_single_views_and_empty_batches(te):
    # V == 1: the only view has nothing to be aligned to
    sc = fr.make_scene("clean", 1, 1, 6, 23, 2)
    normal = check_normals(te, sc, True, 0.05, "V == 1")
    for target in (None, np.zeros((1, 1), np.int32), np.full((1, 1), 5, np.int32)):
        system = check_system(te, sc, normal, True, target, 0.1, "V == 1")
        assert (host(system) == 0).all()
        assert not check_update(te, system, sc["R"], sc["t"], target, "V == 1", min_count=0).any()
    R, t, info = te.depth_icp(*[dev(sc[k]) for k in ("depth", "ray", "K", "R", "t")], iters=2)
    assert np.array_equal(host(R), sc["R"]) and np.array_equal(host(t), sc["t"]) and not host(info["ok"]).any()
    # B == 0: empty outputs of the right shapes, nothing launched
    H, W = 6, 23
    d0 = torch.empty((0, 3, H, W), device="cuda")
    ray, K = dev(sc["ray"]), dev(sc["K"])
    R0, t0 = torch.empty((0, 3, 3, 3), device="cuda"), torch.empty((0, 3, 3), device="cuda")
    n0 = te.depth_normals(d0, ray)
    assert n0.shape == (0, 3, H, W, 3)
    s0, r0, a0 = te.depth_icp_system(d0, n0, ray, K, R0, t0, return_maps=True)
    assert s0.shape == (0, 3, 29) and r0.shape == (0, 3, H, W) and a0.shape == (0, 3, H, W) and a0.dtype == torch.int64
    Ru, tu, ok = te.depth_icp_update(s0, R0, t0)
    assert Ru.shape == (0, 3, 3, 3) and tu.shape == (0, 3, 3) and ok.shape == (0, 3)
    Ri, ti, info = te.depth_icp(d0, ray, K, R0, t0, iters=3)
    assert Ri.shape == (0, 3, 3, 3) and info["count"].shape == (3, 0, 3) and info["ok"].shape == (0, 3)


def test_bad_inputs_are_rejected_loudly(te):
    sc = ir.make_corner(1, 2, 5, 7, 1)
    depth, ray, K, R, t, valid = [dev(sc[k]) for k in ("depth", "ray", "K", "R", "t", "valid")]
    normal = te.depth_normals(depth, ray)
    system = te.depth_icp_system(depth, normal, ray, K, R, t)
    target = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    wide = torch.zeros((1, 2, 5, 14), device="cuda")[..., ::2]              # the right shape, not contiguous
    assert wide.shape == depth.shape and not wide.is_contiguous()
    with pytest.raises(RuntimeError, match="contiguous"):
        te.depth_normals(wide, ray)
    with pytest.raises(RuntimeError, match="contiguous"):
        te.depth_icp_system(depth, torch.zeros((1, 2, 5, 7, 6), device="cuda")[..., ::2], ray, K, R, t)
    with pytest.raises(RuntimeError, match="contiguous"):
        te.depth_icp_system(depth, normal, ray, K, R.transpose(2, 3), t)
    with pytest.raises(RuntimeError, match="contiguous"):
        te.depth_icp_update(system, R.transpose(2, 3), t)
    with pytest.raises(RuntimeError, match="contiguous"):
        te.depth_icp(depth, ray, K, R, t, target=torch.zeros((1, 4), dtype=torch.int32, device="cuda")[:, ::2])
    # wrong device: any one tensor left on the host
    for args in ((depth.cpu(), ray), (depth, ray.cpu()), (depth, ray, valid.cpu())):
        with pytest.raises(RuntimeError):
            te.depth_normals(*args)
    for k in range(6):
        args = [depth, normal, ray, K, R, t]
        args[k] = args[k].cpu()
        with pytest.raises(RuntimeError):
            te.depth_icp_system(*args)
    with pytest.raises(RuntimeError):
        te.depth_icp_system(depth, normal, ray, K, R, t, target=target.cpu())
    with pytest.raises(RuntimeError):
        te.depth_icp_system(depth, normal, ray, K, R, t, valid=valid.cpu())
    for k in range(3):
        args = [system, R, t]
        args[k] = args[k].cpu()
        with pytest.raises(RuntimeError):
            te.depth_icp_update(*args)
    with pytest.raises(RuntimeError):
        te.depth_icp(depth, ray, K, R.cpu(), t)
    # flat poses: the other track ops take them by element count, depth_icp sizes its update by them and refuses
    for bad_R, bad_t in ((R.reshape(2, 3, 3), t), (R.reshape(6, 3), t), (R, t.reshape(2, 3)), (R, t.reshape(-1))):
        with pytest.raises(RuntimeError, match=r"R must be shaped \[B,V,3,3\] and t \[B,V,3\]"):
            te.depth_icp(depth, ray, K, bad_R, bad_t)
    flat = te.depth_icp_system(depth, normal, ray, K, R.reshape(2, 3, 3), t.reshape(2, 3))   # fine here: sized by depth
    assert torch.equal(bits(flat), bits(system))
    # wrong dtype or shape of target, normal and system
    for bad in (target.long(), target.float(), target[:, :1], target.reshape(2, 1), [[0, 0]]):
        with pytest.raises(RuntimeError, match="target must be"):
            te.depth_icp_system(depth, normal, ray, K, R, t, target=bad)
        with pytest.raises(RuntimeError, match="target must be"):
            te.depth_icp_update(system, R, t, target=bad)
    with pytest.raises(RuntimeError, match="normal must be shaped"):
        te.depth_icp_system(depth, normal[..., :2].contiguous(), ray, K, R, t)
    with pytest.raises(RuntimeError):
        te.depth_icp_update(system.float(), R, t)
    with pytest.raises(RuntimeError, match="system"):
        te.depth_icp_update(system[..., :28].contiguous(), R, t)
