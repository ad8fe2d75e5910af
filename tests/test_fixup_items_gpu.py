"""GPU parity of the fix-up pass on prepared patterns (ncc_fixup.hip: pattern-side tables filled by `prepare_pattern`,
items of one listed pattern window x one frame x one block of 64 disparities) and of the table-less kernel next to it.

Every case is held against the reference-order kernel (`xcorrvol_batch(algo='exact')` + `argmax_disp`): indices bit for
bit, the volume entries of listed windows bit for bit, every other entry within 1e-5 |b| + 1e-6.  The inputs list on both
sides -- a pattern with a constant left part and a constant band (listed pattern windows, listed fully clamped runs), frames
with one flat patch (listed frame windows) -- and each case first asserts, from the lists the pre-pass leaves in the
workspace, that both lists are non-empty and that some pixel is patched by two different listed windows.

Shapes: odd frame counts (the table path has no two-frame groups), D on both sides of the 64 and 128 block edges, D = 1,
more than one workgroup of items; the cap case lists more pattern windows than the table holds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BS, TAIL = 9, 4                      # block size; bs - 1 - bs // 2: windows x <= -TAIL are one fully clamped window
TAB_CAP = 4096                       # rows of the pattern-side table (kFixTabCap, csrc/ctd_ncc_fast.h)
SHAPES = [(1, 9, 64, 1), (3, 13, 64, 37), (2, 20, 128, 64), (3, 20, 128, 65), (2, 11, 256, 128), (1, 12, 256, 130)]


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_inputs(te, N, H, W, D, per_frame=False, constant_pattern=False):
    """(raw frames, their LCN, pattern): flat patch in every frame (it stays flat under the LCN), constant left part and
    constant band in the pattern, the band under the frames' patch."""
    rs = np.random.RandomState(1000 * N + 100 * H + W + D + (7 if per_frame else 0))
    raw = (rs.rand(N, 1, H, W) * 0.8 + 0.1).astype(np.float32)
    top = min(H, 13)
    raw[:, :, :top, W // 4:W // 4 + 32] = 0.5              # 32 columns: 10 of them keep a flat 9 x 9 window after LCN radius 5
    nb = N if per_frame else 1
    b = rs.randn(nb, 1, H, W).astype(np.float32)
    if constant_pattern:
        b[:] = 0.375
    else:
        b[:, :, :max(9, 2 * H // 3), :12] = 0.25           # constant left part: listed windows and listed runs
        b[:, :, :top, W // 4 + 8:W // 4 + 22] = -0.5       # constant band, under the frames' patch
    raw_d = dev(raw)
    x, _ = te.lcn(raw_d, 5, 0.05)
    p = dev(b) if per_frame else dev(b[0])
    return raw_d, x, p


def listing(x, p, D, raw=None):
    """The lists a fast call's first stage leaves in its workspace, decoded: (frame entries, pattern entries), each an int
    array [n, 3] of (image, row, column), and the call's volume.  The call is the plain volume call (pre-pass kernel), or,
    with `raw` (the frames before their LCN), the fused call, whose streaming LCN kernel lists the frame windows itself."""
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    N, _, H, W = x.shape
    per_frame = p.dim() == 4
    stride1, s = (H * W if per_frame else 0), torch.cuda.current_stream().cuda_stream
    vol = torch.empty((N, D, H, W), device="cuda")
    if raw is None:
        ws = torch.zeros(L.ctd_xcorrvol_workspace_bytes(N, 1, H, W, D, BS, 1), dtype=torch.uint8, device="cuda")
        st = L.ctd_xcorrvol_f32(x.data_ptr(), p.data_ptr(), stride1, vol.data_ptr(), N, 1, H, W, D, BS, 1, ws.data_ptr(),
                                ws.numel(), 0, s)
    else:
        ws = torch.zeros(L.ctd_xcorrvol_argmax_workspace_bytes(N, 1, H, W, D, BS, 1), dtype=torch.uint8, device="cuda")
        y, sd = torch.empty_like(raw), torch.empty_like(raw)
        idx = torch.empty((N, H, W), dtype=torch.int64, device="cuda")
        best = torch.empty((N, H, W), device="cuda")
        st = L.ctd_lcn_xcorrvol_argmax_f32(raw.data_ptr(), y.data_ptr(), sd.data_ptr(), 5, 0.05, 0, p.data_ptr(), stride1,
                                           vol.data_ptr(), idx.data_ptr(), best.data_ptr(), N, H, W, D, BS, 1, 1e-5,
                                           ws.data_ptr(), ws.numel(), 0, s)
    assert st == 0
    torch.cuda.synchronize()
    al = lambda v, a: (v + a - 1) // a * a
    xoff = (D + 15) // 16 * 16 + 32 + 3
    W1, Wp, img1 = al(W + 4 + xoff, 4), al(W + 8, 4), (N if per_frame else 1)
    off = 3 * al(N * H * Wp * 4, 256) + 3 * al(img1 * H * W1 * 4, 256)
    n_a, n_b, n_r, n_a_ranked = ws[off:off + 16].view(torch.int32).tolist()
    if raw is not None:
        n_a = n_a_ranked                       # a ranked call clears slot 0 at its end and keeps the count in slot 3
    off_a = off + 256
    off_b = off_a + al(N * H * W * 8, 256)

    def decode(o, n):
        e = ws[o:o + 8 * n].view(torch.int64).cpu().numpy()
        return np.stack([e >> 40, (e >> 20) & 0xFFFFF, (e & 0xFFFFF) - 0x80000], 1).astype(np.int64).reshape(n, 3)

    la, lb = decode(off_a, n_a), decode(off_b, n_b)
    assert int((lb[:, 2] == -TAIL).sum()) == n_r
    return la, lb, vol


def listed_mask(la, lb, N, H, W, D, per_frame):
    """mask [N, D, H, W] of the outputs listed windows take part in, and per pixel the number of distinct listed windows"""
    mask = np.zeros((N, D, H, W), bool)
    count = np.zeros((N, H, W), np.int64)
    for z, h, w in la:
        mask[z, :, h, w] = True
        count[z, h, w] += 1
    xs = np.maximum(np.arange(W)[None, :] - np.arange(D)[:, None], -TAIL)      # [D, W] window column of output (d, w)
    for z in sorted(set(lb[:, 0].tolist())):
        for h in sorted(set(lb[lb[:, 0] == z, 1].tolist())):
            cols = lb[(lb[:, 0] == z) & (lb[:, 1] == h), 2]
            hit = np.isin(xs, cols)                                              # [D, W]
            n_win = np.array([len(set(xs[hit[:, w], w].tolist())) for w in range(W)])
            for f in ([z] if per_frame else range(N)):
                mask[f, :, h, :] |= hit
                count[f, h, :] += n_win
    return mask, count


class Case:
    """inputs, lists and the reference-order results of one shape, computed once"""

    def __init__(self, te, N, H, W, D, per_frame=False, constant_pattern=False):
        self.N, self.H, self.W, self.D, self.per_frame = N, H, W, D, per_frame
        self.raw, self.x, self.p = make_inputs(te, N, H, W, D, per_frame, constant_pattern)
        self.la, self.lb, self.plain = listing(self.x, self.p, D)
        self.mask_np, self.count = listed_mask(self.la, self.lb, N, H, W, D, per_frame)
        self.mask = torch.from_numpy(self.mask_np).cuda()
        self.mask_fused = None
        self.vol_e = te.xcorrvol_batch(self.x, self.p, D, BS, algo="exact")
        self.idx_e, self.best_e = te.argmax_disp(self.vol_e)

    def use_fused_listing(self):
        """the fused call lists the frame windows in its streaming LCN kernel (f32 statistics): windows at the rim of a
        flat patch may fall on the other side of the listing threshold than in the pre-pass, so the volume of a fused
        call is held to ITS lists; shapes the fused kernel does not cover run the unfused calls and keep theirs"""
        from connecting_the_dots_amd import _lib
        if not _lib.lib().ctd_lcn_xcorrvol_supported(self.H, self.W, self.D, 5, BS):
            self.mask_fused = self.mask
            return
        la, lb, _ = listing(self.x, self.p, self.D, raw=self.raw)
        assert len(la) > 0 and sorted(map(tuple, lb)) == sorted(map(tuple, self.lb))
        mask, count = listed_mask(la, lb, self.N, self.H, self.W, self.D, self.per_frame)
        assert int(count.max()) >= 2
        print("listed frame windows: pre-pass %d, fused call %d" % (len(self.la), len(la)))
        self.mask_fused = torch.from_numpy(mask).cuda()

    def precondition(self):
        assert len(self.la) > 0 and len(self.lb) > 0, (len(self.la), len(self.lb))
        assert int(self.count.max()) >= 2, "no pixel is patched by two different listed windows"

    def check_volume(self, vol, what, fused=False):
        mask = self.mask_fused if fused else self.mask
        assert torch.equal(vol[mask], self.vol_e[mask]), "%s: listed volume entries differ from algo='exact'" % what
        err = (vol - self.vol_e).abs()
        assert bool((err <= 1e-5 * self.vol_e.abs() + 1e-6).all()), "%s: %g" % (what, float(err.max()))

    def check_ranked(self, out, what, volume, fused=False):
        idx, best = out[0], out[1]
        bad = int((idx != self.idx_e).sum())
        assert bad == 0, "%s: %d of %d indices differ from the reference-order argmax" % (what, bad, idx.numel())
        tol = self.vol_e.abs().amax(-3) * 1e-5 + 2e-6                 # fast score + key resolution, as tests/test_rank_gpu.py
        assert bool(((best - self.best_e).abs() <= tol).all()), what
        if volume:
            self.check_volume(out[2], what, fused)


@pytest.mark.parametrize("N,H,W,D", SHAPES)
def test_call_kinds_against_exact(te, N, H, W, D):
    """prepared / unprepared x fused / unfused x with / without a volume, and the unranked call"""
    c = Case(te, N, H, W, D)
    c.precondition()
    c.use_fused_listing()
    c.check_volume(c.plain, "plain unprepared")
    h = te.prepare_pattern(c.p, N, D, BS)
    results = {}
    for prepared in (None, h):
        tag = "prepared" if prepared is not None else "unprepared"
        for rv in (True, False):
            out = te.xcorrvol_argmax(c.x, c.p, D, BS, return_volume=rv, algo="fast", prepared=prepared)
            c.check_ranked(out, "%s unfused volume=%s" % (tag, rv), rv)
            results[(tag, "unfused", rv)] = out
            out = te.lcn_xcorrvol_argmax(c.raw, c.p, D, BS, 5, 0.05, return_volume=rv, lcn_algo="exact", prepared=prepared)
            assert torch.equal(out[0], c.x), "fused LCN differs from lcn(algo='exact')"
            c.check_ranked(out[2:], "%s fused volume=%s" % (tag, rv), rv, fused=True)
            results[(tag, "fused", rv)] = out[2:]
    # the table path gives the table-less kernel's bits: index, best score, volume
    for kind in ("unfused", "fused"):
        for rv in (True, False):
            a, b = results[("prepared", kind, rv)], results[("unprepared", kind, rv)]
            assert all(torch.equal(u, v) for u, v in zip(a, b)), (kind, rv)
    # unranked call on the prepared pattern: the same volume as unprepared
    assert torch.equal(te.xcorrvol_batch(c.x, c.p, D, BS, algo="fast", prepared=h), c.plain)


@pytest.mark.parametrize("N,H,W,D", SHAPES)
def test_per_frame_pattern(te, N, H, W, D):
    """in1 as [N,1,H,W]: one item per (listed window of frame f's pattern, block of 64 disparities)"""
    c = Case(te, N, H, W, D, per_frame=True)
    c.precondition()
    c.check_volume(c.plain, "plain unprepared")
    h = te.prepare_pattern(c.p, N, D, BS)
    want = te.xcorrvol_argmax(c.x, c.p, D, BS, return_volume=True, algo="fast")
    c.check_ranked(want, "unprepared", True)
    got = te.xcorrvol_argmax(c.x, c.p, D, BS, return_volume=True, algo="fast", prepared=h)
    c.check_ranked(got, "prepared", True)
    assert all(torch.equal(u, v) for u, v in zip(got, want))
    got_n = te.xcorrvol_argmax(c.x, c.p, D, BS, algo="fast", prepared=h)
    c.check_ranked(got_n, "prepared, no volume", False)
    assert torch.equal(te.xcorrvol_batch(c.x, c.p, D, BS, algo="fast", prepared=h), c.plain)


def test_tables_persist_between_calls(te):
    """two consecutive calls on one prepared handle, different frames: the second equals a fresh unprepared call bit for
    bit -- the tables and lists were not clobbered and the frame-window counter returned to zero"""
    N, H, W, D = 3, 20, 128, 65
    c = Case(te, N, H, W, D)
    c.precondition()
    h = te.prepare_pattern(c.p, N, D, BS)
    first = te.xcorrvol_argmax(c.x, c.p, D, BS, return_volume=True, algo="fast", prepared=h)
    c.check_ranked(first, "first call", True)
    x2 = c.x.flip(0).flip(2).contiguous()                                # other frames: the flat patch is at the bottom now
    got = te.xcorrvol_argmax(x2, c.p, D, BS, return_volume=True, algo="fast", prepared=h)
    want = te.xcorrvol_argmax(x2, c.p, D, BS, return_volume=True, algo="fast")
    assert all(torch.equal(u, v) for u, v in zip(got, want))
    vol_e = te.xcorrvol_batch(x2, c.p, D, BS, algo="exact")
    assert torch.equal(got[0], te.argmax_disp(vol_e)[0])
    got_n = te.xcorrvol_argmax(x2, c.p, D, BS, algo="fast", prepared=h)
    assert torch.equal(got_n[0], want[0])


def test_more_listed_windows_than_table_rows(te):
    """an all-constant pattern lists every window, H x (W + 4) of them: the smallest such count above the table's cap at a
    width the all-D kernel takes (and, the table living behind the list's entries, far more than it has rows for here).
    Windows without a table row go through the in-kernel staging of the same launch."""
    N, H, W, D = 2, 32, 128, 64
    c = Case(te, N, H, W, D, constant_pattern=True)
    c.precondition()
    assert TAB_CAP < len(c.lb) <= H * (W + TAIL), len(c.lb)
    c.check_volume(c.plain, "plain unprepared")
    h = te.prepare_pattern(c.p, N, D, BS)
    for rv in (True, False):
        got = te.xcorrvol_argmax(c.x, c.p, D, BS, return_volume=rv, algo="fast", prepared=h)
        c.check_ranked(got, "prepared volume=%s" % rv, rv)
        want = te.xcorrvol_argmax(c.x, c.p, D, BS, return_volume=rv, algo="fast")
        assert all(torch.equal(u, v) for u, v in zip(got, want)), rv
    assert torch.equal(te.xcorrvol_batch(c.x, c.p, D, BS, algo="fast", prepared=h), c.plain)
