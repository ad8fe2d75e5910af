"""CPU helpers of the LCN exactness tests (a plain module, not a conftest): the exactness rule of f64 box sums, the trap
frames that catch a sliding sum keeping a rounding error past its window, and a numpy emulation of the two summation
orders (the oracle's fresh sums and the streaming kernel's per-column sliding sums, lcn_stream.hip before its sums were
made fresh).

Exactness rule.  A sum of f32 values in f64 is exact in ANY order when, with hi = ceil(log2 sum |v|) (which bounds every
partial sum, whatever the order) and lo = the lowest set bit over the nonzero values, hi - lo <= 53: every partial sum is
then an integer multiple of 2^lo below 2^hi.  Here hi is taken as floor(log2 sum |v|) + 1, the same except at exact
powers of two, where it is one more (conservative).  The rule is applied separately to the x sum and to the sum of the
f32 squares x*x (data**2 is an f32 tensor, networks.py:528).  Where it holds for both sums of a window, every summation
order gives the same f64 box sums, so every LCN kernel that forms them in f64 and applies the reference's f32 tail
carries the oracle's bits there.

Trap motif (one column, rows from p): ten rows of 100, t = 2^-40 (1 + m), 1, 2^-24, then zeros.  The window of the 1,
the 2^-24 and nine zeros sums to 1 + 2^-24 exactly, an f32 tie that rounds to 1.  A sliding sum V = (V + new) - old
that took t in while the 100s were in the column keeps about 2e-14 of t's rounding after t has left, and rounds the tie
to 1 + 2^-23.  Whether a motif is armed depends on where the band of rows that the streaming kernel slides over starts
(it starts with a fresh sum), so motifs are laid out at many row offsets and columns."""
import numpy as np
import torch
import torch.nn.functional as F

MOTIF_ROWS = 22          # 100 x 10, t, 1, 2^-24, nine zeros: the tie window is rows p + 11 .. p + 21
MOTIF_COL_STEP = 12      # columns of two motifs: no 11-column window holds both
TIE_ROW = 16             # centre row of the tie window, from the motif's first row

# streaming kernel geometry (lcn_stream.hip)
LS_VALID, LS_MAX_BAND, LS_R = 232, 64, 5


def _reflect_pad(t, r):
    return F.pad(t, (r, r, r, r), mode="reflect")


def lowest_bit(v):
    """exponent of the lowest set bit of each nonzero f32 value (v = M 2^(E - 24), M an integer); +inf at zeros"""
    v = np.asarray(v, np.float32).astype(np.float64)
    f, e = np.frexp(np.abs(v))
    m = np.round(f * 2.0 ** 24).astype(np.int64)
    low = np.log2((m & -m).astype(np.float64), where=m > 0, out=np.zeros_like(f))
    return np.where(v != 0, e - 24 + low, np.inf)


def _window_exact(v, radius):
    t = torch.from_numpy(np.ascontiguousarray(v, np.float32).astype(np.float64))
    k = torch.ones(1, 1, 2 * radius + 1, 2 * radius + 1, dtype=torch.float64)
    s = F.conv2d(_reflect_pad(t.abs(), radius), k).numpy()
    lo = torch.from_numpy(np.where(np.isinf(lowest_bit(v)), 1e9, lowest_bit(v)))
    lo = -F.max_pool2d(_reflect_pad(-lo, radius), 2 * radius + 1, stride=1).numpy()
    hi = np.floor(np.log2(np.where(s > 0, s, 1.0))) + 1
    return (s == 0) | (hi - lo <= 53)


def exact_windows(x, radius):
    """bool [N,1,H,W]: True where both f64 box sums of the (2r+1)^2 reflect-padded window (of x and of the f32 x*x) are
    exact in any summation order (the rule in the module docstring)"""
    x = np.asarray(x, np.float32)
    return _window_exact(x, radius) & _window_exact(x * x, radius)


def trap_frames(N, H, W, seed=0):
    """[N,1,H,W] f32 zero frames with trap motifs: columns MOTIF_COL_STEP apart and at least 12 from either border, in
    every column a run of motifs MOTIF_ROWS apart from a row offset that changes with the column and the frame (so that
    motifs meet every position relative to a band start), a different t = 2^-40 (1 + m) for every motif.  Returns
    (x, motifs) with motifs a list of (frame, first row, column)."""
    rs = np.random.RandomState(seed)
    x = np.zeros((N, 1, H, W), np.float32)
    motifs = []
    for f in range(N):
        for j, c in enumerate(range(12, W - 12, MOTIF_COL_STEP)):
            p = 6 + (7 * j + 5 * f) % MOTIF_ROWS
            while p + MOTIF_ROWS <= H - 6:
                x[f, 0, p:p + 10, c] = 100.0
                x[f, 0, p + 10, c] = np.float32(2.0 ** -40 * (1 + rs.rand()))
                x[f, 0, p + 11, c] = 1.0
                x[f, 0, p + 12, c] = np.float32(2.0 ** -24)
                motifs.append((f, p, c))
                p += MOTIF_ROWS
    return x, motifs


def oracle_sums(x, radius):
    """the oracle's order (ctd_oracle_lcn_f32, lcn_kernel): per row the 2r+1 reflected columns in ascending order from
    0, then per output the 2r+1 reflected row sums in ascending order from 0, all in f64.  (S1, S2) [N,1,H,W] f64 of x
    and of the f32 x*x."""
    x = np.asarray(x, np.float32)
    N, _, H, W = x.shape
    out = []
    for v in (x.astype(np.float64), (x * x).astype(np.float64)):
        p = np.pad(v, ((0, 0), (0, 0), (0, 0), (radius, radius)), mode="reflect")
        r = np.zeros_like(v)
        for d in range(2 * radius + 1):
            r = r + p[..., d:d + W]
        p = np.pad(r, ((0, 0), (0, 0), (radius, radius), (0, 0)), mode="reflect")
        s = np.zeros_like(v)
        for d in range(2 * radius + 1):
            s = s + p[:, :, d:d + H]
        out.append(s)
    return tuple(out)


def stream_layout(N, H, W, n_cu):
    """(band_rows, n_bands) of lcn_stream_f32 for this shape on a device with n_cu compute units"""
    n_strips = -(-W // LS_VALID)
    n_bands = (4 * n_cu) // (N * n_strips)
    n_bands = min(n_bands, H // 8)
    n_bands = max(n_bands, 1, -(-H // LS_MAX_BAND))
    band_rows = -(-H // n_bands)
    return band_rows, -(-H // band_rows)


def stream_sums(x, n_cu, sliding=True):
    """the streaming kernel's order at radius 5 (lcn_prepass_stream_kernel<double> before its sums were made fresh): per
    band and column an 11-row f64 sum, the first one accumulated from 0, every next one V = (V + new) - old; then the 11
    column sums of a window added in ascending order.  (The kernel adds the 11 column sums as a tree; on trap frames
    every other column of a tie window sums to exactly 0, so the order there does not matter.)  sliding=False: a fresh
    ascending 11-row sum per row instead.  Returns (S1, S2) as oracle_sums."""
    x = np.asarray(x, np.float32)
    N, _, H, W = x.shape
    R, NR = LS_R, 2 * LS_R + 1
    band_rows, n_bands = stream_layout(N, H, W, n_cu)
    vs = (x.astype(np.float64)[:, 0], (x * x).astype(np.float64)[:, 0])
    cols = [np.zeros((N, H, W)), np.zeros((N, H, W))]

    def refl(i):
        return -i if i < 0 else (2 * (H - 1) - i if i > H - 1 else i)

    for b in range(n_bands):
        h_lo, h_hi = b * band_rows, min(b * band_rows + band_rows, H)
        ry_first, ry_last = max(h_lo - 4, 0), min(h_hi - 1 + 4, H - 1)
        u0, n_raw = ry_first - R, ry_last - ry_first + NR
        feed = [refl(u0 + k) for k in range(n_raw)]
        for v, c in zip(vs, cols):
            V = np.zeros((N, W))
            for k in range(NR):
                V = V + v[:, feed[k]]
            for k in range(NR - 1, n_raw):
                cur = ry_first + k - (NR - 1)
                if not sliding:
                    V = np.zeros((N, W))
                    for j in range(k - NR + 1, k + 1):
                        V = V + v[:, feed[j]]
                if h_lo <= cur < h_hi:
                    c[:, cur] = V
                if sliding and k + 1 < n_raw:
                    V = (V + v[:, feed[k + 1]]) - v[:, feed[k + 1 - NR]]
    out = []
    for c in cols:
        p = np.pad(c, ((0, 0), (0, 0), (R, R)), mode="reflect")
        s = np.zeros_like(c)
        for d in range(NR):
            s = s + p[..., d:d + W]
        out.append(s[:, None])
    return tuple(out)


def f32_tail(x, S1, S2, radius, eps):
    """the reference's f32 elementwise tail on f64 box sums rounded once (networks.py:529-532, oracle order):
    (y, std) f32"""
    x = np.asarray(x, np.float32)
    cnt = np.float32((2 * radius + 1) ** 2)
    boxs, boxs2 = S1.astype(np.float32), S2.astype(np.float32)
    avgs = boxs / cnt
    var = boxs2 / cnt - avgs * avgs + np.float32(1e-6)
    sd = np.sqrt(var) + np.float32(eps)
    return (x - avgs) / sd, sd


def armed(x, motifs, n_cu):
    """the motifs whose tie pixel gets another f32 box sum from the sliding order than from the oracle's"""
    o1 = oracle_sums(x, LS_R)[0].astype(np.float32)
    s1 = stream_sums(x, n_cu)[0].astype(np.float32)
    return [m for m in motifs if o1[m[0], 0, m[1] + TIE_ROW, m[2]] != s1[m[0], 0, m[1] + TIE_ROW, m[2]]]


def hdr_block_frames(N, H, W, seed=0, block=16):
    """high dynamic range in blocks: every block x block square has its own scale 2^-e (e = 0 .. 30) and values
    scale (0.5 + 0.5 u); the windows inside a block are exact (32 bits for x and for x*x), those that straddle blocks
    of scales more than 2^10 apart are not"""
    rs = np.random.RandomState(seed)
    e = rs.randint(0, 31, size=(N, 1, -(-H // block), -(-W // block)))
    scale = np.repeat(np.repeat(2.0 ** -e, block, 2), block, 3)[:, :, :H, :W]
    return (scale * (0.5 + 0.5 * rs.rand(N, 1, H, W))).astype(np.float32)


def hdr_frames(N, H, W, seed=0):
    """high dynamic range: O(1) values mixed with values of 2^-30 .. 2^-12 (a quarter of the samples)"""
    rs = np.random.RandomState(seed)
    x = rs.rand(N, 1, H, W)
    small = rs.rand(N, 1, H, W) < 0.25
    x[small] = 2.0 ** rs.uniform(-30, -12, size=int(small.sum()))
    return x.astype(np.float32)
