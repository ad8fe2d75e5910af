"""Phase timeline of the two post kernels of the ranked call (fix-up, tail) from a -DCTD_STAMPS build
(csrc/ctd_post_stamps.h), at the bench shape, each kernel behind the all-D kernel of the same call:
    tools/build_variant.sh stamps_fix connecting_the_dots_amd/csrc/ncc_fixup.hip -DCTD_STAMPS
    tools/build_variant.sh stamps_fix_before connecting_the_dots_amd/csrc/ncc_fixup.hip -DCTD_STAMPS -DCTD_FIXUP_NO_TABLE
    tools/build_variant.sh stamps_tail connecting_the_dots_amd/csrc/argmax_rerank.hip -DCTD_STAMPS
    python tools/post_timeline.py tools/variants/libctd_stamps_fix.so fixup
    python tools/post_timeline.py tools/variants/libctd_stamps_tail.so tail
Every wavefront stamps the shader clock at the phase boundaries of its first item.  Printed, over the item-carrying
wavefronts: median and p90 of each phase (cycles and us), of the whole first item and of the wavefront's start after the
kernel's first wavefront; and how many item-carrying workgroups started after the first item-carrying wavefront had
finished its item (workgroups that were not resident in the first round)."""
import ctypes, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import workloads
from connecting_the_dots_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
from connecting_the_dots_amd import torchext as te
which = sys.argv[2] if len(sys.argv) > 2 else "fixup"
raw = ctypes.CDLL(_lib.LIB_PATH)
H, W, N, D = 432, 512, 16, 128
fr = torch.from_numpy(np.stack([workloads.uniform_frame(1234 + i, H, W) for i in range(N)])).cuda()
pat = torch.from_numpy(workloads.syn_dot_pattern(H, W, seed=42)[None, None]).cuda()
x, _ = te.lcn(fr, 5, 0.05)
p = te.lcn(pat, 5, 0.05)[0][0].contiguous()
prepared = te.prepare_pattern(p, N, D, 9)                  # as the bench step: the pattern half of the pre-pass once
for _ in range(int(os.environ.get("CTD_WARM_CALLS", "300"))):         # sustained clocks first; the last call is the one read
    te.xcorrvol_argmax(x, p, D, 9, return_volume=True, algo="fast", prepared=prepared)
torch.cuda.synchronize()

WORDS, WAVES = 16, 16384
buf = np.zeros(WAVES * WORDS, dtype=np.uint32)
fn = getattr(raw, "ctd_debug_read_%s_stamps" % which)
fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
assert fn(buf.ctypes.data, buf.nbytes) == 0
st = buf.reshape(WAVES, WORDS).astype(np.int64)
st = st[st[:, 15] == 1]
PHASES = {
    "fixup": ["entry -> counters read", "-> list entry read", "-> pattern side ready", "-> span staged", "-> means done",
              "-> chains done", "-> best / idx compared", "-> stores issued", "-> exit of the first item"],
    "tail": ["entry -> counters read", "-> list entry read", "-> column read", "-> rows staged", "-> re-scored", "-> written"],
}
ROLES = {"fixup": {0: "fix-up"}, "tail": {0: "resolve", 1: "runs", 2: "decode"}}
diff = lambda a, b: (a - b) & 0xffffffff
print("kernel: %s   wavefronts with a row: %d   workgroups: %d" % (which, len(st), (len(st) + 3) // 4))
t0_real = st[:, 10].min()
for role, name in ROLES[which].items():
    r = st[st[:, 12] == role]
    it = r[r[:, 14] == 1]
    print("== role %s: %d wavefronts, %d carried an item" % (name, len(r), len(it)))
    if len(it) == 0:
        continue
    life_clk, life_real = diff(it[:, 9], it[:, 0]), diff(it[:, 11], it[:, 10])
    mhz = np.median(life_clk[life_real > 50] / life_real[life_real > 50]) * 100.0 if (life_real > 50).any() else float("nan")
    print("   shader clock by the 100 MHz counter: %.0f MHz" % mhz)
    us = lambda c: c / mhz
    prev = 0
    for k, label in enumerate(PHASES[which], start=1):
        if which == "tail" and role != 0 and k in (3, 4, 5):
            continue
        d = diff(it[:, k], it[:, prev])
        d = d[(it[:, k] != 0) & (d < 1 << 30)]
        prev = k
        if len(d):
            print("   %-28s median %7.0f cycles %6.2f us   p90 %7.0f cycles %6.2f us" % (
                label, np.median(d), us(np.median(d)), np.percentile(d, 90), us(np.percentile(d, 90))))
    print("   %-28s median %7.0f cycles %6.2f us   p90 %7.0f cycles %6.2f us   max %6.2f us" % (
        "first item, entry -> exit", np.median(life_clk), us(np.median(life_clk)), np.percentile(life_clk, 90),
        us(np.percentile(life_clk, 90)), us(life_clk.max())))
    start = diff(it[:, 10], t0_real) / 100.0
    print("   start after the kernel's first wavefront: median %.2f us, p90 %.2f, max %.2f" % (
        np.median(start), np.percentile(start, 90), start.max()))
    first_done = diff(it[:, 11], t0_real).min()
    late = diff(it[:, 10], t0_real) > first_done
    print("   item-carrying wavefronts that started after the first finished item (not resident in the first round): "
          "%d of %d (about %d workgroups)" % (late.sum(), len(it), (late.sum() + 3) // 4))
    end = diff(it[:, 11], t0_real) / 100.0
    print("   last stamp of the role after the kernel's first wavefront: %.2f us" % end.max())
