"""The CPU helpers of the LCN exactness tests (tests/lcn_traps.py): the exactness rule, and the emulation of the two
summation orders that tells how many trap motifs a band layout arms -- so that the GPU trap test cannot test nothing."""
import numpy as np
import pytest

from tests import lcn_traps as T


def test_lowest_bit():
    v = np.array([1.0, 0.75, 2.0 ** -40 * 1.5, 3 * 2.0 ** 20, 0.0, -0.5, 1 + 2.0 ** -23], np.float32)
    assert list(T.lowest_bit(v)) == [0, -2, -41, 20, np.inf, -1, -23]


def test_exact_windows_rule():
    x = np.zeros((1, 1, 30, 30), np.float32)
    x[0, 0, 10, 10] = 2.0 ** 20
    x[0, 0, 12, 12] = 2.0 ** -40                              # span 61 bits: not exact together
    x[0, 0, 25, 25] = 1 + 2.0 ** -23
    ex = T.exact_windows(x, 5)
    assert not ex[0, 0, 11, 11] and ex[0, 0, 25, 25] and ex[0, 0, 0, 29]
    x[0, 0, 12, 12] = 2.0 ** -10                              # x: 31 bits, x*x: 60 bits
    ex = T.exact_windows(x, 5)
    assert not ex[0, 0, 11, 11]
    x[0, 0, 12, 12] = 2.0 ** -1                               # x*x: 42 bits
    assert T.exact_windows(x, 5)[0, 0, 11, 11]


def test_emulated_oracle_order_is_the_oracles(oracle):
    """the numpy oracle order + f32 tail carries oracle.lcn's bits (trap frames, hdr frames), and so does the streaming
    order with fresh sums"""
    for x in (T.trap_frames(2, 120, 150)[0], T.hdr_frames(2, 40, 60)):
        y0, s0 = oracle.lcn(x, 5, 0.05)
        y, s = T.f32_tail(x, *T.oracle_sums(x, 5), 5, 0.05)
        assert np.array_equal(y, y0) and np.array_equal(s, s0)
        y, s = T.f32_tail(x, *T.stream_sums(x, 256, sliding=False), 5, 0.05)
        assert np.array_equal(y, y0) and np.array_equal(s, s0)


# (N, H, W) of tests/test_lcn_f64_gpu.py's trap test, and CU counts of a few devices (MI355X: 256)
@pytest.mark.parametrize("N,H,W", [(2, 432, 512), (1, 200, 464), (3, 97, 236)])
@pytest.mark.parametrize("n_cu", [256, 304, 80, 1])
def test_traps_are_armed(N, H, W, n_cu, capsys):
    """a sliding sum misrounds at least 30 % of the tie windows whatever the band layout (MIN_ARMED of the GPU test),
    and every pixel where it differs from the oracle has exact f64 sums"""
    x, motifs = T.trap_frames(N, H, W, seed=H + W)
    armed = T.armed(x, motifs, n_cu)
    y0, s0 = T.f32_tail(x, *T.oracle_sums(x, 5), 5, 0.05)
    y, s = T.f32_tail(x, *T.stream_sums(x, n_cu), 5, 0.05)
    diff = (y != y0) | (s != s0)
    with capsys.disabled():
        print("\n%s, %d CUs (band rows, bands) %s: %d of %d traps armed, %d pixels differ" % (
            (N, H, W), n_cu, T.stream_layout(N, H, W, n_cu), len(armed), len(motifs), int(diff.sum())))
    assert len(armed) >= 0.3 * len(motifs)
    assert not (diff & ~T.exact_windows(x, 5)).any()
