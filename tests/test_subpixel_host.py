"""CPU-only checks of the sub-pixel refinement (ctd_xcorrvol_subpixel_f32, ctd_costvol_subpixel_f32): the exports, the
workspace query, argument validation before any HIP call and the Python surface."""
import ctypes
import inspect

NAMES = ("ctd_xcorrvol_subpixel_workspace_bytes", "ctd_xcorrvol_subpixel_f32", "ctd_costvol_subpixel_f32")


def test_symbols_are_exported_and_bound():
    from connecting_the_dots_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n
    assert _lib.lib().ctd_version() == 5


def test_workspace_query():
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    shared = L.ctd_xcorrvol_subpixel_workspace_bytes(16, 432, 512, 128, 9, 0)
    per_frame = L.ctd_xcorrvol_subpixel_workspace_bytes(16, 432, 512, 128, 9, 1)
    assert 0 < shared < per_frame
    # the frame quotients, one pattern's quotients and its (mean, sum of squares) plane over W + D - 1 centres
    assert shared >= 4 * 16 * 432 * 512 + 4 * 432 * 512 + 8 * 432 * (512 + 127)
    assert shared % 256 == 0
    assert L.ctd_xcorrvol_subpixel_workspace_bytes(1, 432, 512, 129, 9, 0) > \
        L.ctd_xcorrvol_subpixel_workspace_bytes(1, 432, 512, 128, 9, 0)
    assert L.ctd_xcorrvol_subpixel_workspace_bytes(0, 432, 512, 128, 9, 0) == 0
    assert L.ctd_xcorrvol_subpixel_workspace_bytes(1, 0, 512, 128, 9, 0) == 0
    assert L.ctd_xcorrvol_subpixel_workspace_bytes(1, 432, 512, 0, 9, 0) == 0
    assert L.ctd_xcorrvol_subpixel_workspace_bytes(1, 432, 512, 128, 8, 0) == 0
    assert L.ctd_xcorrvol_subpixel_workspace_bytes(1, 432, 512, 128, -1, 0) == 0


class _Buf:
    """a host buffer standing in for device pointers: validation must reject before it is ever dereferenced"""

    def __init__(self, n):
        self.raw = ctypes.create_string_buffer(n + 512)
        a = ctypes.addressof(self.raw)
        self.ptr = (a + 255) // 256 * 256


def test_ncc_validation_needs_no_gpu():
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    H, W, D = 8, 8, 4
    nws = L.ctd_xcorrvol_subpixel_workspace_bytes(1, H, W, D, 3, 0)
    ws = _Buf(nws)
    p = ws.ptr                                      # any non-NULL pointer

    def call(bs=3, mode=0, stride=0, D=D, ptrs=(p, p, p, p), wsp=ws.ptr, nbytes=nws, frames=1):
        return L.ctd_xcorrvol_subpixel_f32(ptrs[0], ptrs[1], stride, ptrs[2], ptrs[3], None, frames, H, W, D, bs, mode,
                                           wsp, nbytes, -1, None)

    assert call(bs=8) == 1                          # even block size
    assert call(bs=0) == 1
    assert call(bs=-3) == 1
    assert call(mode=2) == 1                        # mode outside {0, 1}
    assert call(mode=-1) == 1
    assert call(mode=2 | 0x100) == 1
    assert call(stride=7) == 1                      # stride neither 0 nor H * W
    assert call(stride=-1) == 1
    assert call(D=0) == 1
    assert call(frames=-1) == 1
    for k in range(4):                              # NULL in0 / in1 / idx / disp
        ptrs = [p] * 4
        ptrs[k] = None
        assert call(ptrs=tuple(ptrs)) == 1
    assert call(wsp=None) == 1                      # workspace missing, too small, misaligned
    assert call(nbytes=nws - 1) == 1
    assert call(wsp=ws.ptr + 4) == 1
    assert call(nbytes=0) == 1
    # no frames: nothing to do, nothing touched
    assert call(frames=0, ptrs=(None,) * 4, wsp=None, nbytes=0) == 0


def test_cost_validation_needs_no_gpu():
    from connecting_the_dots_amd import _lib
    L = _lib.lib()
    p = _Buf(64).ptr

    def call(bs=3, ty=3, mode=1, stride=0, D=4, ptrs=(p, p, p, p), frames=1):
        return L.ctd_costvol_subpixel_f32(ptrs[0], ptrs[1], stride, ptrs[2], ptrs[3], None, frames, 8, 8, D, bs, ty, 0.5,
                                          mode, -1, None)

    assert call(bs=8) == 1
    assert call(bs=0) == 1
    assert call(ty=4) == 1
    assert call(ty=-1) == 1
    assert call(mode=2) == 1
    assert call(mode=0x100) == 1                    # the prepared flag belongs to the NCC call only
    assert call(stride=63) == 1
    assert call(D=0) == 1
    for k in range(4):
        ptrs = [p] * 4
        ptrs[k] = None
        assert call(ptrs=tuple(ptrs)) == 1
    assert call(frames=0, ptrs=(None,) * 4) == 0


def test_python_surface():
    from connecting_the_dots_amd import torchext as te
    sig = inspect.signature(te.xcorrvol_subpixel)
    assert list(sig.parameters)[:6] == ["in0", "in1", "idx", "n_disps", "block_size", "mode"]
    assert sig.parameters["mode"].default == "parabola"
    sig = inspect.signature(te.costvol_subpixel)
    assert list(sig.parameters) == ["im", "pattern", "idx", "n_disps", "block_size", "type", "eps", "mode"]
    assert sig.parameters["mode"].default == "equiangular"
    for fn in (te.xcorrvol_argmax, te.lcn_xcorrvol_argmax, te.costvol_argmin):
        assert inspect.signature(fn).parameters["subpixel"].default is None
    for fn in (te.xcorrvol_subpixel, te.costvol_subpixel):
        assert "0.5 * ((sm - sp) / den)" in fn.__doc__ and "0.5 * ((cm - cp) / (cp - c0))" in fn.__doc__
    assert "census" in te.costvol_subpixel.__doc__
