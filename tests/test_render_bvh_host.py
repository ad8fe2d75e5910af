"""CPU-only checks of the BVH ray caster's C ABI: exports, byte-size queries, and argument validation that returns
CTD_ERR_INVALID_ARG / CTD_ERR_WORKSPACE before any HIP call (so without a GPU)."""
import ctypes

import pytest

from connecting_the_dots_amd import _lib

INVALID, WORKSPACE = 1, 2
FAKE = 1 << 20                       # an aligned, never dereferenced "device pointer"


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def test_exports_and_sizes(lib):
    for name in ("ctd_mesh_bvh_bytes", "ctd_mesh_bvh_workspace_bytes", "ctd_mesh_bvh_build_f32",
                 "ctd_render_mesh_proj_bvh_f32", "ctd_render_mesh_bvh_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ctd_mesh_bvh_bytes(-1) == 0 and lib.ctd_mesh_bvh_workspace_bytes(-1) == 0
    assert lib.ctd_mesh_bvh_bytes((1 << 28) + 1) == 0
    assert lib.ctd_mesh_bvh_bytes(0) == 64
    prev = 0
    for n in (1, 2, 5, 257, 4096, 4097, 10 ** 6, 1 << 28):
        b, w = lib.ctd_mesh_bvh_bytes(n), lib.ctd_mesh_bvh_workspace_bytes(n)
        assert b % 16 == 0 and b >= 64 + (2 * n - 1) * 48 + n * 48 and b > prev
        assert w >= n * 24                                   # two key and two value buffers at least
        prev = b


def build(lib, verts=FAKE, n_verts=3, faces=FAKE, n_faces=1, bvh=FAKE, bvh_bytes=None, ws=FAKE, ws_bytes=None):
    bvh_bytes = lib.ctd_mesh_bvh_bytes(max(n_faces, 0)) if bvh_bytes is None else bvh_bytes
    ws_bytes = lib.ctd_mesh_bvh_workspace_bytes(max(n_faces, 0)) if ws_bytes is None else ws_bytes
    return lib.ctd_mesh_bvh_build_f32(verts, n_verts, faces, n_faces, bvh, bvh_bytes, ws, ws_bytes, None, 0, None)


def test_build_validation(lib):
    assert build(lib, n_faces=-1) == INVALID
    assert build(lib, n_verts=-1) == INVALID
    assert build(lib, bvh=None) == INVALID
    assert build(lib, verts=None) == INVALID
    assert build(lib, faces=None) == INVALID
    assert build(lib, ws=None) == INVALID
    assert build(lib, bvh=FAKE + 4) == INVALID                  # 16-byte alignment
    assert build(lib, bvh_bytes=lib.ctd_mesh_bvh_bytes(1) - 1) == INVALID
    assert build(lib, ws_bytes=lib.ctd_mesh_bvh_workspace_bytes(1) - 1) == WORKSPACE
    assert build(lib, n_faces=(1 << 28) + 1, bvh_bytes=1 << 62, ws_bytes=1 << 62) == INVALID


def test_render_validation(lib):
    cam = (ctypes.c_float * 16)()
    sh = (ctypes.c_float * 4)()
    cp, sp = ctypes.addressof(cam), ctypes.addressof(sh)

    def proj(**kw):
        a = dict(bvh=FAKE, verts=FAKE, colors=FAKE, nv=3, faces=FAKE, nf=1, cam=cp, W=8, H=8, proj=cp, PW=8, PH=8,
                 shader=sp, pattern=FAKE, depth=FAKE, color=FAKE, normal=FAKE)
        a.update(kw)
        return lib.ctd_render_mesh_proj_bvh_f32(a["bvh"], a["verts"], a["colors"], a["nv"], a["faces"], a["nf"], a["cam"],
                                                a["W"], a["H"], a["proj"], a["PW"], a["PH"], a["shader"], a["pattern"],
                                                0.0, 0.35, a["depth"], a["color"], a["normal"], 0, None)

    for kw in (dict(bvh=None), dict(bvh=FAKE + 8), dict(nf=-1), dict(W=0), dict(PH=0), dict(cam=None), dict(proj=None),
               dict(shader=None), dict(pattern=None), dict(color=None), dict(verts=None), dict(faces=None),
               dict(colors=None), dict(W=40000, H=40000)):
        assert proj(**kw) == INVALID, kw

    def mesh(**kw):
        a = dict(bvh=FAKE, verts=FAKE, colors=FAKE, normals=FAKE, nv=3, faces=FAKE, nf=1, cam=cp, W=8, H=8, shader=sp,
                 depth=FAKE, color=FAKE, normal=FAKE)
        a.update(kw)
        return lib.ctd_render_mesh_bvh_f32(a["bvh"], a["verts"], a["colors"], a["normals"], a["nv"], a["faces"], a["nf"],
                                           a["cam"], a["W"], a["H"], a["shader"], a["depth"], a["color"], a["normal"], 0,
                                           None)

    for kw in (dict(bvh=None), dict(nf=-1), dict(H=-1), dict(cam=None), dict(shader=None), dict(verts=None),
               dict(normals=None), dict(colors=None)):
        assert mesh(**kw) == INVALID, kw
