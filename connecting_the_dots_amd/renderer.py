"""Mirror of the reference's `renderer` package (renderer/cyrender.pyx:80-200) on top of libctd_hip.so.

Same class names and call signatures as the Cython module the data generator uses
(data/create_syn_data.py:152-160):

    cam = PyCamera(fx, fy, px, py, R, t, width, height)
    data = PyRenderInput(verts=..., colors=..., normals=..., faces=...)
    r = PyRenderer(cam, PyShader(0.5, 1.5, 0.0, 10), engine='gpu')
    r.mesh_proj(data, proj, pattern, d_alpha=0, d_beta=0.35)
    im, depth, ambient = r.color(), r.depth(), r.normal()

numpy in, numpy out like the reference; `render_mesh_proj` / `render_mesh` below are the tensor-level calls that keep
everything on the device.  Both renderers of the reference are provided (`mesh_proj`, the one the data pipeline
uses, and the plain `mesh`); there is no CPU engine in this package (engine='cpu' raises: the CPU path lives on as
the test oracle).
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._meshargs import CTD_ERR_UNSUPPORTED, _cuda_tensors


def _cam_params(fx, fy, px, py, R, t):
    R = np.asarray(R, np.float32)
    t = np.asarray(t, np.float32)
    if R.shape != (3, 3):
        raise Exception('invalid R matrix')                      # cyrender.pyx:85
    if t.shape != (3,):
        raise Exception('invalid t vector')
    return np.ascontiguousarray(np.concatenate([[fx, fy, px, py], R.reshape(9), t]).astype(np.float32))


class PyCamera:
    def __init__(self, fx, fy, px, py, R, t, width, height):
        self.params = _cam_params(fx, fy, px, py, R, t)
        self.width, self.height = int(width), int(height)


class PyShader:
    def __init__(self, ka, kd, ks, alpha):
        self.params = np.array([ka, kd, ks, alpha], np.float32)


class PyRenderInput:
    def __init__(self, verts=None, colors=None, normals=None, faces=None):
        self.verts = self.colors = self.normals = self.faces = None
        self._bvh = None
        if verts is not None:
            self.set_verts(verts)
        if normals is not None:
            self.set_normals(normals)
        if colors is not None:
            self.set_colors(colors)
        if faces is not None:
            self.set_faces(faces)

    @staticmethod
    def _nx3(a, dtype, what):
        a = np.ascontiguousarray(a, dtype)
        if a.ndim != 2 or a.shape[1] != 3:
            raise Exception('%s has to be a Nx3 matrix' % what)
        return a

    def set_verts(self, verts):
        self.verts = self._nx3(verts, np.float32, 'verts')
        self._bvh = None                  # PyRenderer(accel='bvh') cache: built from verts and faces

    def set_colors(self, colors):
        self.colors = self._nx3(colors, np.float32, 'colors')

    def set_normals(self, normals):
        self.normals = self._nx3(normals, np.float32, 'normals')

    def set_faces(self, faces):
        self.faces = self._nx3(faces, np.int32, 'faces')
        self._bvh = None


class MeshBVH:
    """Bounding volume hierarchy of one static mesh, built on the device (ctd_mesh_bvh_build_f32) for the `bvh=`
    argument of render_mesh_proj / render_mesh.  Renders through it are bit-identical to the brute-force caster.

    verts [n,3] f32, faces [m,3] int32: CUDA tensors or numpy (copied to `device`).  The tree belongs to exactly these
    tensors (kept referenced here): pass `bvh.verts` / `bvh.faces`, or the same tensors, unchanged, to the renderers.
    `.depth` is the tree depth, `.nbytes` the buffer size, `.n_faces` the face count.  A tree deeper than the
    traversal stack is not usable (`.usable` False); the renderers then fall back to the brute-force caster."""

    def __init__(self, verts, faces, device=None):
        dev = torch.device(device) if device is not None else (
            verts.device if isinstance(verts, torch.Tensor) and verts.is_cuda else
            torch.device("cuda", torch.cuda.current_device()))
        up = lambda a, dt: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(dev, dt).contiguous()
        self.verts, self.faces = up(verts, torch.float32), up(faces, torch.int32)
        if self.verts.ndim != 2 or self.verts.shape[1] != 3 or self.faces.ndim != 2 or self.faces.shape[1] != 3:
            raise RuntimeError("verts and faces must be [n,3] and [m,3]")
        n_verts, self.n_faces = self.verts.shape[0], self.faces.shape[0]
        if self.n_faces and bool(((self.faces < 0) | (self.faces >= n_verts)).any()):
            raise RuntimeError("faces index outside [0, %d)" % n_verts)
        l = _lib.lib()
        self.nbytes = int(l.ctd_mesh_bvh_bytes(self.n_faces))
        if self.nbytes == 0:
            raise RuntimeError("mesh too large for a BVH (%d faces)" % self.n_faces)
        self.buffer = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        ws = torch.empty(max(1, int(l.ctd_mesh_bvh_workspace_bytes(self.n_faces))), dtype=torch.uint8, device=dev)
        depth = ctypes.c_int(0)
        st = l.ctd_mesh_bvh_build_f32(self.verts.data_ptr(), n_verts, self.faces.data_ptr(), self.n_faces,
                                      self.buffer.data_ptr(), self.nbytes, ws.data_ptr(), ws.numel(),
                                      ctypes.byref(depth), dev.index, torch.cuda.current_stream(dev).cuda_stream)
        self.depth = depth.value
        self.usable = st == 0
        if st not in (0, CTD_ERR_UNSUPPORTED):
            _lib.check(st, "mesh_bvh_build")

    def matches(self, verts, faces):
        return verts.data_ptr() == self.verts.data_ptr() and faces.data_ptr() == self.faces.data_ptr() and \
            tuple(verts.shape) == tuple(self.verts.shape) and tuple(faces.shape) == tuple(self.faces.shape)


def _check_bvh(bvh, verts, faces):
    if not isinstance(bvh, MeshBVH):
        raise TypeError("bvh must be a MeshBVH")
    if not bvh.matches(verts, faces):
        raise RuntimeError("bvh was built from other verts / faces tensors")
    return bvh.usable


def _render(brute, tree, who, bvh, verts, faces, args):
    """brute(*args), or with a usable tree of these tensors tree(the tree's buffer, *args)"""
    if bvh is not None and _check_bvh(bvh, verts, faces):
        _lib.check(tree(bvh.buffer.data_ptr(), *args), who + " (bvh)")
    else:
        _lib.check(brute(*args), who)


def render_mesh_proj(verts, colors, faces, cam, proj, shader, pattern, d_alpha=1.0, d_beta=0.0, bvh=None):
    """verts, colors [n,3] f32, faces [m,3] int32, pattern [ph,pw,3] f32: CUDA tensors; cam, proj: PyCamera; shader:
    PyShader -> (depth [H,W], color [H,W,3], normal [H,W,3]) CUDA tensors (normal zero where nothing is hit).
    bvh: a MeshBVH of these verts / faces, or None (brute force); both give the same bits."""
    _cuda_tensors((verts, "verts", torch.float32), (colors, "colors", torch.float32), (faces, "faces", torch.int32),
                  (pattern, "pattern", torch.float32))
    if tuple(pattern.shape) != (proj.height, proj.width, 3):
        raise Exception('pattern has to be a %dx%dx3 tensor' % (proj.height, proj.width))      # cyrender.pyx:197
    dev = verts.device
    depth = torch.empty((cam.height, cam.width), dtype=torch.float32, device=dev)
    color = torch.empty((cam.height, cam.width, 3), dtype=torch.float32, device=dev)
    normal = torch.zeros((cam.height, cam.width, 3), dtype=torch.float32, device=dev)
    args = (verts.data_ptr(), colors.data_ptr(), verts.shape[0], faces.data_ptr(), faces.shape[0],
            cam.params.ctypes.data, cam.width, cam.height, proj.params.ctypes.data, proj.width, proj.height,
            shader.params.ctypes.data, pattern.data_ptr(), float(d_alpha), float(d_beta), depth.data_ptr(), color.data_ptr(),
            normal.data_ptr(), dev.index, torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    _render(L.ctd_render_mesh_proj_f32, L.ctd_render_mesh_proj_bvh_f32, "render_mesh_proj", bvh, verts, faces, args)
    return depth, color, normal


def render_mesh(verts, colors, normals, faces, cam, shader, bvh=None):
    """RenderMeshFunctor (render.h:150-223): verts, colors, normals [n,3] f32, faces [m,3] int32 CUDA tensors ->
    (depth [H,W], color [H,W,3], normal [H,W,3]) CUDA tensors.  bvh: as for render_mesh_proj."""
    _cuda_tensors((verts, "verts", torch.float32), (colors, "colors", torch.float32), (normals, "normals", torch.float32),
                  (faces, "faces", torch.int32))
    if colors.shape != verts.shape or normals.shape != verts.shape:
        raise RuntimeError("colors and normals must have one row per vertex")
    dev = verts.device
    depth = torch.empty((cam.height, cam.width), dtype=torch.float32, device=dev)
    color = torch.empty((cam.height, cam.width, 3), dtype=torch.float32, device=dev)
    normal = torch.empty((cam.height, cam.width, 3), dtype=torch.float32, device=dev)
    args = (verts.data_ptr(), colors.data_ptr(), normals.data_ptr(), verts.shape[0], faces.data_ptr(), faces.shape[0],
            cam.params.ctypes.data, cam.width, cam.height, shader.params.ctypes.data, depth.data_ptr(), color.data_ptr(),
            normal.data_ptr(), dev.index, torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    _render(L.ctd_render_mesh_f32, L.ctd_render_mesh_bvh_f32, "render_mesh", bvh, verts, faces, args)
    return depth, color, normal


class PyRenderer:
    def __init__(self, cam, shader, engine='gpu', n_threads=1, device=None, accel=None):
        """accel=None: brute-force ray casting; accel='bvh': a MeshBVH per PyRenderInput, built at its first render and
        kept until its verts or faces are set again (same output bits either way)."""
        if engine != 'gpu':
            raise Exception('invalid engine' if engine != 'cpu' else
                            "engine='cpu' is not part of this package (the CPU renderer is the test oracle)")
        if accel not in (None, 'bvh'):
            raise Exception("invalid accel (None or 'bvh')")
        self.cam, self.shader, self.accel = cam, shader, accel
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.depth_buffer = np.zeros((cam.height, cam.width), np.float32)
        self.color_buffer = np.zeros((cam.height, cam.width, 3), np.float32)
        self.normal_buffer = np.zeros((cam.height, cam.width, 3), np.float32)

    def depth(self):
        return self.depth_buffer

    def color(self):
        return self.color_buffer

    def normal(self):
        return self.normal_buffer

    def _store(self, d, c, n):
        self.depth_buffer[...] = d.cpu().numpy()
        self.color_buffer[...] = c.cpu().numpy()
        self.normal_buffer[...] = n.cpu().numpy()

    def _mesh_tensors(self, input):
        """(verts, faces, bvh) on the device; with accel='bvh' the tree and its tensors are cached on the input"""
        up = lambda a: torch.from_numpy(a).to(self.device)
        if self.accel != 'bvh':
            return up(input.verts), up(input.faces), None
        b = input._bvh
        if b is None or b.verts.device != self.device:
            b = input._bvh = MeshBVH(input.verts, input.faces, device=self.device)
        return b.verts, b.faces, b

    def mesh(self, input):
        up = lambda a: torch.from_numpy(a).to(self.device)
        verts, faces, bvh = self._mesh_tensors(input)
        self._store(*render_mesh(verts, up(input.colors), up(input.normals), faces, self.cam, self.shader, bvh=bvh))

    def mesh_proj(self, input, proj, pattern, d_alpha=1, d_beta=0):
        pattern = np.ascontiguousarray(pattern, np.float32)
        if pattern.shape != (proj.height, proj.width, 3):
            raise Exception('pattern has to be a %dx%dx3 tensor' % (proj.height, proj.width))
        up = lambda a: torch.from_numpy(a).to(self.device)
        verts, faces, bvh = self._mesh_tensors(input)
        d, c, n = render_mesh_proj(verts, up(input.colors), faces, self.cam, proj, self.shader, up(pattern), d_alpha,
                                   d_beta, bvh=bvh)
        self._store(d, c, n)
