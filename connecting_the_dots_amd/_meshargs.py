"""What the mesh modules (meshops, mesheval, meshcolor, meshsmooth, meshsimplify, meshsdf) and the renderer share above the C calls: the checks
of [rows,3] tensors and of flags, the choice of a tree for a query and the call that falls back from it, and the steps
every `*_tsdf_mesh` function takes.  Private: the public names stay in the modules that use these."""
import torch

from . import _lib
from .mesh import TsdfMesh
from .torchext._common import _check

CTD_ERR_UNSUPPORTED = 3


def _nx3(t, who, name, dtype, rows=None, letter="n"):
    """t: a contiguous CUDA tensor of `dtype` shaped [rows,3]; rows=None takes any number of rows and words it
    [letter,3].  The device is checked before the dtype and the dtype before the shape."""
    _check(t, "%s: %s" % (who, name), (dtype,))
    if t.dim() != 2 or t.shape[1] != 3 or (rows is not None and t.shape[0] != rows):
        raise RuntimeError("%s: %s must be shaped [%s,3], got %s" % (who, name, letter if rows is None else rows,
                                                                     tuple(t.shape)))
    return t


def _cuda_tensors(*args):
    """the renderers' check of (tensor, name, dtype) triples, whatever their shapes"""
    for t, name, dtype in args:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == dtype):
            raise RuntimeError("%s must be a contiguous CUDA tensor of dtype %s" % (name, dtype))


def _flag(x, name, who):
    if not isinstance(x, bool):
        raise RuntimeError("%s: %s must be True or False" % (who, name))
    return int(x)


def _ptr_or(t, spare):
    """an empty tensor has no storage, but the C calls want their required pointers all the same (they read and write
    nothing through them then): the workspace stands in"""
    return t.data_ptr() or spare.data_ptr()


def _resolve_bvh(bvh, verts, faces, who, min_faces):
    """bvh: None, 'auto' or a renderer.MeshBVH -> a usable MeshBVH of these tensors, or None (brute force).  'auto' builds
    one when the mesh has at least min_faces faces: the caller's AUTO_BVH_MIN_FACES, which it reads at the call."""
    from .renderer import MeshBVH                            # at the call: renderer imports this module
    if bvh is None:
        return None
    if isinstance(bvh, str):
        if bvh != "auto":
            raise RuntimeError("%s: bvh must be None, 'auto' or a renderer.MeshBVH" % who)
        if faces.shape[0] < min_faces or bool(((faces < 0) | (faces >= verts.shape[0])).any()):
            return None                                   # small, or faces the tree's build may not read
        bvh = MeshBVH(verts, faces)
    elif not isinstance(bvh, MeshBVH):
        raise RuntimeError("%s: bvh must be None, 'auto' or a renderer.MeshBVH" % who)
    elif not bvh.matches(verts, faces):
        raise RuntimeError("%s: bvh was built from other verts / faces tensors" % who)
    return bvh if bvh.usable else None


def _call_tree_then_brute(fn, head, tree, tail, who):
    """fn(*head, the tree's buffer, *tail) when there is a tree; fn(*head, None, *tail) when there is none or the tree
    is deeper than the traversal stack (CTD_ERR_UNSUPPORTED).  Any other status raises in the name of `who`."""
    st = CTD_ERR_UNSUPPORTED
    if tree is not None:
        st = fn(*head, tree.buffer.data_ptr(), *tail)
    if st == CTD_ERR_UNSUPPORTED:
        st = fn(*head, None, *tail)
    _lib.check(st, who)


def _tsdf_mesh_arg(m, who):
    if not isinstance(m, TsdfMesh):
        raise RuntimeError("%s: m must be a mesh.TsdfMesh" % who)
    return m


def _cat_or_empty(parts, like):
    """the per-track results one after the other; for a mesh without tracks an empty tensor like `like`"""
    return torch.cat(parts) if parts else like[:0].clone()
