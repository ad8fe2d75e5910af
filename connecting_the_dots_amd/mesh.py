"""The triangle mesh of a truncated signed distance volume (include/ctd_hip_mesh.h, csrc/tsdf_mesh.hip) and PLY files.

    m = mesh.tsdf_mesh(tsdf, weight, origin, voxel)           # marching cubes over the volume of torchext.tsdf_integrate
    verts, faces, _ = m.track(0)                              # [n,3] f32, [k,3] int32: what the ray caster takes
    bvh = renderer.MeshBVH(verts, faces)                      # ... renderer.render_mesh / render_mesh_proj(..., bvh=bvh)
    mesh.save_ply("model.ply", verts, faces)

The vertices are exactly the points of `torchext.tsdf_surface_points` (one per zero-crossing grid edge, ascending src);
the faces index them, so the mesh is welded without hashing or merging.  No fallback: a missing kernel is an error.
"""
import numpy as np
import torch

from . import _lib
from .torchext._common import _call, _integer, _number, _ptr, _stream, _workspace
from .torchext.tsdf import _tsdf_inputs, tsdf_surface_points

_RULE = """
    The rule (include/ctd_hip_mesh.h).  Cell (i,j,k) has the corners n = dx + 2*dy + 4*dz at voxel (i+dx, j+dy, k+dz);
    it is meshed when all eight are usable (weight >= min_weight and |tsdf| < 1), and bit n of its case is set when
    T_n < 0.  Edge e = 4*c + r runs along axis c from the r-th corner with coordinate c == 0; the vertex on a crossing
    edge is the surface point with src = 3*g(lower corner) + c.  On each cell face two crossing edges are joined by one
    segment, four by two segments that separate the inside corners; the segments close into loops, each starting at its
    lowest e and running so that (v1-v0) x (v2-v0) of its triangles points from inside towards free space, in ascending
    order of their lowest e; a loop is a fan from the first apex for which no fan diagonal joins two edges of one cell
    face.  Faces are int32 and track-local, in ascending cell order and table order within a cell.  Nothing is removed:
    points on edges of no meshed cell stay as unreferenced vertices, and a crossing at a voxel whose tsdf is exactly 0
    can yield zero-area triangles.  No atomics: the same bits on every run."""


class TsdfMesh:
    """What `tsdf_mesh` returns.  verts [M,3] f32, src [M] int64 and normals [M,3] f32 (None without return_normals) are
    the outputs of `torchext.tsdf_surface_points`; faces [F,3] int32 holds track-local indices, the tracks one after the
    other; n_verts_per_track and n_faces_per_track are int64 [B]."""

    def __init__(self, verts, src, normals, faces, n_verts_per_track, n_faces_per_track, counts):
        self.verts, self.src, self.normals, self.faces = verts, src, normals, faces
        self.n_verts_per_track, self.n_faces_per_track = n_verts_per_track, n_faces_per_track
        self._counts = counts                                   # host copy: [(n_verts, n_faces)] per track

    @property
    def n_tracks(self):
        return len(self._counts)

    def tracks(self):
        """-> (b, verts_b, faces_b, normals_b, v0) for every track in order: the slices of `track(b)`, and the row of
        verts, src and normals at which the track's vertices start.  No copy and no synchronisation."""
        v0 = 0
        for b, (nv, _) in enumerate(self._counts):
            yield (b,) + self.track(b) + (v0,)
            v0 += nv

    def track(self, b):
        """-> (verts_b [n,3] f32, faces_b [k,3] int32, normals_b [n,3] f32 or None): contiguous slices, no copy and no
        synchronisation; they go straight into `renderer.MeshBVH(verts_b, faces_b)` and `renderer.render_mesh`."""
        b = _integer(b, "b", "TsdfMesh.track", 0, self.n_tracks - 1, "an integer in [0, %d)" % self.n_tracks)
        v0, f0 = (sum(c[k] for c in self._counts[:b]) for k in (0, 1))
        nv, nf = self._counts[b]
        return (self.verts[v0:v0 + nv], self.faces[f0:f0 + nf],
                None if self.normals is None else self.normals[v0:v0 + nv])


def tsdf_mesh(tsdf, weight, origin, voxel, min_weight=1.0, return_normals=False):
    """The triangle mesh of a volume -> `TsdfMesh`.  The vertices come from `torchext.tsdf_surface_points`, called here
    with the same arguments; the faces call then counts, the counts are read back once (one synchronisation) to size
    the output, and a second call fills it.  Not differentiable."""
    who = "tsdf_mesh"
    min_weight = _number(min_weight, "min_weight", who, lo_open=True)
    dev, B, nx, ny, nz, voxel = _tsdf_inputs(tsdf, weight, origin, voxel, who)
    out = tsdf_surface_points(tsdf, weight, origin, voxel, min_weight=min_weight, return_normals=bool(return_normals))
    verts, src, n_verts = out[:3]
    normals = out[3] if return_normals else None
    n_faces = torch.zeros((B,), dtype=torch.int64, device=dev)
    counts = []
    L = _lib.lib()
    if B > 0:
        ws = _workspace(L.ctd_tsdf_mesh_workspace_bytes(B, nx, ny, nz), dev)

        def call(faces, capacity):
            _call(L.ctd_tsdf_mesh_faces_i32, who, _ptr(tsdf), _ptr(weight), min_weight, _ptr(faces), _ptr(n_faces), capacity,
                  B, nx, ny, nz, _ptr(ws), ws.numel(), dev.index, _stream(dev))

        call(None, 0)
        counts = [tuple(c) for c in torch.stack([n_verts, n_faces], 1).cpu().tolist()]
    total = sum(c[1] for c in counts)
    faces = torch.empty((total, 3), dtype=torch.int32, device=dev)
    if total > 0:
        call(faces, total)
    return TsdfMesh(verts, src, normals, faces, n_verts, n_faces, counts)


tsdf_mesh.__doc__ += _RULE


# ---------------------------------------------------------------------------------------------------------------------
# PLY, binary little-endian, host side
# ---------------------------------------------------------------------------------------------------------------------
def _host(a, dtype, what, cols=3):
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype != dtype or a.ndim != 2 or a.shape[1] != cols:
        raise RuntimeError("save_ply: %s must be %s [n,%d], got %s %s" % (what, np.dtype(dtype).name, cols, a.dtype,
                                                                        a.shape))
    return np.ascontiguousarray(a)


def _vertex_dtype(normals, colors):
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(fields)


_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def save_ply(path, verts, faces, normals=None, colors=None):
    """Writes a triangle mesh as binary little-endian PLY: verts f32 [n,3], faces int32 [m,3], and optionally normals
    f32 [n,3] (nx, ny, nz) and colors uint8 [n,3] (red, green, blue).  Tensors (of any device) and numpy arrays are
    taken; the values are written bit for bit, NaNs included."""
    verts, faces = _host(verts, np.float32, "verts"), _host(faces, np.int32, "faces")
    normals, colors = _host(normals, np.float32, "normals"), _host(colors, np.uint8, "colors")
    n = len(verts)
    for a, what in ((normals, "normals"), (colors, "colors")):
        if a is not None and len(a) != n:
            raise RuntimeError("save_ply: %s must have one row per vertex" % what)
    if faces.size and (faces.min() < 0 or faces.max() >= n):
        raise RuntimeError("save_ply: a face refers to a vertex outside [0, %d)" % n)
    vdt = _vertex_dtype(normals is not None, colors is not None)
    v = np.zeros(n, vdt)
    for k, name in enumerate(("x", "y", "z")):
        v[name] = verts[:, k]
    if normals is not None:
        for k, name in enumerate(("nx", "ny", "nz")):
            v[name] = normals[:, k]
    if colors is not None:
        for k, name in enumerate(("red", "green", "blue")):
            v[name] = colors[:, k]
    f = np.zeros(len(faces), _FACE_DTYPE)
    f["n"], f["v"] = 3, faces
    kinds = {"<f4": "float", "u1": "uchar", "|u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", "comment connecting_the_dots_amd.mesh", "element vertex %d" % n]
    header += ["property %s %s" % (kinds[vdt[name].str], name) for name in vdt.names]
    header += ["element face %d" % len(faces), "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())


def load_ply(path):
    """Reads a PLY written by `save_ply` -> (verts f32 [n,3], faces int32 [m,3], normals f32 [n,3] or None, colors uint8
    [n,3] or None) as numpy arrays.  Anything else than that layout raises."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise RuntimeError("load_ply: %s is not a PLY file" % path)
    lines = [ln.split() for ln in data[:end].decode("ascii").split("\n")[1:] if ln and not ln.startswith("comment")]
    body = data[end + len(b"end_header\n"):]
    if not lines or lines[0] != ["format", "binary_little_endian", "1.0"]:
        raise RuntimeError("load_ply: only binary_little_endian 1.0 is read")
    elements, props = [], {}
    for ln in lines[1:]:
        if ln[0] == "element" and len(ln) == 3:
            elements.append((ln[1], int(ln[2])))
            props[ln[1]] = []
        elif ln[0] == "property" and elements:
            props[elements[-1][0]].append(tuple(ln[1:]))
        else:
            raise RuntimeError("load_ply: unexpected header line %r" % " ".join(ln))
    if [e[0] for e in elements] != ["vertex", "face"] or props["face"] != [("list", "uchar", "int", "vertex_indices")]:
        raise RuntimeError("load_ply: a vertex element and a face element of uchar-counted int lists expected")
    names = [p[-1] for p in props["vertex"]]
    normals, colors = "nx" in names, "red" in names
    vdt = _vertex_dtype(normals, colors)
    want = [({"<f4": "float"}.get(vdt[k].str, "uchar"), k) for k in vdt.names]
    if props["vertex"] != want:
        raise RuntimeError("load_ply: vertex properties %s are not those save_ply writes" % (names,))
    n, m = elements[0][1], elements[1][1]
    if len(body) != n * vdt.itemsize + m * _FACE_DTYPE.itemsize:
        raise RuntimeError("load_ply: %d bytes of data, %d expected" % (len(body), n * vdt.itemsize + m * _FACE_DTYPE.itemsize))
    v = np.frombuffer(body, vdt, n)
    f = np.frombuffer(body, _FACE_DTYPE, m, n * vdt.itemsize)
    if m and (f["n"] != 3).any():
        raise RuntimeError("load_ply: only triangles are read")

    def cols(keys, dtype):
        return np.ascontiguousarray(np.stack([v[k] for k in keys], 1).astype(dtype, copy=False)).reshape(n, 3)

    return (cols(("x", "y", "z"), np.float32), np.ascontiguousarray(f["v"]).astype(np.int32).reshape(m, 3),
            cols(("nx", "ny", "nz"), np.float32) if normals else None,
            cols(("red", "green", "blue"), np.uint8) if colors else None)
