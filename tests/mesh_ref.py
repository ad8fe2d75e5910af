"""Numpy restatement of the rule of include/ctd_hip_mesh.h (ctd_tsdf_mesh_faces_i32): the triangle table built from the
rule with code of its own (it does not read csrc/ctd_mc_table.h, and where tools/make_mc_table.py orients a loop with the
geometry of the unit cube, this file orients the segments on the cell faces combinatorially), and `faces`, the indexed
triangles of a volume over the points of tests/tsdf_ref.surface_points."""
import numpy as np

F = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
def _xyz(n):
    return (n & 1, (n >> 1) & 1, (n >> 2) & 1)


def _edges():
    """edge e = 4*c + r -> (lower corner, upper corner): along axis c from the r-th corner with coordinate c == 0"""
    out = []
    for c in range(3):
        for n in range(8):
            if _xyz(n)[c] == 0:
                out.append((n, n | (1 << c)))
    return out


EDGES = _edges()


def _edge_between(a, b):
    return EDGES.index((min(a, b), max(a, b)))


def _rings():
    """the six cell faces, each as its four corners counter-clockwise as seen from outside the cell"""
    rings = []
    for c in range(3):
        a, b = [x for x in range(3) if x != c]
        for side in (0, 1):
            ring = [(side << c) | (da << a) | (db << b) for da, db in ((0, 0), (1, 0), (1, 1), (0, 1))]
            # a -> b turns about +x for (y,z), about -y for (x,z), about +z for (x,y); outside is +c at side 1, -c at side 0
            turns_about_plus_c = c != 1
            if turns_about_plus_c != (side == 1):
                ring.reverse()
            rings.append(ring)
    return rings


RINGS = _rings()


def _on_one_face(e0, e1):
    """do the edges e0 and e1 lie on a common cell face?"""
    for d in range(3):
        for side in (0, 1):
            if all(_xyz(n)[d] == side for n in EDGES[e0] + EDGES[e1]):
                return True
    return False


def _successors(case):
    """crossing edge -> the next crossing edge of its loop: on every face, each run of inside corners (in the ring's order)
    is cut off by one segment, from the ring edge that enters the run to the ring edge that leaves it, which keeps the
    inside corners on the right as seen from outside the cell"""
    inside = [(case >> n) & 1 for n in range(8)]
    nxt = {}
    for ring in RINGS:
        for i in range(4):
            if inside[ring[i]] and not inside[ring[i - 1]]:        # a run starts at ring[i]
                j = i
                while inside[ring[(j + 1) % 4]]:
                    j += 1
                enter = _edge_between(ring[i - 1], ring[i])
                leave = _edge_between(ring[j % 4], ring[(j + 1) % 4])
                assert enter not in nxt
                nxt[enter] = leave
    return nxt


def case_loops(case):
    nxt = _successors(case)
    crossing = sorted(e for e, (a, b) in enumerate(EDGES) if ((case >> a) & 1) != ((case >> b) & 1))
    assert sorted(nxt) == crossing and sorted(nxt.values()) == crossing, case
    loops, seen = [], set()
    for e in crossing:
        if e in seen:
            continue
        loop = [e]
        while nxt[loop[-1]] != e:
            loop.append(nxt[loop[-1]])
        seen.update(loop)
        loops.append(loop)
    return loops


def loop_fan(loop):
    """-> (triangles, position of the apex in the loop)"""
    m = len(loop)
    for apex in range(m):
        q = [loop[(apex + i) % m] for i in range(m)]
        if not any(_on_one_face(q[0], q[i]) for i in range(2, m - 1)):
            return [(q[0], q[i], q[i + 1]) for i in range(1, m - 1)], apex
    raise AssertionError("no admissible apex in %s" % (loop,))


def case_triangles(case, plain_fan=False):
    out = []
    for loop in case_loops(case):
        if plain_fan:
            out += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
        else:
            out += loop_fan(loop)[0]
    return out


TABLE = [case_triangles(c) for c in range(256)]
PLAIN_TABLE = [case_triangles(c, plain_fan=True) for c in range(256)]


def _table_arrays(table):
    n_tri = np.array([len(t) for t in table], np.int64)
    tri = np.zeros((256, 5, 3), np.int64)
    for c, ts in enumerate(table):
        for k, t in enumerate(ts):
            tri[c, k] = t
    return n_tri, tri


# ---------------------------------------------------------------------------------------------------------------------
# the faces of a volume
# ---------------------------------------------------------------------------------------------------------------------
def cell_cases(tsdf, weight, min_weight=1.0):
    """-> case int64 [B,nz-1,ny-1,nx-1] and meshed bool of the same shape (case 0 where a cell is not meshed)"""
    B, nz, ny, nx = tsdf.shape
    with np.errstate(invalid="ignore"):
        use = (weight >= F(min_weight)) & (np.abs(tsdf) < F(1))
        neg = tsdf < 0
    shape = (B, max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0))
    meshed = np.ones(shape, bool)
    case = np.zeros(shape, np.int64)
    for n in range(8):
        dx, dy, dz = _xyz(n)
        sl = (slice(None), slice(dz, dz + shape[1]), slice(dy, dy + shape[2]), slice(dx, dx + shape[3]))
        meshed &= use[sl]
        case |= neg[sl].astype(np.int64) << n
    return np.where(meshed, case, 0), meshed


def crossing_flags(tsdf, weight, min_weight=1.0):
    """bool [B,nz,ny,nx,3]: the crossings of include/ctd_hip_tsdf.h, one per surface point, in src order when flattened"""
    B, nz, ny, nx = tsdf.shape
    with np.errstate(invalid="ignore"):
        use = (weight >= F(min_weight)) & (np.abs(tsdf) < F(1))
        neg = tsdf < 0
    emit = np.zeros((B, nz, ny, nx, 3), bool)
    emit[:, :, :, :-1, 0] = use[:, :, :, :-1] & use[:, :, :, 1:] & (neg[:, :, :, :-1] != neg[:, :, :, 1:])
    emit[:, :, :-1, :, 1] = use[:, :, :-1] & use[:, :, 1:] & (neg[:, :, :-1] != neg[:, :, 1:])
    emit[:, :-1, :, :, 2] = use[:, :-1] & use[:, 1:] & (neg[:, :-1] != neg[:, 1:])
    return emit


def faces(tsdf, weight, min_weight=1.0, table=None):
    """-> faces int32 [F,3] (track-local indices into the track's surface points, the tracks one after the other, cells
    ascending, table order within a cell) and n_faces_per_track int64 [B]"""
    B, nz, ny, nx = tsdf.shape
    assert tsdf.dtype == F and weight.dtype == F
    n_tri, tri = _table_arrays(TABLE if table is None else table)
    case, _ = cell_cases(tsdf, weight, min_weight)
    emit = crossing_flags(tsdf, weight, min_weight)
    out, counts = [], []
    for b in range(B):
        flags = emit[b].reshape(-1)                                 # [nvox*3], src order
        rank = np.cumsum(flags) - flags                             # track-local index of the point of a set flag
        cz, cy, cx = np.nonzero(n_tri[case[b]] > 0)                  # ascending (k, j, i): ascending cell order
        cs = case[b][cz, cy, cx]
        k = n_tri[cs]
        cell = np.repeat(np.arange(len(cs)), k)
        t = np.arange(k.sum()) - np.repeat(np.cumsum(k) - k, k)
        e = tri[cs[cell], t]                                        # [F_b,3] edge ids
        c, r = e // 4, e % 4
        lower = np.array([[EDGES[4 * cc + rr][0] for rr in range(4)] for cc in range(3)], np.int64)[c, r]
        gi = cx[cell][:, None] + (lower & 1)
        gj = cy[cell][:, None] + ((lower >> 1) & 1)
        gk = cz[cell][:, None] + ((lower >> 2) & 1)
        src = ((gk * ny + gj) * nx + gi) * 3 + c
        assert flags[src].all(), "a face refers to an edge without a surface point"
        out.append(rank[src].astype(np.int32).reshape(-1, 3))
        counts.append(len(e))
    allf = np.concatenate(out) if out else np.zeros((0, 3), np.int32)
    return np.ascontiguousarray(allf.reshape(-1, 3).astype(np.int32)), np.array(counts, np.int64).reshape(B)


# ---------------------------------------------------------------------------------------------------------------------
# checks shared by the tests
# ---------------------------------------------------------------------------------------------------------------------
def directed_edge_counts(tris):
    """the multiset of directed edges of triangles [F,3] -> dict (a, b) -> count"""
    out = {}
    for a, b in np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]]).tolist():
        out[(a, b)] = out.get((a, b), 0) + 1
    return out


def is_closed_oriented_manifold(tris):
    """every directed edge occurs exactly once and its reverse exactly once"""
    d = directed_edge_counts(tris)
    return all(v == 1 for v in d.values()) and all((b, a) in d for (a, b) in d)


def sphere_volume(n, radius, centre=None, scale=0.25):
    """tsdf [1,n,n,n] = clip((|x - centre| - radius) * scale, -0.9, 0.9): negative inside; all weights 1"""
    centre = [(n - 1) / 2.0 + 0.13, (n - 1) / 2.0 - 0.21, (n - 1) / 2.0 + 0.07] if centre is None else centre
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    d = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius
    return np.clip(d * scale, -0.9, 0.9).astype(F)[None], np.ones((1, n, n, n), F), np.asarray(centre)
