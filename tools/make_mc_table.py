"""Generates connecting_the_dots_amd/csrc/ctd_mc_table.h, the triangle table of ctd_tsdf_mesh_faces_i32, from the rule
of include/ctd_hip_mesh.h and prints it:
    python tools/make_mc_table.py > connecting_the_dots_amd/csrc/ctd_mc_table.h
tests/test_tsdf_mesh_host.py checks that the committed header is this output, and the table against a second
implementation of the rule (tests/mesh_ref.py, which orients the loops combinatorially where this file does it with
the geometry of the unit cube).

The rule.  Corner n = dx + 2*dy + 4*dz of a cell; bit n of the case is set when the corner is inside (T < 0).  Edge
e = 4*c + r runs along axis c from the r-th corner (ascending n) whose coordinate c is 0.  On each of the six cell faces
the crossing edges are joined by segments: two crossing edges by one segment, four by two segments, each around one
inside corner.  The segments close into loops.  A loop starts at its lowest e and runs in the direction for which its
triangles' (v1-v0) x (v2-v0) points from inside towards free space; the loops come in ascending order of their lowest
e.  A loop q of length m is the fan (q0, q_i, q_i+1), i = 1 .. m-2, after rotating it to the first apex, in loop order
from the start, for which no fan diagonal joins two edges of one cell face.
"""
import sys

import numpy as np

CORNERS = np.array([[n & 1, (n >> 1) & 1, (n >> 2) & 1] for n in range(8)], dtype=np.int64)


def edge_ends(e):
    """(lower corner, upper corner) of edge e"""
    c, r = divmod(e, 4)
    lower = [n for n in range(8) if CORNERS[n][c] == 0][r]
    return lower, lower + (1 << c)


EDGES = [edge_ends(e) for e in range(12)]
EDGE_OF = {frozenset(ends): e for e, ends in enumerate(EDGES)}
MID = np.array([(CORNERS[a] + CORNERS[b]) / 2.0 for a, b in EDGES])


def cell_faces():
    """the six faces as four corners in cyclic order"""
    out = []
    for c in range(3):
        a, b = [x for x in range(3) if x != c]
        for side in (0, 1):
            ring = []
            for da, db in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[c], p[a], p[b] = side, da, db
                ring.append(p[0] + 2 * p[1] + 4 * p[2])
            out.append(ring)
    return out


FACES = cell_faces()
FACES_OF_EDGE = [{f for f, ring in enumerate(FACES) if a in ring and b in ring} for a, b in EDGES]


def segments(case):
    """the segments on the six faces, as pairs of edges"""
    inside = [(case >> n) & 1 for n in range(8)]
    out = []
    for ring in FACES:
        edges = [EDGE_OF[frozenset((ring[i], ring[(i + 1) % 4]))] for i in range(4)]
        crossing = [i for i in range(4) if inside[ring[i]] != inside[ring[(i + 1) % 4]]]
        if len(crossing) == 2:
            out.append((edges[crossing[0]], edges[crossing[1]]))
        elif len(crossing) == 4:
            for i in range(4):                                  # ring edge i-1 ends at corner i, ring edge i starts there
                if inside[ring[i]]:
                    out.append((edges[i - 1], edges[i]))
        else:
            assert not crossing
    return out


def loops(case):
    """the loops of a case: each starts at its lowest edge and is oriented, ascending by that edge"""
    inside = [(case >> n) & 1 for n in range(8)]
    crossing = [e for e, (a, b) in enumerate(EDGES) if inside[a] != inside[b]]
    links = {e: [] for e in crossing}
    for a, b in segments(case):
        links[a].append(b)
        links[b].append(a)
    assert all(len(v) == 2 for v in links.values()), "case %d does not close into loops" % case
    out, seen = [], set()
    for start in crossing:                                      # ascending
        if start in seen:
            continue
        loop, prev, cur = [start], None, start
        while True:
            seen.add(cur)
            nxt = [x for x in links[cur] if x != prev]
            nxt = nxt[0] if nxt else links[cur][0]              # (a loop of two edges does not exist; kept total)
            if nxt == start:
                break
            loop.append(nxt)
            prev, cur = cur, nxt
        assert len(loop) >= 3
        # orientation: the area vector of the loop through the edge midpoints against the sum, over its edges, of the
        # direction from the inside end to the outside end
        area = sum(np.cross(MID[loop[i]], MID[loop[(i + 1) % len(loop)]]) for i in range(len(loop)))
        out_dir = sum((CORNERS[b] - CORNERS[a]) * (1 if inside[a] else -1) for a, b in (EDGES[e] for e in loop))
        s = float(np.dot(area, out_dir))
        assert s != 0.0, "case %d: the orientation test is 0" % case
        if s < 0:
            loop = [loop[0]] + loop[:0:-1]
        out.append(loop)
    return out


def fan(loop):
    """the triangles of a loop, and the apex's position in it"""
    m = len(loop)
    for a in range(m):
        q = loop[a:] + loop[:a]
        if all(not (FACES_OF_EDGE[q[0]] & FACES_OF_EDGE[q[i]]) for i in range(2, m - 1)):
            return [(q[0], q[i], q[i + 1]) for i in range(1, m - 1)], a
    raise AssertionError("no admissible apex")


def table():
    """case -> list of triangles (edge triples)"""
    return [[t for loop in loops(case) for t in fan(loop)[0]] for case in range(256)]


def header():
    tab = table()
    assert max(len(t) for t in tab) == 5
    lines = ["// ctd_mc_table.h -- generated by tools/make_mc_table.py from the rule of include/ctd_hip_mesh.h; do not edit.",
             "// One row of 16 bytes per case: the edge ids of up to 5 triangles (255 behind the last), then the number of",
             "// triangles.  %d triangles in all." % sum(len(t) for t in tab),
             "#pragma once",
             "",
             "#define CTD_MC_TABLE_ROWS \\"]
    for case, tris in enumerate(tab):
        row = [e for t in tris for e in t]
        row += [255] * (15 - len(row)) + [len(tris)]
        lines.append("  {%s}%s" % (", ".join("%3d" % v for v in row), ", \\" if case < 255 else ""))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    sys.stdout.write(header())
