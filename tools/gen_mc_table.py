#!/usr/bin/env python
"""Generates the 256-case marching-cubes table of dreammesh4d_amd/csrc/mc_table.h from the rule below (nothing is copied from a
published table; none is available to this project).

    python tools/gen_mc_table.py            # rewrites dreammesh4d_amd/csrc/mc_table.h
    python tools/gen_mc_table.py --check    # exit status 1 when the committed header differs

Conventions (shared with csrc/isosurface.hip and tests/isosurface_common.py):

* corner c of a cube sits at offset (c >> 2 & 1, c >> 1 & 1, c & 1) along (i, j, k) from the cube's voxel; a case is the bit mask
  of its INSIDE corners (bit c set <=> f >= threshold at corner c);
* edge e = 4 * axis + q runs along `axis` (0 = i, 1 = j, 2 = k) from its base corner to base + unit(axis); the base corner has
  offset 0 along `axis` and the bits of q on the two other axes, the lower axis in bit 0 of q.  The edge belongs to the voxel
  at its base corner: that voxel's +axis edge.

Rule, per case: on each of the six cube faces the crossed edges (ends differ in the inside test) are paired into segments --
two crossings make one segment, four crossings (the ambiguous face: inside corners on one diagonal) make two segments that
each cut off ONE inside corner, so the two inside corners are always separated.  The choice depends on the face's own four
corner states only, so the two cubes sharing a face draw the same segments on it and the surface has no holes.  Each segment
is directed so that, with n the face's outward normal and g the in-face direction from its inside side to its outside side,
it runs along g x n: the boundary of a patch whose normal points toward the outside (lower field values) then runs
counter-clockwise around that normal.  Every crossed edge then has exactly one segment leaving and one arriving (asserted);
following them gives closed loops.  A loop is rotated to start at its smallest edge index and fan-triangulated from there;
loops are listed by ascending smallest edge index.

One amendment to the fan: a diagonal that joins two crossings on the SAME cube face lies in that face (it can only happen on an
ambiguous face, between its two segments), and the neighbouring cube may draw the very same diagonal -- that edge would then
carry four triangles and the mesh would not be a 2-manifold.  18 loops (of 6 and 7 crossings) have such a diagonal when fanned
from their smallest edge; for them the apex moves on, in loop order, to the first crossing whose fan has none (one always
exists: asserted).  No triangle of the table has an edge inside a cube face other than the face's own segments.
"""
import os
import sys

import numpy as np

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dreammesh4d_amd", "csrc", "mc_table.h")


def corner_offset(c):
    return (c >> 2 & 1, c >> 1 & 1, c & 1)


def corner_index(off):
    return off[0] << 2 | off[1] << 1 | off[2]


def edge_base_axis(e):
    """(offset of the base corner, axis) of edge e."""
    axis, q = divmod(e, 4)
    others = [a for a in range(3) if a != axis]
    off = [0, 0, 0]
    off[others[0]] = q & 1
    off[others[1]] = q >> 1 & 1
    return tuple(off), axis


EDGE_BASE = [edge_base_axis(e)[0] for e in range(12)]
EDGE_AXIS = [edge_base_axis(e)[1] for e in range(12)]


def edge_corners(e):
    off, axis = edge_base_axis(e)
    end = list(off)
    end[axis] = 1
    return corner_index(off), corner_index(tuple(end))


def edge_between(ca, cb):
    for e in range(12):
        if set(edge_corners(e)) == {ca, cb}:
            return e
    raise KeyError((ca, cb))


def edge_midpoint(e):
    a, b = edge_corners(e)
    return (np.array(corner_offset(a), float) + np.array(corner_offset(b), float)) / 2


def faces_of_cube():
    """[(outward normal, the face's four corners in cyclic order)]."""
    out = []
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for side in (0, 1):
            cyc = []
            for du, dv in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[axis], off[u], off[v] = side, du, dv
                cyc.append(corner_index(tuple(off)))
            n = np.zeros(3)
            n[axis] = 1.0 if side else -1.0
            out.append((n, cyc))
    return out


CUBE_FACES = faces_of_cube()


def directed(e0, e1, g, n):
    """The segment between the crossings of edges e0 and e1, directed along g x n."""
    d = edge_midpoint(e1) - edge_midpoint(e0)
    s = float(np.dot(d, np.cross(g, n)))
    assert abs(s) > 1e-9
    return (e0, e1) if s > 0 else (e1, e0)


def case_segments(case):
    inside = [bool(case >> c & 1) for c in range(8)]
    segments = []
    for n, cyc in CUBE_FACES:
        pos = [np.array(corner_offset(c), float) for c in cyc]
        centre = sum(pos) / 4
        crossed = [k for k in range(4) if inside[cyc[k]] != inside[cyc[(k + 1) % 4]]]        # edge k joins cyc[k], cyc[k + 1]
        face_edge = lambda k: edge_between(cyc[k], cyc[(k + 1) % 4])
        if len(crossed) == 2:
            g = sum(p for p, c in zip(pos, cyc) if not inside[c]) / sum(1 for c in cyc if not inside[c]) \
                - sum(p for p, c in zip(pos, cyc) if inside[c]) / sum(1 for c in cyc if inside[c])
            segments.append(directed(face_edge(crossed[0]), face_edge(crossed[1]), g, n))
        elif len(crossed) == 4:
            for k in range(4):
                if inside[cyc[k]]:                      # cut this inside corner off: its two face edges are k - 1 and k
                    segments.append(directed(face_edge((k - 1) % 4), face_edge(k), centre - pos[k], n))
        else:
            assert not crossed
    return segments


def case_loops(case):
    """Closed directed loops of edge indices, each starting at its smallest edge, sorted by that edge."""
    segments = case_segments(case)
    nxt = {}
    for a, b in segments:
        assert a not in nxt, (case, segments)
        nxt[a] = b
    crossed = {e for e in range(12) if (case >> edge_corners(e)[0] & 1) != (case >> edge_corners(e)[1] & 1)}
    assert set(nxt) == crossed and set(nxt.values()) == crossed and len(segments) == len(crossed), (case, segments)
    loops, seen = [], set()
    for start in sorted(crossed):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start and len(loop) >= 3, (case, loop)
        loops.append(loop)
    return loops


def edge_faces(e):
    """The two cube faces (indices into CUBE_FACES) edge e lies on."""
    a, b = edge_corners(e)
    return {i for i, (_, cyc) in enumerate(CUBE_FACES) if a in cyc and b in cyc}


EDGE_FACES = [edge_faces(e) for e in range(12)]


def fan_apex(loop):
    """Position in `loop` of the first crossing whose fan has no diagonal inside a cube face."""
    for ap in range(len(loop)):
        r = loop[ap:] + loop[:ap]
        if all(not (EDGE_FACES[r[0]] & EDGE_FACES[r[k]]) for k in range(2, len(r) - 1)):
            return ap
    raise AssertionError(loop)


def case_triangles(case):
    tris = []
    for loop in case_loops(case):
        ap = fan_apex(loop)
        r = loop[ap:] + loop[:ap]
        for k in range(1, len(r) - 1):
            tris.append((r[0], r[k], r[k + 1]))
    return tris


def build_table():
    """-> (tri_count [256], tris [256][max_tris][3] padded with -1, max_tris)."""
    all_tris = [case_triangles(c) for c in range(256)]
    max_tris = max(len(t) for t in all_tris)
    table = -np.ones((256, max_tris, 3), np.int8)
    for c, t in enumerate(all_tris):
        if t:
            table[c, :len(t)] = np.array(t, np.int8)
    return np.array([len(t) for t in all_tris], np.int8), table, max_tris


def render_header():
    count, table, max_tris = build_table()
    lines = ["// mc_table.h -- the 256-case marching-cubes table of csrc/isosurface.hip.  GENERATED by tools/gen_mc_table.py from the",
             "// rule stated there (ambiguous faces always separate their two inside corners; loops fan-triangulated from their smallest",
             "// edge -- from the next crossing whose fan keeps out of the cube's faces where that one does not -- and oriented so that",
             "// normals point toward lower field values); edit the generator, not this file.",
             "//",
             "// corner c: offset (c >> 2 & 1, c >> 1 & 1, c & 1) along (i, j, k); case = bit mask of the inside corners.",
             "// edge e = 4 * axis + q: along `axis` from the base corner kMcEdgeBase[e] (its offset, packed like a corner index).",
             f"// The largest number of triangles of any case is {max_tris}.",
             "#pragma once",
             "#include <stdint.h>",
             "",
             f"#define DM4D_MC_MAX_TRIS {max_tris}",
             "",
             "static __device__ const int8_t kMcEdgeBase[12] = {" + ", ".join(str(corner_index(b)) for b in EDGE_BASE) + "};",
             "static __device__ const int8_t kMcEdgeAxis[12] = {" + ", ".join(str(a) for a in EDGE_AXIS) + "};",
             "",
             "static __device__ const int8_t kMcTriCount[256] = {"]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(int(x)) for x in count[r:r + 32]) + ",")
    lines += ["};", "", "// edge indices of the triangles of every case, three per triangle, -1 past the case's count",
              "static __device__ const int8_t kMcTris[256][DM4D_MC_MAX_TRIS * 3] = {"]
    for c in range(256):
        lines.append("    {" + ", ".join(f"{int(x):2d}" for x in table[c].reshape(-1)) + "},")
    lines += ["};", ""]
    return "\n".join(lines)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    text = render_header()
    if "--check" in argv:
        with open(HEADER_PATH) as fh:
            same = fh.read() == text
        print("mc_table.h is up to date" if same else "mc_table.h differs from the generator's output")
        return 0 if same else 1
    with open(HEADER_PATH, "w") as fh:
        fh.write(text)
    _, _, max_tris = build_table()
    print(f"wrote {HEADER_PATH}: 256 cases, at most {max_tris} triangles per case")
    return 0


if __name__ == "__main__":
    sys.exit(main())
