"""Marching-cubes triangulation table, generated from a stated rule (DESIGN.md section "Mesh extraction").

    python -m nerf_signature_amd.mc_table            # print the maximum triangle count and check the header
    python -m nerf_signature_amd.mc_table --write    # regenerate csrc/mc_tables.h

The header is data and is never edited by hand.  The rule:

- A lattice node is inside when value > threshold; anything else (NaN included) is outside.
- An edge crosses when exactly one of its two ends is inside.
- Face rule: a face with 2 crossings gets one segment; a face with 4 (the checkerboard) gets two, each cutting off one inside corner --
  the two inside corners are never joined across the face diagonal.  The rule reads only the face's 4 corner signs, so the two cells that
  share a face draw the same segments, and the mesh is watertight by construction.
- Orientation: each segment is directed so that, seen from outside the cube, the inside corner it cuts off (a 2-crossing face: any of
  its inside corners) lies on its right.  Every crossing then has one incoming and one outgoing segment, the segments chain into
  closed loops, and every triangle's normal (b-a) x (c-a) points from inside to outside: toward decreasing density.
- Loops are ordered by their lowest edge number.  Each is fan-triangulated from its apex: the lowest-numbered crossing from which no fan
  diagonal (an apex-to-vertex edge that is not a loop segment) joins two crossings on one cube face.  Such a diagonal would lie in the
  face, where the neighbouring cell can draw it too, and the edge would then belong to 4 triangles.
"""
import os
import sys

import numpy as np

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "mc_tables.h")

# corner c = x + 2 y + 4 z: its offset from the cell's min corner
CORNERS = [(c & 1, (c >> 1) & 1, (c >> 2) & 1) for c in range(8)]


def _edges():
    """Edge e: (axis, start corner).  x edges 0..3 at (y, z) = e & 1, e >> 1; y edges 4..7 at (x, z); z edges 8..11 at (x, y).
    Edge e runs from its start corner one step along +axis: it is the `axis` edge owned by the lattice node at the start corner."""
    out = []
    for axis in range(3):
        o1, o2 = [a for a in range(3) if a != axis]
        for e in range(4):
            p = [0, 0, 0]
            p[o1], p[o2] = e & 1, e >> 1
            out.append((axis, p[0] + 2 * p[1] + 4 * p[2]))
    return out


EDGES = _edges()
EDGE_CORNERS = [(c, c | (1 << axis)) for axis, c in EDGES]


def _faces():
    """Face f = 2 axis + side: the cube face at coordinate `side` along `axis`; (its 4 corners, its 4 edges, outward normal)."""
    out = []
    for axis in range(3):
        for side in range(2):
            corners = [c for c in range(8) if CORNERS[c][axis] == side]
            edges = [e for e, (a, b) in enumerate(EDGE_CORNERS) if a in corners and b in corners]
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            out.append((corners, edges, np.array(n, np.float64)))
    return out


FACES = _faces()
EDGE_FACES = [frozenset(f for f, (_, edges, _) in enumerate(FACES) if e in edges) for e in range(12)]


def _mid(e):
    a, b = EDGE_CORNERS[e]
    return (np.array(CORNERS[a], np.float64) + np.array(CORNERS[b], np.float64)) / 2


def _directed(p, q, corner, normal):
    """(p, q) ordered so that `corner` lies on the right of p -> q seen from outside (along -normal)."""
    side = np.dot(np.cross(_mid(q) - _mid(p), np.array(CORNERS[corner], np.float64) - _mid(p)), normal)
    return (p, q) if side < 0 else (q, p)


def face_segments(case):
    """Directed segments (edge, edge) the face rule draws on the 6 faces of the cell of `case` (bit c: corner c inside)."""
    inside = [(case >> c) & 1 for c in range(8)]
    segs = []
    for corners, edges, normal in FACES:
        cross = [e for e in edges if inside[EDGE_CORNERS[e][0]] != inside[EDGE_CORNERS[e][1]]]
        if len(cross) == 2:
            corner = next(c for c in corners if inside[c])
            segs.append(_directed(cross[0], cross[1], corner, normal))
        elif len(cross) == 4:
            for c in corners:
                if inside[c]:
                    pair = [e for e in edges if c in EDGE_CORNERS[e]]
                    segs.append(_directed(pair[0], pair[1], c, normal))
    return segs


def loops(case):
    """The closed loops of the face segments, each as its edge sequence in segment direction from its lowest edge, ordered by that edge."""
    nxt = {}
    for p, q in face_segments(case):
        assert p not in nxt, (case, p)
        nxt[p] = q
    out, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start, (case, loop)
        out.append(loop)
    return out


def _fan_ok(loop, k):
    """True when no diagonal of the fan from loop[k] joins two crossings of one cube face."""
    n = len(loop)
    a = loop[k]
    return all(not (EDGE_FACES[a] & EDGE_FACES[loop[(k + i) % n]]) for i in range(2, n - 1))


def triangles(case):
    """The case's triangles as edge triples, loop by loop, each loop fanned from its apex."""
    tris = []
    for loop in loops(case):
        n = len(loop)
        apex = min((loop[k] for k in range(n) if _fan_ok(loop, k)), default=None)
        assert apex is not None, f"case {case}: no valid apex for loop {loop}"
        k = loop.index(apex)
        ring = loop[k:] + loop[:k]
        tris += [(ring[0], ring[i], ring[i + 1]) for i in range(1, n - 1)]
    return tris


def table():
    """[256] lists of edge triples."""
    return [triangles(case) for case in range(256)]


def render():
    tab = table()
    mx = max(len(t) for t in tab)
    lines = [
        "// GENERATED by `python -m nerf_signature_amd.mc_table --write` -- do not edit.  The rule is stated in nerf_signature_amd/mc_table.py.",
        "//",
        "// Corner c of a cell is at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) from its min corner; the case index has bit c set when corner c",
        "// is inside (value > threshold).  Edge e runs from corner mc_edge_corner[e] one step along axis mc_edge_axis[e] (0 = x, 1 = y, 2 = z):",
    ]
    for e, (axis, c) in enumerate(EDGES):
        lines.append(f"//   edge {e:2d}: corners {EDGE_CORNERS[e][0]} -> {EDGE_CORNERS[e][1]}, axis {'xyz'[axis]}")
    lines += [
        "// It is the `axis` edge owned by the lattice node at that corner.  Per case: mc_tri_count triangles, whose edge triples are",
        "// mc_tri_edges[case][3 t .. 3 t + 2] (unused slots -1); every triangle's normal (b-a) x (c-a) points from inside to outside.",
        "#pragma once",
        "",
        "#include <stdint.h>",
        "",
        f"#define MC_MAX_TRIS {mx}",
        "",
        "static constexpr int8_t mc_edge_corner[12] = {" + ", ".join(str(c) for _, c in EDGES) + "};",
        "static constexpr int8_t mc_edge_axis[12] = {" + ", ".join(str(a) for a, _ in EDGES) + "};",
        "",
        "static constexpr uint8_t mc_tri_count[256] = {",
    ]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(len(t)) for t in tab[r:r + 32]) + ",")
    lines += ["};", "", f"static constexpr int8_t mc_tri_edges[256][3 * MC_MAX_TRIS] = {{"]
    for case, t in enumerate(tab):
        flat = [e for tri in t for e in tri] + [-1] * (3 * (mx - len(t)))
        lines.append("    {" + ", ".join(str(e) for e in flat) + f"}},  // {case}")
    lines += ["};", ""]
    return "\n".join(lines), mx


def main(argv):
    text, mx = render()
    print(f"maximum triangles per cell: {mx}")
    if "--write" in argv:
        with open(HEADER, "w") as f:
            f.write(text)
        print(f"wrote {HEADER}")
        return 0
    same = os.path.exists(HEADER) and open(HEADER).read() == text
    print(f"{HEADER} is {'up to date' if same else 'STALE: rerun with --write'}")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
