"""Case tables of the isosurface (256 cube cases) and contour (16 square cases) kernels, generated from one face rule.

Numbering (shared by the kernels, aegolius_amd.mesh and the tests):
  3-D corner c = dx << 2 | dy << 1 | dz: the point at offset (dx, dy, dz) from the cell's minimum corner, so corner order
      is linear-index order. Case index = sum of 1 << c over the INSIDE corners (f <= level).
  3-D edge e = 4 a + (u << 1 | v): the edge along axis a whose lower corner sits at offset u on the first and v on the
      second of the two other axes (in increasing axis order). Its vertex belongs to that lower corner's point, axis a.
  2-D corner c = dx << 1 | dy; 2-D edge e = 2 a + u, u the offset on the other axis.

The face rule: a square face (or the 2-D cell) with corners c0..c3 in counter-clockwise order (seen from outside the
cube) has an "exit" edge E_i = (c_i, c_{i+1}) where c_i is inside and c_{i+1} outside, and an "entry" edge where it is
the other way round. Each exit is joined to the nearest entry found walking the cycle backwards from it. With two
crossings that is the only pairing; with four (diagonal corners inside) it cuts each inside corner off by itself, so the
two inside corners are separated. The rule reads the face's four corners only, so two cells that share a face draw the
same segments on it (in opposite directions): the mesh is watertight.

A segment exit -> entry has the inside on its left. In 2-D that is the contour's orientation. In 3-D the face segments
are taken entry -> exit (inside on the right, seen from outside the cube); they chain into loops on the cube's surface,
each loop is fan-triangulated from its lowest-numbered edge (the lowest one whose fan draws no diagonal inside a
cube face, for the 18 cases where the lowest edge's fan would: see _fan_apex), and every triangle (v0, v1, v2) then has
(v1 - v0) x (v2 - v0) pointing from the inside corners to the outside ones: toward increasing f.

Run as a script (or through write_inc) to emit csrc/sdfk_mesh_table.inc for the kernels' constant memory.
"""
import os
import sys


def corner_offset3(c):
    return ((c >> 2) & 1, (c >> 1) & 1, c & 1)


def _others(a):
    return [x for x in range(3) if x != a]


def edge_corners3(e):
    """(lower corner, upper corner) of cube edge e."""
    a, r = divmod(e, 4)
    o1, o2 = _others(a)
    d = [0, 0, 0]
    d[o1], d[o2] = (r >> 1) & 1, r & 1
    lo = d[0] << 2 | d[1] << 1 | d[2]
    return lo, lo | (1 << (2 - a))


def edge_axis3(e):
    return e // 4


def _edge_between3(c0, c1):
    diff = c0 ^ c1
    a = {4: 0, 2: 1, 1: 2}[diff]
    lo = min(c0, c1)
    d = corner_offset3(lo)
    o1, o2 = _others(a)
    return 4 * a + (d[o1] << 1 | d[o2])


def faces3():
    """The 6 faces as (axis, side, corner cycle counter-clockwise seen from outside the cube)."""
    out = []
    for a in range(3):
        p, q = _others(a)
        for s in (0, 1):
            cyc = []
            for up, uq in ((0, 0), (1, 0), (1, 1), (0, 1)):
                d = [0, 0, 0]
                d[a], d[p], d[q] = s, up, uq
                cyc.append(d[0] << 2 | d[1] << 1 | d[2])
            # the cycle's normal is e_p x e_q = +e_a for (p, q) = (1, 2), (0, 1) and -e_a for (0, 2); outward is (2s-1) e_a
            sign = -1 if (p, q) == (0, 2) else 1
            if sign != (2 * s - 1):
                cyc = [cyc[0], cyc[3], cyc[2], cyc[1]]
            out.append((a, s, cyc))
    return out


def face_rule(inside):
    """inside: 4 booleans of a counter-clockwise corner cycle -> [(exit i, entry j)] edge positions (E_i = (c_i, c_i+1)),
    the segment exit -> entry having the inside on its left."""
    ex = [inside[i] and not inside[(i + 1) % 4] for i in range(4)]
    en = [not inside[i] and inside[(i + 1) % 4] for i in range(4)]
    segs = []
    for i in range(4):
        if ex[i]:
            j = (i - 1) % 4
            while not en[j]:
                j = (j - 1) % 4
            segs.append((i, j))
    return segs


def face_segments3(case):
    """Directed segments (from edge, to edge) the case draws on each of the 6 faces, entry -> exit: a list per face."""
    out = []
    for a, s, cyc in faces3():
        ins = [bool(case >> c & 1) for c in cyc]
        edges = [_edge_between3(cyc[i], cyc[(i + 1) % 4]) for i in range(4)]
        out.append([(edges[j], edges[i]) for i, j in face_rule(ins)])
    return out


_FACE_EDGES = [{_edge_between3(cyc[i], cyc[(i + 1) % 4]) for i in range(4)} for _, _, cyc in faces3()]


def loops3(case):
    nxt = {}
    for segs in face_segments3(case):
        for u, v in segs:
            assert u not in nxt
            nxt[u] = v
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        loops.append(loop)
    return loops


def _face_diagonal(u, v):
    """Do edges u and v lie on one cube face? (A fan diagonal between them would lie in that face.)"""
    return any(u in fe and v in fe for fe in _FACE_EDGES)


def _fan_apex(loop):
    """The loop's lowest-numbered edge whose fan has no diagonal inside a cube face. Such a diagonal is not one of the
    face's segments, and the neighbouring cell may draw the same one: the edge would then belong to four triangles. For
    238 of the 256 cases the lowest-numbered edge itself qualifies; one always does."""
    m = len(loop)
    for apex in sorted(loop):
        k = loop.index(apex)
        if not any(_face_diagonal(apex, loop[(k + j) % m]) for j in range(2, m - 1)):
            return k
    raise AssertionError("no fan apex for loop %r" % (loop,))


def triangles3(case):
    """Triangles of one cube case as edge triples, in table order: per loop (in the order of their lowest edges) a fan
    from its apex (_fan_apex), following the loop."""
    tris = []
    for loop in loops3(case):
        k = _fan_apex(loop)
        ring = loop[k:] + loop[:k]
        for j in range(1, len(ring) - 1):
            tris.append((ring[0], ring[j], ring[j + 1]))
    return tris


def crossing_edges3(case):
    return sorted(e for e in range(12) if (case >> edge_corners3(e)[0] & 1) != (case >> edge_corners3(e)[1] & 1))


# ---- 2-D --------------------------------------------------------------------------------------------------------------
SQUARE_CYCLE = (0, 2, 3, 1)     # corners (0,0), (1,0), (1,1), (0,1): counter-clockwise in the (x, y) plane


def edge_corners2(e):
    a, u = divmod(e, 2)
    lo = (u if a == 1 else 0) << 1 | (u if a == 0 else 0)
    return lo, lo | (1 << (1 - a))


def _edge_between2(c0, c1):
    a = 0 if (c0 ^ c1) == 2 else 1
    lo = min(c0, c1)
    return 2 * a + ((lo & 1) if a == 0 else (lo >> 1))


def segments2(case):
    """Directed segments (from edge, to edge) of one square case, inside on the left, ordered by their first edge."""
    ins = [bool(case >> c & 1) for c in SQUARE_CYCLE]
    edges = [_edge_between2(SQUARE_CYCLE[i], SQUARE_CYCLE[(i + 1) % 4]) for i in range(4)]
    return sorted((edges[i], edges[j]) for i, j in face_rule(ins))


# ---- tables -----------------------------------------------------------------------------------------------------------
_TABLES = None


def tables():
    """dict: tri (256 lists of edge triples), tmax, seg (16 lists of edge pairs), smax."""
    global _TABLES
    if _TABLES is None:
        tri = [triangles3(c) for c in range(256)]
        seg = [segments2(c) for c in range(16)]
        _TABLES = dict(tri=tri, tmax=max(len(t) for t in tri), seg=seg, smax=max(len(s) for s in seg))
    return _TABLES


def inc_text():
    t = tables()
    tmax, smax = t["tmax"], t["smax"]
    lines = ["// generated by aegolius_amd/_mctable.py - do not edit",
             "#define SDFK_MC_TMAX %d" % tmax, "#define SDFK_MS_SMAX %d" % smax,
             "static __constant__ unsigned char sdfk_mc_ntri[256] = {%s};" % ", ".join(str(len(x)) for x in t["tri"]),
             "static __constant__ unsigned char sdfk_mc_tri[256][%d] = {" % (3 * tmax)]
    for x in t["tri"]:
        flat = [e for tr in x for e in tr] + [0] * (3 * (tmax - len(x)))
        lines.append("    {%s}," % ", ".join(map(str, flat)))
    lines.append("};")
    lines.append("static __constant__ unsigned char sdfk_ms_nseg[16] = {%s};" % ", ".join(str(len(x)) for x in t["seg"]))
    lines.append("static __constant__ unsigned char sdfk_ms_seg[16][%d] = {" % (2 * smax))
    for x in t["seg"]:
        flat = [e for s in x for e in s] + [0] * (2 * (smax - len(x)))
        lines.append("    {%s}," % ", ".join(map(str, flat)))
    lines.append("};")
    return "\n".join(lines) + "\n"


def write_inc(out_path):
    new = inc_text()
    if not os.path.exists(out_path) or open(out_path).read() != new:
        with open(out_path, "w") as f:
            f.write(new)
    return out_path


if __name__ == "__main__":
    write_inc(sys.argv[1] if len(sys.argv) > 1 else
              os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "sdfk_mesh_table.inc"))
