"""Writes sdfest_amd/csrc/mesh_tables.hpp: the marching-cubes case tables of sdfest_amd/csrc/mesh.hip.

    python tools/gen_mesh_tables.py            (re-writes the header; it is committed)

Conventions
  corner c = dx + 2 dy + 4 dz     (dx along grid axis 0 = i, dy along 1 = j, dz along 2 = k)
  edge   e = 4 a + (the two other offsets, the lower axis first)   for the edge along axis a
  case     = sum over the corners of (v_c < level) << c            ("inside" = below the level)

The tables are DERIVED, not typed in.  On each of the cube's six faces the crossed edges are joined by segments that
depend on that face's four corner signs alone: an unambiguous face has one segment; an ambiguous face (the two
inside corners on a diagonal) cuts every inside corner off on its own, i.e. the OUTSIDE corners connect across the
face.  Each segment is directed so that, seen from outside the cube, the inside corner lies on its right; the
neighbouring cube sees the same face from the other side and so the same segment reversed.  The segments of a case
chain into closed loops on the cube's surface (every crossed edge lies on two faces: one segment in, one out), and
each loop is fanned from its lowest-numbered edge.  The fan keeps the loop's direction, which makes
(b - a) x (c - a) point toward increasing SDF.  tests/test_mesh_cpu.py checks all of this case by case.
"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "sdfest_amd", "csrc", "mesh_tables.hpp")


def corner_pos(c):
    return (c & 1, (c >> 1) & 1, (c >> 2) & 1)


def edges():
    """[(corner0, corner1, axis)] by edge id"""
    out = []
    for a in range(3):
        others = [b for b in range(3) if b != a]
        for m in range(4):
            off = [0, 0, 0]
            off[others[0]] = m & 1
            off[others[1]] = (m >> 1) & 1
            c0 = off[0] + 2 * off[1] + 4 * off[2]
            out.append((c0, c0 | (1 << a), a))
    return out


EDGES = edges()


def faces():
    """[(axis, side, corners in cyclic order)]: the face at coordinate `side` of `axis`"""
    out = []
    for a in range(3):
        b, c = [x for x in range(3) if x != a]
        for side in (0, 1):
            cyc = []
            for (ob, oc) in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[a], off[b], off[c] = side, ob, oc
                cyc.append(off[0] + 2 * off[1] + 4 * off[2])
            out.append((a, side, cyc))
    return out


FACES = faces()


def edge_id(c0, c1):
    for e, (a0, a1, _) in enumerate(EDGES):
        if {a0, a1} == {c0, c1}:
            return e
    raise KeyError((c0, c1))


def mid(e):
    c0, c1, _ = EDGES[e]
    p0, p1 = corner_pos(c0), corner_pos(c1)
    return tuple(0.5 * (x + y) for x, y in zip(p0, p1))


def sub(p, q):
    return tuple(x - y for x, y in zip(p, q))


def crossp(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def dotp(u, v):
    return sum(x * y for x, y in zip(u, v))


def face_segments(case, face):
    """the directed segments (edge_from, edge_to) of one face of one case"""
    a, side, cyc = face
    normal = [0, 0, 0]
    normal[a] = 1 if side else -1
    ins = [(case >> c) & 1 for c in cyc]
    fe = [edge_id(cyc[i], cyc[(i + 1) % 4]) for i in range(4)]   # face edge i joins cyc[i] and cyc[i+1]
    segs = []
    # every inside corner whose two face edges are both crossed is cut off on its own (covers one inside corner and
    # the ambiguous diagonal); otherwise the one pair of crossed edges is joined
    crossed = [i for i in range(4) if ins[i] != ins[(i + 1) % 4]]
    if not crossed:
        return []
    pairs = []
    if len(crossed) == 4:
        for i in range(4):
            if ins[i]:
                pairs.append(((i - 1) % 4, i, i))          # edges before and after inside corner i
    else:
        assert len(crossed) == 2
        inside_corner = next(i for i in range(4) if ins[i])
        pairs.append((crossed[0], crossed[1], inside_corner))
    for (i, j, k) in pairs:
        e0, e1 = fe[i], fe[j]
        p, q, ic = mid(e0), mid(e1), corner_pos(cyc[k])
        s = dotp(crossp(sub(q, p), sub(ic, p)), normal)
        assert s != 0
        segs.append((e0, e1) if s < 0 else (e1, e0))
    return segs


def case_triangles(case):
    nxt = {}
    for f in FACES:
        for (u, v) in face_segments(case, f):
            assert u not in nxt
            nxt[u] = v
    tris = []
    todo = set(nxt)
    while todo:
        start = min(todo)
        loop = [start]
        while nxt[loop[-1]] != start:
            loop.append(nxt[loop[-1]])
        todo -= set(loop)
        for i in range(1, len(loop) - 1):
            tris.append((loop[0], loop[i], loop[i + 1]))
    return tris


def tables():
    edge_mask, tri = [], []
    for case in range(256):
        m = 0
        for e, (c0, c1, _) in enumerate(EDGES):
            if ((case >> c0) & 1) != ((case >> c1) & 1):
                m |= 1 << e
        edge_mask.append(m)
        t = [v for tr in case_triangles(case) for v in tr]
        assert len(t) <= 15, (case, len(t))
        tri.append(t + [-1] * (16 - len(t)))
    return edge_mask, tri


def main():
    edge_mask, tri = tables()
    lines = [
        "// mesh_tables.hpp -- marching-cubes case tables of mesh.hip (host and device).",
        "// GENERATED by tools/gen_mesh_tables.py: edit that script, not this file.  Corner c = dx + 2 dy + 4 dz,",
        "// edge e = 4 a + (the two other offsets, lower axis first) along axis a, case bit c = (v_c < level).",
        "// Ambiguous faces: every inside corner is cut off on its own (the outside corners connect across the face).",
        "#pragma once",
        "",
        "namespace sdfr {",
        "namespace mesh {",
        "",
        "// the corners (0 / 1 offsets along the three axes) of edge e",
        "constexpr unsigned char kEdgeCorner0[12] = {" + ", ".join(str(c0) for c0, _, _ in EDGES) + "};",
        "constexpr unsigned char kEdgeAxis[12] = {" + ", ".join(str(a) for _, _, a in EDGES) + "};",
        "",
        "// bit e set = edge e is crossed",
        "constexpr unsigned short kEdgeMask[256] = {",
    ]
    for r in range(0, 256, 16):
        lines.append("    " + ", ".join(f"0x{m:03x}" for m in edge_mask[r:r + 16]) + ",")
    lines += ["};", "", "// up to 5 triangles as edge triples, -1 terminated",
              "constexpr signed char kTriTable[256][16] = {"]
    for case in range(256):
        lines.append("    {" + ", ".join(str(v) for v in tri[case]) + "},")
    lines += ["};", "", "// triangles per case", "constexpr unsigned char kTriCount[256] = {"]
    ntri = [sum(1 for v in t if v >= 0) // 3 for t in tri]
    for r in range(0, 256, 32):
        lines.append("    " + ", ".join(str(n) for n in ntri[r:r + 32]) + ",")
    lines += ["};", "", "}  // namespace mesh", "}  // namespace sdfr", ""]
    with open(OUT, "w") as f:
        f.write("\n".join(lines))
    print(f"wrote {OUT}: max {max(ntri)} triangles per case")


if __name__ == "__main__":
    main()
