"""Host restatement of the reference's mesh densification (densify/utils.py: densify, pushAndSort), and the synthetic
meshes the densification tests, the F17 fixture and tools/bench_densify.py use.

oracle_densify restates the split from the per-edge face lists documented in include/dpc_render.h, and pops edges from
a heap keyed (-length, edge index): the reference keeps a list sorted by length that inserts after every edge of equal
length, with a stable initial sort, so its pop order is exactly that total order.  Lengths are np.linalg.norm(V[lo] - V[hi]) as
numpy computes it with OpenBLAS, sqrt(fma(dz, dz, fma(dy, dy, dx * dx))), with the fma done exactly in integers so the
oracle does not depend on the host's BLAS.
"""
import heapq
import math
from fractions import Fraction

import numpy as np


def _sq_fma(d, c):
    """fma(d, d, c) for finite d and c >= 0, correctly rounded."""
    md, ed = math.frexp(d)
    mc, ec = math.frexp(c)
    a, b = int(md * 9007199254740992.0), int(mc * 9007199254740992.0)  # exact 53-bit integers
    ep, ec = 2 * (ed - 53), ec - 53
    e = min(ep, ec) if c else ep
    n = ((a * a) << (ep - e)) + ((b << (ec - e)) if c else 0)
    try:
        return math.ldexp(float(n), e)  # int -> float rounds to nearest even; the scaling is exact for normal results
    except OverflowError:
        return float(Fraction(d) * Fraction(d) + Fraction(c))


def edge_length(p, q):
    """np.linalg.norm(p - q) for 3-vectors: sqrt(fma(dz, dz, fma(dy, dy, dx * dx)))."""
    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return math.sqrt(_sq_fma(dz, _sq_fma(dy, dx * dx)))


def oracle_densify(V, E, F, n, record=False):
    """densify_single.py's "points" for a mesh (V, E, F) as load_obj_mesh returns it: V followed by n midpoints.

    Restated from the semantics documented in include/dpc_render.h (dpc_densify): every edge keeps an ordered list of
    the faces on it.  Initially the lists are in ascending face order.  Splitting edge (a, b) appends the midpoint m and
    the edges [a, m], [b, m]; then, for each face on the edge in list order, with o its third vertex, the faces
    (a, o, m) and (b, o, m) take the old face's place in the lists of edges (a, o) and (b, o), are appended to the lists
    of [a, m] and [b, m] respectively, and the new median edge [o, m] gets the list [(a, o, m), (b, o, m)].

    With record=True also returns (pops, children): the length of every popped edge in pop order, and for every split
    the list of (child length, parent length) of the edges it created."""
    pts = [tuple(float(x) for x in row) for row in np.asarray(V, dtype=np.float64)]
    ends, length, faces_on = [], [], []
    by_pair = {}  # unordered vertex pair of a live edge -> its id
    heap = []

    def new_edge(p, q, faces):
        eid = len(ends)
        ends.append((p, q))
        length.append(edge_length(pts[p], pts[q]))
        faces_on.append(faces)
        by_pair[frozenset((p, q))] = eid
        heapq.heappush(heap, (-length[eid], eid))  # pop order: longest first, then lowest id
        return eid

    for p, q in np.asarray(E).reshape(-1, 2).tolist():
        new_edge(int(p), int(q), [])
    tris = [tuple(int(x) for x in t) for t in np.asarray(F).reshape(-1, 3)]
    for fid, t in enumerate(tris):
        for x, y in ((t[0], t[1]), (t[0], t[2]), (t[1], t[2])):
            faces_on[by_pair[frozenset((x, y))]].append(fid)

    pops, children = [], []
    for _ in range(n):
        _, e = heapq.heappop(heap)
        a, b = ends[e]
        del by_pair[frozenset((a, b))]
        m = len(pts)
        pts.append(tuple((pts[a][k] + pts[b][k]) / 2 for k in range(3)))
        first = len(ends)
        side_a = new_edge(a, m, [])
        side_b = new_edge(b, m, [])
        for fid in faces_on[e]:
            t = tris[fid]
            (o,) = set(t) - {a, b}
            fa, fb = len(tris), len(tris) + 1
            tris.append(tuple(m if x == b else x for x in t))
            tris.append(tuple(m if x == a else x for x in t))
            for other, sub in ((a, fa), (b, fb)):
                lst = faces_on[by_pair[frozenset((other, o))]]
                lst[lst.index(fid)] = sub
            faces_on[side_a].append(fa)
            faces_on[side_b].append(fb)
            new_edge(o, m, [fa, fb])
        if record:
            pops.append(length[e])
            children.append([(length[c], length[e]) for c in range(first, len(ends))])
    out = np.array(pts, dtype=np.float64)
    return (out, pops, children) if record else out


# ---------------------------------------------------------------------------------------------------------------------
# synthetic .obj texts


def _obj(V, F, extra=""):
    lines = ["v %r %r %r" % tuple(float(x) for x in v) for v in V]
    lines += ["f %d %d %d" % tuple(int(i) + 1 for i in f) for f in F]
    return "# synthetic mesh\n" + extra + "\n".join(lines) + "\n"


def sphere_box_obj(n_lat=12, n_lon=16, box=(0.25, 0.5, 0.75), box_div=1, center=(0.13, 0.07, 0.21)):
    """A UV sphere (n_lat bands, n_lon sectors, radius 0.4 around `center`) and an axis-aligned box whose sides are
    split into box_div x box_div squares of two triangles: many edges of exactly equal length."""
    V, F = [], []
    cx, cy, cz = center
    V.append((cx, cy, cz + 0.4))
    for i in range(1, n_lat):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * math.pi * j / n_lon
            V.append((cx + 0.4 * math.sin(th) * math.cos(ph), cy + 0.4 * math.sin(th) * math.sin(ph), cz + 0.4 * math.cos(th)))
    V.append((cx, cy, cz - 0.4))
    ring = lambda i, j: 1 + (i - 1) * n_lon + (j % n_lon)
    for j in range(n_lon):
        F.append((0, ring(1, j), ring(1, j + 1)))
        F.append((len(V) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            F.append((ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)))
            F.append((ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)))
    # the box [0.7, 0.7 + bx] x [-0.3, -0.3 + by] x [0.1, 0.1 + bz], each side a box_div x box_div grid
    lo, size = np.array([0.7, -0.3, 0.1]), np.array(box)
    for axis in range(3):
        u, w = [a for a in range(3) if a != axis]
        for side in (0, 1):
            base = len(V)
            for a in range(box_div + 1):
                for b in range(box_div + 1):
                    p = lo.copy()
                    p[axis] += side * size[axis]
                    p[u] += size[u] * a / box_div
                    p[w] += size[w] * b / box_div
                    V.append(tuple(p))
            idx = lambda a, b: base + a * (box_div + 1) + b
            for a in range(box_div):
                for b in range(box_div):
                    F.append((idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)))
                    F.append((idx(a, b), idx(a + 1, b + 1), idx(a, b + 1)))
    # shared box-side vertices are duplicated; that keeps the sides separate components, as many ShapeNet files do
    return _obj(V, F)


def icosphere_obj(level=1, radius=0.5, center=(0.11, -0.05, 0.23)):
    """A subdivided icosahedron projected to a sphere: near-equilateral faces, so a round's band often holds two or three
    edges of one face."""
    t = (1 + 5 ** 0.5) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    V = [np.array(v, dtype=np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(level):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = V[a] + V[b]
                V.append(m / np.linalg.norm(m))
                cache[k] = len(V) - 1
            return cache[k]

        for a, b, c in F:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = nf
    return _obj([tuple(np.array(center) + radius * v) for v in V], F)


def grid_obj(nx, ny, z=0.5):
    """nx x ny unit squares in the plane z (off the origin, so every face has rank 3), each cut into two triangles: the
    sides all tie at length 1 and the diagonals at sqrt(2)."""
    V = [(float(i), float(j), z) for i in range(nx + 1) for j in range(ny + 1)]
    idx = lambda i, j: i * (ny + 1) + j
    F = []
    for i in range(nx):
        for j in range(ny):
            F.append((idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)))
            F.append((idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)))
    return _obj(V, F)


# A file with the reference parser's corner cases: comments, a material line, vn / vt lines, "f a/b/c" and "f a//c"
# forms, a quad (its fourth index is ignored), edge 1-2 on three faces (non-manifold), face 1 2 3 repeated in another
# order (dropped as a duplicate), a degenerate face (2 2 3), a face through the origin (7 8 9: rank 2) and a face in a
# plane through the origin (10 11 12: z = 0), and vertex 6, which no face uses.
MESSY_OBJ = """# messy mesh
mtllib messy.mtl
o part
v 0.1 0.2 0.3
v 1.0 0.1 0.2
v 0.2 1.1 0.3
v 0.3 0.2 1.4
v 1.2 1.3 0.1
v 5.0 5.0 5.0
v 0.0 0.0 0.0
v 2.0 2.0 2.0
v 0.5 -1.0 0.25
v 1.0 0.0 0.0
v 0.0 1.0 0.0
v 1.0 1.0 0.0
vn 0.0 0.0 1.0
vt 0.5 0.5
usemtl m
s off
f 1 2 3
f 1/1/1 2/1/1 4/1/1
f 1//1 2//1 5//1
f 3 2 1
f 1 3 4 5
f 2 2 3
f 7 8 9
f 10 11 12
f 4 5 3
"""

# Every face is the one triangle: removeWeirdDuplicate leaves no faces, the three edges stay.
ONE_TRIANGLE_OBJ = """v 0.1 0.2 0.3
v 1.0 0.1 0.2
v 0.2 1.1 0.3
f 1 2 3
f 2 3 1
"""
