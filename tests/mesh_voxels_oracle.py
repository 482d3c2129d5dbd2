"""Numpy definition of the mesh voxeliser of include/dpc_render.h (dpc_voxelise_meshes, dpc_voxel_carve): the surface
rule (closed cube against closed triangle by 13 separating axes), the two fills ("carve": what no axis direction sees
into; "parity": ray crossings along grid axis 0 with the top-left rule) and the counts, plus the seeded meshes the tests
and the fixture tests/golden/f26_mesh_voxels.npz share.

Everything is elementwise fp64 with every operation written out in the order the kernels use (csrc/dpc_mesh_voxels.hip):
no dot products, no fused multiply-add, so each bit has one right answer.  The arrays only batch the same scalar formula
over the candidate nodes (or columns) of ONE face; faces are walked one by one."""
import numpy as np

from voxels_oracle import pack_bits, shape_of  # noqa: F401  (the bit layout and the grid of a config are shared)

FILLS = ("none", "carve", "parity")
STATUS_BAD_INDEX, STATUS_NONFINITE = 1, 8
MAX_COORD = 2.0 ** 64        # DPC_MESH_VOXEL_MAX_COORD: a coordinate of that size or beyond counts as not finite


def grid_coordinates(V, shape):
    """u_c = (v_c + 0.5) * (G_c - 1) in fp64 (fp32 vertices widen exactly)."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    g1 = np.array([shape[0] - 1, shape[1] - 1, shape[2] - 1], dtype=np.float64)
    return (v + 0.5) * g1


def _faces(V, F, shape):
    """([3,3] grid coordinates of every face that is kept, status bits, kept faces with a vertex outside the cube)."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    u = grid_coordinates(v, shape)
    F = np.asarray(F).reshape(-1, 3)
    out = []
    status = outside = 0
    for f in F:
        if (f < 0).any() or (f >= len(v)).any():
            status |= STATUS_BAD_INDEX
            continue
        p = v[f]
        if not (np.abs(p) < MAX_COORD).all():                          # a NaN too
            status |= STATUS_NONFINITE
            continue
        if ((p < -0.5) | (p > 0.5)).any():
            outside += 1
        out.append(u[f])
    return out, status, outside


def _range(lo, hi, G):
    """Integer nodes a .. b (inclusive) of [lo, hi] clamped to 0 .. G - 1, compared as fp64 before any conversion."""
    a, b = max(lo, 0.0), min(hi, float(G - 1))
    return (int(a), int(b)) if a <= b else (0, -1)


def _min3(a, b, c):
    return np.minimum(np.minimum(a, b), c)


def _max3(a, b, c):
    return np.maximum(np.maximum(a, b), c)


def face_nodes(u, shape):
    """The nodes [k,3] (int64) whose closed cube of half-size 1/2 meets the closed triangle u [3,3] (grid coordinates)."""
    r = []
    for c in range(3):
        lo, hi = min(min(u[0, c], u[1, c]), u[2, c]), max(max(u[0, c], u[1, c]), u[2, c])
        r.append(_range(np.ceil(lo - 0.5), np.floor(hi + 0.5), shape[c]))
    if any(b < a for a, b in r):
        return np.zeros((0, 3), dtype=np.int64)
    n = np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in r], indexing="ij"), axis=-1).reshape(-1, 3)
    nf = n.astype(np.float64)
    # the vertices translated to the node; the edges and the normal are the face's own (they do not move)
    p = [[u[v, c] - nf[:, c] for c in range(3)] for v in range(3)]
    e = [[u[1, c] - u[0, c] for c in range(3)], [u[2, c] - u[1, c] for c in range(3)], [u[0, c] - u[2, c] for c in range(3)]]
    nr = [e[0][1] * e[1][2] - e[0][2] * e[1][1], e[0][2] * e[1][0] - e[0][0] * e[1][2], e[0][0] * e[1][1] - e[0][1] * e[1][0]]
    sep = np.zeros(len(n), dtype=bool)
    for c in range(3):                                               # the box axes
        sep |= (_min3(p[0][c], p[1][c], p[2][c]) > 0.5) | (_max3(p[0][c], p[1][c], p[2][c]) < -0.5)
    d = (nr[0] * p[0][0] + nr[1] * p[0][1]) + nr[2] * p[0][2]        # the face normal
    rad = 0.5 * ((abs(nr[0]) + abs(nr[1])) + abs(nr[2]))
    sep |= (d > rad) | (d < -rad)
    for k in range(3):                                               # edge x box axis: axis k, components i and j
        i, j = (k + 1) % 3, (k + 2) % 3
        for ed in e:
            q = [ed[i] * p[v][j] - ed[j] * p[v][i] for v in range(3)]
            rad = 0.5 * (abs(ed[i]) + abs(ed[j]))
            sep |= (_min3(q[0], q[1], q[2]) > rad) | (_max3(q[0], q[1], q[2]) < -rad)
    return n[~sep]


def surface(V, F, shape):
    """(bool [D,H,W], status bits, kept faces with a vertex outside the cube)."""
    faces, status, outside = _faces(V, F, shape)
    grid = np.zeros(shape, dtype=bool)
    for u in faces:
        n = face_nodes(u, shape)
        grid[n[:, 0], n[:, 1], n[:, 2]] = True
    return grid, status, outside


def carve(grid):
    """A node stays iff every grid line through it has a set node at an index <= its own and one at an index >= its own."""
    g = np.asarray(grid, dtype=bool)
    out = np.ones(g.shape, dtype=bool)
    for ax in range(g.ndim - 3, g.ndim):
        before = np.logical_or.accumulate(g, axis=ax)
        after = np.flip(np.logical_or.accumulate(np.flip(g, axis=ax), axis=ax), axis=ax)
        out &= before & after
    return out


def _edge(P, Q, cy, cx):
    """The edge function of P -> Q at the columns (cy, cx), evaluated from the lexicographically smaller endpoint and
    negated when that is Q: two faces sharing the edge see equal or exactly opposite values."""
    swap = P[0] > Q[0] or (P[0] == Q[0] and P[1] > Q[1])
    A, B = (Q, P) if swap else (P, Q)
    val = (B[1] - A[1]) * (cy - A[0]) - (B[0] - A[0]) * (cx - A[1])
    return -val if swap else val


def face_crossings(u, shape):
    """(y [k], x [k], toggle plane [k] in 0 .. D) of the columns along axis 0 that the face u [3,3] crosses."""
    D, H, W = shape
    none = (np.zeros(0, dtype=np.int64),) * 3
    P = [(u[v, 1], u[v, 2]) for v in range(3)]
    z = [u[v, 0] for v in range(3)]
    area = _edge(P[0], P[1], np.float64(P[2][0]), np.float64(P[2][1]))
    if area == 0:
        return none
    neg = area < 0
    ya, yb = _range(np.ceil(min(min(P[0][0], P[1][0]), P[2][0])), np.floor(max(max(P[0][0], P[1][0]), P[2][0])), H)
    xa, xb = _range(np.ceil(min(min(P[0][1], P[1][1]), P[2][1])), np.floor(max(max(P[0][1], P[1][1]), P[2][1])), W)
    if yb < ya or xb < xa:
        return none
    cy, cx = (a.reshape(-1) for a in np.meshgrid(np.arange(ya, yb + 1), np.arange(xa, xb + 1), indexing="ij"))
    fy, fx = cy.astype(np.float64), cx.astype(np.float64)
    inside = np.ones(len(cy), dtype=bool)
    w = []
    for a, b in ((1, 2), (2, 0), (0, 1)):                            # w_v belongs to the edge opposite vertex v
        val = _edge(P[a], P[b], fy, fx)
        dy, dx = P[b][0] - P[a][0], P[b][1] - P[a][1]
        if neg:
            val, dy, dx = -val, -dy, -dx
        top_left = dy > 0 or (dy == 0 and dx < 0)
        inside &= (val > 0) | ((val == 0) & top_left)
        w.append(val)
    total = (w[0] + w[1]) + w[2]
    inside &= total != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        zs = ((w[0] * z[0] + w[1] * z[1]) + w[2] * z[2]) / total
    k = np.ceil(zs[inside])
    k = np.minimum(np.maximum(k, 0.0), float(D)).astype(np.int64)
    return cy[inside], cx[inside], k


def parity(V, F, shape):
    """(bool [D,H,W]: the prefix XOR along axis 0 of the crossings' toggles, open columns: those crossed an odd number
    of times)."""
    D, H, W = shape
    faces, _, _ = _faces(V, F, shape)
    toggles = np.zeros((D + 1, H, W), dtype=np.int64)
    for u in faces:
        y, x, k = face_crossings(u, shape)
        np.add.at(toggles, (k, y, x), 1)
    par = (np.cumsum(toggles[:D], axis=0) & 1).astype(bool)
    return par, int((toggles.sum(axis=0) & 1).sum())


def voxelise_mesh(V, F, shape, fill="carve"):
    """(bool [D,H,W], info [2] int32: (kept faces with a vertex outside the cube, open columns: 0 unless the fill is
    "parity"), status bits)."""
    if fill not in FILLS:
        raise ValueError("fill must be one of %s" % (FILLS,))
    s, status, outside = surface(V, F, shape)
    opened = 0
    if fill == "carve":
        s = carve(s)
    elif fill == "parity":
        par, opened = parity(V, F, shape)
        s = s | par
    return s, np.array([outside, opened], dtype=np.int32), status


# ---------------------------------------------------------------------------------------------------------------
# seeded meshes
def icosphere(subdivisions, radius=0.4, centre=(0.0, 0.0, 0.0), dtype=np.float64):
    """(V [n,3], F [20 * 4^s, 3] int32): a closed, consistently oriented sphere; shared vertices are shared."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, dtype=np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(subdivisions):
        mid, G = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = V[a] + V[b]
                V.append(p / np.linalg.norm(p))
                mid[key] = len(V) - 1
            return mid[key]

        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            G += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = G
    V = np.array(V) * radius + np.asarray(centre, dtype=np.float64)
    return V.astype(dtype), np.array(F, dtype=np.int32)


def hemisphere(subdivisions, radius=0.4, dtype=np.float64):
    """The faces of the icosphere whose centroid has a positive axis-0 coordinate: an open shell."""
    V, F = icosphere(subdivisions, radius, dtype=np.float64)
    keep = V[F][:, :, 0].mean(axis=1) > 0
    return V.astype(dtype), F[keep]


def box(lo, hi, dtype=np.float64):
    """An axis-aligned closed box of 12 outward-facing triangles, corners lo and hi ([3] each)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    V = np.array([[(lo, hi)[(i >> 2) & 1][0], (lo, hi)[(i >> 1) & 1][1], (lo, hi)[i & 1][2]] for i in range(8)])
    F = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return V.astype(dtype), np.array(F, dtype=np.int32)


def node_box(a, b, shape, dtype=np.float64):
    """The box whose faces pass through the node centres a and b ([3] node indices) of a grid."""
    g1 = np.array(shape, dtype=np.float64) - 1.0
    return box(np.asarray(a, dtype=np.float64) / g1 - 0.5, np.asarray(b, dtype=np.float64) / g1 - 0.5, dtype)


def soup(n, seed, size=0.02, dtype=np.float32):
    """n small triangles scattered through the cube (some poke out of it): (V [3n,3], F [n,3])."""
    rng = np.random.default_rng(seed)
    c = rng.random((n, 1, 3)) * 1.04 - 0.52
    V = (c + (rng.random((n, 3, 3)) - 0.5) * size).reshape(-1, 3)
    return V.astype(dtype), np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def join(*meshes):
    """One mesh of several (V, F): vertices concatenated, indices shifted."""
    Vs, Fs, o = [], [], 0
    for V, F in meshes:
        Vs.append(np.asarray(V))
        Fs.append(np.asarray(F).reshape(-1, 3) + o)
        o += len(V)
    return np.concatenate(Vs), np.concatenate(Fs).astype(np.int32)


def mixed_batch(dtype=np.float32, tiny=2000):
    """The batch of the GPU tests: no faces; one face; zero-area and repeated-vertex faces; a face spanning the grid among
    `tiny` small ones; faces partly and wholly outside the cube; a NaN vertex beside good faces."""
    d = dtype
    tri = (np.array([[-0.3, -0.2, -0.1], [0.25, 0.1, -0.2], [0.0, 0.3, 0.35]], dtype=d), np.array([[0, 1, 2]], dtype=np.int32))
    degenerate = (np.array([[-0.4, -0.4, -0.4], [0.4, 0.4, 0.4], [0.0, 0.0, 0.0], [0.2, -0.3, 0.1], [0.2, -0.3, 0.4]], dtype=d),
                  np.array([[0, 1, 2], [3, 3, 3], [3, 4, 4], [3, 4, 3]], dtype=np.int32))     # collinear, a point, two segments
    span = (np.array([[-0.5, -0.5, -0.5], [0.5, 0.5, -0.45], [0.5, -0.5, 0.5]], dtype=d), np.array([[0, 1, 2]], dtype=np.int32))
    outside = (np.array([[0.3, 0.3, 0.3], [0.9, 0.4, 0.2], [0.4, 0.8, 0.45], [0.7, 0.7, 0.7], [0.9, 0.7, 0.8], [0.8, 0.9, 0.7],
                         [-2.0, 0.0, 0.0], [3.0, 0.1, 0.0], [0.0, 0.0, 2.5]], dtype=d),
               np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8]], dtype=np.int32))
    nan = (np.array([[0.1, 0.1, 0.1], [np.nan, 0.2, 0.2], [0.3, 0.1, 0.2], [-0.3, -0.3, -0.3], [-0.1, -0.3, -0.2], [-0.2, -0.1, -0.3],
                     [0.0, np.inf, 0.0]], dtype=d), np.array([[0, 1, 2], [3, 4, 5], [3, 6, 5]], dtype=np.int32))
    return [(np.zeros((0, 3), dtype=d), np.zeros((0, 3), dtype=np.int32)), tri, degenerate, join(span, soup(tiny, 5, dtype=d)), outside, nan,
            (np.zeros((4, 3), dtype=d), np.zeros((0, 3), dtype=np.int32))]


def face_points(V, F, per_face, seed):
    """Points on the faces: the vertices, the edge midpoints and per_face random barycentric points of each, fp64."""
    rng = np.random.default_rng(seed)
    v = np.asarray(V).astype(np.float64)[np.asarray(F).reshape(-1, 3)]
    pts = [v.reshape(-1, 3), ((v + np.roll(v, 1, axis=1)) * 0.5).reshape(-1, 3)]
    b = rng.random((len(v), per_face, 3))
    b /= b.sum(axis=2, keepdims=True)
    pts.append(np.einsum("fpk,fkc->fpc", b, v).reshape(-1, 3))
    return np.concatenate(pts)


GOLDEN_CASES = (
    ("cube11", (11, 11, 11), "float64"), ("cube_off", (9, 9, 9), "float32"), ("ico1_5", (5, 5, 5), "float32"),
    ("ico2_8x9x9", (8, 9, 9), "float64"), ("ico2_33", (33, 33, 33), "float32"), ("hemi2_12x16x16", (12, 16, 16), "float32"),
    ("soup_16", (16, 16, 16), "float32"), ("mixed2_2", (2, 2, 2), "float32"),
)


def golden_mesh(key, dtype):
    if key == "cube11":
        return node_box((2, 2, 2), (8, 8, 8), (11, 11, 11), dtype)
    if key == "cube_off":
        return box((-0.31, -0.23, -0.17), (0.27, 0.33, 0.41), dtype)
    if key.startswith("ico1"):
        return icosphere(1, 0.43, (0.01, -0.02, 0.03), dtype)
    if key.startswith("ico2"):
        return icosphere(2, 0.41, (0.02, 0.01, -0.03), dtype)
    if key.startswith("hemi2"):
        return hemisphere(2, 0.42, dtype)
    if key == "soup_16":
        return soup(60, 11, 0.3, dtype)
    if key == "mixed2_2":
        return mixed_batch(dtype, tiny=20)[3]
    raise KeyError(key)


def golden_cases():
    """(key, shape, V, F) of every recorded case."""
    for key, shape, dtype in GOLDEN_CASES:
        V, F = golden_mesh(key, np.dtype(dtype).type)
        yield key, shape, V, F
