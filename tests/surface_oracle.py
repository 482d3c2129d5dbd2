"""Numpy restatement of the iso-surface rule of include/dpc_render.h (dpc_surface_count / dpc_surface_extract), vectorised
so that a 128^3 smooth field takes a few seconds.  It derives its own triangulation table by walking each face's perimeter
(tools/gen_surface_table.py derives the committed one from triple products); the rule fixes every loop's start, the loops'
order and the fan, so the two must agree row for row.

    table()                       int8 [256,16]: triangle count, then 5 x 3 cell-edge ids padded with -1
    extract(grid, iso)            (verts float64 [n,3], faces int32 [m,3], nonfinite bool) of one [D,H,W] grid
    unit_cube(verts, shape)       column c -> V_c / (G_c - 1) - 0.5
    augment(verts, faces)         the vertices, then the edge midpoints of the (0,1), (1,2), (0,2) blocks
"""
import functools

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------


def _corner_id(off):
    return 4 * off[0] + 2 * off[1] + off[2]


def _edge_id(p, q):
    """The id 4*a + u_b + 2*u_c of the cell edge between the corners (offset triples) p and q."""
    a = [i for i in range(3) if p[i] != q[i]]
    assert len(a) == 1
    a = a[0]
    lo = p if p[a] == 0 else q
    b, c = [i for i in range(3) if i != a]
    return 4 * a + lo[b] + 2 * lo[c]


def _face_cycle(axis, side):
    """The four corners of the face `axis` = `side`, counter-clockwise for a viewer outside the cell."""
    b, c = [i for i in range(3) if i != axis]
    cyc = []
    for ub, uc in ((0, 0), (1, 0), (1, 1), (0, 1)):
        off = [0, 0, 0]
        off[axis], off[b], off[c] = side, ub, uc
        cyc.append(tuple(off))
    # (e_b, e_c, e_axis) is right-handed for axis 0 and 2, left-handed for axis 1; the viewer sits on the side of the face
    ccw_about_plus_axis = axis != 1
    outward_is_plus = side == 1
    return cyc if ccw_about_plus_axis == outward_is_plus else cyc[::-1]


def _case_triangles(case):
    inside = lambda off: bool(case >> _corner_id(off) & 1)
    nxt = {}
    for axis in range(3):
        for side in (0, 1):
            cyc = _face_cycle(axis, side)
            for i in range(4):
                # a run of inside corners met on the walk: entered over the edge (i, i+1), left over a later edge
                if not inside(cyc[i]) and inside(cyc[(i + 1) % 4]):
                    j = i + 1
                    while inside(cyc[(j + 1) % 4]):
                        j += 1
                    entry = _edge_id(cyc[i], cyc[(i + 1) % 4])
                    leave = _edge_id(cyc[j % 4], cyc[(j + 1) % 4])
                    assert entry not in nxt
                    nxt[entry] = leave
    tris, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, e = [], start
        while e not in seen:
            seen.add(e)
            loop.append(e)
            e = nxt[e]
        assert e == start
        tris += [(loop[0], loop[i], loop[i + 1]) for i in range(1, len(loop) - 1)]
    return tris


@functools.lru_cache(maxsize=None)
def _table():
    t = np.full((256, 16), -1, dtype=np.int8)
    for case in range(256):
        tris = _case_triangles(case)
        t[case, 0] = len(tris)
        flat = [e for tri in tris for e in tri]
        t[case, 1:1 + len(flat)] = flat
    t.setflags(write=False)
    return t


def table():
    return _table()


def edge_owner(e):
    """(offsets of the owning corner, axis) of cell edge e."""
    a, j = divmod(int(e), 4)
    b, c = [i for i in range(3) if i != a]
    off = [0, 0, 0]
    off[b], off[c] = j & 1, j >> 1
    return tuple(off), a


# ---------------------------------------------------------------------------------------------------------------------
# one grid
# ---------------------------------------------------------------------------------------------------------------------
def extract(grid, iso):
    """(verts float64 [n,3], faces int32 [m,3], nonfinite): the surface of one [D,H,W] grid at the level iso.  nonfinite:
    a crossing edge has an end that is NaN or infinite (its vertex is written as it comes out)."""
    g = np.asarray(grid)
    assert g.ndim == 3
    v = g.astype(np.float64)
    iso = np.float64(iso)
    D, H, W = v.shape
    with np.errstate(invalid="ignore"):
        inside = v > iso                                   # False for a NaN
    flat = np.arange(D * H * W, dtype=np.int64).reshape(D, H, W)
    keys, coords, nonfinite = [], [], False
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = inside[lo] != inside[hi]
        idx = np.nonzero(cross)
        va, vb = v[lo][idx], v[hi][idx]
        nonfinite |= bool((~np.isfinite(va) | ~np.isfinite(vb)).any())
        with np.errstate(all="ignore"):
            t = (iso - va) / (vb - va)
        p = np.stack([i.astype(np.float64) for i in idx], axis=1) if len(va) else np.zeros((0, 3))
        p[:, a] = p[:, a] + t
        keys.append(3 * flat[lo][idx] + a)
        coords.append(p)
    keys, coords = np.concatenate(keys), np.concatenate(coords)
    order = np.argsort(keys, kind="stable")
    verts = np.ascontiguousarray(coords[order])
    vid = np.full(3 * D * H * W, -1, dtype=np.int64)
    vid[keys[order]] = np.arange(len(order))
    if min(D, H, W) < 2:
        return verts, np.zeros((0, 3), dtype=np.int32), nonfinite
    case = np.zeros((D - 1, H - 1, W - 1), dtype=np.int64)
    for k in range(8):
        dd, dh, dw = (k >> 2) & 1, (k >> 1) & 1, k & 1
        case |= inside[dd:D - 1 + dd, dh:H - 1 + dh, dw:W - 1 + dw].astype(np.int64) << k
    T = table().astype(np.int64)
    cells = np.nonzero(T[case, 0] > 0)                     # C order: ascending flat index of corner 0
    rows = T[case[cells]]
    edges = rows[:, 1:].reshape(-1, 5, 3)
    keep = np.arange(5)[None, :] < rows[:, :1]
    # the key 3*f(owner) + a of every edge id, per cell
    own = np.array([edge_owner(e)[0] for e in range(12)], dtype=np.int64)
    axis = np.array([edge_owner(e)[1] for e in range(12)], dtype=np.int64)
    e = np.where(edges >= 0, edges, 0)
    d = cells[0][:, None, None] + own[e, 0]
    h = cells[1][:, None, None] + own[e, 1]
    w = cells[2][:, None, None] + own[e, 2]
    faces = vid[3 * ((d * H + h) * W + w) + axis[e]][keep]
    assert (faces >= 0).all()
    return verts, np.ascontiguousarray(faces.astype(np.int32)), nonfinite


def unit_cube(verts, shape):
    """Column c -> V_c / (G_c - 1) - 0.5 in fp64: the node grid of voxelise."""
    out = np.array(verts, dtype=np.float64)
    for c in range(3):
        out[:, c] = out[:, c] / np.float64(shape[c] - 1) - 0.5
    return out


def augment(verts, faces):
    """The reference's augment_mesh order: the vertices, then the midpoints 0.5 * (v[i1] + v[i2]) of every face's
    (0,1) corners, then (1,2), then (0,2); duplicates kept."""
    blocks = [verts] + [0.5 * (verts[faces[:, k1]] + verts[faces[:, k2]]) for k1, k2 in ((0, 1), (1, 2), (0, 2))]
    return np.concatenate(blocks, axis=0)


# ---------------------------------------------------------------------------------------------------------------------
# what the tests check of a mesh, and their inputs
# ---------------------------------------------------------------------------------------------------------------------
def directed_edge_counts(faces):
    """{(i, j): how often the directed edge i -> j occurs}."""
    out = {}
    for a, b, c in np.asarray(faces).tolist():
        for e in ((a, b), (b, c), (c, a)):
            out[e] = out.get(e, 0) + 1
    return out


def signed_volume(verts, faces):
    v0, v1, v2 = (verts[faces[:, k]] for k in range(3))
    return float((v0 * np.cross(v1, v2)).sum() / 6.0)


def euler_characteristic(verts, faces):
    edges = {tuple(sorted(e)) for e in directed_edge_counts(faces)}
    return len(verts) - len(edges) + len(faces)


def ball(shape, dtype=np.float32, sigma=0.25, centre=(0.03, -0.02, 0.01)):
    """A Gaussian ball in the cube [-1/2, 1/2]^3 sampled at the nodes of a [D,H,W] grid."""
    ax = [np.linspace(-0.5, 0.5, s) if s > 1 else np.zeros(1) for s in shape]
    d, h, w = np.meshgrid(*ax, indexing="ij")
    r2 = (d - centre[0]) ** 2 + (h - centre[1]) ** 2 + (w - centre[2]) ** 2
    return np.exp(-r2 / (2 * sigma * sigma)).astype(dtype)


def blobs(G, seed, n=40, dtype=np.float32):
    """A smooth field: the sum of Gaussian blobs on a G^3 grid (about 10^5 surface vertices at 128^3 and the level 0.1)."""
    rng = np.random.default_rng(seed)
    out = np.zeros((G, G, G))
    for _ in range(n):
        out += ball((G, G, G), np.float64, sigma=0.03 + 0.03 * rng.random(), centre=tuple(rng.random(3) * 0.8 - 0.4))
    return out.astype(dtype)


def noise(shape, seed, dtype=np.float32, border=True):
    """Uniform noise in [0, 1); with `border`, a zero shell around it (the surface is then closed)."""
    g = np.random.default_rng(seed).random(shape).astype(dtype)
    if border:
        for a in range(3):
            sl = [slice(None)] * 3
            sl[a] = 0
            g[tuple(sl)] = 0
            sl[a] = -1
            g[tuple(sl)] = 0
    return g


def one_cell_cases(values=None, seed=0, iso=0.37):
    """[256,2,2,2] float32 grids, grid c being case c: corner k inside iff bit k of c.  values None: 0 / 1; "seeded": values
    in (0, 1) on the right side of `iso`."""
    g = np.zeros((256, 2, 2, 2), dtype=np.float32)
    rng = np.random.default_rng(seed)
    for c in range(256):
        for k in range(8):
            ins = bool(c >> k & 1)
            if values is None:
                x = 1.0 if ins else 0.0
            else:
                x = iso + (1.0 - iso) * (0.05 + 0.9 * rng.random()) if ins else iso * (0.05 + 0.9 * rng.random())
            g[c, (k >> 2) & 1, (k >> 1) & 1, k & 1] = x
    return g
