"""The definition of dpc_mesh_winding and dpc_mesh_winding_voxels (include/dpc_render.h), on the host.

    face_terms / mesh_sums / mesh_winding   numpy fp64, elementwise: the rule for one face, its quantisation to 2^-40 and
                                            the int64 sum over the faces
    face_term_mp / mesh_sums_mp             the same rule with mpmath at 50 digits (det, whose sign and zero decide, in
                                            exact rational arithmetic): the exact terms, quantised, and their sum
    voxel_sums / winding_grid               the node centres of voxelise_meshes' frame and the integer compare

One face (V0, V1, V2), the caller's order, seen from P:
    a = V0 - P, b = V1 - P, c = V2 - P;  det = a . (b x c);  den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|
    t = atan2(det, den) / (2 pi), 0 when det == 0;  q = rint(t 2^40)
(Van Oosterom and Strackee's solid angle of a triangle, as Jacobson, Kavan and Sorkine-Hornung's generalized winding
numbers use it.)  A face with a NaN or infinite vertex, or one of magnitude >= 2^64, is skipped (STATUS_NONFINITE), a face
with an index outside the mesh is skipped (STATUS_BAD_INDEX); a point that is not finite gets sum 0 and w = NaN.

Tolerance.  Away from the surface an fp64 term is right to about 1e-16 against the quantum 2^-40 ~ 9e-13, so a quantised
term differs from the quantised exact term by at most one quantum: |sum - sum_mp| <= bound(V, F), the usable faces.  The
conditioning fails only next to edges (a point 1e-9 of the extent from a cube's edge moves by thousands of quanta), so
every compared query keeps CLEARANCE times the mesh's extent from the surface.
"""
from fractions import Fraction

import numpy as np

STATUS_BAD_INDEX, STATUS_NONFINITE = 1, 8
MAX_COORD = 2.0 ** 64        # DPC_MESH_VOXEL_MAX_COORD
FRAC_BITS = 40               # DPC_WINDING_FRAC_BITS
SCALE = 2.0 ** FRAC_BITS
CLEARANCE = 1e-3
TWO_PI = 2.0 * np.pi


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _norm(a):
    return np.sqrt(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2])


def face_terms(P, V0, V1, V2):
    """t [n,f] float64 for the points P [n,3] and the faces (V0, V1, V2) [f,3] each."""
    p = np.asarray(P, dtype=np.float64).reshape(-1, 1, 3)
    a, b, c = (np.asarray(x, dtype=np.float64).reshape(1, -1, 3) - p for x in (V0, V1, V2))
    bxc = np.stack([b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1], b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2],
                    b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]], axis=-1)
    det = _dot(a, bxc)
    la, lb, lc = _norm(a), _norm(b), _norm(c)
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    return np.where(det == 0, 0.0, np.arctan2(det, den) / TWO_PI)


def quantise(t):
    return np.rint(np.asarray(t) * SCALE).astype(np.int64)


def threshold_q(threshold):
    return int(np.rint(float(threshold) * SCALE))


def kept_faces(V, F):
    """(the usable faces [k,3], status bits): every index inside the mesh, every vertex finite and below MAX_COORD."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F).reshape(-1, 3).astype(np.int64)
    status = 0
    inside = ((F >= 0) & (F < len(v))).all(axis=1) if len(F) else np.zeros(0, dtype=bool)
    if not inside.all():
        status |= STATUS_BAD_INDEX
    F = F[inside]
    with np.errstate(invalid="ignore"):
        ok = (np.abs(v[F]) < MAX_COORD).all(axis=(1, 2)) if len(F) else np.zeros(0, dtype=bool)
    if not ok.all():
        status |= STATUS_NONFINITE
    return F[ok], status


def bound(V, F):
    """The most a device sum may differ from mesh_sums_mp's, in quanta: one per usable face."""
    return len(kept_faces(V, F)[0])


def _finite_points(P):
    P = np.asarray(P).astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return P, (np.abs(P) < MAX_COORD).all(axis=1)


def mesh_sums(P, V, F):
    """(sums int64 [n], status) of the points P [n,3] about the mesh (V, F)."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    P, fin = _finite_points(P)
    Fk, status = kept_faces(v, F)
    if not fin.all():
        status |= STATUS_NONFINITE
    out = np.zeros(len(P), dtype=np.int64)
    Pz = np.where(fin[:, None], P, 0.0)
    for s in range(0, len(Fk), 4096):
        f = Fk[s:s + 4096]
        out += quantise(face_terms(Pz, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])).sum(axis=1)
    out[~fin] = 0
    return out, status


def winding_of(sums, P=None):
    """w = sums 2^-40, NaN where P (optional) is not finite."""
    w = np.asarray(sums).astype(np.float64) * (1.0 / SCALE)
    if P is not None:
        w[~_finite_points(P)[1]] = np.nan
    return w


def mesh_winding(P, V, F):
    sums, status = mesh_sums(P, V, F)
    return winding_of(sums, P), status


# --- 50 digits -------------------------------------------------------------------------------------------------------
def face_term_mp(p, v0, v1, v2):
    """The exact t of one face as an mpmath number (50 digits); det is formed in rational arithmetic, so its zero and
    its sign are exact."""
    import mpmath

    with mpmath.workdps(50):
        fr = lambda x: [Fraction(float(t)) for t in x]
        p, v0, v1, v2 = fr(p), fr(v0), fr(v1), fr(v2)
        a, b, c = ([x[k] - p[k] for k in range(3)] for x in (v0, v1, v2))
        det = (a[0] * (b[1] * c[2] - b[2] * c[1]) + a[1] * (b[2] * c[0] - b[0] * c[2]) + a[2] * (b[0] * c[1] - b[1] * c[0]))
        if det == 0:
            return mpmath.mpf(0)
        mp = lambda x: mpmath.mpf(x.numerator) / mpmath.mpf(x.denominator)
        dot = lambda x, y: mp(x[0] * y[0] + x[1] * y[1] + x[2] * y[2])
        la, lb, lc = (mpmath.sqrt(dot(x, x)) for x in (a, b, c))
        den = la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb
        return mpmath.atan2(mp(det), den) / (2 * mpmath.pi)


def mesh_sums_mp(P, V, F):
    """mesh_sums with every term exact before it is quantised: (sums int64 [n], status)."""
    import mpmath

    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    P, fin = _finite_points(P)
    Fk, status = kept_faces(v, F)
    if not fin.all():
        status |= STATUS_NONFINITE
    out = np.zeros(len(P), dtype=np.int64)
    with mpmath.workdps(50):
        scale = mpmath.mpf(2) ** FRAC_BITS
        for i in np.nonzero(fin)[0]:
            out[i] = sum(int(mpmath.nint(face_term_mp(P[i], v[f[0]], v[f[1]], v[f[2]]) * scale)) for f in Fk)
    return out, status


# --- grids -----------------------------------------------------------------------------------------------------------
def node_centres(shape):
    """[D H W, 3] float64: node n of axis c at n / (G_c - 1) - 0.5, in the bit grids' flat order."""
    axes = [np.arange(g, dtype=np.float64) / float(g - 1) - 0.5 for g in shape]
    return np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)


def voxel_sums(V, F, shape):
    return mesh_sums(node_centres(shape), V, F)


def winding_grid(V, F, shape, threshold=0.5):
    """bool [D,H,W]: sum > rint(threshold 2^40); a mesh without faces gives an empty grid."""
    if len(np.asarray(F).reshape(-1, 3)) == 0:
        return np.zeros(shape, dtype=bool)
    return (voxel_sums(V, F, shape)[0] > threshold_q(threshold)).reshape(shape)


# --- small meshes ----------------------------------------------------------------------------------------------------
def cube(lo, hi, dtype=np.float64, lid=True):
    """The box [lo, hi] (3-vectors) as 12 triangles wound outward; without lid the two faces of its +axis-0 side are
    left out (an open box)."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    V = np.array([[(hi if (k >> (2 - c)) & 1 else lo)[c] for c in range(3)] for k in range(8)], dtype=np.float64)
    # vertex k = 4 x + 2 y + z of the corner bits; each side's two triangles counter-clockwise seen from outside
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    if not lid:
        quads.pop(1)
    F = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int32)
    return V.astype(dtype), F


VOX_LO, VOX_HI = (-0.3141592653589793, -0.2718281828459045, -0.1732050807568877), (0.2236067977499790, 0.3316624790355400, 0.2645751311064591)
VOX_SHAPES = ((8, 8, 8), (16, 8, 8))


def voxel_cases(dtype=np.float32):
    """The meshes of the grid tests: a box placed at irrational offsets, so that no node centre of VOX_SHAPES lies within
    CLEARANCE of its surface (tests/test_winding_host.py checks it), closed, and open with its lid removed."""
    return {"cube": cube(VOX_LO, VOX_HI, dtype), "open_box": cube(VOX_LO, VOX_HI, dtype, lid=False)}


def tetrahedron(dtype=np.float64):
    V = np.array([[0.31, 0.07, -0.22], [-0.19, 0.33, 0.05], [-0.11, -0.29, 0.17], [0.02, 0.04, 0.41]], dtype=np.float64)
    F = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], dtype=np.int32)
    c = V.mean(axis=0)
    for k, f in enumerate(F):   # outward: the normal points away from the centroid
        n = np.cross(V[f[1]] - V[f[0]], V[f[2]] - V[f[0]])
        if np.dot(n, V[f[0]] - c) < 0:
            F[k] = f[::-1]
    return V.astype(dtype), F
