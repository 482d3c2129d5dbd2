"""The definition of dpc_point_mesh_distance (include/dpc_render.h) and of the F-score, on the host.

    tri_d2 / mesh_d2              numpy fp64, Ericson's region walk ("Real-Time Collision Detection", 5.1.5): the seven
                                  Voronoi regions of the triangle decided one after the other, the closest point formed, and
                                  its squared distance -- a different formulation from the kernel's (which clamps the three
                                  segment parameters and selects), so an agreement is not an agreement of two copies
    tri_d2_exact / mesh_d2_exact  the same definition in exact rational arithmetic (fractions.Fraction), for small inputs
    fscore_rule                   precision, recall and F at thresholds from given distances

Rules: a zero-area face (two or three coincident vertices, or collinear ones) is the segment or point it degenerates to;
a face with a NaN or infinite vertex, or one of magnitude >= 2^64, is skipped (status bit STATUS_NONFINITE); a mesh whose
faces are all skipped gives +inf.

The unit in which the tests measure an error is 2^-52 S^2, S the largest absolute coordinate among the row's points and
finite vertices (unit()).  tests/golden/f28_point_mesh.npz records, per case, the worst error of mesh_d2 against
mesh_d2_exact in that unit; the GPU test allows 8 times the largest of them.
"""
from fractions import Fraction

import numpy as np

STATUS_BAD_INDEX, STATUS_NONFINITE = 1, 8
MAX_COORD = 2.0 ** 64        # DPC_MESH_VOXEL_MAX_COORD


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _segment_d2(p, a, b):
    """Squared distance from p to the segment a b (a zero-length segment is the point a); broadcasting [...,3]."""
    ab, ap = b - a, p - a
    e = _dot(ab, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(e > 0, np.clip(_dot(ap, ab) / np.where(e > 0, e, 1.0), 0.0, 1.0), 0.0)
    r = ap - t[..., None] * ab
    return _dot(r, r)


def tri_d2(P, A, B, C):
    """Squared distances [n,f] from the points P [n,3] to the triangles (A, B, C) [f,3] each, fp64: Ericson's region walk;
    a triangle whose cross product is exactly zero is the longest of its three segments (which contains the others)."""
    p = np.asarray(P, dtype=np.float64).reshape(-1, 1, 3)
    a, b, c = (np.asarray(x, dtype=np.float64).reshape(1, -1, 3) for x in (A, B, C))
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = 1.0 / (va + vb + vc)
        v, w = vb * denom, vc * denom
    shape = np.broadcast(ap[..., 0], ab[..., 0]).shape
    full = lambda x: np.broadcast_to(x, shape + (3,))
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    closest = [full(a), full(b), a + v_ab[..., None] * ab, full(c), a + w_ac[..., None] * ac, b + w_bc[..., None] * (c - b),
               a + ab * v[..., None] + ac * w[..., None]]
    q = closest[6]
    for cond, x in reversed(list(zip(conds, closest[:6]))):   # the first condition that holds wins
        q = np.where(cond[..., None], x, q)
    r = p - q
    out = _dot(r, r)
    n = np.cross(ab, ac)
    flat = (n == 0).all(axis=-1)                               # [1,f]
    if flat.any():
        seg = np.minimum(np.minimum(_segment_d2(p, a, b), _segment_d2(p, a, c)), _segment_d2(p, b, c))
        out = np.where(np.broadcast_to(flat, out.shape), seg, out)
    return out


def kept_faces(V, F):
    """(faces [k,3] of the mesh whose vertices are all finite and below MAX_COORD in magnitude, status bits)."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        ok = (np.abs(v[F]) < MAX_COORD).all(axis=(1, 2)) if len(F) else np.zeros(0, dtype=bool)
    return F[ok], (0 if ok.all() else STATUS_NONFINITE)


def mesh_d2(P, V, F):
    """(squared distances [n] fp64 from P [n,3] to the union of the mesh's kept faces, +inf when there is none; status)."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    P = np.asarray(P).astype(np.float64).reshape(-1, 3)
    Fk, status = kept_faces(v, F)
    if len(Fk) == 0 or len(P) == 0:
        return np.full(len(P), np.inf), status
    out = np.full(len(P), np.inf)
    for a in range(0, len(Fk), 4096):
        f = Fk[a:a + 4096]
        out = np.minimum(out, tri_d2(P, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]).min(axis=1))
    return out, status


def unit(P, V):
    """2^-52 S^2, S the largest absolute coordinate among the points and the finite vertices."""
    v = np.asarray(V).astype(np.float64).reshape(-1)
    p = np.asarray(P).astype(np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        v = v[np.abs(v) < MAX_COORD]
    S = max(np.abs(v).max(initial=0.0), np.abs(p).max(initial=0.0))
    return 2.0 ** -52 * S * S


# --- exact ---------------------------------------------------------------------------------------------------------
def _fr(x):
    return [Fraction(float(t)) for t in x]


def _fdot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _fsub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _fsegment(p, a, b):
    ab, ap = _fsub(b, a), _fsub(p, a)
    e = _fdot(ab, ab)
    t = Fraction(0) if e == 0 else min(max(_fdot(ap, ab) / e, Fraction(0)), Fraction(1))
    r = [ap[k] - t * ab[k] for k in range(3)]
    return _fdot(r, r)


def tri_d2_exact(p, a, b, c):
    """The squared distance from p to the closed triangle (a, b, c) as a Fraction: the foot point of the plane when the
    triangle has area and the foot point lies inside it, the nearest of the three segments otherwise."""
    p, a, b, c = _fr(p), _fr(a), _fr(b), _fr(c)
    e0, e1, d = _fsub(b, a), _fsub(c, a), _fsub(p, a)
    aa, bb, cc = _fdot(e0, e0), _fdot(e0, e1), _fdot(e1, e1)
    det = aa * cc - bb * bb
    if det > 0:
        d0, d1 = _fdot(d, e0), _fdot(d, e1)
        s, t = (cc * d0 - bb * d1) / det, (aa * d1 - bb * d0) / det
        if s >= 0 and t >= 0 and s + t <= 1:
            r = [d[k] - s * e0[k] - t * e1[k] for k in range(3)]
            return _fdot(r, r)
    return min(_fsegment(p, a, b), _fsegment(p, a, c), _fsegment(p, b, c))


def mesh_d2_exact(P, V, F, slack=1e-6):
    """Exact squared distances (Fractions, None for +inf) from P to the mesh.  Rational arithmetic is slow, so for each
    point only the faces whose numpy distance is within slack * S^2 of the numpy minimum are evaluated exactly: numpy's
    error is some 2^-52 S^2, ten orders below the slack, so the exact minimum is among them."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    P = np.asarray(P).astype(np.float64).reshape(-1, 3)
    Fk, _ = kept_faces(v, F)
    if len(Fk) == 0:
        return [None] * len(P)
    u = unit(P, v) * 2.0 ** 52 * slack
    out = []
    for p in P:
        d = tri_d2(p[None], v[Fk[:, 0]], v[Fk[:, 1]], v[Fk[:, 2]])[0]
        near = np.nonzero(d <= d.min() + u)[0]
        out.append(min(tri_d2_exact(p, v[Fk[j, 0]], v[Fk[j, 1]], v[Fk[j, 2]]) for j in near))
    return out


def rounded(exact):
    """Exact values rounded once to fp64 (None -> +inf)."""
    return np.array([np.inf if x is None else float(x) for x in exact], dtype=np.float64)   # float(Fraction) rounds correctly


# --- F-score -------------------------------------------------------------------------------------------------------
def fscore_rule(d_pred, d_gt, thresholds):
    """[T,3] (precision, recall, F): d_pred the distances of the prediction's points to the ground truth, d_gt those of the
    ground truth's points to the prediction; strict <; F = 2PR / (P + R), 0 where P + R = 0; an empty side gives NaN."""
    d_pred, d_gt = np.asarray(d_pred, dtype=np.float64), np.asarray(d_gt, dtype=np.float64)
    out = np.zeros((len(thresholds), 3))
    for k, tau in enumerate(thresholds):
        with np.errstate(invalid="ignore", divide="ignore"):
            p = np.float64((d_pred < tau).sum()) / np.float64(len(d_pred))
            r = np.float64((d_gt < tau).sum()) / np.float64(len(d_gt))
            f = np.float64(0.0) if p + r == 0 else 2.0 * p * r / (p + r)
        out[k] = (p, r, f)
    return out


def nearest_d(src, tgt):
    """Brute-force nearest-neighbour distances src -> tgt in the arithmetic of point_cloud_distance: the squared distance
    summed as (dx^2 + dy^2) + dz^2 in the clouds' common dtype, then sqrt; +inf for an empty target."""
    dt = np.float64 if (np.asarray(src).dtype == np.float64 or np.asarray(tgt).dtype == np.float64) else np.float32
    s, t = np.asarray(src).astype(dt).reshape(-1, 3), np.asarray(tgt).astype(dt).reshape(-1, 3)
    if len(t) == 0:
        return np.full(len(s), np.inf)
    d = s[:, None, :] - t[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.sqrt(d2.min(axis=1))


# --- the recorded cases --------------------------------------------------------------------------------------------
def placed_face(p, h=0.003, size=0.01):
    """A triangle in the plane x0 = p[0] - h whose interior lies under the point p: nearer to p than anything of a soup
    that keeps clear of it."""
    a = np.array([p[0] - h, p[1] - size, p[2] - size])
    return np.stack([a, a + (0, 3 * size, 0), a + (0, 0, 3 * size)])
