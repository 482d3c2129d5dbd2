"""The definition of dpc_point_mesh_closest (include/dpc_render.h) on the host: besides the squared distance of
tests/point_mesh_oracle.py, the nearest face, the closest point Q of it and Q's weights on the face's vertices.

    tri_closest / mesh_closest              numpy fp64, Ericson's region walk ("Real-Time Collision Detection", 5.1.5), which
                                            forms the closest point q on its way to the distance; the weights are the
                                            barycentric coordinates the walk ends with.  A formulation different from the
                                            kernel's (foot point of the plane, or endpoint + t E of the nearest segment)
    tri_closest_exact / mesh_closest_exact  the same definition in exact rational arithmetic: the closest point of a
                                            triangle with rational vertices to a rational point is rational
    face_normals                            (V1 - V0) x (V2 - V0) over its length in the caller's winding, numpy's
                                            elementwise fp64 arithmetic, zeros for a cross product without length

Rules beyond point_mesh_oracle's: the nearest face is the lowest index among the faces of least d2 (np.argmin), indexed
within F as passed (skipped faces keep their index and never win); the weights are on the face's vertices in the order F
lists them, non-negative, and sum to 1; a mesh without a usable face gives d2 = +inf, face = -1, NaN q and weights.

The unit in which the tests measure an error of a point is 2^-52 S, S the largest absolute coordinate among the row's points
and finite vertices (unit_len()).  tests/golden/f31_closest.npz records, per case, the worst error of mesh_closest's q and
of sum w V rebuilt (exactly) from its weights against the Q it stores (the exact Q rounded once to fp64) in that unit; the
GPU test allows 8 times the recorded ratios.
"""
from fractions import Fraction

import numpy as np

import point_mesh_oracle as PM

_dot = PM._dot


def unit_len(P, V):
    """2^-52 S, S as in point_mesh_oracle.unit."""
    return float(np.sqrt(PM.unit(P, V) * 2.0 ** 52)) * 2.0 ** -52


def _segment(p, a, b):
    """(q, t) of the point of the segment a b nearest to p (a zero-length segment is the point a); broadcasting [...,3]."""
    ab, ap = b - a, p - a
    e = _dot(ab, ab)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(e > 0, np.clip(_dot(ap, ab) / np.where(e > 0, e, 1.0), 0.0, 1.0), 0.0)
    return a + t[..., None] * ab, t


def tri_closest(P, A, B, C):
    """(d2 [n,f], q [n,f,3], w [n,f,3]) from the points P [n,3] to the triangles (A, B, C) [f,3] each, fp64: Ericson's region
    walk; w weighs (A, B, C).  A triangle whose cross product is exactly zero is the nearest of its three segments."""
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
    zero, one = np.zeros(shape), np.ones(shape)
    bary = lambda x, y, z: np.stack(np.broadcast_arrays(x, y, z), axis=-1)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    closest = [full(a), full(b), a + v_ab[..., None] * ab, full(c), a + w_ac[..., None] * ac, b + w_bc[..., None] * (c - b),
               a + ab * v[..., None] + ac * w[..., None]]
    weights = [bary(one, zero, zero), bary(zero, one, zero), bary(1.0 - v_ab, v_ab, zero), bary(zero, zero, one),
               bary(1.0 - w_ac, zero, w_ac), bary(zero, 1.0 - w_bc, w_bc), bary(1.0 - v - w, v, w)]
    q, wt = closest[6], weights[6]
    for cond, x, y in reversed(list(zip(conds, closest[:6], weights[:6]))):   # the first condition that holds wins
        q = np.where(cond[..., None], x, q)
        wt = np.where(cond[..., None], y, wt)
    n = np.cross(ab, ac)
    flat = np.broadcast_to((n == 0).all(axis=-1), shape)                        # [n,f]
    if flat.any():
        segs = [_segment(p, a, b), _segment(p, a, c), _segment(p, b, c)]
        sw = [bary(1.0 - segs[0][1], segs[0][1], zero), bary(1.0 - segs[1][1], zero, segs[1][1]), bary(zero, 1.0 - segs[2][1], segs[2][1])]
        sd = np.stack([_dot(p - s[0], p - s[0]) for s in segs])
        k = sd.argmin(axis=0)                                                    # the first of equals
        sq = np.choose(k[..., None], [full(s[0]) for s in segs])
        sw = np.choose(k[..., None], sw)
        q = np.where(flat[..., None], sq, q)
        wt = np.where(flat[..., None], sw, wt)
    r = p - q
    return _dot(r, r), q, wt


def usable(V, F):
    """[f] bool: the faces whose vertices are all finite and below MAX_COORD in magnitude."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (np.abs(v[F]) < PM.MAX_COORD).all(axis=(1, 2)) if len(F) else np.zeros(0, dtype=bool)


def mesh_closest(P, V, F):
    """(d2 [n], face [n] int32, q [n,3], w [n,3], status) of P against the mesh: the lowest index among the usable faces of
    least d2; +inf, -1, NaN, NaN when there is none."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    P = np.asarray(P).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F).reshape(-1, 3)
    ok = usable(v, F)
    n = len(P)
    d2, face = np.full(n, np.inf), np.full(n, -1, dtype=np.int32)
    q, w = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    kept = np.nonzero(ok)[0]
    for a in range(0, len(kept), 4096):
        idx = kept[a:a + 4096]
        f = F[idx]
        d, qq, ww = tri_closest(P, v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
        k = d.argmin(axis=1) if n else np.zeros(0, dtype=np.int64)
        rows = np.arange(n)
        better = d[rows, k] < d2                                                 # strict: an earlier block keeps a tie
        d2 = np.where(better, d[rows, k], d2)
        face = np.where(better, idx[k], face).astype(np.int32)
        q = np.where(better[:, None], qq[rows, k], q)
        w = np.where(better[:, None], ww[rows, k], w)
    return d2, face, q, w, (0 if ok.all() else PM.STATUS_NONFINITE)


def face_normals(V, F):
    """[f,3]: (V1 - V0) x (V2 - V0) / its length, every operation rounded on its own in the order written here; zeros where
    the cross product has no length."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F).reshape(-1, 3)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        a, b = v[F[:, 1]] - v[F[:, 0]], v[F[:, 2]] - v[F[:, 0]]
        c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
        length = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        return np.where((length > 0)[:, None], c / np.where(length > 0, length, 1.0)[:, None], 0.0)


# --- exact ---------------------------------------------------------------------------------------------------------
_fr, _fdot, _fsub = PM._fr, PM._fdot, PM._fsub


def _fsegment(p, a, b):
    """(d2, q, t) of the segment a b in Fractions."""
    ab, ap = _fsub(b, a), _fsub(p, a)
    e = _fdot(ab, ab)
    t = Fraction(0) if e == 0 else min(max(_fdot(ap, ab) / e, Fraction(0)), Fraction(1))
    q = [a[k] + t * ab[k] for k in range(3)]
    r = _fsub(p, q)
    return _fdot(r, r), q, t


def tri_closest_exact(p, a, b, c):
    """(d2, q [3], w [3]) in Fractions: the foot point of the plane when the triangle has area and the foot point lies
    inside it, the nearest of the three segments (the first of equals in the order ab, ac, bc) otherwise."""
    p, a, b, c = _fr(p), _fr(a), _fr(b), _fr(c)
    e0, e1, d = _fsub(b, a), _fsub(c, a), _fsub(p, a)
    aa, bb, cc = _fdot(e0, e0), _fdot(e0, e1), _fdot(e1, e1)
    det = aa * cc - bb * bb
    if det > 0:
        d0, d1 = _fdot(d, e0), _fdot(d, e1)
        s, t = (cc * d0 - bb * d1) / det, (aa * d1 - bb * d0) / det
        if s >= 0 and t >= 0 and s + t <= 1:
            q = [a[k] + s * e0[k] + t * e1[k] for k in range(3)]
            r = _fsub(p, q)
            return _fdot(r, r), q, [1 - s - t, s, t]
    zero = Fraction(0)
    segs = [_fsegment(p, a, b), _fsegment(p, a, c), _fsegment(p, b, c)]
    k = min(range(3), key=lambda j: segs[j][0])
    d2, q, t = segs[k]
    return d2, q, [[1 - t, t, zero], [1 - t, zero, t], [zero, 1 - t, t]][k]


def mesh_closest_exact(P, V, F, slack=1e-6, near=1e-9):
    """Per point a dict: d2 (the exact least squared distance, None when no face is usable), q (the exact closest point of
    the lowest exact minimiser, 3 Fractions), argmin (the faces whose exact d2 equals it, ascending), near (the faces whose
    exact d2 is at most (1 + near) times it), second (the least exact d2 outside argmin among the candidates, or None),
    same_q (every face of `near` has the same exact closest point).  As in point_mesh_oracle.mesh_d2_exact, only the faces
    whose numpy distance is within slack * S^2 of the numpy minimum are evaluated exactly."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    P = np.asarray(P).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F).reshape(-1, 3)
    kept = np.nonzero(usable(v, F))[0]
    out = []
    if len(kept) == 0:
        return [dict(d2=None, q=None, argmin=[], near=[], second=None, same_q=True) for _ in P]
    u = PM.unit(P, v) * 2.0 ** 52 * slack
    Fk = F[kept]
    for p in P:
        d = PM.tri_d2(p[None], v[Fk[:, 0]], v[Fk[:, 1]], v[Fk[:, 2]])[0]
        cand = np.nonzero(d <= d.min() + u)[0]
        ex = {int(kept[j]): tri_closest_exact(p, v[Fk[j, 0]], v[Fk[j, 1]], v[Fk[j, 2]]) for j in cand}
        least = min(e[0] for e in ex.values())
        argmin = sorted(j for j, e in ex.items() if e[0] == least)
        near_set = sorted(j for j, e in ex.items() if e[0] <= least * (1 + Fraction(near)))
        rest = [e[0] for j, e in ex.items() if e[0] != least]
        q = ex[argmin[0]][1]
        out.append(dict(d2=least, q=q, argmin=argmin, near=near_set, second=min(rest) if rest else None,
                        same_q=all(ex[j][1] == q for j in near_set)))
    return out


def combine_exact(w, tri):
    """sum_k w[k] tri[k] in Fractions from fp64 weights [3] and fp64 vertices [3,3]: what the weights say Q is."""
    w = _fr(w)
    return [sum(w[k] * Fraction(float(tri[k][c])) for k in range(3)) for c in range(3)]


def point_error(q, exact):
    """max_c |q[c] - exact[c]| as a float, q fp64 [3] or Fractions, exact Fractions."""
    return float(max(abs((x if isinstance(x, Fraction) else Fraction(float(x))) - e) for x, e in zip(q, exact)))
