"""The definition of dpc_ray_mesh_intersect (include/dpc_render.h) on the host.

    ray_mesh          numpy fp64, elementwise, one operation per expression in the order the header lists them: numpy
                      fuses nothing, and the kernels are built with -ffp-contract=off, so the device reproduces every bit
    ray_tri_exact     the same decision and the same t, u, v in exact rational arithmetic (fractions.Fraction on the inputs'
    ray_mesh_exact    exact values): what the rule means before any rounding
    clearance         the conditions under which rounding cannot change a decision, evaluated exactly: the fixture
                      f33_raycast.npz holds only rays that meet them (tests/golden/make_golden_raycast.py)

The rule for one ray O + t D (D not normalised) and one face (V0, V1, V2), dot(a, b) = (ax bx + ay by) + az bz:
    E1 = V1 - V0, E2 = V2 - V0, Pv = D x E2, det = E1 . Pv;          no hit when !(|det| > 0)
    T = O - V0, a = T . Pv, Q = T x E1, b = D . Q;  s = sign(det)
    inside iff s a >= 0 and s b >= 0 and s a + s b <= |det|;         with cull, det < 0 is no hit
    t = (E2 . Q) / det, hit iff inside and t_min <= t <= t_max;      u = a / det, v = b / det, weights ((1 - u) - v, u, v)
Per ray: hits counts the faces hit; the first hit is the smallest t, the lowest face index among bit-equal t; a miss is
t = +inf, face = -1, NaN weights, zero normal.  A face with a vertex that is not finite (or >= 2^64) is skipped with
STATUS_NONFINITE, a face with an index outside the vertices with STATUS_BAD_INDEX; a ray with such an origin or direction
component gives t = NaN, face = -1, hits = 0, NaN weights, zero normal and STATUS_NONFINITE.
"""
from fractions import Fraction

import numpy as np

import closest_oracle as C
import point_mesh_oracle as PM

STATUS_BAD_INDEX, STATUS_NONFINITE = 1, PM.STATUS_NONFINITE
MAX_COORD = PM.MAX_COORD
CLEAR = Fraction(1, 2 ** 20)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack(np.broadcast_arrays(a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), axis=-1)


def _terms(o, d, v0, v1, v2):
    """(det, a, b, c) [n,f] with c = E2 . Q, from o, d [n,1,3] and the vertices [1,f,3]."""
    e1, e2 = v1 - v0, v2 - v0
    pv = _cross(d, e2)
    det = _dot(e1, pv)
    t = o - v0
    a = _dot(t, pv)
    q = _cross(t, e1)
    return det, a, _dot(d, q), _dot(e2, q)


def ray_mesh(O, D, V, F, t_min=0.0, t_max=np.inf, cull_backfaces=False):
    """dict(t [n], face [n] int32, weights [n,3], hits [n] int32, normal [n,3], status) of the rays against the mesh."""
    O = np.asarray(O).astype(np.float64).reshape(-1, 3)
    D = np.asarray(D).astype(np.float64).reshape(-1, 3)
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F).astype(np.int64).reshape(-1, 3)
    n, status = len(O), 0
    in_range = ((F >= 0) & (F < len(v))).all(axis=1) if len(F) else np.zeros(0, dtype=bool)
    if not in_range.all():
        status |= STATUS_BAD_INDEX
    with np.errstate(invalid="ignore"):
        usable = in_range.copy()
        usable[in_range] = (np.abs(v[F[in_range]]) < MAX_COORD).all(axis=(1, 2))
        ray_ok = (np.abs(O) < MAX_COORD).all(axis=1) & (np.abs(D) < MAX_COORD).all(axis=1)
    if (in_range & ~usable).any() or not ray_ok.all():
        status |= STATUS_NONFINITE
    t_best, face, hits = np.full(n, np.inf), np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int32)
    weights, normal = np.full((n, 3), np.nan), np.zeros((n, 3))
    kept = np.nonzero(usable)[0]
    o, d = np.where(ray_ok[:, None], O, 0.0)[:, None, :], np.where(ray_ok[:, None], D, 0.0)[:, None, :]
    rows = np.arange(n)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k0 in range(0, len(kept), 512):
            idx = kept[k0:k0 + 512]
            f = F[idx]
            det, a, b, c = _terms(o, d, v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None])
            s = np.where(det > 0, 1.0, -1.0)
            sa, sb, m = s * a, s * b, np.abs(det)
            inside = (m > 0) & (sa >= 0) & (sb >= 0) & (sa + sb <= m)
            if cull_backfaces:
                inside &= ~(det < 0)
            t = np.where(inside, c / np.where(inside, det, 1.0), np.nan)
            hit = inside & (t >= t_min) & (t <= t_max)
            hits += hit.sum(axis=1).astype(np.int32)
            th = np.where(hit, t, np.inf)
            k = th.argmin(axis=1) if n else np.zeros(0, dtype=np.int64)      # the first of equals: the lowest index
            better = th[rows, k] < t_best                                     # strict: an earlier block keeps a tie
            u, w = a[rows, k] / det[rows, k], b[rows, k] / det[rows, k]
            t_best = np.where(better, th[rows, k], t_best)
            face = np.where(better, idx[k], face).astype(np.int32)
            weights = np.where(better[:, None], np.stack([(1.0 - u) - w, u, w], axis=1), weights)
    got = face >= 0
    if got.any():
        normal[got] = C.face_normals(v, F[face[got]])
    t_best[~ray_ok], face[~ray_ok], hits[~ray_ok] = np.nan, -1, 0
    weights[~ray_ok], normal[~ray_ok] = np.nan, 0.0
    return dict(t=t_best, face=face, weights=weights, hits=hits, normal=normal, status=status)


def hit_points(O, D, t):
    """O + t D in fp64, one multiply and one add per axis; NaN for a miss (t = +inf) and for a NaN t."""
    O, D = np.asarray(O).astype(np.float64).reshape(-1, 3), np.asarray(D).astype(np.float64).reshape(-1, 3)
    t = np.asarray(t, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isfinite(t)[:, None], O + np.where(np.isfinite(t), t, 0.0)[:, None] * D, np.nan)


def cube(lid=True):
    """(V [8,3], F [12,3] or [10,3] int32): the unit cube [0,1]^3 wound outward, vertex 4x + 2y + z; its last two faces are
    the lid z = 1, left out with lid=False."""
    V = np.array([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], dtype=np.int32)
    return V, (F if lid else F[:10].copy())


def fan():
    """(V [9,3], F [8,3] int32): eight triangles in the plane z = 0 around the vertex (0, 0, 0), the ring on the square of
    half-side 1/2: every coordinate is a small dyadic rational, also in fp32."""
    ring = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]
    V = np.array([[0.0, 0.0, 0.0]] + [[0.5 * x, 0.5 * y, 0.0] for x, y in ring])
    F = np.array([[0, 1 + k, 1 + (k + 1) % 8] for k in range(8)], dtype=np.int32)
    return V, F


# --- exact ---------------------------------------------------------------------------------------------------------
_fr, _fdot, _fsub = PM._fr, PM._fdot, PM._fsub


def _fcross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _bounds(t_min, t_max):
    """(t_min, t_max) as Fractions, None for an infinite one."""
    return tuple(None if np.isinf(x) else Fraction(float(x)) for x in (t_min, t_max))


def ray_tri_exact(o, d, v0, v1, v2):
    """(det, t, u, v) in Fractions, t = u = v = None when det == 0; the ray's line is inside the closed triangle iff
    u >= 0, v >= 0 and u + v <= 1."""
    o, d, v0, v1, v2 = _fr(o), _fr(d), _fr(v0), _fr(v1), _fr(v2)
    e1, e2 = _fsub(v1, v0), _fsub(v2, v0)
    pv = _fcross(d, e2)
    det = _fdot(e1, pv)
    if det == 0:
        return det, None, None, None
    t = _fsub(o, v0)
    q = _fcross(t, e1)
    return det, _fdot(e2, q) / det, _fdot(t, pv) / det, _fdot(d, q) / det


def _in_range(t, lo, hi):
    return (lo is None or t >= lo) and (hi is None or t <= hi)


def ray_mesh_exact(O, D, V, F, t_min=0.0, t_max=np.inf, cull_backfaces=False):
    """Per ray a dict: hits (the number of faces hit), face (the lowest index among the hits of least t, -1 for a miss),
    t, u, v (Fractions of that face, None for a miss).  Finite inputs and in-range indices only."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F).reshape(-1, 3)
    lo, hi = _bounds(t_min, t_max)
    out = []
    for o, d in zip(np.asarray(O).astype(np.float64).reshape(-1, 3), np.asarray(D).astype(np.float64).reshape(-1, 3)):
        best, hits = None, 0
        for j, f in enumerate(F):
            det, t, u, w = ray_tri_exact(o, d, v[f[0]], v[f[1]], v[f[2]])
            if det == 0 or (cull_backfaces and det < 0) or u < 0 or w < 0 or u + w > 1 or not _in_range(t, lo, hi):
                continue
            hits += 1
            if best is None or t < best[1]:
                best = (j, t, u, w)
        out.append(dict(hits=hits, face=-1 if best is None else best[0], t=best and best[1], u=best and best[2], v=best and best[3]))
    return out


def clearance(O, D, V, F, t_min=0.0, t_max=np.inf):
    """[n] bool: the rays no rounding can decide differently, each condition evaluated in exact arithmetic.
      every face with det != 0: each of u, v, 1 - u - v is at least 2^-20 away from 0;
      every face: |det| >= 2^-20 |D| |E1 x E2| (squared on both sides; a zero-area face meets it with 0 >= 0);
      every face the ray's line is inside of: |t - t_min| and |t - t_max| >= 2^-20 max(|t|, |bound|, 1) for a finite bound;
      the hit t of two faces differ by at least 2^-20 max(|t|, |t'|), unless the two rows of F are equal (the same vertices
      in the same order give the same bits, and the lower index wins in both arithmetics).
    Finite inputs and in-range indices only."""
    v = np.asarray(V).astype(np.float64).reshape(-1, 3)
    F = np.asarray(F).reshape(-1, 3)
    lo, hi = _bounds(t_min, t_max)
    bounds = [b for b in (lo, hi) if b is not None]
    normal2 = []                                                        # |E1 x E2|^2 of every face
    for f in F:
        v0, v1, v2 = (_fr(v[f[k]]) for k in range(3))
        n = _fcross(_fsub(v1, v0), _fsub(v2, v0))
        normal2.append(_fdot(n, n))

    def clear(o, d):
        dd = _fdot(_fr(d), _fr(d))
        hit = []                                                        # (t, the face's row of F) of every hit
        for f, nn in zip(F, normal2):
            det, t, u, w = ray_tri_exact(o, d, v[f[0]], v[f[1]], v[f[2]])
            if det * det < CLEAR * CLEAR * dd * nn:
                return False
            if det == 0:
                continue
            if min(abs(u), abs(w), abs(1 - u - w)) < CLEAR:
                return False
            if u > 0 and w > 0 and u + w < 1:
                if any(abs(t - b) < CLEAR * max(abs(t), abs(b), 1) for b in bounds):
                    return False
                if _in_range(t, lo, hi):
                    hit.append((t, tuple(int(x) for x in f)))
        hit.sort(key=lambda e: e[0])
        return all(f0 == f1 or t1 - t0 >= CLEAR * max(abs(t0), abs(t1)) for (t0, f0), (t1, f1) in zip(hit, hit[1:]))

    return np.asarray([clear(o, d) for o, d in zip(np.asarray(O).astype(np.float64).reshape(-1, 3),
                                                   np.asarray(D).astype(np.float64).reshape(-1, 3))], dtype=bool)
