"""numpy fp64 restatement of dpc_render_meshes (include/dpc_render.h), vectorised over (face, sample) pairs: what the GPU
tests compare csrc/dpc_mesh_raster.hip with, byte for byte.  tests/test_mesh_render_host.py holds it to a literal
per-sample, per-face Python loop on small cases.  Every product, sum, division and square root is one numpy operation
on float64 arrays, in the header's order."""
import numpy as np

STATUS_BAD_INDEX, STATUS_NONFINITE, STATUS_NEAR = 1, 8, 32
NEAR = 1e-3
AMBIENT, DIFFUSE = 0.25, 0.75
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
PAIRS_PER_PASS = 1 << 21


def rotate(V, R):
    """r_k = (R_k0 p_0 + R_k1 p_1) + R_k2 p_2 for [n,3] points."""
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    return np.stack([(R[k, 0] * V[:, 0] + R[k, 1] * V[:, 1]) + R[k, 2] * V[:, 2] for k in range(3)], axis=1)


def project(V, R, camera_distance, focal_length, S):
    """(x, y, w, d) of every vertex: pixel coordinates (column, row), 1 / d and d; d is NaN for a non-finite vertex."""
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        r = rotate(V, R)
        d = r[:, 0] + np.float64(camera_distance)
        v = (r[:, 1] * np.float64(focal_length)) / d
        u = (r[:, 2] * np.float64(focal_length)) / d
        x = (u + 0.5) * np.float64(S)
        y = (0.5 - v) * np.float64(S)
        w = 1.0 / d
    d = np.where(np.isfinite(V).all(axis=1), d, np.nan)
    return x, y, w, d


def edge(ax, ay, bx, by, px, py):
    """The edge function of a -> b at p on the lexicographically ordered ends, negated when that swapped them."""
    flip = (bx < ax) | ((bx == ax) & (by < ay))
    cx, cy = np.where(flip, bx, ax), np.where(flip, by, ay)
    ex, ey = np.where(flip, ax, bx), np.where(flip, ay, by)
    g = (ex - cx) * (py - cy) - (ey - cy) * (px - cx)
    return np.where(flip, -g, g)


def sample_pos(s, ss):
    """The position of sample column / row s = pixel * ss + sub-sample."""
    s = np.asarray(s)
    j = s // ss
    return j.astype(np.float64) + ((s - j * ss).astype(np.float64) + 0.5) / np.float64(ss)


def cover(X, Y, Wt, area, px, py):
    """(covered, d) of samples (px, py) for faces with vertex arrays X, Y, Wt [..., 3] and signed area `area`."""
    with np.errstate(all="ignore"):
        e0 = edge(X[..., 1], Y[..., 1], X[..., 2], Y[..., 2], px, py)
        e1 = edge(X[..., 2], Y[..., 2], X[..., 0], Y[..., 0], px, py)
        e2 = edge(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1], px, py)
        inside = ((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0))
        iw = ((e0 / area) * Wt[..., 0] + (e1 / area) * Wt[..., 1]) + (e2 / area) * Wt[..., 2]
        ok = inside & (iw > 0)
        d = 1.0 / iw
    return ok, d


def _clamp(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(np.int64)


def face_checks(F, mat, n_verts, n_mats, x, y, d):
    """(valid [f] bool, status bits) of the header's guards."""
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    mat = np.asarray(mat, dtype=np.int64).reshape(-1)
    bad = ((F < 0) | (F >= n_verts)).any(axis=1) | (mat < 0) | (mat >= n_mats)
    Fs = np.where(bad[:, None], 0, F)
    if n_verts == 0:
        return np.zeros(len(F), dtype=bool), (STATUS_BAD_INDEX if len(F) else 0)
    dd, xx, yy = d[Fs], x[Fs], y[Fs]
    nonfinite_d = ~np.isfinite(dd)
    with np.errstate(invalid="ignore"):
        near = ~nonfinite_d & (dd <= NEAR)
    nonfinite_xy = ~nonfinite_d & ~near & ~(np.isfinite(xx) & np.isfinite(yy))
    nf = ((nonfinite_d | nonfinite_xy).any(axis=1)) & ~bad
    nr = near.any(axis=1) & ~bad
    status = (STATUS_BAD_INDEX if bad.any() else 0) | (STATUS_NONFINITE if nf.any() else 0) | (STATUS_NEAR if nr.any() else 0)
    return ~(bad | nf | nr), status


def shade(V, F, R):
    """ambient + diffuse |n_0| / |n| per face, n the camera-space face normal."""
    r = rotate(V, R)
    r0, r1, r2 = r[F[:, 0]], r[F[:, 1]], r[F[:, 2]]
    e1, e2 = r1 - r0, r2 - r0
    n0 = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    n1 = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    n2 = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    nn = np.sqrt((n0 * n0 + n1 * n1) + n2 * n2)
    with np.errstate(all="ignore"):
        cn = np.where(nn > 0, np.abs(n0) / nn, 0.0)
    return AMBIENT + DIFFUSE * cn


def sample_keys(V, F, mat, n_mats, R, camera_distance, focal_length, S, ss):
    """The per-sample minimum keys [n,n] uint64 (EMPTY: background), the status bits and (x, y, w) of the vertices."""
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    n = S * ss
    x, y, w, d = project(V, R, camera_distance, focal_length, S)
    valid, status = face_checks(F, mat, len(V), n_mats, x, y, d)
    keys = np.full(n * n, EMPTY, dtype=np.uint64)
    ids = np.nonzero(valid)[0]
    if len(ids):
        Fv = F[ids]
        X, Y = x[Fv], y[Fv]
        area = edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
        s = np.float64(ss)
        x0 = _clamp(np.floor(X.min(axis=1) * s - 0.5) - 1.0, -1, n)
        x1 = _clamp(np.ceil(X.max(axis=1) * s - 0.5) + 1.0, -1, n)
        y0 = _clamp(np.floor(Y.min(axis=1) * s - 0.5) - 1.0, -1, n)
        y1 = _clamp(np.ceil(Y.max(axis=1) * s - 0.5) + 1.0, -1, n)
        x0, x1, y0, y1 = np.maximum(x0, 0), np.minimum(x1, n - 1), np.maximum(y0, 0), np.minimum(y1, n - 1)
        live = (area != 0) & (x0 <= x1) & (y0 <= y1)
        ids, x0, x1, y0, y1, area = ids[live], x0[live], x1[live], y0[live], y1[live], area[live]
        bw = x1 - x0 + 1
        cnt = bw * (y1 - y0 + 1)
        start = 0
        while start < len(ids):
            stop = start + max(1, int(np.searchsorted(np.cumsum(cnt[start:]), PAIRS_PER_PASS, side="right")))
            sl = slice(start, stop)
            c = cnt[sl]
            which = np.repeat(np.arange(start, stop), c)
            e = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
            dy = e // bw[which]
            sx, sy = x0[which] + (e - dy * bw[which]), y0[which] + dy
            Fw = F[ids[which]]
            ok, dd = cover(x[Fw], y[Fw], w[Fw], area[which], sample_pos(sx, ss), sample_pos(sy, ss))
            with np.errstate(over="ignore"):
                bits = dd[ok].astype(np.float32).view(np.uint32).astype(np.uint64)
            np.minimum.at(keys, (sy * n + sx)[ok], (bits << np.uint64(32)) | ids[which][ok].astype(np.uint64))
            start = stop
    return keys.reshape(n, n), status, (x, y, w)


def render(V, F, mat, Kd, R, camera_distance, focal_length, S, ss):
    """One view: (rgba [S,S,4] uint8, depth [S,S] uint16, face_id [S,S] int32, status bits, covered [S,S] int)."""
    V = np.asarray(V, dtype=np.float64).reshape(-1, 3)
    F = np.asarray(F, dtype=np.int64).reshape(-1, 3)
    mat = np.asarray(mat, dtype=np.int64).reshape(-1)
    Kd = np.asarray(Kd, dtype=np.float64).reshape(-1, 3)
    keys, status, (x, y, w) = sample_keys(V, F, mat, len(Kd), R, camera_distance, focal_length, S, ss)
    n = S * ss
    hit = keys != EMPTY
    face = np.where(hit, keys & np.uint64(0xFFFFFFFF), 0).astype(np.int64)
    acc = np.zeros((S, S, 3))
    covered = np.zeros((S, S), dtype=np.int64)
    best = np.full((S, S), EMPTY, dtype=np.uint64)
    best_d = np.zeros((S, S))
    if hit.any():
        Fs = np.where(hit[..., None], F[face] if len(F) else 0, 0)
        col = np.zeros((n, n, 3))
        sh = np.zeros(len(F))
        used = np.unique(face[hit])
        sh[used] = shade(V, F[used], R)
        col[hit] = Kd[mat[face[hit]]] * sh[face[hit]][:, None]
        sy, sx = np.mgrid[0:n, 0:n]
        X, Y, Wt = x[Fs], y[Fs], w[Fs]
        area = edge(X[..., 0], Y[..., 0], X[..., 1], Y[..., 1], X[..., 2], Y[..., 2])
        _, dd = cover(X, Y, Wt, area, sample_pos(sx, ss), sample_pos(sy, ss))
        for a in range(ss):
            for b in range(ss):
                h, k = hit[a::ss, b::ss], keys[a::ss, b::ss]
                acc = acc + np.where(h[..., None], col[a::ss, b::ss], 0.0)
                covered = covered + h
                better = h & (k < best)
                best = np.where(better, k, best)
                best_d = np.where(better, dd[a::ss, b::ss], best_d)
    any_ = covered > 0
    rgba = np.zeros((S, S, 4), dtype=np.uint8)
    with np.errstate(all="ignore"):
        v = acc / np.maximum(covered, 1)[..., None].astype(np.float64)
        v = np.where(v > 1.0, 1.0, np.where(v >= 0.0, v, 0.0))
        rgba[..., :3] = np.where(any_[..., None], np.floor(255.0 * v + 0.5), 0.0).astype(np.uint8)
        rgba[..., 3] = np.floor(255.0 * (covered.astype(np.float64) / np.float64(ss * ss)) + 0.5).astype(np.uint8)
        q = np.floor(best_d / 10.0 * 65535.0 + 0.5)
        depth = np.where(any_, np.where(q > 65535.0, 65535.0, q), 65535.0).astype(np.uint16)
    face_id = np.where(any_, (best & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    return rgba, depth, face_id, status, covered


def render_views(scenes, views, S, ss):
    """scenes: [(V, F, mat, Kd)]; views: [(scene index, R, camera_distance, focal_length)].  Stacked outputs and the
    OR of the status bits."""
    out = [render(*scenes[m], R, cd, f, S, ss) for m, R, cd, f in views]
    status = 0
    for o in out:
        status |= o[3]
    stack = lambda k, shape, dt: np.stack([o[k] for o in out]) if out else np.zeros((0,) + shape, dtype=dt)
    return stack(0, (S, S, 4), np.uint8), stack(1, (S, S), np.uint16), stack(2, (S, S), np.int32), status


def covered_from_alpha(alpha, ss):
    """The covered-sample count behind an alpha byte (floor(255 c / ss^2 + 0.5) is injective in c for ss <= 4)."""
    table = {int(np.floor(255.0 * (c / (ss * ss)) + 0.5)): c for c in range(ss * ss + 1)}
    return np.vectorize(table.__getitem__, otypes=[np.int64])(np.asarray(alpha))


def box_mesh(boxes):
    """Triangle mesh (V, F, material) of axis-aligned boxes [(lo (3), hi (3))]: 12 faces each, material = box index."""
    V, F, mat = [], [], []
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    for k, (lo, hi) in enumerate(boxes):
        o = len(V)
        V += [[(lo, hi)[(c >> 2) & 1][0], (lo, hi)[(c >> 1) & 1][1], (lo, hi)[c & 1][2]] for c in range(8)]
        for a, b, c, d in quads:
            F += [[o + a, o + b, o + c], [o + a, o + c, o + d]]
            mat += [k, k]
    return np.array(V, dtype=np.float64), np.array(F, dtype=np.int64), np.array(mat, dtype=np.int64)


def sample_surface(V, F, count, seed):
    """`count` points on the faces of a mesh, uniform by area (numpy default_rng(seed))."""
    rng = np.random.default_rng(seed)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    f = rng.choice(len(F), size=count, p=area / area.sum())
    s, t = rng.random(count), rng.random(count)
    fold = s + t > 1.0
    s, t = np.where(fold, 1.0 - s, s), np.where(fold, 1.0 - t, t)
    return a[f] + s[:, None] * (b[f] - a[f]) + t[:, None] * (c[f] - a[f])


def grid_mesh(n, seed=0, half=0.4):
    """A height field of n x n quads (2 n^2 faces that share their edges exactly) over [-half, half]^2 in (x, z), with a
    smooth bump in y; material = the quad's row parity."""
    g = np.linspace(-half, half, n + 1)
    X, Z = np.meshgrid(g, g, indexing="ij")
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(2.0, 5.0, 2)
    Y = 0.08 * np.sin(a * X) * np.cos(b * Z) + 0.05 * X
    V = np.stack([X, Y, Z], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v00 = (i * (n + 1) + j).reshape(-1)
    v01, v10, v11 = v00 + 1, v00 + n + 1, v00 + n + 2
    F = np.stack([np.stack([v00, v10, v11], axis=1), np.stack([v00, v11, v01], axis=1)], axis=1).reshape(-1, 3)
    mat = np.repeat((i.reshape(-1) & 1), 2)
    return V, F.astype(np.int64), mat.astype(np.int64)


def rotation_of(cam_pos):
    from dpc.render import view_rotation

    return view_rotation(cam_pos)


def camera_space(R, r):
    """The .obj-space points whose camera-space coordinates are r [n,3]: p = R^T r."""
    return np.asarray(r, dtype=np.float64) @ np.asarray(R, dtype=np.float64)


def special_scenes(R):
    """Small scenes built in the camera space of rotation R (camera at r_0 = -2, image plane |r_1|, |r_2| <~ 0.53):
    {name: (V, F, material, Kd)}."""
    P = lambda r: camera_space(R, r)
    two = np.array([[0.9, 0.1, 0.1], [0.1, 0.2, 0.9]])
    sq = lambda x0, c, h: [[x0, c[0] - h, c[1] - h], [x0, c[0] + h, c[1] - h], [x0, c[0] + h, c[1] + h], [x0, c[0] - h, c[1] + h]]
    out = {}
    out["one face"] = (P([[0.0, -0.2, -0.3], [0.1, 0.3, -0.1], [-0.1, 0.0, 0.35]]), [[0, 1, 2]], [0], two[:1])
    # two coplanar copies of a square (ties -> the lower index) and a second winding
    out["coplanar duplicates"] = (P(sq(0.0, (0.0, 0.0), 0.25)), [[0, 1, 2], [0, 2, 3], [2, 1, 0], [0, 2, 3]], [0, 0, 1, 1], two)
    out["parallel squares"] = (P(sq(-0.2, (0.05, 0.0), 0.2) + sq(0.2, (-0.05, 0.05), 0.2)),
                               [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], [0, 0, 1, 1], two)
    out["sliver"] = (P([[0.0, -0.4, -0.4], [0.0, 0.4, 0.4001], [0.0, 0.4, 0.4], [0.1, -0.3, 0.2], [0.1, -0.3, 0.2000001],
                        [0.1, 0.35, -0.3]]), [[0, 1, 2], [3, 4, 5]], [0, 1], two)
    out["partly and wholly outside"] = (P([[0.0, 0.2, 0.2], [0.0, 1.5, 0.3], [0.0, 0.3, 1.4], [0.0, 2.0, 2.0], [0.0, 2.5, 2.0],
                                           [0.0, 2.0, 2.6], [0.3, -3.0, -3.0], [0.3, 3.0, -3.0], [0.3, 0.0, 3.0]]),
                                        [[0, 1, 2], [3, 4, 5], [6, 7, 8]], [0, 1, 1], two)
    out["empty"] = (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.int64), two[:1])
    out["zero area"] = (P([[0.0, -0.2, -0.2], [0.0, 0.0, 0.0], [0.0, 0.2, 0.2], [0.0, 0.1, 0.1]]), [[0, 0, 2], [3, 3, 3]], [0, 0],
                        two[:1])
    return {k: (np.asarray(v[0], dtype=np.float64).reshape(-1, 3), np.asarray(v[1], dtype=np.int64).reshape(-1, 3),
                np.asarray(v[2], dtype=np.int64), np.asarray(v[3], dtype=np.float64)) for k, v in out.items()}


def bad_scenes(R):
    """{name: ((V, F, material, Kd), expected status bit)}: every input the status word reports."""
    P = lambda r: camera_space(R, r)
    tri = P([[0.0, -0.2, -0.3], [0.1, 0.3, -0.1], [-0.1, 0.0, 0.35]])
    kd = np.array([[0.5, 0.5, 0.5]])
    nan = tri.copy()
    nan[1, 2] = np.nan
    inf = tri.copy()
    inf[0, 0] = np.inf
    near = P([[-2.0 + 0.5 * NEAR, 0.0, 0.0], [0.0, 0.3, -0.1], [0.0, 0.0, 0.35]])
    behind = P([[-2.5, 0.0, 0.0], [0.0, 0.3, -0.1], [0.0, 0.0, 0.35]])
    good = [3, 4, 5]
    both = lambda bad: np.concatenate([bad, tri])
    return {"nan vertex": ((both(nan), [[0, 1, 2], good], [0, 0], kd), STATUS_NONFINITE),
            "inf vertex": ((both(inf), [[0, 1, 2], good], [0, 0], kd), STATUS_NONFINITE),
            "index beyond": ((tri, [[0, 1, 3], [0, 1, 2]], [0, 0], kd), STATUS_BAD_INDEX),
            "negative index": ((tri, [[0, -1, 2], [0, 1, 2]], [0, 0], kd), STATUS_BAD_INDEX),
            "material beyond": ((tri, [[0, 1, 2], [0, 1, 2]], [1, 0], kd), STATUS_BAD_INDEX),
            "negative material": ((tri, [[0, 1, 2], [0, 1, 2]], [-1, 0], kd), STATUS_BAD_INDEX),
            "near guard": ((both(near), [[0, 1, 2], good], [0, 0], kd), STATUS_NEAR),
            "behind the camera": ((both(behind), [[0, 1, 2], good], [0, 0], kd), STATUS_NEAR)}
