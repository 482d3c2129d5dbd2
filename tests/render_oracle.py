"""numpy restatement of dpc_render_points (include/dpc_render.h): ids, float32 and uint8 images of one cloud, bit for bit.

Elementwise numpy operations in the header's order (no np.dot, @, einsum or np.linalg.norm: BLAS may fuse).  Each point's
hits are computed over its sample box only (the conservative bound of csrc/dpc_raster.hip's rs_box), all points of a
group at once, and merged into the per-sample key array with np.minimum.at: the minimum is order-independent, so the
result is the exhaustive per-sample minimum whatever the grouping.

    scene_points   prediction-frame points -> the renderer's scene frame (p2, -p0, p1)
    render         one cloud under one camera frame -> (image float32 [S,S,3], ids int32 [S ss,S ss])
    to_uint8       floor(255 clip(v, 0, 1) + 0.5)
"""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
GREY = 0.5
PAIRS_PER_GROUP = 1 << 22


def scene_points(p):
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    return np.stack([p[:, 2], -p[:, 0], p[:, 1]], axis=1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def sample_dirs(frame, sx, sy, S, ss, F):
    """D of samples (sx, sy) (arrays): (f + (x_s / F) r) + (y_s / F) u."""
    C, r, u, f = frame
    half = S * 0.5
    j, b = sx // ss, sx % ss
    i, a = sy // ss, sy % ss
    xs = (j.astype(np.float64) + (b.astype(np.float64) + 0.5) / float(ss)) - half
    ys = half - (i.astype(np.float64) + (a.astype(np.float64) + 0.5) / float(ss))
    px, py = xs / F, ys / F
    return np.stack([(f[k] + px * r[k]) + py * u[k] for k in range(3)], axis=-1)


def hit(m, c, D):
    """(hit mask, t) of rays D from C against spheres with m = C - P, c = m.m - rad^2."""
    a, b = dot(D, D), dot(m, D)
    disc = b * b - a * c
    with np.errstate(invalid="ignore"):
        t = (-b - np.sqrt(np.where(disc >= 0.0, disc, 0.0))) / a
    return (c > 0.0) & (disc >= 0.0) & (t > 0.0), t


def boxes(frame, P, rad, S, ss, F):
    """rs_box for every point: (x0, x1, y0, y1) int64 arrays, clipped to the image; x0 > x1 when empty."""
    C, r, u, f = frame
    n = S * ss
    q = P - C
    zc, xc, yc = dot(q, f), dot(q, r), dot(q, u)
    R = rad * (1.0 + 1e-6) + 1e-9 * ((np.abs(zc) + np.abs(xc)) + np.abs(yc))
    behind = zc + R < 0.0
    full = ~(zc - R > 1e-6 * (np.abs(zc) + R)) & ~behind
    d1, d2 = zc - R, zc + R
    xa, xb, ya, yb = xc - R, xc + R, yc - R, yc + R
    half, s = S * 0.5, float(ss)
    with np.errstate(all="ignore"):
        xlo = F * (xa / np.where(xa >= 0.0, d2, d1))
        xhi = F * (xb / np.where(xb >= 0.0, d1, d2))
        ylo = F * (ya / np.where(ya >= 0.0, d2, d1))
        yhi = F * (yb / np.where(yb >= 0.0, d1, d2))
        cl = lambda x: np.clip(np.nan_to_num(x, nan=0.0, posinf=n, neginf=-1), -1, n).astype(np.int64)
        x0 = cl(np.floor((xlo + half) * s - 0.5) - 1.0)
        x1 = cl(np.ceil((xhi + half) * s - 0.5) + 1.0)
        y0 = cl(np.floor((half - yhi) * s - 0.5) - 1.0)
        y1 = cl(np.ceil((half - ylo) * s - 0.5) + 1.0)
    x0, x1 = np.where(full, 0, x0), np.where(full, n - 1, x1)
    y0, y1 = np.where(full, 0, y0), np.where(full, n - 1, y1)
    x0, x1 = np.where(behind, 1, x0), np.where(behind, 0, x1)
    return np.maximum(x0, 0), np.minimum(x1, n - 1), np.maximum(y0, 0), np.minimum(y1, n - 1)


def finite(P, colors, radii):
    ok = bool(np.isfinite(P).all())
    if colors is not None:
        ok = ok and bool(np.isfinite(colors).all())
    if radii is not None:
        ok = ok and bool(np.isfinite(radii).all()) and bool((radii > 0).all())
    return ok


def keys_of(P, frame, S, ss, F, radius, radii=None):
    """The per-sample minimum keys [S ss * S ss] uint64 (EMPTY: background)."""
    n = S * ss
    keys = np.full(n * n, EMPTY, dtype=np.uint64)
    if len(P) == 0:
        return keys
    C = frame[0]
    rad = np.full(len(P), float(radius)) if radii is None else np.asarray(radii, dtype=np.float64)
    x0, x1, y0, y1 = boxes(frame, P, rad, S, ss, F)
    w, h = x1 - x0 + 1, y1 - y0 + 1
    area = np.where((w > 0) & (h > 0), w * h, 0)
    live = np.nonzero(area)[0]
    m_all = C - P
    c_all = dot(m_all, m_all) - rad * rad
    g0 = 0
    while g0 < len(live):  # groups of points whose boxes hold at most PAIRS_PER_GROUP samples (at least one point)
        csum = np.cumsum(area[live[g0:]])
        g1 = g0 + max(1, int(np.searchsorted(csum, PAIRS_PER_GROUP, side="right")))
        idx = live[g0:g1]
        cnt = area[idx]
        pk = np.repeat(idx, cnt)
        e = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        dy, dx = e // w[pk], e % w[pk]
        sx, sy = x0[pk] + dx, y0[pk] + dy
        D = sample_dirs(frame, sx, sy, S, ss, F)
        ok, t = hit(m_all[pk], c_all[pk], D)
        key = (t[ok].astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | pk[ok].astype(np.uint64)
        np.minimum.at(keys, sy[ok] * n + sx[ok], key)
        g0 = g1
    return keys


def shade(P, frame, S, ss, F, radius, keys, colors=None, radii=None):
    """Sample colours [S ss, S ss, 3] fp64 and ids [S ss, S ss] int32 from the keys."""
    n = S * ss
    C = frame[0]
    col = np.ones((n * n, 3))
    ids = np.full(n * n, -1, dtype=np.int32)
    s = np.nonzero(keys != EMPTY)[0]
    if len(s):
        k = (keys[s] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        ids[s] = k
        rad = np.full(len(P), float(radius)) if radii is None else np.asarray(radii, dtype=np.float64)
        Pk, rk = P[k], rad[k]
        m = C - Pk
        D = sample_dirs(frame, s % n, s // n, S, ss, F)
        _, t = hit(m, dot(m, m) - rk * rk, D)
        nd = np.sqrt(dot(D, D))
        H = C + t[:, None] * D
        nrm = (H - Pk) / rk[:, None]
        v = -D / nd[:, None]
        nv = dot(nrm, v)
        sh = 0.4 + 0.6 * np.where(nv > 0.0, nv, 0.0)
        alb = np.full((len(s), 3), GREY) if colors is None else np.asarray(colors, dtype=np.float32)[k].astype(np.float64)
        col[s] = alb * sh[:, None]
    return col.reshape(n, n, 3), ids.reshape(n, n)


def pixels(col, S, ss):
    """The ss^2 sample colours of every pixel summed in row-major (a, b) order onto 0.0, divided once, float32."""
    c = col.reshape(S, ss, S, ss, 3)
    acc = np.zeros((S, S, 3))
    for a in range(ss):
        for b in range(ss):
            acc = acc + c[:, a, :, b, :]
    return (acc / float(ss * ss)).astype(np.float32)


def render(points, frame, S, ss, F, radius=0.01, colors=None, radii=None, scene=False):
    """One cloud ([n,3] prediction-frame points, or scene-frame with scene=True) -> (image float32 [S,S,3], ids int32)."""
    frame = tuple(np.asarray(x, dtype=np.float64) for x in frame)
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3) if scene else scene_points(points)
    if not finite(P, colors, radii):
        return np.ones((S, S, 3), dtype=np.float32), np.full((S * ss, S * ss), -1, dtype=np.int32)
    keys = keys_of(P, frame, S, ss, F, radius, radii)
    col, ids = shade(P, frame, S, ss, F, radius, keys, colors, radii)
    return pixels(col, S, ss), ids


def to_uint8(image):
    return np.floor(np.clip(image.astype(np.float64), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
