"""numpy fp64 restatement of dpc_render_meshes_shaded (include/dpc_render.h): mesh_render_oracle's geometry (project, edge,
cover, sample_keys: the same keys, depth, alpha and face ids) and the header's texture and smooth-normal block for the
colour of a covered sample.  What the GPU tests compare csrc/dpc_mesh_raster.hip's shaded entry with, byte for byte;
tests/test_mesh_shade_host.py holds it to a literal per-sample Python loop.  Every product, sum, division, floor and
square root is one numpy operation on float64 arrays, in the header's order.

A scene here is (V, F, material, Kd) followed by (uv, face_uv, normals, face_vn, mat_tex, textures); a scene of four
entries has no attributes."""
import numpy as np

import mesh_render_oracle as O

PATHS = ("textured", "wrapped", "smooth", "uv_missing", "no_texture", "vn_missing", "vn_zero")


def attributes(scene):
    """(uv [n,2], face_uv [f,3], normals [n,3], face_vn [f,3], mat_tex [k], textures) of a scene; all -1 for a plain one."""
    F = np.asarray(scene[1], dtype=np.int64).reshape(-1, 3)
    k = len(np.asarray(scene[3], dtype=np.float64).reshape(-1, 3))
    if len(scene) < 10:
        none = np.full((len(F), 3), -1, dtype=np.int64)
        return np.zeros((0, 2)), none, np.zeros((0, 3)), none, np.full(k, -1, dtype=np.int64), []
    uv, fuv, vn, fvn, mt, tex = scene[4:10] if not hasattr(scene, "face_uv") else \
        (scene.uv, scene.face_uv, scene.normals, scene.face_vn, scene.mat_tex, scene.textures)
    return (np.asarray(uv, dtype=np.float64).reshape(-1, 2), np.asarray(fuv, dtype=np.int64).reshape(-1, 3),
            np.asarray(vn, dtype=np.float64).reshape(-1, 3), np.asarray(fvn, dtype=np.int64).reshape(-1, 3),
            np.asarray(mt, dtype=np.int64).reshape(-1), [np.asarray(t, dtype=np.uint8) for t in tex])


def attribute_checks(F, mat, n_verts, n_mats, uv, fuv, vn, fvn, mt, n_tex):
    """(bad [f], nonfinite [f]) of the shaded entry's own guards, for faces whose vertex and material indices are good:
    an index below -1 or outside its range; a named uv or normal that is not finite."""
    geom_bad = ((F < 0) | (F >= n_verts)).any(axis=1) | (mat < 0) | (mat >= n_mats)
    bad = ((fuv < -1) | (fuv >= len(uv))).any(axis=1) | ((fvn < -1) | (fvn >= len(vn))).any(axis=1)
    t = mt[np.where(geom_bad, 0, mat)] if n_mats else np.zeros(len(F), dtype=np.int64)
    bad = (bad | (t < -1) | (t >= n_tex)) & ~geom_bad
    fin = np.ones((len(F), 3), dtype=bool)
    if len(uv):
        fin &= (fuv < 0) | (fuv >= len(uv)) | np.isfinite(uv[np.clip(fuv, 0, len(uv) - 1)]).all(axis=-1)
    if len(vn):
        fin &= (fvn < 0) | (fvn >= len(vn)) | np.isfinite(vn[np.clip(fvn, 0, len(vn) - 1)]).all(axis=-1)
    return bad, ~fin.all(axis=1) & ~bad & ~geom_bad


def texture_lookup(tex, u, v):
    """The header's repeat-wrapped bilinear filter of one [h,w,3] uint8 texture at finite (u, v) arrays: [n,3] float64."""
    Ht, Wt = tex.shape[:2]
    fu, fv = u - np.floor(u), v - np.floor(v)
    x = fu * np.float64(Wt) - 0.5
    y = (1.0 - fv) * np.float64(Ht) - 0.5
    xf, yf = np.floor(x), np.floor(y)
    ax, ay = x - xf, y - yf
    bx, by = 1.0 - ax, 1.0 - ay
    x0, x1 = np.mod(xf.astype(np.int64), Wt), np.mod(xf.astype(np.int64) + 1, Wt)
    y0, y1 = np.mod(yf.astype(np.int64), Ht), np.mod(yf.astype(np.int64) + 1, Ht)
    T = tex.astype(np.float64) / 255.0
    top = T[y0, x0] * bx[:, None] + T[y0, x1] * ax[:, None]
    bot = T[y1, x0] * bx[:, None] + T[y1, x1] * ax[:, None]
    return top * by[:, None] + bot * ay[:, None]


def render(scene, R, camera_distance, focal_length, S, ss, textures=True, smooth_normals=True):
    """One view: (rgba [S,S,4] uint8, depth [S,S] uint16, face_id [S,S] int32, status bits, paths): paths counts the
    covered samples that took each way through the shading (PATHS)."""
    V = np.asarray(scene[0], dtype=np.float64).reshape(-1, 3)
    F = np.asarray(scene[1], dtype=np.int64).reshape(-1, 3)
    mat = np.asarray(scene[2], dtype=np.int64).reshape(-1)
    Kd = np.asarray(scene[3], dtype=np.float64).reshape(-1, 3)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    uv, fuv, vn, fvn, mt, tex = attributes(scene)
    if not textures:       # the group travels as NULL pointers: none of it is read or checked
        uv, fuv, mt, tex = np.zeros((0, 2)), np.full_like(fuv, -1), np.full_like(mt, -1), []
    if not smooth_normals:
        vn, fvn = np.zeros((0, 3)), np.full_like(fvn, -1)
    # the guards: a face the attribute checks skip keeps its place (the ids) and covers nothing
    bad, nonfinite = attribute_checks(F, mat, len(V), len(Kd), uv, fuv, vn, fvn, mt, len(tex))
    F1 = np.where(bad[:, None], -1, F)
    x, y, w, d = O.project(V, R, camera_distance, focal_length, S)
    _, status = O.face_checks(F1, mat, len(V), len(Kd), x, y, d)
    if nonfinite.any():
        status |= O.STATUS_NONFINITE
    keys, _, _ = O.sample_keys(V, np.where((bad | nonfinite)[:, None], -1, F), mat, len(Kd), R, camera_distance,
                               focal_length, S, ss)
    n = S * ss
    hit = keys != O.EMPTY
    acc = np.zeros((S, S, 3))
    covered = np.zeros((S, S), dtype=np.int64)
    best = np.full((S, S), O.EMPTY, dtype=np.uint64)
    best_d = np.zeros((S, S))
    paths = dict.fromkeys(PATHS, 0)
    if hit.any():
        sy, sx = np.nonzero(hit)
        face = (keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
        Fh = F[face]
        X, Y, Wt = x[Fh], y[Fh], w[Fh]
        px, py = O.sample_pos(sx, ss), O.sample_pos(sy, ss)
        area = O.edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
        _, dd = O.cover(X, Y, Wt, area, px, py)
        with np.errstate(all="ignore"):
            e = [O.edge(X[:, 1], Y[:, 1], X[:, 2], Y[:, 2], px, py), O.edge(X[:, 2], Y[:, 2], X[:, 0], Y[:, 0], px, py),
                 O.edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], px, py)]
            g = [(e[k] / area) * Wt[:, k] for k in range(3)]
            dc = 1.0 / ((g[0] + g[1]) + g[2])
            assert (dc.view(np.uint64) == dd.view(np.uint64)).all()   # the depth the key was made of
            c = [g[k] * dc for k in range(3)]
            sh = np.zeros(len(F))
            used = np.unique(face)
            sh[used] = O.shade(V, F[used], R)
            shade = sh[face]
            rgb = Kd[mat[face]].copy()
            # texture
            tid = mt[mat[face]]
            has_uv = (fuv[face] >= 0).all(axis=1)
            textured = (tid >= 0) & has_uv
            paths["uv_missing"] = int(((tid >= 0) & ~has_uv).sum())
            paths["no_texture"] = int(((tid < 0) & has_uv).sum())
            if textured.any():
                q = uv[np.where(textured[:, None], fuv[face], 0)]
                u = (c[0] * q[:, 0, 0] + c[1] * q[:, 1, 0]) + c[2] * q[:, 2, 0]
                v = (c[0] * q[:, 0, 1] + c[1] * q[:, 1, 1]) + c[2] * q[:, 2, 1]
                textured &= np.isfinite(u) & np.isfinite(v)
                for t in np.unique(tid[textured]):
                    sel = textured & (tid == t)
                    rgb[sel] = texture_lookup(tex[t], u[sel], v[sel])
                paths["textured"] = int(textured.sum())
                paths["wrapped"] = int((textured & ((u < 0) | (u >= 1) | (v < 0) | (v >= 1))).sum())
            # normals
            smooth = (fvn[face] >= 0).all(axis=1)
            paths["vn_missing"] = int(((fvn[face] >= 0).any(axis=1) & ~smooth).sum())
            if smooth.any():
                mrot = O.rotate(vn, R)[np.where(smooth[:, None], fvn[face], 0)]       # [h, corner, component]
                nrm = [(c[0] * mrot[:, 0, k] + c[1] * mrot[:, 1, k]) + c[2] * mrot[:, 2, k] for k in range(3)]
                nn = np.sqrt((nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2])
                ok = smooth & (nn > 0) & np.isfinite(nn)
                shade = np.where(ok, O.AMBIENT + O.DIFFUSE * (np.abs(nrm[0]) / nn), shade)
                paths["smooth"] = int(ok.sum())
                paths["vn_zero"] = int((smooth & ~ok).sum())
        col = np.zeros((n, n, 3))
        col[hit] = rgb * shade[:, None]
        depth_s = np.zeros((n, n))
        depth_s[hit] = dd
        for a in range(ss):
            for b in range(ss):
                h, k = hit[a::ss, b::ss], keys[a::ss, b::ss]
                acc = acc + np.where(h[..., None], col[a::ss, b::ss], 0.0)
                covered = covered + h
                better = h & (k < best)
                best = np.where(better, k, best)
                best_d = np.where(better, depth_s[a::ss, b::ss], best_d)
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
    return rgba, depth, face_id, status, paths


def render_views(scenes, views, S, ss, textures=True, smooth_normals=True):
    """scenes: plain or shaded; views: [(scene index, R, camera_distance, focal_length)].  Stacked rgba, depth, face_id,
    the OR of the status bits and the per-view paths."""
    out = [render(scenes[m], R, cd, f, S, ss, textures, smooth_normals) for m, R, cd, f in views]
    status = 0
    for o in out:
        status |= o[3]
    stack = lambda k, shape, dt: np.stack([o[k] for o in out]) if out else np.zeros((0,) + shape, dtype=dt)
    return stack(0, (S, S, 4), np.uint8), stack(1, (S, S), np.uint16), stack(2, (S, S), np.int32), status, [o[4] for o in out]


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def checker(h, w, seed):
    """A procedural [h,w,3] uint8 texture: coloured checks over a gradient, every texel its own value."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (2, 2, 3))
    i, j = np.mgrid[0:h, 0:w]
    img = base[(i * 4 // max(h, 1)) % 2, (j * 4 // max(w, 1)) % 2].astype(np.int64)
    img = (img + 37 * i[..., None] + 11 * j[..., None] + rng.integers(0, 40, (h, w, 3))) % 256
    return img.astype(np.uint8)


def grid_normals(V, n):
    """Per-vertex normals of O.grid_mesh(n)'s height field by central differences of y over the (x, z) grid, unnormalised
    on purpose (the renderer does not normalise what it is given)."""
    Y = V[:, 1].reshape(n + 1, n + 1)
    X, Z = V[:, 0].reshape(n + 1, n + 1), V[:, 2].reshape(n + 1, n + 1)
    dy_dx = np.gradient(Y, axis=0) / np.gradient(X, axis=0)
    dy_dz = np.gradient(Y, axis=1) / np.gradient(Z, axis=1)
    return np.stack([-dy_dx, np.ones_like(Y), -dy_dz], axis=-1).reshape(-1, 3)


def shaded_grid(n, seed, textures, uv_range=(0.0, 1.0), with_uv=True, with_vn=True, mat_tex=(0, -1), Kd=None):
    """O.grid_mesh(n) with one uv and one normal per vertex (face_uv = face_vn = F); uvs span uv_range over the grid."""
    V, F, mat = O.grid_mesh(n, seed=seed)
    g = np.linspace(uv_range[0], uv_range[1], n + 1)
    U, W = np.meshgrid(g, g, indexing="ij")
    uv = np.stack([U, W], axis=-1).reshape(-1, 2)
    none = np.full_like(F, -1)
    Kd = np.array([[0.3, 0.3, 0.9], [0.9, 0.9, 0.2]]) if Kd is None else Kd
    return (V, F, mat, Kd, uv if with_uv else np.zeros((0, 2)), F.copy() if with_uv else none,
            grid_normals(V, n) if with_vn else np.zeros((0, 3)), F.copy() if with_vn else none,
            np.asarray(mat_tex, dtype=np.int64), list(textures))
