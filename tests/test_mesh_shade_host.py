"""Host side of the textured, smooth-shaded training views (dpc_render_meshes_shaded, dpc.render.meshviews): the numpy
oracle of tests/mesh_shade_oracle.py against a literal per-sample Python loop and, without attributes, against
mesh_render_oracle; two checks of the texture's orientation and of the perspective correction that share none of the
oracle's conventions; the .obj / .mtl / map_Kd reader; the entry point's refusals before any launch."""
import ctypes
import math

import numpy as np
import pytest

import mesh_render_oracle as O
import mesh_shade_oracle as SO
import test_mesh_render_host as H
from dpc.render import _native
from dpc.render import meshviews as M
from dpc.render import visualise as V

CAM = H.CAM


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against a literal loop
# ---------------------------------------------------------------------------------------------------------------------
def literal(scene, R, cd, f, S, ss):
    """include/dpc_render.h's dpc_render_meshes_shaded as a plain loop over every sample and every face, Python floats."""
    Vx, F, mat, Kd = scene[:4]
    uv, fuv, vn, fvn, mt, tex = SO.attributes(scene)
    uv, vn, Kd = uv.tolist(), vn.tolist(), np.asarray(Kd, dtype=np.float64).reshape(-1, 3).tolist()
    fuv, fvn, mt = fuv.tolist(), fvn.tolist(), mt.tolist()
    R = [[float(x) for x in row] for row in np.asarray(R).reshape(3, 3)]
    rot = lambda p: [(R[k][0] * p[0] + R[k][1] * p[1]) + R[k][2] * p[2] for k in range(3)]
    verts = []
    for p in np.asarray(Vx, dtype=np.float64).reshape(-1, 3):
        p = [float(c) for c in p]
        r = rot(p)
        d = r[0] + cd
        if not all(math.isfinite(c) for c in p):
            verts.append((math.nan, math.nan, math.nan, math.nan, r))
        elif d == 0.0:
            verts.append((math.inf, math.inf, math.inf, d, r))
        else:
            verts.append((((r[2] * f) / d + 0.5) * S, (0.5 - (r[1] * f) / d) * S, 1.0 / d, d, r))

    def edge(a, b, p):
        flip = b[0] < a[0] or (b[0] == a[0] and b[1] < a[1])
        c, e = (b, a) if flip else (a, b)
        g = (e[0] - c[0]) * (p[1] - c[1]) - (e[1] - c[1]) * (p[0] - c[0])
        return -g if flip else g

    status, faces = 0, []
    for k, (tri, m) in enumerate(zip(np.asarray(F).reshape(-1, 3).tolist(), np.asarray(mat).reshape(-1).tolist())):
        if any(i < 0 or i >= len(verts) for i in tri) or m < 0 or m >= len(Kd):
            status |= 1
            continue
        if (any(i < -1 or i >= len(uv) for i in fuv[k]) or any(i < -1 or i >= len(vn) for i in fvn[k])
                or mt[m] < -1 or mt[m] >= len(tex)):
            status |= 1
            continue
        bits = 0
        for i in tri:
            x, y, w, d, _ = verts[i]
            if not math.isfinite(d):
                bits |= 8
            elif d <= 1e-3:
                bits |= 32
            elif not (math.isfinite(x) and math.isfinite(y)):
                bits |= 8
        if any(i >= 0 and not all(math.isfinite(c) for c in uv[i]) for i in fuv[k]):
            bits |= 8
        if any(i >= 0 and not all(math.isfinite(c) for c in vn[i]) for i in fvn[k]):
            bits |= 8
        status |= bits
        if bits:
            continue
        v = [verts[i] for i in tri]
        area = edge(v[0], v[1], v[2])
        if area != 0.0:
            faces.append((k, v, area, m))

    def cover(v, area, px, py):
        e = [edge(v[1], v[2], (px, py)), edge(v[2], v[0], (px, py)), edge(v[0], v[1], (px, py))]
        if not (all(x >= 0 for x in e) or all(x <= 0 for x in e)):
            return None
        g = [(e[q] / area) * v[q][2] for q in range(3)]
        iw = (g[0] + g[1]) + g[2]
        return (1.0 / iw, g) if iw > 0 else None

    def texel(img, row, col, ch):
        return float(img[row % img.shape[0], col % img.shape[1], ch]) / 255.0

    pos = lambda s: (s // ss) + ((s % ss) + 0.5) / ss
    rgba = np.zeros((S, S, 4), dtype=np.uint8)
    depth = np.full((S, S), 65535, dtype=np.uint16)
    fid = np.full((S, S), -1, dtype=np.int32)
    for i in range(S):
        for j in range(S):
            acc, covered, best = [0.0, 0.0, 0.0], 0, None
            for a in range(ss):
                for b in range(ss):
                    px, py = pos(j * ss + b), pos(i * ss + a)
                    win = None
                    for k, v, area, m in faces:
                        hit = cover(v, area, px, py)
                        if hit is None:
                            continue
                        with np.errstate(over="ignore"):
                            key = (int(np.float32(hit[0]).view(np.uint32)) << 32) | k
                        if win is None or key < win[0]:
                            win = (key, hit[0], hit[1], v, m, k)
                    if win is None:
                        continue
                    key, d, g, v, m, k = win
                    r0, r1, r2 = v[0][4], v[1][4], v[2][4]
                    e1 = [r1[c] - r0[c] for c in range(3)]
                    e2 = [r2[c] - r0[c] for c in range(3)]
                    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
                    nn = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                    shade = 0.25 + 0.75 * (abs(n[0]) / nn if nn > 0 else 0.0)
                    c = [g[q] * d for q in range(3)]
                    rgb = [float(x) for x in Kd[m]]
                    if mt[m] >= 0 and min(fuv[k]) >= 0:
                        q = [uv[t] for t in fuv[k]]
                        tu = (c[0] * q[0][0] + c[1] * q[1][0]) + c[2] * q[2][0]
                        tv = (c[0] * q[0][1] + c[1] * q[1][1]) + c[2] * q[2][1]
                        if math.isfinite(tu) and math.isfinite(tv):
                            img = tex[mt[m]]
                            fu, fv = tu - math.floor(tu), tv - math.floor(tv)
                            x = fu * float(img.shape[1]) - 0.5
                            y = (1.0 - fv) * float(img.shape[0]) - 0.5
                            x0, y0 = math.floor(x), math.floor(y)
                            ax, ay = x - x0, y - y0
                            bx, by = 1.0 - ax, 1.0 - ay
                            for ch in range(3):
                                top = texel(img, y0, x0, ch) * bx + texel(img, y0, x0 + 1, ch) * ax
                                bot = texel(img, y0 + 1, x0, ch) * bx + texel(img, y0 + 1, x0 + 1, ch) * ax
                                rgb[ch] = top * by + bot * ay
                    if min(fvn[k]) >= 0:
                        mk = [rot(vn[t]) for t in fvn[k]]
                        nrm = [(c[0] * mk[0][q] + c[1] * mk[1][q]) + c[2] * mk[2][q] for q in range(3)]
                        sq = (nrm[0] * nrm[0] + nrm[1] * nrm[1]) + nrm[2] * nrm[2]
                        ln = math.sqrt(sq) if sq >= 0 else math.nan
                        if ln > 0 and math.isfinite(ln):
                            shade = 0.25 + 0.75 * (abs(nrm[0]) / ln)
                    for ch in range(3):
                        acc[ch] = acc[ch] + rgb[ch] * shade
                    covered += 1
                    if best is None or key < best[0]:
                        best = (key, d)
            if covered:
                for ch in range(3):
                    x = acc[ch] / covered
                    x = 1.0 if x > 1.0 else (x if x >= 0.0 else 0.0)
                    rgba[i, j, ch] = int(math.floor(255.0 * x + 0.5))
                rgba[i, j, 3] = int(math.floor(255.0 * (covered / (ss * ss)) + 0.5))
                depth[i, j] = int(min(65535.0, math.floor(best[1] / 10.0 * 65535.0 + 0.5)))
                fid[i, j] = best[0] & 0xFFFFFFFF
    return rgba, depth, fid, status


def bad_attribute_scenes(R):
    """{name: (scene, expected status bit)}: every input the shaded entry's own guards report; face 1 is always good."""
    P = lambda r: O.camera_space(R, r)
    tri = P([[0.0, -0.2, -0.3], [0.1, 0.3, -0.1], [-0.1, 0.0, 0.35], [0.05, -0.3, 0.1]])
    F, mat, kd = [[0, 1, 2], [0, 2, 3]], [0, 1], np.array([[0.5, 0.6, 0.7], [0.9, 0.3, 0.2]])
    uv = np.array([[0.1, 0.2], [0.9, 0.1], [0.4, 0.8]])
    vn = np.array([[1.0, 0.2, 0.1], [0.9, -0.1, 0.3], [1.0, 0.0, -0.2]])
    tex = [SO.checker(3, 4, 0)]
    ok = [[0, 1, 2], [0, 2, 1]]

    def scene(uv=uv, fuv=ok, vn=vn, fvn=ok, mt=(0, 0), tex=tex):
        return (tri, F, mat, kd, np.asarray(uv, dtype=np.float64), fuv, np.asarray(vn, dtype=np.float64), fvn, list(mt), tex)

    nan_uv, inf_vn = uv.copy(), vn.copy()
    nan_uv[1, 0], inf_vn[0, 2] = np.nan, np.inf
    return {"uv index beyond": (scene(fuv=[[0, 1, 3], ok[1]]), O.STATUS_BAD_INDEX),
            "uv index below -1": (scene(fuv=[[0, -2, 2], ok[1]]), O.STATUS_BAD_INDEX),
            "vn index beyond": (scene(fvn=[[3, 1, 2], ok[1]]), O.STATUS_BAD_INDEX),
            "vn index below -1": (scene(fvn=[[0, 1, -5], ok[1]]), O.STATUS_BAD_INDEX),
            "texture index beyond": (scene(mt=(1, 0)), O.STATUS_BAD_INDEX),
            "texture index below -1": (scene(mt=(-2, -1)), O.STATUS_BAD_INDEX),
            "nan uv": (scene(uv=nan_uv, fuv=[[0, 1, 2], [0, 2, 0]]), O.STATUS_NONFINITE),
            "inf normal": (scene(vn=inf_vn, fvn=[[0, 1, 2], [1, 2, 1]]), O.STATUS_NONFINITE)}


def small_shaded_scenes():
    R = O.rotation_of(CAM)
    tex = [SO.checker(3, 5, 1), SO.checker(1, 1, 2), SO.checker(4, 4, 3)]
    scenes = {}
    scenes["grid wrapped"] = SO.shaded_grid(3, 0, tex[:1], uv_range=(-0.6, 1.7), mat_tex=(0, 0))
    scenes["grid one textured material"] = SO.shaded_grid(2, 1, tex, uv_range=(0.1, 0.9), mat_tex=(2, -1))
    scenes["grid texture only"] = SO.shaded_grid(2, 2, tex[1:2], with_vn=False, mat_tex=(0, 0))
    scenes["grid normals only"] = SO.shaded_grid(3, 3, [], with_uv=False, mat_tex=(-1, -1))
    Vg, F, mat, Kd, uv, fuv, vn, fvn, mt, tx = SO.shaded_grid(3, 4, tex[:1], uv_range=(-1.0, 2.0), mat_tex=(0, 0))
    fuv, fvn, vn = fuv.copy(), fvn.copy(), vn.copy()
    fuv[1, 2], fvn[2, 0], fvn[5] = -1, -1, -1        # partial vt, partial vn, no vn
    vn[F[7]] = 0.0                                    # |n| = 0 over face 7
    scenes["grid fallbacks"] = (Vg, F, mat, Kd, uv, fuv, vn, fvn, mt, tx)
    for name, (scene, _) in bad_attribute_scenes(R).items():
        scenes[name] = scene
    return R, scenes


@pytest.mark.parametrize("name", sorted(small_shaded_scenes()[1]))
@pytest.mark.parametrize("S,ss", [(8, 2), (5, 3)])
def test_oracle_equals_a_literal_loop(name, S, ss):
    R, scenes = small_shaded_scenes()
    want = literal(scenes[name], R, 2.0, 1.875, S, ss)
    got = SO.render(scenes[name], R, 2.0, 1.875, S, ss)
    for what, g, w in zip(("rgba", "depth", "face_id"), got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, what, np.argwhere(g != w)[:3])
    assert got[3] == want[3]
    bad = bad_attribute_scenes(R)
    if name in bad:
        assert got[3] == bad[name][1] and set(np.unique(got[2])) == {-1, 1}      # the bad face is skipped, the other drawn


def test_small_scenes_take_every_path():
    R, scenes = small_shaded_scenes()
    total = dict.fromkeys(SO.PATHS, 0)
    for name, scene in scenes.items():
        for k, v in SO.render(scene, R, 2.0, 1.875, 8, 2)[4].items():
            total[k] += v
    assert all(total[k] > 0 for k in SO.PATHS), total


@pytest.mark.parametrize("S,ss", [(8, 2), (5, 3)])
def test_without_attributes_the_oracle_is_the_flat_one(S, ss):
    R, plain = H._small_scenes()
    for name, scene in plain.items():
        want = O.render(*scene, R, 2.0, 1.875, S, ss)
        for got in (SO.render(scene, R, 2.0, 1.875, S, ss), SO.render(tuple(scene) + SO.attributes(scene), R, 2.0, 1.875, S, ss)):
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got[:3], want[:3])) and got[3] == want[3], name
    _, shaded = small_shaded_scenes()
    for name in ("grid wrapped", "grid fallbacks", "nan uv", "texture index beyond"):
        scene = shaded[name]
        off = SO.render(scene, R, 2.0, 1.875, S, ss, textures=False, smooth_normals=False)
        want = O.render(*scene[:4], R, 2.0, 1.875, S, ss)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(off[:3], want[:3])) and off[3] == want[3], name
        on = SO.render(scene, R, 2.0, 1.875, S, ss)
        if on[3] == 0:       # the geometry does not depend on the attributes
            assert on[1].tobytes() == want[1].tobytes() and on[2].tobytes() == want[2].tobytes()
            assert on[0][..., 3].tobytes() == want[0][..., 3].tobytes() and on[0].tobytes() != want[0].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# two checks that share none of the oracle's conventions
# ---------------------------------------------------------------------------------------------------------------------
QUAD_COLOURS = np.array([[[250, 10, 20], [30, 240, 50]], [[60, 70, 230], [220, 210, 40]]], dtype=np.uint8)   # [row][col]


def facing_quad(R):
    """A quad in the plane r_0 = 0 facing the camera, for S = 8, ss = 1, camera_distance = focal_length = 2: it covers
    the image columns and rows 1.5 .. 5.5, its uv (0, 0) at the image's bottom left and (1, 1) at the top right, with a
    2 x 2 texture.  The texels' centres (u, v = 1/4, 3/4) then fall on the centres of pixel columns and rows 2 and 4."""
    lo, hi = 1.5 / 8 - 0.5, 5.5 / 8 - 0.5            # r_2 = u of the left and right edge; -r_1 likewise for the rows
    corners = [[0.0, -hi, lo], [0.0, -hi, hi], [0.0, -lo, hi], [0.0, -lo, lo]]       # bottom left, bottom right, top right, top left
    uv = [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]
    F = [[0, 1, 2], [0, 2, 3]]
    return (O.camera_space(R, corners), F, [0, 0], [[0.5, 0.5, 0.5]], uv, F, np.zeros((0, 3)), [[-1] * 3] * 2, [0], [QUAD_COLOURS])


def check_facing_quad(rgba):
    """Row 0 of the texture is its top, column 0 its left: the picture of the quad is the texture upright."""
    assert rgba.shape == (8, 8, 4) and (rgba[2:5, 2:5, 3] == 255).all() and rgba[0, 0, 3] == 0
    for (i, j), (row, col) in {(2, 2): (0, 0), (2, 4): (0, 1), (4, 2): (1, 0), (4, 4): (1, 1)}.items():
        assert rgba[i, j, :3].tolist() == QUAD_COLOURS[row, col].tolist(), ((i, j), rgba[i, j], QUAD_COLOURS[row, col])


RECEDING = dict(S=64, ss=1, cd=2.0, f=1.0, near=(-1.0, -0.4), far=(2.0, 1.2), half=0.1)   # (r_0, r_1) of the two edges


def receding_quad(R):
    """A quad from a near edge (v = 0) to a far edge (v = 1), |r_2| <= half, whose 1 x 64 texture is blue below v = 1/2
    and red above."""
    g = RECEDING
    (n0, n1), (f0, f1), h = g["near"], g["far"], g["half"]
    corners = [[n0, n1, -h], [n0, n1, h], [f0, f1, h], [f0, f1, -h]]
    uv = [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]
    tex = np.zeros((64, 1, 3), dtype=np.uint8)
    tex[:32] = (255, 0, 0)       # rows 0 .. 31: the top of the texture, v > 1/2, the far half
    tex[32:] = (0, 0, 255)
    F = [[0, 1, 2], [0, 2, 3]]
    return (O.camera_space(R, corners), F, [0, 0], [[0.5, 0.5, 0.5]], uv, F, np.zeros((0, 3)), [[-1] * 3] * 2, [0], [tex])


def receding_rows():
    """(image row of the quad's 3-D midline, image row of the midpoint between its projected edges)."""
    g = RECEDING
    row = lambda r0, r1: (0.5 - r1 * g["f"] / (r0 + g["cd"])) * g["S"]
    (n0, n1), (f0, f1) = g["near"], g["far"]
    return row(0.5 * (n0 + f0), 0.5 * (n1 + f1)), 0.5 * (row(n0, n1) + row(f0, f1))


def check_receding_quad(rgba):
    """Down the middle column the colour turns from red (far, top) to blue within a pixel of the 3-D midline's row."""
    mid, screen = receding_rows()
    assert abs(mid - screen) > 3.0
    col = rgba[:, RECEDING["S"] // 2]
    seen = np.nonzero(col[:, 3] == 255)[0]
    assert len(seen) > 30
    red = col[seen, 0].astype(int) > col[seen, 2].astype(int)
    last_red = seen[np.nonzero(red)[0].max()]
    assert red[:np.nonzero(red)[0].max() + 1].all() and not red[-1]                  # red above, blue below, one change
    assert abs((last_red + 1.0) - mid) <= 1.0, (last_red, mid, screen)


def test_texture_orientation_on_a_facing_quad():
    R = O.rotation_of(CAM)
    rgba, _, _, status, paths = SO.render(facing_quad(R), R, 2.0, 2.0, 8, 1)
    assert status == 0 and paths["textured"] > 0
    check_facing_quad(rgba)


def test_interpolation_is_perspective_correct_on_a_receding_quad():
    mid, screen = receding_rows()
    assert abs(mid - screen) > 3.0 and 0 < mid < RECEDING["S"] and 0 < screen < RECEDING["S"]
    R = O.rotation_of(CAM)
    g = RECEDING
    rgba, _, _, status, _ = SO.render(receding_quad(R), R, g["cd"], g["f"], g["S"], g["ss"])
    assert status == 0
    check_receding_quad(rgba)


# ---------------------------------------------------------------------------------------------------------------------
# the reader
# ---------------------------------------------------------------------------------------------------------------------
def test_load_obj_scene_shaded(tmp_path):
    img = SO.checker(5, 3, 7)
    (tmp_path / "tex").mkdir()
    V.write_png(str(tmp_path / "tex" / "wood.png"), img)
    V.write_png_rgba(str(tmp_path / "alpha.png"), np.concatenate([img, img[..., :1]], axis=-1))
    (tmp_path / "m.mtl").write_text("newmtl wood\nKd 0.9 0.1 0.2\nmap_Kd -s 1 1 1 tex\\wood.png\nnewmtl plain\nKd 0.1 0.2 0.3\n"
                                    "newmtl gone\nKd 0.4 0.4 0.4\nmap_Kd nowhere.png\nnewmtl rgba\nKd 1 1 1\nmap_Kd alpha.png\n"
                                    "newmtl again\nKd 0.2 0.2 0.2\nmap_Kd tex/wood.png\nnewmtl junk\nKd 0 0 0\nmap_Kd m.mtl\n")
    (tmp_path / "a.obj").write_text(
        "mtllib m.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0 0 1\nvt 0 0\nvt 1 0 0\nvt 1 1\nvt 0.5\nvn 0 0 1\nvn 1 0 0\n"
        "f 1 2 3\nusemtl wood\nf 1/1/1 2/2/2 3/3/1 4/4/2\nusemtl plain\nf 1//1 2//1 5//2\nusemtl gone\nf 5/1 4/2 3/3 2/4 1/1\n"
        "usemtl rgba\nf 1/1/1 2 5//2\nusemtl again\nf 1/1 2/2 5/3\nusemtl junk\nf 1/1 2/2 5/3\n")
    s = M.load_obj_scene_shaded(str(tmp_path / "a.obj"))
    flat = M.load_obj_scene(str(tmp_path / "a.obj"))
    assert isinstance(s, M.ShadedScene) and len(s[:5]) == 5
    for a, b in zip(s[:4], flat[:4]):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all()
    assert s.names == flat[4] == ["", "wood", "plain", "gone", "rgba", "again", "junk"]
    assert s.uv.tolist() == [[0, 0], [1, 0], [1, 1], [0.5, 0]] and s.normals.tolist() == [[0, 0, 1], [1, 0, 0]]
    assert s.F.tolist()[:4] == [[0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 1, 4]]
    assert s.face_uv.tolist() == [[-1, -1, -1], [0, 1, 2], [0, 2, 3], [-1, -1, -1], [0, 1, 2], [0, 2, 3], [0, 3, 0],
                                  [0, -1, -1], [0, 1, 2], [0, 1, 2]]
    assert s.face_vn.tolist() == [[-1, -1, -1], [0, 1, 0], [0, 0, 1], [0, 0, 1], [-1, -1, -1], [-1, -1, -1], [-1, -1, -1],
                                  [0, -1, 1], [-1, -1, -1], [-1, -1, -1]]
    assert s.face_uv.dtype == s.face_vn.dtype == s.mat_tex.dtype == np.int64
    assert s.mat_tex.tolist() == [-1, 0, -1, -1, 1, 0, -1]                   # wood and again share one image
    assert len(s.textures) == 2 and (s.textures[0] == img).all() and (s.textures[1] == img).all()   # alpha dropped
    assert len(s.warnings) == 2 and "nowhere.png" in s.warnings[0] and "'gone'" in s.warnings[0] and "'junk'" in s.warnings[1]
    # a caller's decoder; one that fails is a warning too
    calls = []
    mine = M.load_obj_scene_shaded(str(tmp_path / "a.obj"), load_image=lambda p: calls.append(p) or np.full((2, 2, 4), 9, np.uint8))
    assert len(calls) == 4 and all(t.shape == (2, 2, 3) for t in mine.textures) and mine.warnings == []
    assert calls[0].replace("\\", "/").endswith("tex/wood.png")
    boom = M.load_obj_scene_shaded(str(tmp_path / "a.obj"), load_image=lambda p: 1 / 0)
    assert boom.textures == [] and (boom.mat_tex == -1).all() and len(boom.warnings) == 4
    # no .mtl, no vt, no vn: the flat scene with empty attributes
    (tmp_path / "b.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    b = M.load_obj_scene_shaded(str(tmp_path / "b.obj"))
    assert b.uv.shape == (0, 2) and b.normals.shape == (0, 3) and b.face_uv.tolist() == [[-1] * 3] and b.mat_tex.tolist() == [-1]
    for text, exc in (("f -3 -2 -1", ValueError), ("f 1/-1 2/1 3/1", ValueError), ("f 1//0 2//1 3//1", ValueError),
                      ("f 1/2 2/1 3/1", IndexError), ("f 1//1 2//1 3//2", IndexError), ("f 1 2 4", IndexError)):
        (tmp_path / "c.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\n%s\n" % text)
        with pytest.raises(exc, match="relative" if exc is ValueError else "beyond"):
            M.load_obj_scene_shaded(str(tmp_path / "c.obj"))


def test_scene_checks_before_any_device(tmp_path):
    R = O.rotation_of(CAM)
    good = M.ShadedScene(*facing_quad(R)[:4], ["m"], *facing_quad(R)[4:], [])
    pos = [[CAM]]
    for field, value, match in (("face_uv", [[0, 1, 2]], "face_uv"), ("mat_tex", [0, 0], "mat_tex"), ("uv", np.zeros((4, 3)), "uv"),
                                ("textures", [np.zeros((2, 2, 4), np.uint8)], "texture 0"), ("face_vn", np.zeros((2, 3)), "face_vn"),
                                ("textures", [np.zeros((2, 2, 3), np.float32)], "texture 0")):
        with pytest.raises(ValueError, match="scene 0.*" + match):
            M.render_mesh_views([good._replace(**{field: value})], pos, image_size=8)
    for kw in (dict(image_size=0), dict(supersample=5)):
        with pytest.raises(ValueError, match="refused"):
            M.render_mesh_views([good], pos, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# refusals before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch():
    L = _native.lib()
    meshes = np.array([[0, 4, 0, 2, 0, 1, 0, 3, 0, 2, 0, 1], [4, 3, 2, 1, 1, 2, 3, 0, 2, 5, 1, 1]], dtype=np.int32)
    views = np.array([1, 0, 1], dtype=np.int32)
    tex = np.array([[0, 4, 2], [24, 1, 1]], dtype=np.int64)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(nv=7, nf=3, nk=3, nu=3, nn=7, nt=2, nb=27, m=meshes, v=views, t=tex, S=64, ss=3, W=None, Mn=None):
        return L.dpc_render_meshes_shaded(None, nv, None, None, nf, None, nk, None, nu, None, None, nn, None, None, None, nb,
                                          None, vp(t), nt, None, vp(m), len(m) if Mn is None else Mn, None, vp(v), None,
                                          len(v) if W is None else W, S, ss, None, None, None, None, None, None)

    assert call() == _native.DPC_ERR_NULL
    assert call(W=0) == 0
    big = np.array([[0, 4, 2], [3 << 30, 1, 1]], dtype=np.int64)           # an offset beyond 2 GiB is addressable
    assert call(t=big, nb=(3 << 30) + 3) == _native.DPC_ERR_NULL

    def row(**kw):
        r = meshes.copy()
        for k, val in kw.items():
            r[0, int(k[1:])] = val
        return r

    for bad in (dict(nv=6), dict(nf=2), dict(nk=2), dict(S=0), dict(S=1025), dict(ss=0), dict(ss=5), dict(nv=-1), dict(W=-1),
                dict(W=65536), dict(v=np.array([2], dtype=np.int32)), dict(v=np.array([-1], dtype=np.int32)),
                dict(nu=2), dict(nn=6), dict(nt=1), dict(nu=-1), dict(nn=-1), dict(nt=-1), dict(nb=-1),         # bad ranges
                dict(m=row(c6=-1)), dict(m=row(c7=-1)), dict(m=row(c8=6)), dict(m=row(c10=2)), dict(m=row(c11=3)),
                dict(nb=26), dict(nb=23),                                                                        # texels beyond
                dict(t=np.array([[-1, 4, 2], [24, 1, 1]], dtype=np.int64)), dict(t=np.array([[0, 0, 2], [24, 1, 1]], dtype=np.int64)),
                dict(t=np.array([[0, 4, 65537], [24, 1, 1]], dtype=np.int64)), dict(t=np.array([[4, 4, 2], [24, 1, 1]], dtype=np.int64)),
                dict(t=big), dict(t=np.array([[0, 65536, 65536], [24, 1, 1]], dtype=np.int64))):
        assert call(**bad) == _native.DPC_ERR_SHAPE, bad
    ws = L.dpc_render_meshes_shaded_workspace_bytes(vp(meshes), 2, vp(views), 3)
    assert ws == 2 * 32 + 32 * (3 + 4 + 3) + 8 * (1 + 2 + 1) and ws % 16 == 0
    flat = np.ascontiguousarray(meshes[:, :6])
    assert ws == L.dpc_render_meshes_workspace_bytes(vp(flat), 2, vp(views), 3)
    assert L.dpc_render_meshes_shaded_workspace_bytes(vp(meshes), 2, vp(np.array([5], dtype=np.int32)), 1) == 0
    assert L.dpc_abi_version() == 15
