"""Host side of the training-view renderer (dpc.render.meshviews, csrc/dpc_mesh_raster.hip): the numpy oracle of
tests/mesh_render_oracle.py against a literal per-sample, per-face loop; the camera against fixture F18 (the reference's
own quaternion_from_campos and pc_perspective_transform); the features against create_record's arithmetic; the .obj
reader, the camera sampler, the PNG writers and the argument refusals before any launch."""
import ctypes
import math
import os
import pickle

import numpy as np
import pytest

import mesh_render_oracle as O
from dpc.render import _native
from dpc.render import meshviews as M
from dpc.render import visualise as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAM = (1.2, -0.9, 0.7)


@pytest.fixture(scope="module")
def f18():
    return dict(np.load(os.path.join(GOLDEN, "f18_mesh_views.npz")))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle against a literal loop
# ---------------------------------------------------------------------------------------------------------------------
def literal(Vx, F, mat, Kd, R, cd, f, S, ss):
    """include/dpc_render.h's dpc_render_meshes as a plain loop over every sample and every face, Python floats."""
    R = [[float(x) for x in row] for row in np.asarray(R).reshape(3, 3)]
    verts = []
    for p in np.asarray(Vx, dtype=np.float64).reshape(-1, 3):
        p = [float(c) for c in p]
        r = [(R[k][0] * p[0] + R[k][1] * p[1]) + R[k][2] * p[2] for k in range(3)]
        d = r[0] + cd
        if not all(math.isfinite(c) for c in p):
            verts.append((math.nan, math.nan, math.nan, math.nan, r))
            continue
        if d == 0.0:
            verts.append((math.inf, math.inf, math.inf, d, r))
            continue
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
        bits = 0
        for i in tri:
            x, y, w, d, _ = verts[i]
            if not math.isfinite(d):
                bits |= 8
            elif d <= 1e-3:
                bits |= 32
            elif not (math.isfinite(x) and math.isfinite(y)):
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
        iw = ((e[0] / area) * v[0][2] + (e[1] / area) * v[1][2]) + (e[2] / area) * v[2][2]
        return 1.0 / iw if iw > 0 else None

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
                        d = cover(v, area, px, py)
                        if d is None:
                            continue
                        with np.errstate(over="ignore"):
                            key = (int(np.float32(d).view(np.uint32)) << 32) | k
                        if win is None or key < win[0]:
                            win = (key, d, v, m)
                    if win is None:
                        continue
                    key, d, v, m = win
                    r0, r1, r2 = v[0][4], v[1][4], v[2][4]
                    e1 = [r1[c] - r0[c] for c in range(3)]
                    e2 = [r2[c] - r0[c] for c in range(3)]
                    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
                    nn = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                    shade = 0.25 + 0.75 * (abs(n[0]) / nn if nn > 0 else 0.0)
                    for c in range(3):
                        acc[c] = acc[c] + float(Kd[m][c]) * shade
                    covered += 1
                    if best is None or key < best[0]:
                        best = (key, d)
            if covered:
                for c in range(3):
                    x = acc[c] / covered
                    x = 1.0 if x > 1.0 else (x if x >= 0.0 else 0.0)
                    rgba[i, j, c] = int(math.floor(255.0 * x + 0.5))
                rgba[i, j, 3] = int(math.floor(255.0 * (covered / (ss * ss)) + 0.5))
                depth[i, j] = int(min(65535.0, math.floor(best[1] / 10.0 * 65535.0 + 0.5)))
                fid[i, j] = best[0] & 0xFFFFFFFF
    return rgba, depth, fid, status


def _small_scenes():
    R = O.rotation_of(CAM)
    scenes = dict(O.special_scenes(R))
    for name, (scene, _) in O.bad_scenes(R).items():
        scenes[name] = scene
    Vb, Fb, mb = O.box_mesh([((-0.3, -0.05, -0.25), (0.25, 0.03, 0.3)), ((-0.3, 0.03, -0.25), (-0.22, 0.42, 0.3))])
    scenes["boxes"] = (Vb, Fb, mb, np.array([[0.8, 0.2, 0.2], [0.2, 0.7, 0.3]]))
    Vg, Fg, mg = O.grid_mesh(3)
    scenes["grid"] = (Vg, Fg, mg, np.array([[0.3, 0.3, 0.9], [0.9, 0.9, 0.2]]))
    return R, scenes


@pytest.mark.parametrize("name", sorted(_small_scenes()[1]))
@pytest.mark.parametrize("S,ss", [(8, 2), (5, 3)])
def test_oracle_equals_a_literal_loop(name, S, ss):
    R, scenes = _small_scenes()
    Vx, F, mat, Kd = scenes[name]
    rgba, depth, fid, status, _ = O.render(Vx, F, mat, Kd, R, 2.0, 1.875, S, ss)
    want = literal(Vx, F, mat, np.asarray(Kd), R, 2.0, 1.875, S, ss)
    assert status == want[3]
    assert (fid == want[2]).all(), np.argwhere(fid != want[2])[:5]
    assert rgba.tobytes() == want[0].tobytes() and depth.tobytes() == want[1].tobytes()


def test_special_scenes_show_what_they_are_for():
    R = O.rotation_of(CAM)
    sc = O.special_scenes(R)
    S, ss = 32, 3
    r = lambda name: O.render(*sc[name], R, 2.0, 1.875, S, ss)
    rgba, depth, fid, status, _ = r("coplanar duplicates")
    assert status == 0 and set(np.unique(fid)) == {-1, 0, 1}          # faces 2 and 3 lose every tie
    assert (rgba[fid >= 0][:, 0] > rgba[fid >= 0][:, 2]).all()        # ... and so does their colour
    rgba, depth, fid, status, _ = r("empty")
    assert status == 0 and not rgba.any() and (depth == 65535).all() and (fid == -1).all()
    rgba, depth, fid, status, cov = r("partly and wholly outside")
    assert status == 0 and set(np.unique(fid)) == {0, 2} and (fid >= 0).all()   # face 1 is outside, face 2 fills the image
    assert (fid == 0).any() and (rgba[..., 3] == 255).all()
    rgba, depth, fid, status, _ = r("zero area")
    assert status == 0 and (fid == -1).all()
    rgba, depth, fid, status, _ = r("sliver")
    assert status == 0 and (fid == 0).any() and 0 < rgba[..., 3].max() < 255
    for name, (scene, bit) in O.bad_scenes(R).items():
        rgba, depth, fid, status, _ = O.render(*scene, R, 2.0, 1.875, S, ss)
        assert status == bit, name
        assert set(np.unique(fid)) == {-1, 1}, name                    # the bad face is skipped, the good one drawn


@pytest.mark.parametrize("ss", [1, 3])
def test_no_crack_between_faces_that_share_edges(ss):
    """Every sample inside the projected outline of a tessellated sheet is covered."""
    S = 64
    R = O.rotation_of(CAM)
    n = 24
    g = np.linspace(-0.3, 0.3, n + 1)
    Y, Z = np.meshgrid(g, g, indexing="ij")
    rng = np.random.default_rng(3)
    jitter = np.zeros((n + 1, n + 1, 2))
    jitter[1:-1, 1:-1] = rng.uniform(-0.004, 0.004, (n - 1, n - 1, 2))   # interior vertices move, the outline stays a square
    r = np.stack([np.zeros_like(Y), Y + jitter[..., 0], Z + jitter[..., 1]], axis=-1).reshape(-1, 3)
    _, F, mat = O.grid_mesh(n)
    keys, status, _ = O.sample_keys(O.camera_space(R, r), F, mat, 2, R, 2.0, 1.875, S, ss)
    assert status == 0
    # the outline in pixels: r_0 = 0 is a plane parallel to the image, so the sheet projects to an exact square
    lo, hi = (0.5 - 0.3 * 1.875 / 2.0) * S, (0.5 + 0.3 * 1.875 / 2.0) * S
    p = O.sample_pos(np.arange(S * ss), ss)
    inside = (p > lo + 1e-9) & (p < hi - 1e-9)
    want = inside[:, None] & inside[None, :]
    assert want.sum() > 100 * ss * ss
    assert (keys[want] != O.EMPTY).all()
    assert (keys[~(((p >= lo - 1e-9) & (p <= hi + 1e-9))[:, None] & ((p >= lo - 1e-9) & (p <= hi + 1e-9))[None, :])] == O.EMPTY).all()


def test_pooling_128_at_ss2_is_64_at_ss4(f18):
    R = O.rotation_of(f18["cam_pos"][0])
    scene = (f18["V"], f18["F"], f18["material"], f18["Kd"])
    fine = O.render(*scene, R, 2.0, 1.875, 128, 2)
    coarse = O.render(*scene, R, 2.0, 1.875, 64, 4)
    pooled = fine[4].reshape(64, 2, 64, 2).sum(axis=(1, 3))
    assert (pooled == coarse[4]).all() and coarse[4].max() == 16 and 0 < (coarse[4] > 0).mean() < 1
    assert (O.covered_from_alpha(fine[0][..., 3], 2) == fine[4]).all()
    assert (O.covered_from_alpha(coarse[0][..., 3], 4) == coarse[4]).all()


# ---------------------------------------------------------------------------------------------------------------------
# the camera against the reference (F18)
# ---------------------------------------------------------------------------------------------------------------------
def pixel_of(dvu, S):
    """(row, column) pixel indices of transformed points (d, v, u)."""
    return np.floor((0.5 - dvu[:, 1]) * S).astype(np.int64), np.floor((dvu[:, 2] + 0.5) * S).astype(np.int64)


def near_mask(alpha_positive):
    """Pixels that are set or have a set pixel among their 8 neighbours."""
    S = alpha_positive.shape[0]
    pad = np.zeros((S + 2, S + 2), dtype=bool)
    pad[1:-1, 1:-1] = alpha_positive
    out = np.zeros((S, S), dtype=bool)
    for di in range(3):
        for dj in range(3):
            out |= pad[di:di + S, dj:dj + S]
    return out


def contained(alpha, dvu):
    """Per point: whether it lands in a pixel with alpha > 0 or next to one (points outside the image: False)."""
    S = alpha.shape[0]
    i, j = pixel_of(dvu, S)
    ok = (i >= 0) & (i < S) & (j >= 0) & (j < S)
    res = np.zeros(len(dvu), dtype=bool)
    res[ok] = near_mask(alpha > 0)[i[ok], j[ok]]
    return res


def full_pixels_have_points(alpha, dvu):
    """Per pixel with alpha = 255: whether a projected point lies within one pixel of it (Chebyshev)."""
    S = alpha.shape[0]
    i, j = pixel_of(dvu, S)
    ok = (i >= 0) & (i < S) & (j >= 0) & (j < S)
    has = np.zeros((S, S), dtype=bool)
    has[i[ok], j[ok]] = True
    return near_mask(has)[alpha == 255]


def check_views_against_f18(f18, alphas, S):
    """Steps 2-4 of the camera check for rendered alpha images [3,S,S] of F18's mesh from F18's cameras."""
    dense = O.sample_surface(f18["V"], f18["F"].astype(np.int64), 200000, 1801)
    failures = {"mirror": 0, "flip": 0, "transpose": 0}
    for w in range(3):
        ref = f18["transformed"][w].copy()
        ref[:, 0] += float(f18["camera_distance"])
        inside = contained(alphas[w], ref)
        assert inside.all(), "view %d: %d of %d reference points miss the render" % (w, (~inside).sum(), len(inside))
        got = full_pixels_have_points(alphas[w], M.view_transform(dense, f18["cam_pos"][w], 2.0, 1.875))
        assert len(got) > 20 and got.all(), "view %d: %d opaque pixels without a surface point" % (w, (~got).sum())
        failures["mirror"] += int((~contained(alphas[w][:, ::-1], ref)).sum())
        failures["flip"] += int((~contained(alphas[w][::-1], ref)).sum())
        failures["transpose"] += int((~contained(alphas[w].T, ref)).sum())
    assert all(n > 0 for n in failures.values()), failures   # the fixture tells the orientations apart


def test_host_transform_reproduces_the_reference(f18):
    for w in range(3):
        got = M.view_transform(f18["points"], f18["cam_pos"][w], float(f18["camera_distance"]), float(f18["focal_length"]))
        got[:, 0] -= float(f18["camera_distance"])
        assert np.abs(got - f18["transformed"][w]).max() <= 1e-12
        R = M.view_rotation(f18["cam_pos"][w])
        q = f18["q"][w] / np.linalg.norm(f18["q"][w])
        from dpc.render import as_rotation_matrix

        assert np.abs(R - as_rotation_matrix(q)).max() <= 1e-15
    cx, cy, cz = f18["cam_pos"][0]
    toward = np.array([[cx, cz, -cy]]) / np.linalg.norm(f18["cam_pos"][0])
    assert np.abs(O.rotate(toward, M.view_rotation(f18["cam_pos"][0])) - [[-1.0, 0.0, 0.0]]).max() < 1e-15


def test_oracle_views_contain_the_reference_projection(f18):
    S, ss = 32, 3
    alphas = [O.render(f18["V"], f18["F"], f18["material"], f18["Kd"], O.rotation_of(c), 2.0, 1.875, S, ss)[0][..., 3]
              for c in f18["cam_pos"]]
    check_views_against_f18(f18, alphas, S)


def depth_order_scene():
    R = O.rotation_of(CAM)
    Vx, F, mat, Kd = O.special_scenes(R)["parallel squares"]
    return R, (Vx, F, mat, Kd)


def check_depth_order(fid, depth, S):
    """Step 5: faces 0, 1 are the square at r_0 = -0.2 (d = 1.8), faces 2, 3 the one at r_0 = +0.2 (d = 2.2)."""
    R, (Vx, F, _, _) = depth_order_scene()
    d = M.view_transform(Vx, CAM, 2.0, 1.875)[:, 0]
    assert np.abs(d[:4] - 1.8).max() < 1e-12 and np.abs(d[4:] - 2.2).max() < 1e-12
    # where both squares cover a pixel's centre the nearer one shows: the overlap is |r_1| and r_2 within both squares
    for (r1, r2) in [(0.0, 0.0), (-0.1, 0.1), (0.1, -0.1)]:
        i_near, j_near = pixel_of(np.array([[1.8, r1 * 1.875 / 1.8, r2 * 1.875 / 1.8]]), S)
        assert fid[i_near[0], j_near[0]] in (0, 1)
        assert abs(depth[i_near[0], j_near[0]] * 10.0 / 65535.0 - 1.8) <= 10.0 / 65535.0
    assert set(np.unique(fid)) == {-1, 0, 1, 2, 3}
    far = np.isin(fid, (2, 3))
    assert np.abs(depth[far] * 10.0 / 65535.0 - 2.2).max() <= 10.0 / 65535.0


def test_depth_order_on_the_oracle():
    R, scene = depth_order_scene()
    _, depth, fid, status, _ = O.render(*scene, R, 2.0, 1.875, 64, 3)
    assert status == 0
    check_depth_order(fid, depth, 64)


def test_camera_extrinsic(f18):
    from dpc.harness.views import camera_from_blender

    for w in range(3):
        E = M.camera_extrinsic(f18["cam_pos"][w], 2.0)
        R = M.view_rotation(f18["cam_pos"][w])
        ours = camera_from_blender(E)          # float32, as the reference's
        want = np.eye(4)
        want[:3, :3], want[:3, 3] = R, (2.0, 0.0, 0.0)
        assert ours.dtype == np.float32 and np.abs(ours - want).max() < 1e-6
        # util/camera.py:15-35 in float64 ...
        their, our = E, np.zeros((4, 4))
        our[0, 0], our[0, 1], our[0, 2] = -their[2, 0], their[2, 2], their[2, 1]
        our[1, 0], our[1, 1], our[1, 2] = their[1, 0], -their[1, 2], -their[1, 1]
        our[2, 0], our[2, 1], our[2, 2] = -their[0, 0], their[0, 2], their[0, 1]
        our[0, 3], our[1, 3], our[2, 3], our[3, 3] = their[2, 3], their[1, 3], their[0, 3], their[3, 3]
        assert (our == want).all()
        # ... and the matrix branch of pc_perspective_transform (point_cloud_to.py:150-172) on it
        intrinsic = np.eye(4)
        intrinsic[1, 1] = intrinsic[2, 2] = 1.875
        xyz1 = np.pad(f18["points"], ((0, 0), (0, 1)), constant_values=1.0)
        pc2 = xyz1 @ (intrinsic @ our).T
        xs, ys, zs = pc2[:, 2] / pc2[:, 0], pc2[:, 1] / pc2[:, 0], pc2[:, 0] - 2.0
        assert np.abs(np.stack([zs, ys, xs], axis=1) - f18["transformed"][w]).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# features, files
# ---------------------------------------------------------------------------------------------------------------------
def create_record_views(imgs, cams, poss, depths16):
    """dpc/run/create_data_torch.py:66-70, 102-162 for images already read (im_size == actual_size), restated."""
    num_views, im_size = imgs.shape[0], imgs.shape[1]
    rgbs = np.zeros((num_views, im_size, im_size, 3), dtype=np.float32)
    masks = np.zeros((num_views, im_size, im_size, 1), dtype=np.float32)
    cameras = np.zeros((num_views, 4, 4), dtype=np.float32)
    cam_pos = np.zeros((num_views, 3), dtype=np.float32)
    depths = np.zeros((num_views, im_size, im_size, 1), dtype=np.float32)
    for k in range(num_views):
        img = imgs[k]
        rgb = img[:, :, 0:3]
        mask = img[:, :, [3]]
        mask = mask / 255.0
        mask_fg = np.repeat(mask, 3, 2)
        mask_bg = 1.0 - mask_fg
        rgb = rgb * mask_fg + np.ones(rgb.shape) * 255.0 * mask_bg
        rgb = rgb / 255.0
        rgbs[k, :, :, :] = rgb
        masks[k, :, :, :] = mask
        cameras[k, :, :] = cams[k]
        cam_pos[k, :] = poss[k]
        dMap = depths16[k].astype(np.float32)
        dMap = dMap * (10 - 0) / (pow(2, 16) - 1) + 0
        depth = (dMap - 0.0) / 10.0
        depth_r = depth * 10.0 + 0.0
        depths[k, :, :] = np.expand_dims(depth_r, -1)
    return {"image": rgbs, "mask": masks, "extrinsic": cameras, "cam_pos": cam_pos, "depth": depths}


def test_features_equal_create_record(tmp_path):
    rng = np.random.default_rng(7)
    rgba = rng.integers(0, 256, (3, 16, 16, 4), dtype=np.uint8)
    rgba[0, :4, :, 3] = 0
    rgba[1, :, :5, 3] = 255
    depth = rng.integers(0, 65536, (3, 16, 16)).astype(np.uint16)
    pos = M.sample_camera_positions(1, 3, 5)[0]
    extr = np.stack([M.camera_extrinsic(p) for p in pos])
    got = M.features_of_views(rgba, depth, pos, extr, "abc", image_size=16)
    want = create_record_views(rgba, extr, pos, depth)
    assert set(got) == set(want) | {"name"} and got["name"] == "abc"
    for k, v in want.items():
        assert got[k].dtype == np.float32 and got[k].shape == v.shape and got[k].tobytes() == v.tobytes(), k
    assert got["image"].shape == (3, 16, 16, 3) and got["mask"].shape == (3, 16, 16, 1)
    assert (got["image"][0, :4] == 1.0).all()                                     # transparent -> white
    plain = M.features_of_views(rgba, name="x", store_camera=False, store_depth=False)
    assert set(plain) == {"image", "mask", "name"}
    with pytest.raises(ValueError, match="render at image_size 64"):
        M.features_of_views(rgba, depth, pos, extr, "abc", image_size=64)
    # what ShapeRecords.__getitem__ reads after a pickle round trip
    path = tmp_path / "abc_features.p"
    path.write_bytes(pickle.dumps(got))
    feature = pickle.loads(path.read_bytes())
    assert feature["image"].transpose(0, 3, 1, 2).shape == (3, 3, 16, 16) and feature["extrinsic"].shape == (3, 4, 4)


def test_png_round_trips(tmp_path):
    rng = np.random.default_rng(2)
    rgba = rng.integers(0, 256, (13, 9, 4), dtype=np.uint8)
    grey = rng.integers(0, 65536, (7, 11)).astype(np.uint16)
    rgb = rng.integers(0, 256, (5, 6, 3), dtype=np.uint8)
    pa, pg, pc = (str(tmp_path / n) for n in ("a.png", "g.png", "c.png"))
    V.write_png_rgba(pa, rgba)
    V.write_png_gray16(pg, grey)
    V.write_png(pc, rgb)
    back = V.read_png_any(pa)
    assert back.dtype == np.uint8 and back.shape == rgba.shape and (back == rgba).all()
    back = V.read_png_any(pg)
    assert back.dtype == np.uint16 and back.shape == grey.shape and (back == grey).all()
    assert (V.read_png_any(pc) == rgb).all() and (V.read_png(pc) == rgb).all()
    data = open(pg, "rb").read()
    assert data[16:26] == (11).to_bytes(4, "big") + (7).to_bytes(4, "big") + bytes([16, 0])
    assert open(pa, "rb").read()[24:26] == bytes([8, 6])
    for bad, fn in ((grey, V.write_png_rgba), (rgba, V.write_png_gray16)):
        with pytest.raises(ValueError):
            fn(pa, bad)


def test_load_obj_scene(tmp_path):
    (tmp_path / "m.mtl").write_text("newmtl red\nKd 0.9 0.1 0.2\nKa 1 1 1\nnewmtl nokd\nNs 3\nnewmtl bright\nKd 1.5 0.5 0.5\n")
    (tmp_path / "a.obj").write_text(
        "mtllib m.mtl missing.mtl\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nv 0 0 1\n"
        "f 1 2 3\nusemtl red\nf 1/1/1 2/2/2 3/3/3 4/4/4\nusemtl nokd\nf 1//1 2//1 5//1\nusemtl red\nf 5 4 3 2 1\n"
        "usemtl bright\nf 1 2 5\n")
    Vx, F, mat, Kd, names = M.load_obj_scene(str(tmp_path / "a.obj"))
    assert Vx.shape == (5, 3) and Vx.dtype == np.float64 and F.dtype == np.int64
    assert F.tolist() == [[0, 1, 2], [0, 1, 2], [0, 2, 3], [0, 1, 4], [4, 3, 2], [4, 2, 1], [4, 1, 0], [0, 1, 4]]
    assert names == ["", "red", "bright"] and mat.tolist() == [0, 1, 1, 0, 1, 1, 1, 2]
    assert Kd.tolist() == [[0.5, 0.5, 0.5], [0.9, 0.1, 0.2], [1.0, 0.5, 0.5]]
    (tmp_path / "b.obj").write_text("mtllib gone.mtl\nusemtl x\nv 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert M.load_obj_scene(str(tmp_path / "b.obj"))[3].tolist() == [[0.5, 0.5, 0.5]]
    (tmp_path / "c.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf -3 -2 -1\n")
    with pytest.raises(ValueError, match="relative"):
        M.load_obj_scene(str(tmp_path / "c.obj"))
    (tmp_path / "d.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(IndexError):
        M.load_obj_scene(str(tmp_path / "d.obj"))


def test_sample_camera_positions():
    a = M.sample_camera_positions(4, 5, 11)
    assert a.shape == (4, 5, 3) and a.dtype == np.float64 and (a == M.sample_camera_positions(4, 5, 11)).all()
    assert (a != M.sample_camera_positions(4, 5, 12)).any()
    assert np.abs(np.linalg.norm(a, axis=-1) - 2.0).max() < 1e-12
    el = np.degrees(np.arcsin(a[..., 2] / 2.0))
    assert el.min() >= -20.0 - 1e-9 and el.max() <= 40.0 + 1e-9
    one = M.sample_camera_positions(1, 1, 0, azimuth_deg=(90, 90), elevation_deg=(30, 30), distance=3.0)[0, 0]
    assert np.abs(one - [0.0, 3.0 * math.cos(math.radians(30)), 1.5]).max() < 1e-12
    for bad in (dict(elevation_deg=(0, 90)), dict(elevation_deg=(-90, 0)), dict(distance=0.0), dict(azimuth_deg=(10, 0))):
        with pytest.raises(ValueError):
            M.sample_camera_positions(1, 1, 0, **bad)
    with pytest.raises(ValueError, match="vertical"):
        M.view_rotation((0.0, 0.0, 2.0))


def test_refusals_before_any_launch():
    L = _native.lib()
    meshes = np.array([[0, 4, 0, 2, 0, 1], [4, 3, 2, 1, 1, 2]], dtype=np.int32)
    views = np.array([1, 0, 1], dtype=np.int32)

    def call(nv=7, nf=3, nk=3, m=meshes, v=views, S=64, ss=3, W=None, Mn=None):
        return L.dpc_render_meshes(None, nv, None, None, nf, None, nk, None, m.ctypes.data_as(ctypes.c_void_p),
                                   len(m) if Mn is None else Mn, None, v.ctypes.data_as(ctypes.c_void_p), None,
                                   len(v) if W is None else W, S, ss, None, None, None, None, None, None)

    assert call() == _native.DPC_ERR_NULL
    assert call(W=0) == 0
    for bad in (dict(nv=6), dict(nf=2), dict(nk=2), dict(S=0), dict(S=1025), dict(ss=0), dict(ss=5), dict(nv=-1), dict(W=-1),
                dict(v=np.array([2], dtype=np.int32)), dict(v=np.array([-1], dtype=np.int32)),
                dict(m=np.array([[0, 4, -1, 2, 0, 1]], dtype=np.int32), v=np.array([0], dtype=np.int32))):
        assert call(**bad) == _native.DPC_ERR_SHAPE, bad
    ws = L.dpc_render_meshes_workspace_bytes(meshes.ctypes.data_as(ctypes.c_void_p), 2, views.ctypes.data_as(ctypes.c_void_p), 3)
    assert ws == 2 * 32 + 32 * (3 + 4 + 3) + 8 * (1 + 2 + 1) and ws % 16 == 0
    assert L.dpc_render_meshes_workspace_bytes(meshes.ctypes.data_as(ctypes.c_void_p), 2,
                                               np.array([5], dtype=np.int32).ctypes.data_as(ctypes.c_void_p), 1) == 0
    # the Python layer asks the same checks first: these raise ValueError, not "no HIP device"
    tri = (np.eye(3), [[0, 1, 2]], [0], [[0.5, 0.5, 0.5]])
    pos = [[[1.0, 1.0, 1.0]]]
    for kw in (dict(image_size=0), dict(image_size=2048), dict(supersample=5)):
        with pytest.raises(ValueError, match="refused"):
            M.render_mesh_views([tri], pos, **kw)
    with pytest.raises(ValueError, match="view 0.*vertical"):
        M.render_mesh_views([tri], [[[0.0, 0.0, 1.0]]])
    with pytest.raises(ValueError, match="scene 0"):
        M.render_mesh_views([(np.eye(3), [[0, 1, 2]], [0, 0], [[0.5, 0.5, 0.5]])], pos)
    with pytest.raises(ValueError, match="Kd"):
        M.render_mesh_views([(np.eye(3), [[0, 1, 2]], [0], [[1.5, 0.5, 0.5]])], pos)
    with pytest.raises(ValueError, match="camera_distance"):
        M.render_mesh_views([tri], pos, camera_distance=0.0)
    with pytest.raises(ValueError, match="cam_pos"):
        M.render_mesh_views([tri], pos + pos)
