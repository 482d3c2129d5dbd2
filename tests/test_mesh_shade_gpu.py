"""Textured, smooth-shaded training views on the GPU (dpc_render_meshes_shaded through dpc.render.meshviews) against the
numpy oracle of tests/mesh_shade_oracle.py, byte for byte: ragged batches that mix plain, textured, smooth and fully shaded
scenes at every supersampling; independence of batching and order; the geometry of the flat call; the switches; the new
status cases; and tools/render_train_data.py --textures --smooth_normals through to one training step."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import mesh_render_oracle as O
import mesh_shade_oracle as SO
import test_mesh_render_gpu as G
import test_mesh_shade_host as H

pytestmark = pytest.mark.gpu

ROOT = G.ROOT
GOLDEN = G.GOLDEN
CAMS = G.CAMS
TEXTURE_SIZES = [(1, 1), (5, 3), (64, 64), (257, 129)]      # width x height


def package_scene(scene):
    """A scene of the oracle's (4 or 10 entries) as dpc.render takes it."""
    from dpc.render import ShadedScene

    return tuple(scene) if len(scene) < 10 else ShadedScene(*scene[:4], None, *scene[4:10], [])


def make_batch():
    """A ragged batch of plain tuples, a textured-only, a smooth-only and fully shaded scenes, one of 100 352 faces; uvs from
    -0.6 to 1.7, textures of every size of TEXTURE_SIZES, faces with partial vt / vn, zero normals and an untextured material."""
    f18 = dict(np.load(os.path.join(GOLDEN, "f18_mesh_views.npz")))
    special = O.special_scenes(O.rotation_of(CAMS[0]))
    tex = {wh: SO.checker(wh[1], wh[0], k) for k, wh in enumerate(TEXTURE_SIZES)}
    big = SO.shaded_grid(224, 0, [tex[(257, 129)], tex[(64, 64)]], uv_range=(-0.6, 1.7), mat_tex=(0, 1))
    textured = SO.shaded_grid(9, 1, [tex[(5, 3)], tex[(1, 1)]], uv_range=(-0.25, 1.25), with_vn=False, mat_tex=(0, 1))
    smooth = SO.shaded_grid(12, 2, [], with_uv=False, mat_tex=(-1, -1))
    Vg, F, mat, Kd, uv, fuv, vn, fvn, mt, tx = SO.shaded_grid(7, 3, [tex[(64, 64)]], uv_range=(0.0, 3.0), mat_tex=(0, -1))
    fuv, fvn, vn = fuv.copy(), fvn.copy(), vn.copy()
    fuv[0::5, 1], fvn[1::5, 2], fvn[2::5] = -1, -1, -1       # partial vt, partial vn, no vn
    vn[F[3::10].reshape(-1)] = 0.0                           # |n| = 0 over some faces
    fallbacks = (Vg, F, mat, Kd, uv, fuv, vn, fvn, mt, tx)
    scenes = [special["one face"], (f18["V"], f18["F"], f18["material"], f18["Kd"]), big, textured, smooth, fallbacks,
              special["empty"], special["coplanar duplicates"]]
    assert len(big[1]) >= 100000
    view_scene = [1, 2, 0, 3, 4, 2, 5, 6, 3, 7, 5, 4, 1]
    view_cam = [0, 1, 0, 0, 2, 3, 0, 0, 3, 0, 1, 1, 2]
    return scenes, np.array(view_scene), np.array([CAMS[c] for c in view_cam])


@pytest.fixture(scope="module")
def batch():
    return make_batch()


def gpu_render(scenes, view_scene, cam_pos, S, ss, **kw):
    import dpc.render as R

    rgba, depth, fid = R.render_mesh_views([package_scene(s) for s in scenes], cam_pos, image_size=S, supersample=ss,
                                           return_face_id=True, view_scene=view_scene, **kw)
    assert rgba.is_cuda and rgba.dtype == torch.uint8 and depth.dtype == torch.uint16 and fid.dtype == torch.int32
    return rgba.cpu().numpy(), depth.cpu().numpy(), fid.cpu().numpy()


def oracle_render(scenes, view_scene, cam_pos, S, ss, **kw):
    views = [(int(m), O.rotation_of(c), 2.0, 1.875) for m, c in zip(view_scene, cam_pos)]
    return SO.render_views(scenes, views, S, ss, **kw)


@pytest.mark.parametrize("ss", [1, 2, 3, 4])
@pytest.mark.parametrize("S", [32, 128, 200])
def test_ragged_batch_equals_the_oracle_by_bytes(batch, S, ss):
    scenes, view_scene, cam_pos = batch
    want = oracle_render(scenes, view_scene, cam_pos, S, ss)
    assert want[3] == 0
    # a condition on the inputs: every way through the shading colours samples of some view
    assert {wh for s in scenes if len(s) > 4 for wh in ((t.shape[1], t.shape[0]) for t in s[9])} == set(TEXTURE_SIZES)
    total = {k: sum(p[k] for p in want[4]) for k in SO.PATHS}
    assert all(total[k] > 0 for k in SO.PATHS), total
    got = gpu_render(scenes, view_scene, cam_pos, S, ss)
    G.assert_same(got, want[:3], "S %d ss %d" % (S, ss))
    assert (got[2][1] >= 0).mean() > 0.1 and got[2][1].max() > 50000            # the large mesh is there


def test_images_do_not_depend_on_batching_order_or_run(batch):
    scenes, view_scene, cam_pos = batch
    S, ss = 72, 3
    whole = gpu_render(scenes, view_scene, cam_pos, S, ss)
    again = gpu_render(scenes, view_scene, cam_pos, S, ss)
    G.assert_same(again, whole, "second run")
    order = np.random.default_rng(0).permutation(len(view_scene))
    shuffled = gpu_render(scenes, view_scene[order], cam_pos[order], S, ss)
    G.assert_same([a[np.argsort(order)] for a in shuffled], whole, "another order")
    for lo, hi in ((0, 2), (2, 3), (3, 9), (9, 13)):                         # another split, scenes renumbered
        used = sorted(set(view_scene[lo:hi].tolist()))
        part = gpu_render([scenes[m] for m in used], np.array([used.index(m) for m in view_scene[lo:hi]]), cam_pos[lo:hi], S, ss)
        G.assert_same(part, [a[lo:hi] for a in whole], "views %d..%d alone" % (lo, hi))
    alone = gpu_render([scenes[3]], np.array([0]), cam_pos[3:4], S, ss)
    G.assert_same(alone, [a[3:4] for a in whole], "one view alone")
    twice = gpu_render([scenes[3], scenes[3]], np.array([1, 0, 1]), cam_pos[[3, 3, 3]], S, ss)    # a scene stored twice
    for k in range(3):
        G.assert_same([a[k:k + 1] for a in twice], alone, "repetition %d" % k)
    # faces in another order within a mesh: the same picture, the ids renamed
    Vx, F, mat, Kd, uv, fuv, vn, fvn, mt, tx = scenes[5]
    perm = np.random.default_rng(1).permutation(len(F))
    here = gpu_render([scenes[5]], np.array([0]), cam_pos[6:7], S, ss)
    moved = gpu_render([(Vx, F[perm], mat[perm], Kd, uv, fuv[perm], vn, fvn[perm], mt, tx)], np.array([0]), cam_pos[6:7], S, ss)
    assert moved[1].tobytes() == here[1].tobytes() and (moved[0][..., 3] == here[0][..., 3]).all()
    seen = moved[2] >= 0
    assert (seen == (here[2] >= 0)).all()
    same = perm[moved[2][seen]] == here[2][seen]            # but for ties in float32 depth, which go to the lower index
    assert same.mean() > 0.99 and (moved[0][seen][same] == here[0][seen][same]).mean() > 0.99


def test_geometry_is_the_flat_calls_and_the_switches(batch):
    scenes, view_scene, cam_pos = batch
    S, ss = 96, 3
    flat = gpu_render([s[:4] for s in scenes], view_scene, cam_pos, S, ss)
    G.assert_same(flat, G.oracle_render([s[:4] for s in scenes], view_scene, cam_pos, S, ss)[:3], "flat")
    shaded = gpu_render(scenes, view_scene, cam_pos, S, ss)
    assert shaded[1].tobytes() == flat[1].tobytes() and shaded[2].tobytes() == flat[2].tobytes()
    assert shaded[0][..., 3].tobytes() == flat[0][..., 3].tobytes()
    for w, m in enumerate(view_scene):                                            # colours: only where there are attributes
        assert (shaded[0][w].tobytes() == flat[0][w].tobytes()) == (len(scenes[m]) == 4 or m == 6), (w, m)
    off = gpu_render(scenes, view_scene, cam_pos, S, ss, textures=False, smooth_normals=False)
    G.assert_same(off, flat, "both switches off")
    absent = [s if len(s) == 4 else tuple(s[:4]) + SO.attributes(s[:4]) for s in scenes]                # every index -1
    G.assert_same(gpu_render(absent, view_scene, cam_pos, S, ss), flat, "attributes absent")
    for kw in (dict(textures=False), dict(smooth_normals=False)):
        got = gpu_render(scenes, view_scene, cam_pos, S, ss, **kw)
        G.assert_same(got, oracle_render(scenes, view_scene, cam_pos, S, ss, **kw)[:3], str(kw))
        assert got[0].tobytes() != shaded[0].tobytes() and got[0].tobytes() != flat[0].tobytes()


def test_orientation_and_perspective_correction():
    rot = O.rotation_of(H.CAM)
    rgba, _, _ = gpu_render([H.facing_quad(rot)], np.array([0]), np.array([H.CAM]), 8, 1, camera_distance=2.0, focal_length=2.0)
    H.check_facing_quad(rgba[0])
    g = H.RECEDING
    rgba, _, _ = gpu_render([H.receding_quad(rot)], np.array([0]), np.array([H.CAM]), g["S"], g["ss"], camera_distance=g["cd"],
                            focal_length=g["f"])
    H.check_receding_quad(rgba[0])


def test_bad_attributes_raise_through_the_status_word():
    import dpc.render as R

    rot = O.rotation_of(CAMS[0])
    good = SO.shaded_grid(3, 0, [SO.checker(4, 4, 0)], mat_tex=(0, 0))
    expect = {"uv index": "texture coordinate index", "texture index": "texture index", "vn index": "normal index",
              "nan uv": "NaN or infinite texture coordinate", "inf normal": "NaN or infinite vertex normal"}
    bad = H.bad_attribute_scenes(rot)
    for name, (scene, bit) in bad.items():
        assert SO.render(scene, rot, 2.0, 1.875, 32, 2)[3] == bit, name
        text = next(v for k, v in expect.items() if name.startswith(k))
        with pytest.raises(R.MeshError, match=text) as err:
            R.render_mesh_views([package_scene(good), package_scene(scene)], [[CAMS[0]], [CAMS[0]]], image_size=32, supersample=2)
        assert "scene 1" in str(err.value), (name, str(err.value))
    # a group that is switched off is not read: its errors go with it
    flat = O.render(*bad["nan uv"][0][:4], rot, 2.0, 1.875, 32, 2)
    got = gpu_render([bad["nan uv"][0]], np.array([0]), np.array([CAMS[0]]), 32, 2, textures=False, smooth_normals=False)
    G.assert_same([a[0] for a in got], flat[:3], "switched off")
    R.render_mesh_views([package_scene(bad["nan uv"][0])], [[CAMS[0]]], image_size=32, textures=False)
    R.render_mesh_views([package_scene(bad["vn index beyond"][0])], [[CAMS[0]]], image_size=32, smooth_normals=False)
    # the rest of a split goes on without the bad models
    errors, saved = {}, {}
    scenes = {"a": package_scene(good), "b": package_scene(bad["uv index beyond"][0]), "c": O.special_scenes(rot)["sliver"],
              "d": package_scene(bad["inf normal"][0])}
    out = R.render_training_views(list("abcd"), lambda n: scenes[n], {n: [CAMS[0], CAMS[1]] for n in "abcd"},
                                  lambda n, rgba, depth, pos: saved.__setitem__(n, (rgba, depth, pos)), errors=errors,
                                  image_size=32, supersample=2)
    assert sorted(out) == ["a", "c"] == sorted(saved) and sorted(errors) == ["b", "d"]
    assert "texture coordinate index" in errors["b"] and "vertex normal" in errors["d"]
    want = SO.render_views([good], [(0, O.rotation_of(c), 2.0, 1.875) for c in CAMS[:2]], 32, 2)
    assert out["a"][0].tobytes() == want[0].tobytes() and out["a"][1].tobytes() == want[1].tobytes()
    with pytest.raises(R.MeshError, match="model 'b'"):
        R.render_training_views(["a", "b"], lambda n: scenes[n], {n: [CAMS[0]] for n in "ab"}, image_size=32, supersample=2)
    # and the split's switches reach the renderer
    off = R.render_training_views(["a"], lambda n: scenes[n], {"a": [CAMS[0]]}, image_size=32, supersample=2, textures=False)
    want = SO.render_views([good], [(0, rot, 2.0, 1.875)], 32, 2, textures=False)
    assert off["a"][0].tobytes() == want[0].tobytes() and off["a"][0].tobytes() != out["a"][0][:1].tobytes()


def write_model(folder, scene, image):
    """model.obj + model.mtl + tex.png of a shaded_grid scene (one uv and one normal per vertex)."""
    import dpc.render as R

    Vx, F, mat, Kd = scene[:4]
    folder.mkdir(parents=True)
    R.write_png(str(folder / "tex.png"), image)
    (folder / "model.mtl").write_text("newmtl m0\nKd %r %r %r\nmap_Kd tex.png\nnewmtl m1\nKd %r %r %r\n" % (*Kd[0].tolist(), *Kd[1].tolist()))
    lines = ["mtllib model.mtl"] + ["v %r %r %r" % tuple(p) for p in Vx.tolist()] + ["vt %r %r" % tuple(p) for p in scene[4].tolist()]
    lines += ["vn %r %r %r" % tuple(p) for p in scene[6].tolist()]
    for k in (0, 1):
        lines += ["usemtl m%d" % k] + ["f " + " ".join("%d/%d/%d" % (i + 1, i + 1, i + 1) for i in f) for f in F[mat == k].tolist()]
    (folder / "model.obj").write_text("\n".join(lines) + "\n")


def test_tool_to_training_step(tmp_path, monkeypatch):
    """Two .obj + .mtl + .png models -> tools/render_train_data.py --textures --smooth_normals --write_features -> the oracle's
    bytes in render_0.png; the features load and pass the view sampler and one training step."""
    import dpc.render as R
    from dpc.harness import TrainStep, sample_views

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_train_data as tool

    cfg = G.Cfg(json.load(open(os.path.join(GOLDEN, "f10_config.json"))))
    S = cfg.input_shape[0]
    models = {"m_hill": (SO.shaded_grid(6, 5, [], uv_range=(-0.5, 1.5)), SO.checker(7, 9, 1)),
              "m_dune": (SO.shaded_grid(4, 6, []), SO.checker(16, 16, 2))}
    (tmp_path / "splits").mkdir()
    (tmp_path / "splits" / "03001627_train.txt").write_text("".join(n + "\n" for n in models))
    for name, (scene, image) in models.items():
        write_model(tmp_path / "shapenet" / "03001627" / name, scene, image)
    monkeypatch.chdir(tmp_path)
    argv = ["--shapenet_path", "shapenet", "--synth_set", "03001627", "--subset", "train", "--out_dir", "renders",
            "--num_views", str(cfg.num_views), "--image_size", str(S), "--seed", "3", "--write_features", "features",
            "--textures", "--smooth_normals"]
    first = tool.main(argv)
    assert first == {"written": list(models), "skipped": [], "failed": {}, "warnings": {}}
    pos = R.sample_camera_positions(2, cfg.num_views, 3)
    for i, name in enumerate(models):
        path = str(tmp_path / "shapenet" / "03001627" / name / "model.obj")
        loaded = R.load_obj_scene_shaded(path)
        assert len(loaded.textures) == 1 and (loaded.textures[0] == models[name][1]).all() and loaded.mat_tex.tolist() == [0, -1]
        assert (loaded.uv == models[name][0][4]).all() and (loaded.normals == models[name][0][6]).all()
        views = [(0, O.rotation_of(pos[i, 0]), 2.0, 1.875)]
        want = SO.render_views([loaded], views, S, 3)
        img = R.read_png_any(str(tmp_path / "renders" / "03001627" / name / "render_0.png"))
        assert img.tobytes() == want[0][0].tobytes() and want[4][0]["textured"] > 0 and want[4][0]["smooth"] > 0
        assert img.tobytes() != O.render_views([loaded[:4]], views, S, 3)[0][0].tobytes()
        dep = R.read_png_any(str(tmp_path / "renders" / "03001627" / name / "depth_0.png"))
        assert dep.tobytes() == want[1][0].tobytes()
    samples = []
    for name in models:
        with open(tmp_path / "features" / ("%s_features.p" % name), "rb") as fh:
            feature = pickle.load(fh)
        assert feature["name"] == name and feature["image"].shape == (cfg.num_views, S, S, 3)
        samples.append({"image": feature["image"].transpose(0, 3, 1, 2), "mask": feature["mask"].transpose(0, 3, 1, 2),
                        "extrinsic": feature["extrinsic"], "cam_pos": feature["cam_pos"]})      # ShapeRecords.__getitem__
    dev = torch.device("cuda")
    raw = {k: torch.from_numpy(np.stack([s[k] for s in samples])).to(dev) for k in samples[0]}     # default collation
    np.random.seed(0)
    inputs = sample_views(cfg, raw, cfg.step_size)
    assert inputs["images"].shape == (4, 3, S, S) and inputs["masks"].shape == (4, 1, S, S)
    assert 0.02 < float(inputs["masks"].mean()) < 0.9
    torch.manual_seed(0)
    step = TrainStep(cfg, dev)
    total, _ = step.loss(inputs["images"], inputs["masks"], global_step=0)
    total.backward()
    assert np.isfinite(float(total.detach())) and float(total.detach()) > 0
    # a texture that is gone: a warning in the summary, the model rendered untextured
    os.remove(str(tmp_path / "shapenet" / "03001627" / "m_dune" / "tex.png"))
    second = tool.main(argv[:4] + ["--subset", "train", "--out_dir", "again"] + argv[8:])
    assert second["written"] == list(models) and second["failed"] == {} and list(second["warnings"]) == ["m_dune"]
    assert "tex.png" in second["warnings"]["m_dune"][0]
    third = tool.main(argv)
    assert third == {"written": [], "skipped": list(models), "failed": {}, "warnings": {}}
