"""The training-view renderer on the GPU (dpc.render.meshviews, csrc/dpc_mesh_raster.hip) against the numpy oracle of
tests/mesh_render_oracle.py, byte for byte: ragged batches, every supersampling and image sizes that are and are not
multiples of the tile, independence of batching and order, the status word's errors; against fixture F18 (the
reference's camera); the pooling identity; and tools/render_train_data.py through to one training step."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import mesh_render_oracle as O
import test_mesh_render_host as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CAMS = [(1.2, -0.9, 0.7), (-0.6, 1.7, 0.45), (-1.5, -0.8, -0.35), (0.3, 1.9, -0.6)]
TWO = np.array([[0.3, 0.3, 0.9], [0.9, 0.9, 0.2]])


@pytest.fixture(scope="module")
def f18():
    return dict(np.load(os.path.join(GOLDEN, "f18_mesh_views.npz")))


@pytest.fixture(scope="module")
def batch(f18):
    """A ragged batch: scenes of 0, 1, ... 100 352 faces; the boxes have three views, interleaved with the others'."""
    special = O.special_scenes(O.rotation_of(CAMS[0]))   # built for camera 0, drawn from two cameras
    scenes = [special["one face"], (f18["V"], f18["F"], f18["material"], f18["Kd"]), O.grid_mesh(224) + (TWO,),
              special["empty"], special["coplanar duplicates"], special["sliver"], special["partly and wholly outside"],
              special["parallel squares"], O.grid_mesh(7, seed=2) + (TWO,), special["zero area"]]
    assert len(scenes[2][1]) >= 100000 and len(scenes[0][1]) == 1
    view_scene = [1, 0, 2, 1, 3, 4, 5, 1, 6, 7, 8, 9, 4, 8]
    view_cam = [0, 0, 1, 1, 0, 0, 0, 2, 0, 0, 3, 0, 3, 1]
    return scenes, np.array(view_scene), np.array([CAMS[c] for c in view_cam])


def gpu_render(scenes, view_scene, cam_pos, S, ss):
    import dpc.render as R

    rgba, depth, fid = R.render_mesh_views(scenes, cam_pos, image_size=S, supersample=ss, return_face_id=True,
                                           view_scene=view_scene)
    assert rgba.is_cuda and rgba.dtype == torch.uint8 and depth.dtype == torch.uint16 and fid.dtype == torch.int32
    return rgba.cpu().numpy(), depth.cpu().numpy(), fid.cpu().numpy()


def oracle_render(scenes, view_scene, cam_pos, S, ss):
    views = [(int(m), O.rotation_of(c), 2.0, 1.875) for m, c in zip(view_scene, cam_pos)]
    return O.render_views(scenes, views, S, ss)


def assert_same(got, want, what):
    for name, g, w in zip(("rgba", "depth", "face_id"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError("%s: %s differs at %d places, first %s: %s vs %s"
                                 % (what, name, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])]))


@pytest.mark.parametrize("ss", [1, 2, 3, 4])
@pytest.mark.parametrize("S", [32, 128, 200])
def test_ragged_batch_equals_the_oracle_by_bytes(batch, S, ss):
    scenes, view_scene, cam_pos = batch
    got = gpu_render(scenes, view_scene, cam_pos, S, ss)
    want = oracle_render(scenes, view_scene, cam_pos, S, ss)
    assert want[3] == 0
    assert_same(got, want[:3], "S %d ss %d" % (S, ss))
    fid = got[2]
    assert (fid[4] == -1).all() and (fid[11] == -1).all() and not got[0][4].any() and (got[1][4] == 65535).all()
    assert (fid[2] >= 0).mean() > 0.1 and fid[2].max() > 50000            # the large mesh is there
    assert set(np.unique(fid[5])) == {-1, 0, 1}                            # coplanar duplicates: ties to the lower index


def test_images_do_not_depend_on_batching_order_or_run(batch):
    scenes, view_scene, cam_pos = batch
    S, ss = 72, 3
    whole = gpu_render(scenes, view_scene, cam_pos, S, ss)
    again = gpu_render(scenes, view_scene, cam_pos, S, ss)
    assert_same(again, whole, "second run")
    order = np.random.default_rng(0).permutation(len(view_scene))
    shuffled = gpu_render(scenes, view_scene[order], cam_pos[order], S, ss)
    assert_same([a[np.argsort(order)] for a in shuffled], whole, "another order")
    for lo, hi in ((0, 3), (3, 4), (4, 9), (9, 14)):                         # another split, scenes renumbered
        used = sorted(set(view_scene[lo:hi].tolist()))
        part = gpu_render([scenes[m] for m in used], np.array([used.index(m) for m in view_scene[lo:hi]]), cam_pos[lo:hi], S, ss)
        assert_same(part, [a[lo:hi] for a in whole], "views %d..%d alone" % (lo, hi))
    alone = gpu_render([scenes[1]], np.array([0]), cam_pos[7:8], S, ss)
    assert_same(alone, [a[7:8] for a in whole], "one view alone")
    # faces in another order within a mesh: the same picture, the ids renamed
    V, F, mat, Kd = scenes[1]
    perm = np.random.default_rng(1).permutation(len(F))
    moved = gpu_render([(V, F[perm], mat[perm], Kd)], np.array([0]), cam_pos[7:8], S, ss)
    assert moved[1].tobytes() == alone[1].tobytes() and (moved[0][..., 3] == alone[0][..., 3]).all()
    seen = moved[2] >= 0
    assert (seen == (alone[2] >= 0)).all()
    assert (mat[perm][moved[2][seen]] == mat[alone[2][seen]]).all()           # the same box shows at every pixel


def test_scene_major_camera_lists_and_cfg(f18):
    import dpc.render as R

    scenes = [(f18["V"], f18["F"], f18["material"], f18["Kd"]), O.grid_mesh(5) + (TWO,)]
    cam = [np.array(CAMS[:3]), np.array(CAMS[3:])]
    cfg = {"camera_distance": 2.5, "focal_length": 1.5}
    rgba, depth = R.render_mesh_views(scenes, cam, cfg, image_size=48, supersample=2)
    assert rgba.shape == (4, 48, 48, 4) and depth.shape == (4, 48, 48)
    views = [(0, O.rotation_of(c), 2.5, 1.5) for c in CAMS[:3]] + [(1, O.rotation_of(CAMS[3]), 2.5, 1.5)]
    want = O.render_views(scenes, views, 48, 2)
    assert rgba.cpu().numpy().tobytes() == want[0].tobytes() and depth.cpu().numpy().tobytes() == want[1].tobytes()
    none = R.render_mesh_views([], [], image_size=16)
    assert none[0].shape == (0, 16, 16, 4)


def test_bad_inputs_raise_through_the_status_word():
    import dpc.render as R

    rot = O.rotation_of(CAMS[0])
    good = O.special_scenes(rot)["one face"]
    expect = {O.STATUS_NONFINITE: "NaN or infinite", O.STATUS_BAD_INDEX: "outside", O.STATUS_NEAR: "camera plane"}
    for name, (scene, bit) in O.bad_scenes(rot).items():
        assert O.render(*scene, rot, 2.0, 1.875, 32, 2)[3] == bit, name
        with pytest.raises(R.MeshError, match=expect[bit]) as err:
            R.render_mesh_views([good, scene], [[CAMS[0]], [CAMS[0]]], image_size=32, supersample=2)
        assert ("scene 1" in str(err.value)), (name, str(err.value))
    # the rest of a split goes on without the bad model
    errors, saved = {}, {}
    scenes = {"a": good, "b": O.bad_scenes(rot)["near guard"][0], "c": O.special_scenes(rot)["sliver"]}
    out = R.render_training_views(["a", "b", "c", "d"], lambda n: scenes[n], {n: [CAMS[0], CAMS[1]] for n in "abcd"},
                                  lambda n, rgba, depth, pos: saved.__setitem__(n, (rgba, depth, pos)), errors=errors,
                                  image_size=32, supersample=2)
    assert sorted(out) == ["a", "c"] == sorted(saved) and sorted(errors) == ["b", "d"] and "camera plane" in errors["b"]
    want = O.render_views([good], [(0, O.rotation_of(c), 2.0, 1.875) for c in CAMS[:2]], 32, 2)
    assert out["a"][0].tobytes() == want[0].tobytes() and out["a"][1].tobytes() == want[1].tobytes()
    with pytest.raises(R.MeshError, match="model 'b'"):
        R.render_training_views(["a", "b"], lambda n: scenes[n], {n: [CAMS[0]] for n in "ab"}, image_size=32, supersample=2)


def test_split_does_not_depend_on_models_per_call(f18):
    import dpc.render as R

    rot = O.rotation_of(CAMS[0])
    sp = O.special_scenes(rot)
    scenes = {"boxes": (f18["V"], f18["F"], f18["material"], f18["Kd"]), "one": sp["one face"], "sq": sp["parallel squares"],
              "grid": O.grid_mesh(9) + (TWO,)}
    names = list(scenes)
    pos = R.sample_camera_positions(len(names), 3, 4)
    runs = [R.render_training_views(names, lambda n: scenes[n], pos, models_per_call=k, image_size=40, supersample=3, **kw)
            for k, kw in ((1, {}), (3, {}), (64, {}), (64, dict(workspace_limit=1)))]
    for other in runs[1:]:
        for n in names:
            assert other[n][0].tobytes() == runs[0][n][0].tobytes() and other[n][1].tobytes() == runs[0][n][1].tobytes()
    want = O.render_views([scenes["grid"]], [(0, O.rotation_of(c), 2.0, 1.875) for c in pos[3]], 40, 3)
    assert runs[0]["grid"][0].tobytes() == want[0].tobytes()


def test_views_contain_the_reference_projection(f18):
    S, ss = 32, 3
    scene = (f18["V"], f18["F"], f18["material"], f18["Kd"])
    rgba, _, _ = gpu_render([scene], np.zeros(3, dtype=np.int64), f18["cam_pos"], S, ss)
    H.check_views_against_f18(f18, [rgba[w][..., 3] for w in range(3)], S)


def test_depth_order():
    rot, scene = H.depth_order_scene()
    _, depth, fid = gpu_render([scene], np.array([0]), np.array([H.CAM]), 64, 3)
    H.check_depth_order(fid[0], depth[0], 64)


def test_pooling_128_at_ss2_is_64_at_ss4(f18, batch):
    scenes, view_scene, cam_pos = batch
    fine = gpu_render(scenes, view_scene, cam_pos, 128, 2)[0][..., 3]
    coarse = gpu_render(scenes, view_scene, cam_pos, 64, 4)[0][..., 3]
    cf, cc = O.covered_from_alpha(fine, 2), O.covered_from_alpha(coarse, 4)
    assert (cf.reshape(-1, 64, 2, 64, 2).sum(axis=(2, 4)) == cc).all()
    assert cc.max() == 16 and ((cc > 0) & (cc < 16)).any()


class Cfg(dict):
    __getattr__ = dict.__getitem__


def test_tool_to_training_step(tmp_path, monkeypatch):
    """Two .obj + .mtl models -> tools/render_train_data.py --write_features -> the features load, are stacked as
    ShapeRecords.__getitem__ and the loader's collation stack them, pass the view sampler and one training step."""
    import dpc.render as R
    from dpc.harness import TrainStep, sample_views

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import render_train_data as tool

    cfg = Cfg(json.load(open(os.path.join(GOLDEN, "f10_config.json"))))
    S = cfg.input_shape[0]
    boxes = {"m_chair": [((-0.24, -0.04, -0.2), (0.2, 0.03, 0.24)), ((-0.24, 0.03, -0.2), (-0.17, 0.34, 0.24))],
             "m_table": [((-0.3, 0.1, -0.2), (0.3, 0.15, 0.2)), ((-0.05, -0.3, -0.05), (0.05, 0.1, 0.05))]}
    (tmp_path / "splits").mkdir()
    (tmp_path / "splits" / "03001627_train.txt").write_text("".join(n + "\n" for n in boxes))
    for name, bx in boxes.items():
        V, F, mat = O.box_mesh(bx)
        d = tmp_path / "shapenet" / "03001627" / name
        d.mkdir(parents=True)
        (d / "model.mtl").write_text("newmtl m0\nKd 0.8 0.2 0.2\nnewmtl m1\nKd 0.2 0.3 0.9\n")
        lines = ["mtllib model.mtl"] + ["v %r %r %r" % tuple(p) for p in V.tolist()]
        for k in (0, 1):
            lines += ["usemtl m%d" % k] + ["f %d %d %d" % tuple(i + 1 for i in f) for f in F[mat == k].tolist()]
        (d / "model.obj").write_text("\n".join(lines) + "\n")
    monkeypatch.chdir(tmp_path)
    argv = ["--shapenet_path", "shapenet", "--synth_set", "03001627", "--subset", "train", "--out_dir", "renders",
            "--num_views", str(cfg.num_views), "--image_size", str(S), "--seed", "3", "--write_features", "features"]
    first = tool.main(argv)
    assert first == {"written": list(boxes), "skipped": [], "failed": {}}
    # the archive's layout, and files the readers read back
    import scipy.io

    pos = R.sample_camera_positions(2, cfg.num_views, 3)
    for i, name in enumerate(boxes):
        for k in range(cfg.num_views):
            img = R.read_png_any(str(tmp_path / "renders" / "03001627" / name / ("render_%d.png" % k)))
            dep = R.read_png_any(str(tmp_path / "renders" / "03001627" / name / ("depth_%d.png" % k)))
            cam = scipy.io.loadmat(str(tmp_path / "renders" / "03001627" / name / ("camera_%d.mat" % k)))
            assert img.shape == (S, S, 4) and dep.shape == (S, S) and dep.dtype == np.uint16 and img[..., 3].max() == 255
            assert np.abs(cam["pos"].reshape(3) - pos[i, k]).max() == 0 and cam["extrinsic"].shape == (4, 4)
            assert (cam["extrinsic"] == R.camera_extrinsic(pos[i, k])).all()
        want = O.render_views([R.load_obj_scene(str(tmp_path / "shapenet" / "03001627" / name / "model.obj"))[:4]],
                              [(0, O.rotation_of(pos[i, 0]), 2.0, 1.875)], S, 3)
        assert img.shape and R.read_png_any(str(tmp_path / "renders" / "03001627" / name / "render_0.png")).tobytes() == want[0][0].tobytes()
    samples = []
    for name in boxes:
        with open(tmp_path / "features" / ("%s_features.p" % name), "rb") as fh:
            feature = pickle.load(fh)
        assert feature["name"] == name and feature["image"].shape == (cfg.num_views, S, S, 3)
        assert feature["image"].dtype == feature["mask"].dtype == feature["depth"].dtype == np.float32
        samples.append({"image": feature["image"].transpose(0, 3, 1, 2), "mask": feature["mask"].transpose(0, 3, 1, 2),
                        "extrinsic": feature["extrinsic"], "cam_pos": feature["cam_pos"]})      # ShapeRecords.__getitem__
    dev = torch.device("cuda")
    raw = {k: torch.from_numpy(np.stack([s[k] for s in samples])).to(dev) for k in samples[0]}     # default collation
    assert raw["image"].shape == (2, cfg.num_views, 3, S, S) and raw["mask"].shape == (2, cfg.num_views, 1, S, S)
    np.random.seed(0)
    inputs = sample_views(cfg, raw, cfg.step_size)
    assert inputs["images"].shape == (4, 3, S, S) and inputs["masks"].shape == (4, 1, S, S) and inputs["matrices"].shape == (4, 4, 4)
    assert 0.02 < float(inputs["masks"].mean()) < 0.9
    torch.manual_seed(0)
    step = TrainStep(cfg, dev)
    total, _ = step.loss(inputs["images"], inputs["masks"], global_step=0)
    total.backward()
    assert np.isfinite(float(total.detach())) and float(total.detach()) > 0
    second = tool.main(argv)
    assert second == {"written": [], "skipped": list(boxes), "failed": {}}
