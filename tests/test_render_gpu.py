"""Point-cloud rendering on the GPU (csrc/dpc_raster.hip, dpc.render.visualise): ids, float32 and uint8 images against the
numpy oracle of tests/render_oracle.py by bytes, over ragged batches with awkward scenes; independence from batching;
reproducibility; the reference's render_point_cloud signature; the runner and its tool; refusals."""
import ctypes
import importlib.util
import os
import types

import numpy as np
import pytest
import scipy.io
import torch

import render_oracle as O
import dpc.render as R
from dpc.render import _native
from dpc.render import visualise as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = (140.0, 15.0, 2.0)


def cam_pred(az, el, d):
    C = V.camera_frame(az, el, d)[0]
    return np.array([-C[1], C[2], C[0]])  # the camera position in the prediction frame


def scene(n, seed, dtype=np.float32):
    """n tanh-distributed points with duplicates, a sphere around the camera and one behind it, points outside the
    frustum and on the image border."""
    rng = np.random.default_rng(seed)
    p = np.tanh(rng.standard_normal((n, 3))) * 0.5
    if n >= 8:
        p[1] = p[0]                              # a duplicate: the lower index wins every tie
        p[2] = cam_pred(*CAM)                    # the camera inside a sphere: never drawn
        p[3] = 1.7 * cam_pred(*CAM)              # behind the camera
        p[4] = [3.0, 0.0, 0.0]                   # outside the frustum
        p[5] = [0.0, 0.5333, 0.0]                # near the top border
    return p.astype(dtype)


def check(clouds, S, ss, colors=None, radii=None, cams=CAM, point_size=0.01):
    az, el, d = cams
    f32, ids = R.render_point_clouds(clouds, az, el, d, image_size=S, supersample=ss, colors=colors, radii=radii,
                                     point_size=point_size, dtype=torch.float32, return_ids=True)
    u8 = R.render_point_clouds(clouds, az, el, d, image_size=S, supersample=ss, colors=colors, radii=radii,
                               point_size=point_size)
    f32, ids, u8 = f32.cpu().numpy(), ids.cpu().numpy(), u8.cpu().numpy()
    P = len(clouds)
    per = lambda v, p: v[p] if np.ndim(v) else v
    for p in range(P):
        frame = V.camera_frame(per(az, p), per(el, p), per(d, p))
        img, wid = O.render(np.asarray(clouds[p], dtype=np.float64), frame, S, ss, 60.0 / 32.0 * S, point_size,
                            None if colors is None else colors[p], None if radii is None else radii[p])
        assert (ids[p] == wid).all(), (p, S, ss, np.argwhere(ids[p] != wid)[:5])
        assert f32[p].tobytes() == img.tobytes(), (p, S, ss)
        assert u8[p].tobytes() == O.to_uint8(img).tobytes(), (p, S, ss)
    return f32, ids


@pytest.mark.parametrize("S,ss,sizes", [(64, 3, (0, 1, 2, 500, 8000, 16000)), (17, 4, (0, 1, 2, 500, 8000)),
                                        (1, 2, (2, 500, 8000)), (256, 1, (0, 2, 500, 8000)), (256, 3, (500, 8000)),
                                        (512, 2, (1, 500))])
def test_ragged_batches_equal_the_oracle(S, ss, sizes):
    clouds = [scene(n, 10 + i, np.float32 if i % 2 else np.float64) for i, n in enumerate(sizes)]
    _, ids = check(clouds, S, ss)
    if S >= 64:
        assert (ids >= 0).any() and (ids == -1).any()


def test_colors_radii_and_large_spheres_equal_the_oracle():
    rng = np.random.default_rng(3)
    clouds = [scene(500, 1), scene(8, 2, np.float64), scene(300, 3)]
    colors = [rng.random((500, 3)).astype(np.float32), None, rng.random((300, 3)).astype(np.float32)]
    big = np.full(8, 0.02)
    big[6] = 0.4                     # a sphere spanning several 16-pixel tiles
    big[7] = 0.15
    radii = [None, big, rng.uniform(0.005, 0.03, 300)]
    for S, ss in ((64, 4), (100, 3), (512, 1)):
        check(clouds, S, ss, colors, radii)


def test_per_cloud_cameras_equal_the_oracle():
    clouds = [scene(400, 5), scene(400, 6), scene(400, 7)]
    check(clouds, 48, 3, cams=([140.0, 0.0, 275.0], [15.0, -30.0, 60.0], [2.0, 1.2, 3.0]))


def test_batch_composition_and_reruns_do_not_change_images():
    clouds = [scene(n, 20 + n) for n in (700, 0, 3000, 1, 8000)]
    a = R.render_point_clouds(clouds, image_size=96, supersample=3, dtype=torch.float32).cpu().numpy()
    b = R.render_point_clouds(clouds, image_size=96, supersample=3, dtype=torch.float32).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    order = [4, 2, 0, 3, 1]
    c = R.render_point_clouds([clouds[i] for i in order], image_size=96, supersample=3, dtype=torch.float32).cpu().numpy()
    for k, i in enumerate(order):
        assert c[k].tobytes() == a[i].tobytes()
    for i in range(len(clouds)):
        one = R.render_point_clouds([scene(5, 99), clouds[i]], image_size=96, supersample=3, dtype=torch.float32)
        assert one[1].cpu().numpy().tobytes() == a[i].tobytes()


def test_render_point_cloud_is_the_references_signature():
    pc = scene(4000, 8)
    cfg = {"vis_azimuth": 30.0, "vis_elevation": 20.0, "vis_dist": 2.5, "render_image_size": 128,
           "render_cycles_samples": 500}
    img = R.render_point_cloud(pc, cfg)
    want = R.render_point_clouds([pc], 30.0, 20.0, 2.5, image_size=128)[0].cpu().numpy()
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (128, 128, 3)
    assert img.tobytes() == want.tobytes()
    default = types.SimpleNamespace(vis_azimuth=140.0, vis_elevation=15.0, vis_dist=2.0, render_image_size=256,
                                    render_cycles_samples=500)  # dpc/resources/default_config.yaml:167-171
    img = R.render_point_cloud(torch.from_numpy(pc).reshape(1, -1, 3), default)
    assert img.tobytes() == R.render_point_clouds([pc])[0].cpu().numpy().tobytes()
    from render.render_point_cloud import render_point_cloud  # the overlay the notebooks import
    assert render_point_cloud is R.render_point_cloud


def test_render_split_is_independent_of_models_per_call():
    names = ["m%d" % i for i in range(7)]
    data = {n: np.stack([scene(300 + 50 * i, 30 + i), scene(300 + 50 * i, 60 + i)]) for i, n in enumerate(names)}
    load = lambda n: None if n == "m3" else data[n]
    want = R.render_point_clouds([data[n][0] for n in names if n != "m3"], image_size=64).cpu().numpy()
    for step in (1, 3, 256):
        saved = {}
        got = R.render_split(names, load, save=saved.__setitem__, models_per_call=step, image_size=64)
        assert list(got) == [n for n in names if n != "m3"] and list(saved) == list(got)
        for k, n in enumerate(got):
            assert got[n].tobytes() == want[k].tobytes() and saved[n] is got[n]
    second = R.render_split(names[:2], load, view=1, image_size=64)
    assert second["m0"].tobytes() == R.render_point_clouds([data["m0"][1]], image_size=64)[0].cpu().numpy().tobytes()


def test_colored_subsets_render_as_specified():
    model = scene(600, 40)
    rng = np.random.default_rng(4)
    idx = rng.random((2, 600)) < 0.2
    colors = np.array([[1.0, 0.0, 0.0], [0.0, 0.3, 1.0]], dtype=np.float32)
    got = R.render_split(["a"], lambda n: model[None], colored_subsets=(idx, colors), image_size=80)["a"]
    rest = ~idx.any(axis=0)
    pts = np.concatenate([model[rest], model[idx[0]], model[idx[1]]])
    cols = np.concatenate([np.full((rest.sum(), 3), 0.5, np.float32), np.repeat(colors[:1], idx[0].sum(), 0),
                           np.repeat(colors[1:], idx[1].sum(), 0)])
    rads = np.concatenate([np.full(rest.sum(), 0.0075), np.full(idx[0].sum(), 0.01), np.full(idx[1].sum(), 0.01)])
    img, _ = O.render(pts, V.camera_frame(*CAM), 80, 3, 1.875 * 80, 0.01, cols, rads)
    assert got.tobytes() == O.to_uint8(img).tobytes()
    assert (got[..., 0] > 200).any() and (got[..., 2] > 200).any()


def _tool():
    spec = importlib.util.spec_from_file_location("render_predictions", os.path.join(ROOT, "tools", "render_predictions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tool_writes_pngs_of_the_in_memory_images(tmp_path):
    inp, out = tmp_path / "pred", tmp_path / "render"
    inp.mkdir()
    clouds = {"a": np.stack([scene(900, 50), scene(900, 51)]), "b": scene(1200, 52)[None], "c": scene(700, 53)[None]}
    R.save_predictions(str(inp / "a_pc.pkl"), clouds["a"], camera_pose=np.zeros((2, 4), np.float32))
    np.savez(str(inp / "b_pc.npz"), clouds["b"])
    scipy.io.savemat(str(inp / "c_pc.mat"), {"points": clouds["c"]})
    tool = _tool()
    res = tool.main(["--inp_dir", str(inp), "--out_dir", str(out), "--render_image_size", "72", "--like_train_data",
                     "--models_per_call", "2"])
    assert sorted(res["written"]) == ["a", "b", "c"] and res["skipped"] == []
    want = R.render_point_clouds([clouds[n][0] for n in "abc"], image_size=72).cpu().numpy()
    for k, n in enumerate("abc"):
        assert V.read_png(str(out / ("%s.png" % n))).tobytes() == want[k].tobytes()
    again = tool.main(["--inp_dir", str(inp), "--out_dir", str(out), "--render_image_size", "72"])
    assert again["written"] == [] and sorted(again["skipped"]) == ["a", "b", "c"]
    (tmp_path / "list.txt").write_text("a\nmissing\n")
    with pytest.raises(AssertionError, match="missing"):
        tool.main(["--inp_dir", str(inp), "--out_dir", str(tmp_path / "r2"), "--models_list", str(tmp_path / "list.txt")])


def test_nonfinite_values_and_bad_tables_are_refused():
    good = scene(300, 70)
    bad = good.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="cloud 1"):
        R.render_point_clouds([good, bad, good])
    with pytest.raises(ValueError, match="cloud 0"):
        R.render_point_clouds([good], colors=[np.full((300, 3), np.inf, np.float32)])
    with pytest.raises(ValueError, match="cloud 0"):
        R.render_point_clouds([good], radii=[np.zeros(300)])
    # the kernel leaves a flagged image white and the others as they are
    dev = torch.device("cuda")
    L = _native.lib()
    pts = torch.from_numpy(np.concatenate([O.scene_points(good), O.scene_points(bad)])).to(dev)
    table = np.array([[0, 300], [300, 300]], dtype=np.int32)
    frames = torch.from_numpy(np.tile(np.concatenate(V.camera_frame(*CAM)), (2, 1))).to(dev)
    image = torch.empty((2, 32, 32, 3), dtype=torch.float32, device=dev)
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    td = torch.from_numpy(table).to(dev)
    host = table.ctypes.data_as(ctypes.c_void_p)
    rc = L.dpc_render_points(_native.ptr(pts), None, None, 600, _native.ptr(td), host, 2, _native.ptr(frames), 32, 2, 60.0,
                             0.01, _native.ptr(image), None, _native.ptr(status), _native.stream_ptr(dev))
    assert rc == 0 and int(status.item()) == _native.DPC_STATUS_NONFINITE
    assert (image[1] == 1.0).all() and not (image[0] == 1.0).all()
    over = np.array([[0, 300], [300, 301]], dtype=np.int32)
    rc = L.dpc_render_points(_native.ptr(pts), None, None, 600, _native.ptr(td), over.ctypes.data_as(ctypes.c_void_p), 2,
                             _native.ptr(frames), 32, 2, 60.0, 0.01, _native.ptr(image), None, _native.ptr(status),
                             _native.stream_ptr(dev))
    assert rc == _native.DPC_ERR_SHAPE
    with pytest.raises(ValueError, match="refused"):
        R.render_point_clouds([good], image_size=4097)
    with pytest.raises(ValueError, match="refused"):
        R.render_point_clouds([good], supersample=0)
