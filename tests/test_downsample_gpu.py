"""Voxel-grid downsampling on the GPU (csrc/dpc_downsample.hip): every output point, count and the (kx, ky, kz) order
against the numpy oracle of tests/test_downsample_host.py by bytes; independence from batching; reproducibility;
refusals; and the file tool and eval_chamfer on the GT it writes."""
import os

import numpy as np
import pytest
import scipy.io
import torch

import dpc.render as R
from test_downsample_host import oracle_downsample

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lattice(vs, n_side=12):
    """Points (j + 0.5) * vs with a point at 0: (x - lo) / vs = j + 1 lands on a voxel face (exactly when vs is dyadic),
    plus copies one ulp either side of each coordinate."""
    j = np.arange(n_side) + 0.5
    g = np.stack(np.meshgrid(j, j[:5], j[:3], indexing="ij"), -1).reshape(-1, 3) * vs
    g = np.concatenate([np.zeros((1, 3)), g])
    return np.concatenate([g, np.nextafter(g, np.inf), np.nextafter(g, -np.inf)])


def _batch(dtype, seed=0):
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 2, 63, 64, 65, 1000, 4097, 150000]
    clouds = [(rng.random((n, 3)) - 0.5) * rng.uniform(0.2, 1.5) for n in sizes]
    clouds[6][500:700] = clouds[6][0:200]                     # exact duplicates
    clouds.append(_lattice(0.25))
    clouds.append(_lattice(0.05))
    clouds.append(rng.random((200000, 3)) * 0.09 + 0.3)       # one voxel of 200 000 points at vs >= 0.2
    return [c.astype(dtype) for c in clouds]


def _same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("vs", [1e-3, 0.01, 0.05, 0.2, 0.25])
def test_parity_with_the_oracle(dtype, vs):
    clouds = _batch(dtype)
    out = R.voxel_down_sample(clouds, vs)
    assert len(out) == len(clouds)
    for i, (c, o) in enumerate(zip(clouds, out)):
        assert o.is_cuda
        _same(o, oracle_downsample(c, vs), (i, len(c)))
    if vs >= 0.2:
        assert out[-1].shape == (1, 3)


def test_device_inputs_and_mixed_dtypes():
    clouds = _batch(np.float64, seed=3)[5:9]
    mixed = [torch.from_numpy(c).cuda() if i % 2 else c.astype(np.float32) for i, c in enumerate(clouds)]
    out = R.voxel_down_sample(mixed, 0.01)
    for i, (c, o) in enumerate(zip(mixed, out)):
        host = c.cpu().numpy() if isinstance(c, torch.Tensor) else c
        _same(o, oracle_downsample(host, 0.01), i)
    single = R.voxel_down_sample(clouds[2], 0.01)
    _same(single, oracle_downsample(clouds[2], 0.01), "single")


def test_independent_of_batching_and_reproducible():
    clouds = _batch(np.float64, seed=1)
    batch = [o.cpu().numpy() for o in R.voxel_down_sample(clouds, 0.05)]
    for i, c in enumerate(clouds):
        alone = R.voxel_down_sample([c], 0.05)[0]
        _same(alone, batch[i], ("alone", i))
    perm = np.random.default_rng(5).permutation(len(clouds))
    shuffled = R.voxel_down_sample([clouds[k] for k in perm], 0.05)
    for j, k in enumerate(perm):
        _same(shuffled[j], batch[k], ("permuted", k))
    again = R.voxel_down_sample(clouds, 0.05)
    for i in range(len(clouds)):
        _same(again[i], batch[i], ("repeat", i))


def test_downsample_split_matches_and_ignores_grouping():
    clouds = _batch(np.float64, seed=2)
    names = ["m%d" % i for i in range(len(clouds))]
    data = dict(zip(names, clouds))
    data["m3"] = None                                           # skipped, as a model without a dense cloud
    saved = {}
    res = R.downsample_split(names, data.get, 0.01, save=saved.__setitem__, clouds_per_call=3)
    assert list(res) == [n for n in names if n != "m3"] and set(saved) == set(res)
    one = R.downsample_split(names, data.get, 0.01, clouds_per_call=100)
    for n in res:
        _same(res[n], oracle_downsample(data[n], 0.01), n)
        assert res[n].tobytes() == one[n].tobytes() and saved[n] is res[n]


def test_refusals_and_recovery():
    good = np.random.default_rng(0).random((1000, 3))
    unit = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    with pytest.raises(ValueError, match="too small"):
        R.voxel_down_sample([good, unit], 1e-10)               # open3d: vs * (2^31 - 1) < the padded extent
    with pytest.raises(ValueError, match="64 bits"):
        R.voxel_down_sample([unit, good], 1e-9)                # 3 x 30 key bits: accepted by open3d, beyond a 64-bit key
    assert len(oracle_downsample(unit, 1e-9)) == 2
    bad = good.copy()
    bad[17, 2] = np.nan
    with pytest.raises(ValueError, match="cloud 1"):
        R.voxel_down_sample([good, bad], 0.01)
    inf = good.astype(np.float32)
    inf[3, 0] = np.inf
    with pytest.raises(ValueError, match="cloud 0"):
        R.voxel_down_sample([inf], 0.01)
    _same(R.voxel_down_sample([good], 0.01)[0], oracle_downsample(good, 0.01), "after the refusals")


def _dense_model(rng, n):
    """Points on the faces of two random boxes: a closed surface, as densified GT is."""
    pts = []
    for _ in range(2):
        lo = rng.uniform(-0.5, 0.0, 3)
        hi = lo + rng.uniform(0.2, 0.5, 3)
        u = rng.uniform(lo, hi, size=(n // 2, 3))
        axis = rng.integers(0, 3, n // 2)
        side = rng.integers(0, 2, n // 2)
        u[np.arange(n // 2), axis] = np.where(side == 1, hi[axis], lo[axis])
        pts.append(u)
    return np.concatenate(pts)


def test_tool_writes_open3d_points_and_eval_chamfer_reads_them(tmp_path):
    import importlib.util

    spec = importlib.util.spec_from_file_location("downsample_gt", os.path.join(ROOT, "tools", "downsample_gt.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(11)
    names = ["model_a", "model_b", "model_c"]
    dense_dir = tmp_path / "dense" / "03001627"
    dense_dir.mkdir(parents=True)
    dense = {}
    for k, name in enumerate(names):
        dense[name] = _dense_model(rng, 20000 + 5000 * k)
        scipy.io.savemat(str(dense_dir / ("%s.mat" % name)), {"points": dense[name]})
    argv = ["--inp_dir", str(tmp_path / "dense"), "--out_dir", str(tmp_path / "down"), "--synth_set", "03001627"]
    first = tool.main(argv)
    assert first == {"written": names, "skipped": []}
    ref = {n: oracle_downsample(dense[n], 0.01) for n in names}
    down_dir = tmp_path / "down" / "03001627"
    for n in names:
        _same(scipy.io.loadmat(str(down_dir / ("%s.mat" % n)))["points"], ref[n], n)
    assert tool.main(argv) == {"written": [], "skipped": names}

    preds = tmp_path / "preds"
    preds.mkdir()
    for n in names:
        pts = np.stack([_dense_model(rng, 2000) * 1.05 for _ in range(3)]).astype(np.float32)
        R.save_predictions(str(preds / ("%s_pc.pkl" % n)), pts)
    from_files = R.eval_chamfer(str(preds), names, lambda n: scipy.io.loadmat(str(down_dir / ("%s.mat" % n)))["points"])
    from_oracle = R.eval_chamfer(str(preds), names, ref.get)
    assert from_files["model_names"] == names
    assert from_files["chamfer"].tobytes() == from_oracle["chamfer"].tobytes()
    assert from_files["final"].tobytes() == from_oracle["final"].tobytes()
