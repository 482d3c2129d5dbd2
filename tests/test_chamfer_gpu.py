"""Batched Chamfer evaluation on the GPU (csrc/dpc_chamfer.hip): per-point distances and indices against
point_cloud_distance (pinned by F11), per-pair means against np.mean bit for bit, the F16 split from the reference's own
arithmetic bit for bit, independence from batching, agreement with the per-view loop, and argument refusals."""
import numpy as np
import pytest
import torch

import dpc.render as R

pytestmark = pytest.mark.gpu


def _cloud(rng, n, dtype):
    return (rng.random((n, 3)) - 0.5).astype(dtype)


def _ragged(dtype, seed=0):
    """About 40 directed pairs over one buffer: sizes 1 .. 20000, shared targets, duplicates, one-point targets, an empty
    source.  Returns (points [n,3] numpy, pairs [P,4])."""
    rng = np.random.default_rng(seed)
    sizes = [1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4096, 8191, 8192, 8193, 20000, 3000, 513]
    clouds = [_cloud(rng, n, dtype) for n in sizes]
    clouds[14][500:600] = clouds[14][0:100]           # duplicates: exact ties
    clouds.append(np.round(_cloud(rng, 2000, dtype) * 16) / 16)   # a lattice: many ties
    start = np.cumsum([0] + [len(c) for c in clouds])
    pairs = []
    for i in range(len(sizes)):
        pairs.append((start[i], sizes[i], start[(i + 5) % len(sizes)], sizes[(i + 5) % len(sizes)]))
    lat = len(clouds) - 1
    for i in (3, 14, 18, 19):
        pairs.append((start[i], sizes[i], start[lat], 2000))          # shared target
        pairs.append((start[lat], 2000, start[i], sizes[i]))
    pairs += [(start[19], 20000, start[0], 1), (start[2], 0, start[4], 63), (start[2], 0, start[0], 0),
              (start[lat], 2000, start[lat], 2000), (start[14], 1000, start[14], 1000)]
    return np.concatenate(clouds), np.array(pairs, dtype=np.int64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_per_point_and_mean_parity(dtype):
    pts, pairs = _ragged(dtype)
    dev = torch.from_numpy(pts).cuda()
    mean, dist, idx = R.nearest_batched(dev, pairs, return_distances=True)
    assert dist.dtype == (torch.float64 if dtype == np.float64 else torch.float32) and idx.dtype == torch.int64
    assert dist.shape[0] == int(pairs[:, 1].sum())
    mean, dist, idx = mean.cpu().numpy(), dist.cpu().numpy(), idx.cpu().numpy()
    off = 0
    for p, (s0, ns, t0, nt) in enumerate(pairs):
        if ns == 0:
            assert np.isnan(mean[p])
            continue
        _, rd, ri = R.point_cloud_distance(dev[s0:s0 + ns], dev[t0:t0 + nt])
        rd, ri = rd.cpu().numpy(), ri.cpu().numpy()
        assert rd.tobytes() == dist[off:off + ns].tobytes(), p
        assert np.array_equal(ri, idx[off:off + ns]), p
        ref = np.mean(rd.astype(np.float64))
        assert np.float64(mean[p]).tobytes() == np.float64(ref).tobytes(), (p, mean[p], ref)
        off += ns


def _f16_predictions(f16, rotated=False):
    return [(f16["pred0"], f16["nums0"]), (f16["pred1"], None), (f16["pred2"], None)], [f16["gt0"], f16["gt1"], f16["gt2"]]


@pytest.fixture(scope="module")
def f16(golden):
    return golden("f16_chamfer_split.npz")


@pytest.mark.parametrize("rotated", [False, True])
def test_f16_chamfer_of_split_bit_for_bit(f16, rotated):
    preds, gts = _f16_predictions(f16)
    rot = f16["rotation"] if rotated else None
    got = R.chamfer_of_split(preds, gts, reference_rotation=rot)
    key = "_rot" if rotated else ""
    assert got.dtype == np.float64 and got.shape == (3, 2, 2)
    assert got.tobytes() == f16["chamfer" + key].tobytes(), (got, f16["chamfer" + key])
    assert (np.mean(got, axis=(0, 1)) * 100).tobytes() == f16["final" + key].tobytes()


def test_f16_pair_distances(f16):
    mean, dist, idx = R.nearest_batched(torch.from_numpy(np.concatenate([f16["gt0"], f16["pred0"][0].astype(np.float64)])).cuda(),
                                        [[9000, 8500, 0, 9000]], return_distances=True)
    assert dist.cpu().numpy().tobytes() == f16["pair_dist"].tobytes()
    assert np.array_equal(idx.cpu().numpy().astype(np.float64), f16["pair_idx"])
    assert float(mean[0]) == float(f16["chamfer"][0, 0, 0])


@pytest.mark.parametrize("rotated", [False, True])
def test_f16_eval_chamfer_from_files(f16, tmp_path, rotated):
    preds, gts = _f16_predictions(f16)
    names = ["m0", "m1", "m2", "missing_gt", "missing_pkl"]
    for name, (pts, nums) in zip(names, preds):
        R.save_predictions(str(tmp_path / ("%s_pc.pkl" % name)), pts, num_points=nums)
    R.save_predictions(str(tmp_path / "missing_gt_pc.pkl"), f16["pred2"])
    gt_of = dict(zip(names, gts))
    out_dir = tmp_path / "exp"
    out_dir.mkdir()
    res = R.eval_chamfer(str(tmp_path), names, gt_of.get, reference_rotation=f16["rotation"] if rotated else None,
                         out_name="test", out_dir=str(out_dir))
    key = "_rot" if rotated else ""
    assert res["model_names"] == ["m0", "m1", "m2"]
    assert res["chamfer"].tobytes() == f16["chamfer" + key].tobytes()
    assert res["final"].tobytes() == f16["final" + key].tobytes()
    line = (out_dir / "chamfer_test.txt").read_text()
    assert line == "{} {}\n".format(f16["final" + key][0], f16["final" + key][1])


def test_independent_of_batching_and_reproducible():
    rng = np.random.default_rng(5)
    src, tgt = _cloud(rng, 3000, np.float64), _cloud(rng, 20000, np.float64)
    alone = R.nearest_batched(torch.from_numpy(np.concatenate([src, tgt])).cuda(), [[0, 3000, 3000, 20000]],
                              return_distances=True)
    # the same pair inside a 500-pair batch (one target slice per pair there)
    others = [_cloud(rng, int(n), np.float64) for n in rng.integers(200, 2000, 498)]
    clouds = [src, tgt] + others
    start = np.cumsum([0] + [len(c) for c in clouds])
    pairs = [[start[2 + k], len(others[k]), start[2 + (k + 1) % len(others)], len(others[(k + 1) % len(others)])]
             for k in range(len(others) // 2)]
    at = len(pairs)
    pairs.append([0, 3000, 3000, 20000])
    pairs += [[start[2 + k], len(others[k]), start[1], 20000] for k in range(len(others) // 2, len(others) - 1)]
    assert len(pairs) == 498
    pairs += [[start[1], 20000, 0, 3000], [0, 3000, 3000, 20000]]
    buf = torch.from_numpy(np.concatenate(clouds)).cuda()
    mean, dist, idx = R.nearest_batched(buf, pairs, return_distances=True)
    off = int(np.array(pairs)[:at, 1].sum())
    assert dist[off:off + 3000].cpu().numpy().tobytes() == alone[1].cpu().numpy().tobytes()
    assert torch.equal(idx[off:off + 3000], alone[2])
    assert mean[at].item() == alone[0][0].item() and mean[-1].item() == alone[0][0].item()
    again = R.nearest_batched(buf, pairs, return_distances=True)
    assert all(torch.equal(a, b) for a, b in zip((mean, dist, idx), again))


def test_models_per_call_does_not_change_the_result():
    rng = np.random.default_rng(9)
    preds, gts = [], []
    for m in range(15):
        pts = rng.random((3, 700, 3)).astype(np.float32) - 0.5
        nums = rng.integers(1, 701, 3)
        preds.append((pts, nums))
        gts.append(rng.random((int(rng.integers(300, 1500)), 3)) - 0.5)
    q = np.array([[0.3, -0.2, 0.9, 0.1]])
    ref = R.chamfer_of_split(preds, gts, reference_rotation=q, models_per_call=256)
    for k in (1, 7):
        assert R.chamfer_of_split(preds, gts, reference_rotation=q, models_per_call=k).tobytes() == ref.tobytes()
    assert R.chamfer_of_split(preds, gts, reference_rotation=q).tobytes() == ref.tobytes()


@pytest.mark.parametrize("case", ["plain_f32", "rotated_f64"])
def test_agrees_with_the_per_view_loop(case):
    rng = np.random.default_rng(11)
    dt = np.float32 if case == "plain_f32" else np.float64
    q = np.array([[0.9, 0.1, -0.3, 0.2]]) if case == "rotated_f64" else None
    preds, gts = [], []
    for m in range(4):
        preds.append((rng.random((3, 900, 3)).astype(dt) - 0.5, np.array([900, 400, 850])))
        gts.append(rng.random((1200, 3)) - 0.5)
    got = R.chamfer_of_split(preds, gts, reference_rotation=q)
    for m in range(4):
        old = R.chamfer_of_predictions(preds[m][0], gts[m], reference_rotation=q, num_points=preds[m][1])
        assert np.allclose(got[m], old, rtol=1e-13, atol=0), (m, got[m], old)


def test_refusals_come_before_any_launch():
    a = np.zeros((4, 3))
    bad = a.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match=r"preds\[1\]"):
        R.chamfer_batched([a, bad], [a, a])
    inf = a.copy()
    inf[0, 0] = np.inf
    with pytest.raises(ValueError, match=r"gts\[0\]"):
        R.chamfer_batched([a], [inf])
    with pytest.raises(ValueError):
        R.chamfer_batched([a], [np.zeros((0, 3))])
    with pytest.raises(ValueError):
        R.chamfer_batched([a, a], [a], gt_of=[0, 3])
    with pytest.raises(ValueError):
        R.chamfer_of_split([(np.zeros((2, 4, 3)), np.array([4, 9]))], [a])
    # an empty prediction against an empty GT is no error: NaN in both directions, as np.mean of nothing
    out = R.chamfer_batched([np.zeros((0, 3))], [np.zeros((0, 3))]).cpu().numpy()
    assert np.isnan(out).all()
