"""GPU tests of dpc_knn_batched, dpc_pca_normals and the normal-consistency metric against the fixture f30_normals.npz and
the numpy oracle (tests/normals_oracle.py).  The k-NN lists are exact (bit for bit, fp32 and fp64); the normals are held to
the fixture's measured tolerance: 8 x max_ratio units of 2^-52 trace / (l1 - l0) for the angle, 8 x max_eval_ratio units of
2^-52 trace for the eigenvalues (the factor pays for another formulation and fused arithmetic; neither figure comes from
the kernels)."""
import numpy as np
import pytest
import torch

import normals_oracle as O

pytestmark = pytest.mark.gpu
EPS = O.EPS


@pytest.fixture(scope="module")
def f30(golden):
    return golden("f30_normals.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _status(dev):
    """The status word of dev, read and cleared."""
    from dpc.render._ops import status_word

    word = status_word(dev)
    bits = int(word.item())
    word.zero_()
    return bits


@pytest.fixture(autouse=True)
def clean_status(dev):
    """Every test starts from a zero status word, and leaves one: the status is 0 after every clean case."""
    _status(dev)
    yield
    assert _status(dev) == 0


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_knn_is_exact_on_every_fixture_case(f30, dev, tag):
    """Query counts around each workgroup size, reference counts around k and the tile, every k of the list, padding,
    a ragged batch: idx and d2 equal the oracle's bit for bit."""
    import dpc.render as R

    dtype = np.float32 if tag == "f32" else np.float64
    pool = torch.from_numpy(f30["pool"].astype(dtype)).to(dev)
    for name in f30["knn_cases"]:
        k, rows = int(f30["knn_%s_k" % name]), f30["knn_%s_rows" % name]
        idx, d2 = R.knn_batched(pool, rows, k, return_distances=True)
        assert idx.dtype == torch.int32 and tuple(idx.shape) == (int(rows[:, 1].sum()), k) and _np(d2).dtype == dtype
        assert np.array_equal(_np(idx), f30["knn_%s_idx_%s" % (name, tag)]), name
        assert np.array_equal(_np(d2), f30["knn_%s_d2_%s" % (name, tag)]), name
        assert torch.equal(R.knn_batched(pool, rows, k), idx), name              # without the distances
    pad_i, pad_d = f30["knn_pad_k64_idx_" + tag], f30["knn_pad_k64_d2_" + tag]
    assert (pad_i[:, 40:] == -1).all() and np.isinf(pad_d[:, 40:]).all() and (pad_i[:, :40] >= 0).all()


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_knn_ties_go_to_the_lower_index(f30, dev, tag):
    import dpc.render as R

    lat = f30["lattice"].astype(np.float32 if tag == "f32" else np.float64)
    idx, d2 = R.knn_batched(lat, [(0, 125, 0, 125)], 7, return_distances=True)
    assert np.array_equal(_np(idx), f30["lattice_idx_" + tag]) and np.array_equal(_np(d2), f30["lattice_d2_" + tag])
    tie = _np(d2)[:, 1:] == _np(d2)[:, :-1]
    assert int(tie.sum()) == 527 and (_np(idx)[:, 1:][tie] > _np(idx)[:, :-1][tie]).all()


def test_knn_does_not_depend_on_row_order_or_batching(f30, dev):
    import dpc.render as R

    pool = torch.from_numpy(f30["pool"].astype(np.float32)).to(dev)
    rows = f30["knn_ragged_k16_rows"]
    idx, d2 = R.knn_batched(pool, rows, 16, return_distances=True)
    first = np.concatenate([[0], np.cumsum(rows[:, 1])])
    perm = [4, 2, 0, 3, 1]
    pi, pd = R.knn_batched(pool, rows[perm], 16, return_distances=True)
    at = 0
    for r in perm:
        n = int(rows[r, 1])
        assert torch.equal(pi[at:at + n], idx[first[r]:first[r + 1]]) and torch.equal(pd[at:at + n], d2[first[r]:first[r + 1]])
        at += n
    for r in range(len(rows)):
        oi, od = R.knn_batched(pool, rows[r:r + 1], 16, return_distances=True)
        assert torch.equal(oi, idx[first[r]:first[r + 1]]) and torch.equal(od, d2[first[r]:first[r + 1]])
    again = R.knn_batched(pool, rows, 16, return_distances=True)
    assert torch.equal(again[0], idx) and torch.equal(again[1], d2)


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_a_nan_reference_is_no_candidate_and_is_reported(f30, dev, tag):
    import dpc.render as R
    from dpc.render import _native, normals

    dtype = np.float32 if tag == "f32" else np.float64
    P = f30["pool"][:700].astype(dtype)
    P[600, 1] = np.nan                                         # in the second tile of the references [50, 700)
    rows = np.asarray([(0, 40, 50, 650)], dtype=np.int32)
    want_i, want_d, status = O.knn(P[:40], P[50:700], 8, dtype)
    assert status == O.STATUS_NONFINITE and not (want_i == 550).any()
    idx, d2, _ = normals._knn(torch.from_numpy(P).to(dev), rows, 8, dev, True)
    assert np.array_equal(_np(idx), want_i) and np.array_equal(_np(d2), want_d)
    assert _status(dev) == _native.DPC_STATUS_NONFINITE
    with pytest.raises(ValueError, match="points holds a NaN or inf"):
        R.knn_batched(torch.from_numpy(P).to(dev), rows, 8)
    with pytest.raises(ValueError, match=r"clouds\[1\] holds a NaN or inf"):
        R.estimate_normals([torch.from_numpy(P[:50]).to(dev), torch.from_numpy(P).to(dev)])
    with pytest.raises(ValueError, match=r"gts\[0\] holds a NaN or inf"):
        R.normal_consistency([torch.from_numpy(P[:50]).to(dev)], [torch.from_numpy(P).to(dev)])


def test_pca_on_a_plane_a_line_and_too_few_points(dev):
    import dpc.render as R
    from dpc.render import normals

    rng = np.random.default_rng(5)
    plane = np.concatenate([rng.integers(-512, 513, size=(40, 2)) / 1024.0, np.full((40, 1), 0.25)], axis=1)
    tol = 8 * EPS
    for cloud in (plane, plane.astype(np.float32)):
        for k in (3, 16):
            (n,), (w,) = R.estimate_normals([cloud], k=k, return_eigenvalues=True)
            n, w = _np(n), _np(w)
            idx = O.knn(cloud, cloud, k, cloud.dtype.type)[0]
            collinear = O.pca_normals(cloud, cloud, idx)[1][:, 1] <= tol      # three neighbours on one line: any normal
            assert (np.abs(n[~collinear, :2]) <= tol).all() and (n[~collinear, 2] == 1.0).all() and (~collinear).sum() >= 38
            assert (w[:, 0] <= tol * w.sum(axis=1)).all()
            up = _np(R.estimate_normals([cloud], k=k, viewpoints=[[0.1, 0.2, 3.0]])[0])
            down = _np(R.estimate_normals([cloud], k=k, viewpoints=[[0.1, 0.2, -3.0]])[0])
            assert (up[~collinear, 2] == 1.0).all() and (down[~collinear, 2] == -1.0).all()
            assert ((up * (np.array([0.1, 0.2, 3.0]) - cloud)).sum(axis=1) >= 0).all()
    # c = 1 and c = 2 valid slots: the zero normal, the eigenvalues still those of C
    for c in (1, 2):
        (n,), (w,) = R.estimate_normals([plane[:c]], k=5, return_eigenvalues=True)
        assert (_np(n) == 0).all() and np.allclose(_np(w), O.estimate_normals(plane[:c], 5)[1], rtol=0, atol=1e-15)
    # collinear points: a unit vector orthogonal to the line
    t = np.arange(12) / 8.0
    line = np.stack([0.5 + t, 0.25 - 2 * t, 3 * t], axis=1)
    (n,), (w,) = R.estimate_normals([line], k=6, return_eigenvalues=True)
    n, w = _np(n), _np(w)
    along = np.array([1.0, -2.0, 3.0]) / np.sqrt(14.0)
    assert (np.abs(np.linalg.norm(n, axis=1) - 1) <= 4 * EPS).all() and (np.abs(n @ along) <= 64 * EPS).all()
    assert (w[:, 1] <= 64 * EPS * w[:, 2]).all()
    # an index outside [-1, r_count) is no address: reported, and counted as an invalid slot
    pts = torch.from_numpy(plane).to(dev)
    rows = np.asarray([(0, 40, 0, 40)], dtype=np.int32)
    idx, _, rows_d = normals._knn(pts, rows, 4, dev, False)
    idx[3, 1], idx[5, 2] = 40, -7
    got, _ = normals._pca(pts, rows, rows_d, 4, idx, None, dev, False)
    from dpc.render import _native

    assert _status(dev) == _native.DPC_STATUS_BAD_INDEX
    want = O.pca_normals(plane, plane, _np(idx))[0]
    assert np.abs(_np(got) - want).max() <= tol and np.isfinite(_np(got)).all()


def test_pca_meets_the_accuracy_rule_on_sphere_box_and_torus(f30, dev):
    import dpc.render as R

    angle, evals = 8 * float(f30["max_ratio"]), 8 * float(f30["max_eval_ratio"])
    for name in f30["pca_cases"]:
        cloud = f30["pca_%s_cloud" % name.split("_")[0]]
        k = int(name.split("_k")[1])
        (n,), (w,) = R.estimate_normals([cloud], k=k, return_eigenvalues=True)
        n, w = _np(n), _np(w)
        en, ew, wide = f30["pca_%s_exact_normals" % name], f30["pca_%s_exact_evals" % name], f30["pca_%s_wide" % name]
        u, _ = O.unit(ew)
        tr = ew.sum(axis=1)
        ratio = (O.sin_angle(n, en)[wide] / u[wide]).max()
        eratio = (np.abs(w - ew) / (EPS * tr[:, None])).max()
        print("%s: angle %.2f of %.2f units, eigenvalues %.2f of %.2f units" % (name, ratio, angle, eratio, evals))
        assert (~wide).mean() <= 0.01 and ratio <= angle and eratio <= evals, name
        assert (np.abs(np.linalg.norm(n, axis=1) - 1.0) <= 4 * EPS).all(), name
        C = O.covariance(cloud, f30["pca_%s_idx" % name])[0]
        assert (np.einsum("qi,qij,qj->q", n, C, n) <= ew[:, 0] + angle * EPS * tr).all(), name
        assert (n[np.arange(len(n)), np.argmax(np.abs(n), axis=1)] > 0).all() and (w[:, :-1] <= w[:, 1:]).all(), name
    # fp32 input widens exactly: the same rule against the oracle's eigh on the widened cloud
    c32 = f30["pca_torus_cloud"].astype(np.float32)
    (n,), (w,) = R.estimate_normals([c32], k=16, return_eigenvalues=True)
    on, ow = O.estimate_normals(c32, 16)
    u, gap = O.unit(ow)
    ok = gap >= O.MIN_GAP
    assert ok.mean() >= 0.99 and (O.sin_angle(_np(n), on)[ok] <= (angle + float(f30["max_ratio"])) * u[ok]).all()
    assert (np.abs(_np(w) - ow) <= (evals + float(f30["max_eval_ratio"])) * EPS * ow.sum(axis=1, keepdims=True)).all()


def test_estimate_normals_on_a_list_equals_one_call_per_cloud(f30, dev):
    import dpc.render as R

    clouds = [f30["pca_sphere_cloud"], f30["pca_box_cloud"].astype(np.float32), f30["pca_torus_cloud"][:100],
              f30["pca_torus_cloud"][:2].astype(np.float32), f30["pool"][:300].astype(np.float32)]
    vps = np.asarray([[0, 0, 2.0], [2.0, 0, 0], [0, 2.0, 0], [1, 1, 1], [-1, 0.5, 2]])
    for kw in ({}, {"viewpoints": vps}):
        n, w = R.estimate_normals(clouds, k=16, return_eigenvalues=True, **kw)
        for i, c in enumerate(clouds):
            one = {k: v[i:i + 1] for k, v in kw.items()}
            (n1,), (w1,) = R.estimate_normals([c], k=16, return_eigenvalues=True, **one)
            assert n[i].dtype == torch.float64 and tuple(n[i].shape) == (len(c), 3)
            assert torch.equal(n[i], n1) and torch.equal(w[i], w1), i
    n = R.estimate_normals(clouds, k=16, viewpoints=vps)
    for i, c in enumerate(clouds[:3]):
        assert ((_np(n[i]) * (vps[i] - c.astype(np.float64))).sum(axis=1) >= 0).all()


@pytest.fixture(scope="module")
def pairs(f30):
    """Two predictions (fp32, one a jittered copy of the sphere, one of the torus) with their GT clouds (fp64) and the
    oracle's normals and consistency."""
    rng = np.random.default_rng(11)
    gts = [f30["pca_sphere_cloud"], f30["pca_torus_cloud"]]
    preds = [(g[rng.permutation(len(g))[:180]] + 0.003 * rng.normal(size=(180, 3))).astype(np.float32) for g in gts]
    n_gt = [O.estimate_normals(g, 16)[0] for g in gts]
    n_pred = [O.estimate_normals(p, 16)[0] for p in preds]
    want = np.stack([O.normal_consistency(p, g, a, b) for p, g, a, b in zip(preds, gts, n_pred, n_gt)])
    return preds, gts, n_pred, n_gt, want


def _tolerances(pred, gt, k, f30):
    """What (a, b) may differ by when both sides' normals are estimated: a normal within the angle t of the oracle's moves
    a |dot| by at most sin t <= min(t, 1), so a pair's mean moves by the mean over its points of the tolerances of the
    point's own normal and of its neighbour's -- the kernel's 8 x max_ratio units plus the oracle's own max_ratio."""
    def per_point(cloud):
        u, _ = O.unit(O.estimate_normals(cloud, k)[1])
        return np.minimum(9 * float(f30["max_ratio"]) * u, 1.0)

    tp, tg = per_point(pred), per_point(gt)
    ta = float(np.mean(tp + tg[O.nearest(pred, gt, np.float64)]))
    tb = float(np.mean(tg + tp[O.nearest(gt, pred, np.float64)]))
    return np.array([ta, tb, (ta + tb) / 2.0]) + 4 * EPS


def test_normal_consistency_against_the_oracle(f30, dev, pairs):
    import dpc.render as R

    preds, gts, n_pred, n_gt, want = pairs
    got = _np(R.normal_consistency(preds, gts, pred_normals=n_pred, gt_normals=n_gt))
    print("supplied normals: max difference %.3g" % np.abs(got - want).max())
    assert got.shape == (2, 3) and np.abs(got - want).max() <= 4 * EPS
    est = _np(R.normal_consistency(preds, gts, k=16))
    for i in range(2):
        tol = _tolerances(preds[i], gts[i], 16, f30)
        print("estimated normals, pair %d: differences %s of %s" % (i, np.abs(est[i] - want[i]), tol))
        assert (np.abs(est[i] - want[i]) <= tol).all()
    # views share one GT copy; grouping does not change a bit
    both = R.normal_consistency([preds[0], preds[1], preds[0]], gts, gt_of=[0, 1, 0], k=16)
    assert np.array_equal(_np(both), est[[0, 1, 0]])


def test_normal_consistency_closed_forms(f30, dev, pairs):
    import dpc.render as R

    preds, gts, n_pred, n_gt, _ = pairs
    g = gts[0]
    n = _np(R.estimate_normals([g], k=16)[0])
    same = _np(R.normal_consistency([g], [g], pred_normals=[n], gt_normals=[n]))
    assert np.abs(same - 1.0).max() <= 4 * EPS
    assert np.abs(_np(R.normal_consistency([g], [g], k=16)) - 1.0).max() <= 4 * EPS
    ez, ex = np.tile([0.0, 0.0, 1.0], (len(g), 1)), np.tile([1.0, 0.0, 0.0], (180, 1))
    assert (_np(R.normal_consistency([preds[0]], [g], pred_normals=[ex], gt_normals=[ez])) == 0).all()
    zero = np.zeros((180, 3))
    assert (_np(R.normal_consistency([preds[0]], [g], pred_normals=[zero], gt_normals=[ez])) == 0).all()
    out = _np(R.normal_consistency([preds[0][:0], preds[0]], [g], gt_of=[0, 0], k=16))
    assert np.isnan(out[0]).all() and np.isfinite(out[1]).all()


def test_normal_consistency_of_split(f30, dev, pairs):
    import dpc.render as R
    from dpc.render._split import _host_unit_quaternion, _rotate

    preds, gts, _, _, _ = pairs
    rng = np.random.default_rng(3)
    models = [(np.stack([p, p[rng.permutation(180)], (p + 0.01).astype(np.float32)]), None) for p in preds]
    models.append((models[0][0][:, ::-1].copy(), None))
    gt3 = gts + [gts[0]]
    res = {step: R.normal_consistency_of_split(models, gt3, k=8, models_per_call=step) for step in (1, 2, 3)}
    assert res[1].shape == (3, 3, 3) and res[1].dtype == np.float64 and np.isfinite(res[1]).all()
    assert res[1].tobytes() == res[2].tobytes() == res[3].tobytes()
    direct = _np(R.normal_consistency([v for m, _ in models for v in m], gt3, gt_of=[0] * 3 + [1] * 3 + [2] * 3, k=8))
    assert np.array_equal(direct.reshape(3, 3, 3), res[3])
    # a per-view num_points truncates the view
    nums = np.array([180, 90, 180])
    cut = R.normal_consistency_of_split([(models[0][0], nums)], gts[:1], k=8)
    assert np.array_equal(cut[0, 0], res[1][0, 0]) and not np.array_equal(cut[0, 1], res[1][0, 1])
    assert np.array_equal(cut[0, 1], _np(R.normal_consistency([models[0][0][1, :90]], gts[:1], k=8))[0])
    # reference_rotation: the views rotated and prepared by hand
    q = np.array([[0.9, 0.1, -0.3, 0.2]])
    rot = R.normal_consistency_of_split(models[:2], gts, k=8, reference_rotation=q)
    qn = _host_unit_quaternion(q)
    by_hand = [v for m, _ in models[:2] for v in _rotate(torch.from_numpy(m), qn, dev)]
    assert by_hand[0].dtype == torch.float64
    assert np.array_equal(rot.reshape(6, 3), _np(R.normal_consistency(by_hand, gts, gt_of=[0] * 3 + [1] * 3, k=8)))
    assert not np.array_equal(rot, res[1][:2])
    # supplied GT normals are used as they are
    ez = [np.tile([0.0, 0.0, 1.0], (len(g), 1)) for g in gts]
    given = R.normal_consistency_of_split(models[:2], gts, gt_normals=ez, k=8)
    assert not np.array_equal(given, res[1][:2]) and np.isfinite(given).all()
