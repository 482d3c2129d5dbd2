"""Host-side checks of the k-NN search, the PCA normals and the normal-consistency metric (no GPU): the numpy oracle
(tests/normals_oracle.py) against the fixture f30_normals.npz, the oracle's k-NN against a brute-force loop, every refusal
of the four Python functions and of the two entry points before a device is needed, and the exported symbols and
constants."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import normals_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def f30(golden):
    return golden("f30_normals.npz")


class _DeviceLookedFor(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """Valid arguments get as far as looking for a device, and no further, whatever this machine has."""
    from dpc.render import _batch

    def device(*a, **k):
        raise _DeviceLookedFor()

    monkeypatch.setattr(_batch, "device", device)


def test_oracle_knn_meets_the_fixture(f30):
    for name in f30["knn_cases"]:
        k, rows = int(f30["knn_%s_k" % name]), f30["knn_%s_rows" % name]
        for dtype, tag in ((np.float32, "f32"), (np.float64, "f64")):
            P = f30["pool"].astype(dtype)
            idx = np.concatenate([O.knn(P[a:a + n], P[b:b + m], k, dtype)[0] for a, n, b, m in rows])
            d2 = np.concatenate([O.knn(P[a:a + n], P[b:b + m], k, dtype)[1] for a, n, b, m in rows])
            assert idx.dtype == np.int32 and d2.dtype == dtype
            assert np.array_equal(idx, f30["knn_%s_idx_%s" % (name, tag)]), (name, tag)
            assert np.array_equal(d2, f30["knn_%s_d2_%s" % (name, tag)]), (name, tag)


def test_fixture_was_placed_from_the_library_constants(f30):
    from dpc.render import _native

    T = _native.DPC_KNN_TILE
    assert int(f30["tile"]) == T and f30["k_values"].tolist() == [1, 2, 8, 16, 30, 64]
    assert {_native.knn_block(k) for k in range(1, _native.DPC_KNN_MAX_K + 1)} == {256, 128, 64}
    for B in (256, 128, 64):
        k = int(f30["knn_queries_b%d_k" % B])
        assert _native.knn_block(k) == B and f30["knn_queries_b%d_rows" % B][:, 1].tolist() == [1, B - 1, B, B + 1]
    k = int(f30["knn_refs_k8_k"])
    assert f30["knn_refs_k8_rows"][:, 3].tolist() == [1, k - 1, k, k + 1, T - 1, T, T + 1, 2 * T + 1]
    assert {int(f30["knn_self_k%d_k" % k]) for k in (1, 2, 8, 16, 30, 64)} == {1, 2, 8, 16, 30, 64}
    rows = f30["knn_ragged_k16_rows"]
    assert (rows[:, 1] == 0).any() and (rows[2, 2:] == rows[3, 2:]).all() and (rows[4, :2] != rows[4, 2:]).any()


def test_oracle_knn_against_a_brute_force_loop(f30):
    P = f30["pool"]
    for dtype in (np.float32, np.float64):
        for k, (a, n, b, m) in ((3, (0, 9, 40, 11)), (5, (7, 4, 7, 4)), (1, (0, 3, 0, 3))):
            idx, d2, status = O.knn(P[a:a + n], P[b:b + m], k, dtype)
            bi, bd = O.knn_brute(P[a:a + n], P[b:b + m], k, dtype)
            assert status == 0 and np.array_equal(idx, bi) and np.array_equal(d2, bd)
    lat = f30["lattice"].astype(np.float32)
    bi, bd = O.knn_brute(lat[:30], lat, 7)
    assert np.array_equal(bi, f30["lattice_idx_f32"][:30]) and np.array_equal(bd, f30["lattice_d2_f32"][:30])
    # padding, and a NaN reference among finite ones: the others are ranked as without it
    idx, d2, _ = O.knn(P[:2], P[10:13], 5)
    assert (idx[:, 3:] == -1).all() and np.isinf(d2[:, 3:]).all() and (idx[:, :3] >= 0).all()
    refs = P[10:20].copy()
    clean = O.knn(P[:4], np.delete(refs, 3, axis=0), 4)[0]
    refs[3, 1] = np.nan
    idx, _, status = O.knn(P[:4], refs, 4)
    assert status == O.STATUS_NONFINITE and np.array_equal(idx, clean + (clean >= 3))


def test_lattice_ties_go_to_the_lower_index(f30):
    idx, d2 = f30["lattice_idx_f32"], f30["lattice_d2_f32"]
    tie = d2[:, 1:] == d2[:, :-1]
    assert int(tie.sum()) == int(f30["lattice_ties"]) == 527
    assert (idx[:, 1:][tie] > idx[:, :-1][tie]).all() and (idx[:, 0] == np.arange(125)).all()
    # at the k-th place: every reference left out that ties with the last slot has a higher index than it
    full = O.d2_matrix(f30["lattice"], f30["lattice"], np.float32)
    for q in range(125):
        out = np.setdiff1d(np.arange(125), idx[q])
        same = out[full[q, out] == d2[q, -1]]
        assert (same > idx[q, -1]).all() and (full[q, out] >= d2[q, -1]).all()


def test_oracle_pca_meets_the_fixture_within_the_recorded_ratios(f30):
    assert 0 < float(f30["max_ratio"]) <= 16.0 and float(f30["max_eval_ratio"]) >= 1.0
    for name in f30["pca_cases"]:
        cloud = f30["pca_%s_cloud" % name.split("_")[0]]
        k = int(name.split("_k")[1])
        idx = O.knn(cloud, cloud, k, np.float64)[0]
        assert np.array_equal(idx, f30["pca_%s_idx" % name])
        n, w, status = O.pca_normals(cloud, cloud, idx)
        en, ew, wide = f30["pca_%s_exact_normals" % name], f30["pca_%s_exact_evals" % name], f30["pca_%s_wide" % name]
        u, gap = O.unit(ew)
        assert status == 0 and np.array_equal(wide, gap >= float(f30["min_gap"])) and (~wide).mean() <= 0.01
        assert (O.sin_angle(n, en)[wide] <= float(f30["max_ratio"]) * u[wide]).all(), name
        assert (np.abs(w - ew) <= float(f30["max_eval_ratio"]) * O.EPS * ew.sum(axis=1, keepdims=True)).all(), name
        assert (np.abs(np.linalg.norm(n, axis=1) - 1.0) <= 4 * O.EPS).all()
        big = np.abs(n).max(axis=1)
        assert (n[np.arange(len(n)), np.argmax(np.abs(n), axis=1)] == big).all()       # the canonical sign


def test_oracle_pca_rules_on_closed_forms():
    plane = np.array([[0, 0, 0.25], [1, 0, 0.25], [0, 1, 0.25], [1, 1, 0.25], [0.5, 0.25, 0.25]])
    idx = np.tile(np.arange(5, dtype=np.int32), (5, 1))
    n, w, _ = O.pca_normals(plane, plane, idx)
    assert np.array_equal(n, np.tile([0.0, 0.0, 1.0], (5, 1))) and (w[:, 0] == 0).all()
    up = O.pca_normals(plane, plane, idx, viewpoint=[0.3, 0.3, 5.0])[0]
    down = O.pca_normals(plane, plane, idx, viewpoint=[0.3, 0.3, -5.0])[0]
    assert (up[:, 2] == 1).all() and (down[:, 2] == -1).all()
    few = np.array([[0, 1, -1, -1, -1]], dtype=np.int32)
    n, w, status = O.pca_normals(plane[:1], plane, few)
    assert status == 0 and (n == 0).all() and np.allclose(w, [[0, 0, 0.25]])
    n, w, status = O.pca_normals(plane[:1], plane, np.array([[0, 1, 2, 7, -1]], dtype=np.int32))
    assert status == O.STATUS_BAD_INDEX and abs(n[0, 2]) == 1.0
    assert np.array_equal(O.orient(np.array([[-0.6, 0.6, 0.5], [0.0, -1.0, 0.0]])), [[0.6, -0.6, -0.5], [0.0, 1.0, 0.0]])


def test_oracle_consistency_rules(f30):
    cloud = f30["pca_sphere_cloud"]
    n, _ = O.estimate_normals(cloud, 16)
    assert np.abs(O.normal_consistency(cloud, cloud, n, n) - 1.0).max() <= 4 * O.EPS
    ortho = np.cross(n, np.roll(n, 1, axis=1))
    assert np.abs(O.normal_consistency(cloud, cloud, ortho, n)).max() <= 4 * O.EPS
    assert np.isnan(O.normal_consistency(np.zeros((0, 3)), cloud, np.zeros((0, 3)), n)).all()
    radial = cloud / np.linalg.norm(cloud, axis=1, keepdims=True)
    assert O.normal_consistency(cloud.astype(np.float32), cloud, radial, n)[2] > 0.95


def test_header_symbols_constants_and_abi():
    from dpc.render import _native, normals

    header = open(os.path.join(ROOT, "include", "dpc_render.h")).read()
    assert int(re.search(r"#define DPC_ABI_VERSION (\d+)", header).group(1)) == 15 == _native.lib().dpc_abi_version()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("dpc_knn_batched", "dpc_pca_normals"):
        assert name in _native.SYMBOLS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, header), name
    for name in ("DPC_KNN_MAX_K", "DPC_KNN_TILE"):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == getattr(_native, name), name
    assert (normals.MAX_K, normals.TILE) == (64, _native.DPC_KNN_TILE)
    m = re.search(r"#define DPC_KNN_BLOCK\(k\) \(\(k\) <= (\d+) \? (\d+) : \(k\) <= (\d+) \? (\d+) : (\d+)\)", header)
    a, ba, b, bb, bc = (int(x) for x in m.groups())
    assert all(_native.knn_block(k) == (ba if k <= a else bb if k <= b else bc) for k in range(1, 65))
    # the lists of a workgroup and the staged tile fit 64 KiB of LDS at every k, with two workgroups per CU at k <= 16
    for k in range(1, 65):
        lds = _native.knn_block(k) * k * 12 + 3 * _native.DPC_KNN_TILE * 8
        assert lds <= 64 * 1024 and (k > 16 or 2 * lds <= 160 * 1024)
    import dpc.render as R

    for name in ("knn_batched", "estimate_normals", "normal_consistency", "normal_consistency_of_split"):
        assert name in R.__all__ and callable(getattr(R, name)), name


def _table(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 4))


def test_entry_points_check_before_they_touch_a_device():
    from dpc.render import _native

    L = _native.lib()
    knn = lambda n, d, k, rows=None: L.dpc_knn_batched(None, n, 0, None, d.ctypes.data, len(d) if rows is None else rows, k, None,
                                                       None, None, None)
    pca = lambda n, d, k: L.dpc_pca_normals(None, n, 1, None, d.ctypes.data, len(d), k, None, None, None, None, None, None)
    good = _table([(0, 5, 5, 4), (2, 0, 0, 9), (0, 9, 0, 9)])
    for call in (knn, pca):
        assert call(9, good, 3) == _native.DPC_ERR_NULL and call(9, good, 64) == _native.DPC_ERR_NULL
        assert call(9, good, 0) == call(9, good, 65) == call(9, good, -1) == _native.DPC_ERR_SHAPE
        assert call(8, good, 3) == _native.DPC_ERR_SHAPE                                    # a range outside [0, n_pts)
        assert call(-1, good, 3) == _native.DPC_ERR_SHAPE
        for bad in ((-1, 2, 0, 3), (0, -2, 0, 3), (0, 2, -1, 3), (0, 2, 0, -3), (8, 2, 0, 3), (0, 2, 7, 3)):
            assert call(9, _table([good[0], bad]), 3) == _native.DPC_ERR_SHAPE, bad
        assert call(9, _table([(0, 0, 0, 9)]), 3) == 0                                     # no queries: nothing to do
        # 2^31 - 1 output slots are the most: 33554432 queries x 64 slots pass the limit, x 63 do not
        big = _table([(0, 1 << 25, 0, 1 << 25)])
        assert call(1 << 25, big, 64) == _native.DPC_ERR_SHAPE and call(1 << 25, big, 63) == _native.DPC_ERR_NULL
    assert knn(9, good, 3, rows=0) == 0 and knn(9, good, 3, rows=-1) == _native.DPC_ERR_SHAPE
    assert L.dpc_knn_batched(None, 9, 0, None, None, 3, 3, None, None, None, None) == _native.DPC_ERR_NULL


def test_every_refusal_comes_before_a_device_is_looked_for(no_device):
    import dpc.render as R

    rng = np.random.default_rng(0)
    A, B = rng.random((20, 3)).astype(np.float32), rng.random((30, 3))
    nan = A.copy()
    nan[4, 1] = np.nan
    inf = B.copy()
    inf[0, 0] = np.inf
    rows = [(0, 20, 0, 20)]

    def refused(fn, *a, match, **k):
        with pytest.raises(ValueError, match=match):
            fn(*a, **k)

    # knn_batched
    for k in (0, 65, -3, 2.0, True, None):
        refused(R.knn_batched, A, rows, k, match="k must be an integer")
    refused(R.knn_batched, A[:, :2], rows, 3, match=r"points must be \[n,3\]")
    refused(R.knn_batched, A, [(0, 20, 0)], 3, match=r"\[R,4\]")
    refused(R.knn_batched, A, np.zeros((1, 4)), 3, match=r"integer \[R,4\]")
    refused(R.knn_batched, A, [(0, 21, 0, 20)], 3, match="invalid row table")
    refused(R.knn_batched, A, [(0, 20, -1, 20)], 3, match="invalid row table")
    refused(R.knn_batched, A, [(0, 1 << 40, 0, 20)], 3, match="fit int32")
    refused(R.knn_batched, nan, rows, 3, match="points holds a NaN or inf")
    with pytest.raises(_DeviceLookedFor):
        R.knn_batched(A, rows, 3)
    with pytest.raises(_DeviceLookedFor):
        R.knn_batched(torch.from_numpy(B), np.asarray(rows), 64, return_distances=True)
    # estimate_normals
    refused(R.estimate_normals, [A, B], k=0, match="k must be an integer")
    refused(R.estimate_normals, [A, B.T], match=r"clouds\[1\] must be \[n,3\]")
    refused(R.estimate_normals, [A, B], viewpoints=[[0, 0, 1]], match=r"viewpoints must be \[2,3\]")
    refused(R.estimate_normals, [A, B], viewpoints=[[0, 0, 1], [0, np.nan, 1]], match="viewpoints")
    refused(R.estimate_normals, [A, B], viewpoints="up", match="viewpoints")
    refused(R.estimate_normals, [A, inf], match=r"clouds\[1\] holds a NaN or inf")
    with pytest.raises(_DeviceLookedFor):
        R.estimate_normals([A, B], k=30, viewpoints=[[0, 0, 1], [1, 0, 0]], return_eigenvalues=True)
    # normal_consistency
    refused(R.normal_consistency, [A], [B], k=65, match="k must be an integer")
    refused(R.normal_consistency, [A, A], [B], match="need gt_of")
    refused(R.normal_consistency, [A, A], [B], gt_of=[0, 1], match="gt_of must map")
    refused(R.normal_consistency, [A, A], [B], gt_of=[0], match="gt_of must map")
    refused(R.normal_consistency, [A], [B[:0]], match="GT cloud 0 is empty")
    refused(R.normal_consistency, [A[:, :1]], [B], match=r"preds\[0\] must be \[n,3\]")
    refused(R.normal_consistency, [A], [B], pred_normals=[A, A], match="2 pred_normals for 1 preds")
    refused(R.normal_consistency, [A], [B], pred_normals=[A[:19]], match="19 normals for the 20 points")
    refused(R.normal_consistency, [A], [B], gt_normals=[B[:, :2]], match=r"gt_normals\[0\] must be \[n,3\]")
    refused(R.normal_consistency, [A], [B], gt_normals=[B[:5]], match="5 normals for the 30 points")
    refused(R.normal_consistency, [nan], [B], match=r"preds\[0\] holds a NaN or inf")
    refused(R.normal_consistency, [A, A], [B, inf], gt_of=[1, 1], match=r"gts\[1\] holds a NaN or inf")
    refused(R.normal_consistency, [nan], [B], pred_normals=[A], gt_normals=[B], match=r"preds\[0\] holds a NaN or inf")
    with pytest.raises(_DeviceLookedFor):
        R.normal_consistency([A, A[:0]], [B], gt_of=[0, 0], pred_normals=[A, A[:0]])
    # normal_consistency_of_split
    preds = [(np.stack([A, A]), np.array([20, 7]))]
    refused(R.normal_consistency_of_split, preds, [B, B], match="1 predictions and 2 GT clouds")
    refused(R.normal_consistency_of_split, preds, [B], models_per_call=0, match="models_per_call")
    refused(R.normal_consistency_of_split, preds, [B], k=0, match="k must be an integer")
    refused(R.normal_consistency_of_split, [(A, None)], [B], match=r"\[V,N,3\]")
    refused(R.normal_consistency_of_split, [(np.stack([A, A]), np.array([20, 21]))], [B], match="num_points")
    refused(R.normal_consistency_of_split, preds + [(A[None], None)], [B, B], match="same number of views")
    refused(R.normal_consistency_of_split, preds, [B[:0]], match="GT cloud 0 is empty")
    refused(R.normal_consistency_of_split, preds, [B], gt_normals=[B[:3]], match="3 normals for the 30 points")
    refused(R.normal_consistency_of_split, preds, [B], reference_rotation=np.ones((2, 4)), match="quaternion")
    refused(R.normal_consistency_of_split, [(np.stack([nan, A]), None)], [B], match=r"predictions\[0\] holds a NaN or inf")
    refused(R.normal_consistency_of_split, preds, [inf], match=r"gt_clouds\[0\] holds a NaN or inf")
    with pytest.raises(_DeviceLookedFor):
        R.normal_consistency_of_split(preds, [B], gt_normals=[B], reference_rotation=np.array([[1.0, 0.0, 0.0, 0.0]]))
    assert R.normal_consistency_of_split([], []).shape == (0, 0, 3)
