"""CPU side of the batched Chamfer evaluation (no GPU): the float64 summation order the kernels reproduce, the F16 fixture
(tests/golden/make_golden_chamfer.py, from the reference's own code) restated with a numpy brute force, and the argument
checks of dpc_nearest_batched's C ABI, which return before anything touches a device.

np_sum restates np.add.reduce on a contiguous float64 array as the installed numpy does it: buffers of 8192 elements from
the start, each summed with pairwise_sum, the buffer sums added left to right onto 0.0.  k_chamfer_chunks / k_chamfer_mean
(csrc/dpc_chamfer.hip) implement exactly this; if numpy ever changes its order, test_np_sum_is_numpys_order fails first."""
import ctypes

import numpy as np
import pytest
import torch

BUF = 8192


def pairwise_sum(a):
    n = len(a)
    if n < 8:
        r = 0.0
        for x in a:
            r += x
        return r
    if n <= 128:
        r = [a[j] for j in range(8)]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] += a[i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for k in range(i, n):
            res += a[k]
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise_sum(a[:n2]) + pairwise_sum(a[n2:])


def np_sum(a):
    a = np.asarray(a, dtype=np.float64)
    s = 0.0
    for b in range(0, len(a), BUF):
        s += pairwise_sum(a[b:b + BUF].tolist())
    return np.float64(s)


def np_mean(a):
    return np.float64(np_sum(a) / np.float64(len(a))) if len(a) else np.float64(np.nan)


def _values(rng, n):
    """Positive and negative values across many magnitudes, so any change of order shows in the last bits."""
    return rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)


@pytest.mark.parametrize("n", list(range(1, 301)) + [1000, 8000, 8001, 8191, 8192, 8193, 16384, 20000, 65536, 100000])
def test_np_sum_is_numpys_order(n):
    rng = np.random.default_rng(n)
    for a in (_values(rng, n), rng.random(n), rng.random(n).astype(np.float32).astype(np.float64)):
        ref_sum, ref_mean = np.add.reduce(a), np.mean(a)
        got = np_sum(a)
        assert got.tobytes() == np.float64(ref_sum).tobytes(), (n, got, ref_sum)
        assert np_mean(a).tobytes() == np.float64(ref_mean).tobytes(), (n, np_mean(a), ref_mean)


def nearest_np(src, tgt, chunk=256):
    """point_cloud_distance's arithmetic in numpy: d = t - s, (d0*d0 + d1*d1) + d2*d2, sqrt, first minimum of the sqrt."""
    dt = np.result_type(src.dtype, tgt.dtype)
    s, t = src.astype(dt), tgt.astype(dt)
    dist = np.empty(len(s), dtype=dt)
    idx = np.empty(len(s), dtype=np.int64)
    for a in range(0, len(s), chunk):
        d = t[None, :, :] - s[a:a + chunk, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        dd = np.sqrt(d2)
        j = np.argmin(dd, axis=1)
        idx[a:a + chunk] = j
        dist[a:a + chunk] = dd[np.arange(len(j)), j]
    return dist, idx


@pytest.fixture(scope="module")
def f16(golden):
    return golden("f16_chamfer_split.npz")


def f16_models(f16):
    return [(f16["pred0"], f16["nums0"], f16["gt0"]), (f16["pred1"], None, f16["gt1"]), (f16["pred2"], None, f16["gt2"])]


def restate(models, rotate=None):
    """chamfer [M,V,2] from nearest_np and np_mean; rotate(points [V,N,3]) -> rotated numpy points."""
    out = []
    for pts, nums, gt in models:
        if rotate is not None:
            pts = rotate(pts)
        rows = []
        for i in range(pts.shape[0]):
            pred = pts[i] if nums is None else pts[i, :nums[i]]
            rows.append([np_mean(nearest_np(pred, gt)[0]), np_mean(nearest_np(gt, pred)[0])])
        out.append(rows)
    return np.array(out, dtype=np.float64)


def test_f16_pair_distances_restated(f16):
    dist, idx = nearest_np(f16["pred0"][0], f16["gt0"])
    assert dist.astype(np.float64).tobytes() == f16["pair_dist"].tobytes()
    assert np.array_equal(idx.astype(np.float64), f16["pair_idx"])


def test_f16_chamfer_restated_bit_for_bit(f16):
    chamfer = restate(f16_models(f16))
    assert chamfer.tobytes() == f16["chamfer"].tobytes()
    assert (np.mean(chamfer, axis=(0, 1)) * 100).tobytes() == f16["final"].tobytes()


def test_f16_rotation_path_restated_bit_for_bit(f16):
    """chamfer_of_split's rotation (host q / |q|, then the reference's quaternion products) evaluated in CPU torch gives the
    reference's rotated clouds; with them the restated means are F16's."""
    from dpc.render._split import _host_unit_quaternion, _rotate

    qn = _host_unit_quaternion(f16["rotation"])
    rotate = lambda p: _rotate(torch.from_numpy(p), qn, torch.device("cpu")).numpy()
    assert rotate(f16["pred0"]).dtype == np.float64
    chamfer = restate(f16_models(f16), rotate)
    assert chamfer.tobytes() == f16["chamfer_rot"].tobytes()
    assert (np.mean(chamfer, axis=(0, 1)) * 100).tobytes() == f16["final_rot"].tobytes()


def _c(a, dtype=np.int32):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_chamfer_workspace_bytes():
    from dpc.render import _native

    L = _native.lib()
    d, pd = _c([[0, 300, 300, 20000], [300, 20000, 0, 300], [0, 0, 300, 5]])
    n64, n32 = L.dpc_chamfer_workspace_bytes(3, pd, 1), L.dpc_chamfer_workspace_bytes(3, pd, 0)
    # at least the distances of every output point, one partial (distance, index) per point, and the prefixes
    assert n64 >= 20300 * (8 + 8 + 4) + 4 * 4 * 4
    assert n32 < n64 and n32 % 16 == 0 and n64 % 16 == 0
    assert L.dpc_chamfer_workspace_bytes(0, pd, 1) == 0
    assert L.dpc_chamfer_workspace_bytes(3, None, 1) == 0
    for bad in ([[0, -1, 0, 5]], [[-1, 1, 0, 5]], [[0, 1, -2, 5]], [[0, 1, 0, -5]], [[0, 4, 0, 0]],
                [[0, 2 ** 31 - 1, 0, 1], [0, 1, 0, 1]]):
            b, pb = _c(bad)
            assert L.dpc_chamfer_workspace_bytes(len(bad), pb, 1) == 0, bad


@pytest.mark.parametrize("case", ["ok", "empty_source", "pairs_neg", "n_pts_neg", "neg_count", "neg_start", "neg_tgt_start",
                                  "neg_tgt_count", "src_range", "tgt_range", "empty_target", "too_many_points"])
def test_nearest_batched_argument_checks_come_before_any_launch(case):
    """With NULL device pointers a valid call gets as far as DPC_ERR_NULL: every DPC_ERR_SHAPE below is returned before
    the library looks at a device pointer or launches anything."""
    from dpc.render import _native

    L = _native.lib()
    desc = [[0, 10, 10, 5], [10, 5, 0, 10], [3, 0, 0, 0]]
    n_pts, pairs = 15, 3
    if case == "empty_source":
        desc[0][1] = 0
    elif case == "pairs_neg":
        pairs = -1
    elif case == "n_pts_neg":
        n_pts = -1
    elif case == "neg_count":
        desc[1][1] = -1
    elif case == "neg_start":
        desc[1][0] = -5
    elif case == "neg_tgt_start":
        desc[0][2] = -1
    elif case == "neg_tgt_count":
        desc[0][3] = -1
    elif case == "src_range":
        n_pts = 14
    elif case == "tgt_range":
        desc[0][2] = 11
    elif case == "empty_target":
        desc[1][3] = 0
    elif case == "too_many_points":
        desc = [[0, 2 ** 30, 0, 1], [0, 2 ** 30, 0, 1]]
        n_pts, pairs = 2 ** 30, 2
    d, pd = _c(desc)
    rc = L.dpc_nearest_batched(None, n_pts, 1, None, pd, pairs, None, None, None, None, None)
    if case in ("ok", "empty_source"):
        assert rc == _native.DPC_ERR_NULL   # the arguments passed, the missing buffers stop it
    else:
        assert rc == _native.DPC_ERR_SHAPE
    assert L.dpc_nearest_batched(None, 0, 1, None, None, 0, None, None, None, None, None) == 0   # P = 0: nothing to do


def test_chamfer_python_refuses_bad_arguments_without_a_device():
    from dpc.render import chamfer_batched, chamfer_of_split, nearest_batched

    a = np.zeros((4, 3))
    with pytest.raises(ValueError):
        nearest_batched(np.zeros((10, 3)), [[0, 5, 5, 0]])          # empty target
    with pytest.raises(ValueError):
        nearest_batched(np.zeros((10, 3)), [[0, 5, 6, 5]])          # target range past the buffer
    with pytest.raises(ValueError):
        nearest_batched(np.zeros((10, 3)), [[0, 5, 5]])             # not [P,4]
    with pytest.raises(ValueError):
        chamfer_batched([a], [np.zeros((0, 3))])
    with pytest.raises(ValueError):
        chamfer_batched([a, a], [a], gt_of=[0, 1])
    with pytest.raises(ValueError):
        chamfer_batched([a], [a], gt_of=[0.5])
    with pytest.raises(ValueError):
        chamfer_batched([np.zeros((4, 2))], [a])
    pts = np.zeros((2, 4, 3), np.float32)
    for nums in ([4], [4, 5], [-1, 2], [1.5, 2.0]):
        with pytest.raises(ValueError):
            chamfer_of_split([(pts, np.asarray(nums))], [a])
    with pytest.raises(ValueError):
        chamfer_of_split([(pts, None)], [np.zeros((0, 3))])
    with pytest.raises(ValueError):
        chamfer_of_split([(pts, None), (np.zeros((3, 4, 3)), None)], [a, a])     # views differ
    with pytest.raises(ValueError):
        chamfer_of_split([(pts, None)], [a], reference_rotation=np.ones((4,)))
