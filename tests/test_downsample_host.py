"""CPU side of the voxel-grid downsampling (no GPU): the numpy oracle of open3d's VoxelDownSample that the GPU tests
compare against by bytes, pinned to a literal per-point dict loop of the semantics in include/dpc_render.h and to
hand-computed answers; the binding's refusals and dpc_voxel_downsample's C-ABI checks, which return before anything
touches a device.

oracle_downsample is vectorised but keeps the one order that matters: every voxel's sum is sequential in input order,
starting from 0.0.  After a stable sort by key, level k adds the k-th member of every voxel that has one, so no voxel ever
sees a tree reduction (np.sum and np.add.reduceat would: they sum pairwise)."""
import ctypes
import math

import numpy as np
import pytest

INT_MAX = 2147483647


def _bounds(p, vs):
    mn = p.min(axis=0) if len(p) else np.zeros(3)
    mx = p.max(axis=0) if len(p) else np.zeros(3)
    lo, hi = mn - vs * 0.5, mx + vs * 0.5
    if not vs > 0 or vs * INT_MAX < (hi - lo).max():
        raise ValueError("voxel_size is too small")
    return lo


def oracle_downsample(points, voxel_size):
    """open3d's PointCloud::VoxelDownSample in fp64, voxels in ascending (kx, ky, kz) order: [m,3] float64."""
    p = np.asarray(points).astype(np.float64)   # float32 widens exactly
    vs = float(voxel_size)
    lo = _bounds(p, vs)
    n = len(p)
    if n == 0:
        return np.zeros((0, 3))
    key = np.floor((p - lo) / vs).astype(np.int64)   # subtract, then an IEEE division, then floor
    order = np.lexsort((key[:, 2], key[:, 1], key[:, 0]))  # stable: equal keys keep input order
    ks, ps = key[order], p[order]
    head = np.ones(n, dtype=bool)
    head[1:] = (ks[1:] != ks[:-1]).any(axis=1)
    starts = np.flatnonzero(head)
    cnt = np.diff(np.append(starts, n))
    acc = np.zeros((len(starts), 3))
    by = np.argsort(-cnt, kind="stable")
    neg = -cnt[by]
    for k in range(int(cnt.max())):
        live = by[:np.searchsorted(neg, -k, side="left")]   # the voxels with more than k members
        acc[live] += ps[starts[live] + k]
    return acc / cnt[:, None].astype(np.float64)


def literal_downsample(points, voxel_size):
    """The pseudocode of include/dpc_render.h, one point at a time with Python floats (IEEE doubles)."""
    p = np.asarray(points).astype(np.float64)
    vs = float(voxel_size)
    lo = [float(v) for v in _bounds(p, vs)]
    acc = {}
    for x in p.tolist():
        key = tuple(int(math.floor((x[c] - lo[c]) / vs)) for c in range(3))
        a = acc.setdefault(key, [0.0, 0.0, 0.0, 0])
        for c in range(3):
            a[c] += x[c]
        a[3] += 1
    rows = [[acc[k][c] / float(acc[k][3]) for c in range(3)] for k in sorted(acc)]
    return np.array(rows, dtype=np.float64).reshape(-1, 3)


def _random_cloud(rng, n):
    kind = rng.integers(3)
    if kind == 0:
        return rng.random((n, 3)) - 0.5
    if kind == 1:
        return np.round(rng.random((n, 3)) * 8) / 8            # a lattice: many points on voxel faces
    return (rng.standard_normal((n, 3)) * 0.2).astype(np.float32)


@pytest.mark.parametrize("seed", range(12))
def test_oracle_is_the_per_point_loop(seed):
    rng = np.random.default_rng(seed)
    for n in (1, 2, 5, 64, 300, 2000):
        p = _random_cloud(rng, n)
        for vs in (1e-3, 0.01, 0.05, 0.2, 0.125, 1.0, float(rng.uniform(0.005, 0.5))):
            ref = literal_downsample(p, vs)
            got = oracle_downsample(p, vs)
            assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), (n, vs)


def test_two_points_are_averaged():
    p = np.array([[0.1, 0.2, 0.3], [0.13, 0.21, 0.33]])
    want = np.array([[(0.0 + 0.1 + 0.13) / 2, (0.0 + 0.2 + 0.21) / 2, (0.0 + 0.3 + 0.33) / 2]])
    assert oracle_downsample(p, 1.0).tobytes() == want.tobytes()


def test_points_on_voxel_faces_go_to_the_upper_voxel():
    # min 0, vs 1: lo = -0.5, so (x - lo) / vs is 0.5, 0.75, 1.0, 2.0: x = 0.5 and 1.5 sit exactly on faces
    p = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.5, 0.0, 0.0], [1.5, 0.0, 0.0]])
    want = np.array([[0.125, 0.0, 0.0], [0.5, 0.0, 0.0], [1.5, 0.0, 0.0]])
    assert oracle_downsample(p, 1.0).tobytes() == want.tobytes()
    # just below a face the subtraction rounds first: one ulp below 0.5 gives x - lo = 1.0 (on the face), two ulps below
    # give the double just under 1.0 (the lower voxel)
    q = p.copy()
    q[2, 0] = np.nextafter(0.5, 0.0)
    assert q[2, 0] - (-0.5) == 1.0 and oracle_downsample(q, 1.0)[1, 0] == q[2, 0]
    q[2, 0] = np.nextafter(q[2, 0], 0.0)
    out = oracle_downsample(q, 1.0)
    assert len(out) == 2 and out[0, 0] == (0.0 + 0.0 + 0.25 + q[2, 0]) / 3


def test_empty_and_one_point_clouds():
    assert oracle_downsample(np.zeros((0, 3)), 0.01).shape == (0, 3)
    one = np.array([[-0.0, 1.5, -2.25]])
    out = oracle_downsample(one, 0.01)
    assert out.tolist() == [[0.0, 1.5, -2.25]]
    assert not np.signbit(out[0, 0])   # the sum starts at +0.0: 0.0 + -0.0 = +0.0


def test_sum_is_sequential_not_pairwise():
    x = np.full(1000, 1.1e-16)
    x[0] = 1.0
    seq = 0.0
    for v in x:
        seq += v
    assert seq == 1.0 and np.sum(x) != seq                        # the fixture tells the two orders apart
    assert np.add.reduceat(x, [0])[0] != seq
    p = np.zeros((1000, 3))
    p[:, 0] = x
    out = oracle_downsample(p, 10.0)
    assert out.shape == (1, 3) and out[0, 0] == seq / 1000.0


def test_oracle_refuses_what_open3d_refuses():
    p = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    for vs in (0.0, -1.0, 1e-10):
        with pytest.raises(ValueError):
            oracle_downsample(p, vs)
    assert len(oracle_downsample(p, 1e-9)) == 2   # 1e-9 * (2^31 - 1) > 1 + 1e-9: accepted by open3d


@pytest.mark.parametrize("vs", [0.0, -0.01, float("nan"), float("inf"), "0.01", None])
def test_binding_refuses_bad_voxel_size_before_any_device_use(vs):
    import dpc.render as R

    with pytest.raises(ValueError, match="voxel_size"):
        R.voxel_down_sample([np.zeros((4, 3))], vs)
    with pytest.raises(ValueError, match="voxel_size"):
        R.downsample_split(["a"], lambda name: np.zeros((4, 3)), vs)


@pytest.mark.parametrize("bad", [np.zeros((4, 2)), np.zeros((4,)), np.zeros((2, 4, 3)), np.zeros((4, 3), dtype=np.int64)])
def test_binding_refuses_bad_clouds_before_any_device_use(bad):
    import dpc.render as R

    with pytest.raises(ValueError, match="cloud 1"):
        R.voxel_down_sample([np.zeros((4, 3)), bad], 0.01)
    assert R.voxel_down_sample([], 0.01) == []


def test_c_abi_checks_come_before_any_launch():
    """With NULL device pointers a valid call gets as far as DPC_ERR_NULL: every DPC_ERR_SHAPE below is returned before
    anything touches a device."""
    from dpc.render import _native

    L = _native.lib()

    def call(desc, n_pts, vs=0.01, clouds=None):
        d = np.ascontiguousarray(np.asarray(desc, dtype=np.int32).reshape(-1, 2))
        c = len(d) if clouds is None else clouds
        return L.dpc_voxel_downsample(None, n_pts, 1, None, d.ctypes.data_as(ctypes.c_void_p), c, vs,
                                      None, None, None, None, None, None)

    assert call([[0, 10], [10, 0], [3, 5]], 10) == _native.DPC_ERR_NULL
    assert call([[0, 10]], 10, clouds=0) == 0                         # nothing to do
    for vs in (0.0, -1.0, float("nan"), float("inf")):
        assert call([[0, 10]], 10, vs) == _native.DPC_ERR_SHAPE
    assert call([[0, 11]], 10) == _native.DPC_ERR_SHAPE                # past the end of the buffer
    assert call([[-1, 2]], 10) == _native.DPC_ERR_SHAPE
    assert call([[0, -2]], 10) == _native.DPC_ERR_SHAPE
    assert call([[0, 10]], -1) == _native.DPC_ERR_SHAPE
    assert call([[0, 10]], 10, clouds=-1) == _native.DPC_ERR_SHAPE
    assert call([[0, INT_MAX]] * 2, INT_MAX) == _native.DPC_ERR_SHAPE  # more than 2^31 - 2 members
    assert L.dpc_downsample_workspace_bytes(0, 10) == 0 and L.dpc_downsample_workspace_bytes(3, -1) == 0
    ws = L.dpc_downsample_workspace_bytes(1356, 120000 * 1356)
    M = 120000 * 1356
    T = -(-M // 4096)
    assert 28 * M + 2056 * T + 56 * 1356 + 1024 <= ws <= 28 * M + 2056 * T + 56 * 1356 + 2048   # include/dpc_render.h
    assert L.dpc_downsample_workspace_bytes(5, 0) > 0
