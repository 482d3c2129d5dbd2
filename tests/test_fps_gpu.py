"""Farthest-point sampling on the GPU (csrc/dpc_fps.hip) against the numpy restatement of its rule (tests/fps_oracle.py).

Everything is compared exactly: the contract of dpc_fps (include/dpc_render.h) fixes the distance expression, its
operation order and the tie rule, so indices and radius2 have one right answer, bit for bit.  The sweep of
`oracle_sweep` runs once per module: every size at which the launcher changes the kernel (1024 | 1025, 4096 | 4097,
8192 | 8193), the wave and workgroup edges (63, 64, 65, 1023), a full permutation (n = m = 257), the largest real cloud
(12647) and the cap (16384), for fp32 and fp64, on random clouds and on an integer lattice whose distances tie exactly."""
import ctypes
import re

import numpy as np
import pytest
import torch

import dpc.render as R
import fps_oracle as O
from dpc.render import _native
from test_abi_and_host import device_object_output

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
KINDS = ["random", "lattice"]
# (n, m): m = min(n, 96) for the small sizes, 8 rounds where only the size matters
SIZES = [(n, min(n, 96)) for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 4097)] + \
        [(257, 257), (4096, 8), (8192, 8), (8193, 8), (12647, 8), (_native.DPC_FPS_MAX_POINTS, 8)]
# k_fps<fp64 input, threads, points per thread>: the launcher's size classes (csrc/dpc_fps.hip)
EXPECTED = {"k_fps<%d, %d, %d>" % (f, t, p) for f in (0, 1) for t, p in ((256, 4), (1024, 4), (1024, 8), (1024, 16))}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sample(clouds, m, first=None):
    """farthest_point_sample on numpy clouds -> numpy (indices list, radius2 list)."""
    idx, rad = R.farthest_point_sample([dev(c) for c in clouds], m, first=first, return_radius=True)
    assert all(i.dtype == torch.int32 and i.is_cuda for i in idx) and all(r.dtype == torch.float64 for r in rad)
    return [i.cpu().numpy() for i in idx], [r.cpu().numpy() for r in rad]


def same(got, ref, what):
    assert got[0].tolist() == ref[0].tolist(), what
    assert got[1].tobytes() == ref[1].tobytes(), what


@pytest.fixture(scope="module")
def oracle_sweep():
    """{(kind, dtype name): (clouds, firsts, device results, oracle results)} and the instantiations the sweep launched."""
    out, launched = {}, set()
    for kind in KINDS:
        for dtype in DTYPES:
            clouds = [O.clouds(kind, n, 7 * n + len(kind), dtype) for n, _ in SIZES]
            ms = [m for _, m in SIZES]
            firsts = [(3 * n) // 7 for n, _ in SIZES]
            got = {}

            def run():
                got["r"] = sample(clouds, ms, firsts)

            launched |= _native.launched_instantiations(run, torch.device("cuda"))
            ref = [O.fps(c, m, f) for c, m, f in zip(clouds, ms, firsts)]
            out[kind, np.dtype(dtype).name] = (clouds, firsts, got["r"], ref)
    assert R.check_status() == 0
    return out, launched


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", KINDS)
def test_exact_parity_with_the_oracle(oracle_sweep, kind, dtype):
    clouds, firsts, got, ref = oracle_sweep[0][kind, np.dtype(dtype).name]
    for k, (n, m) in enumerate(SIZES):
        what = "%s %s n %d m %d first %d" % (kind, np.dtype(dtype).name, n, m, firsts[k])
        assert got[0][k].shape == (m,) and got[1][k].shape == (m,), what
        same((got[0][k], got[1][k]), ref[k], what)


def test_the_sweep_launches_every_compiled_instantiation(oracle_sweep):
    """The k_fps instantiations in the launch record over the sweep == the launcher's class table == the kernel symbols
    of dpc_fps.o: an instantiation added without a size in SIZES that reaches it fails here."""
    launched = {i for i in oracle_sweep[1] if i.startswith("k_fps")}
    assert launched == EXPECTED, sorted(launched ^ EXPECTED)
    built = set()
    for line in device_object_output("dpc_fps.o", ["llvm-readelf", "-sW"]).splitlines():
        f = line.split()
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)(\w+)$", f[7]) if len(f) >= 8 and f[3] == "FUNC" else None
        if m:
            n = int(m.group(1))
            name, rest = m.group(2)[:n], m.group(2)[n:]
            targs = re.match(r"I((?:Li-?\d+E)+)E", rest)
            built.add(name + ("<%s>" % ", ".join(re.findall(r"Li(-?\d+)E", targs.group(1))) if targs else ""))
    built = {b for b in built if b.startswith("k_fps")}
    assert launched == built, sorted(launched ^ built)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_fp32_clouds_and_their_fp64_copies_give_the_same_indices(kind):
    sizes = [(65, 65), (1025, 96), (4097, 64), (8193, 32)]
    c32 = [O.clouds(kind, n, 11 * n, np.float32) for n, _ in sizes]
    ms = [m for _, m in sizes]
    a, b = sample(c32, ms), sample([c.astype(np.float64) for c in c32], ms)
    for k in range(len(sizes)):
        same((a[0][k], a[1][k]), (b[0][k], b[1][k]), "n %d" % sizes[k][0])


# 3 ---------------------------------------------------------------------------------------------------------------
def test_known_answers_on_the_device():
    line = np.stack([np.arange(17.0), np.zeros(17), np.zeros(17)], axis=1)
    coincident = np.tile(np.array([[0.25, -0.5, 3.0]], dtype=np.float32), (70, 1))
    idx, rad = sample([line, line.astype(np.float32), coincident, line], [17, 17, 70, 3], first=[0, 0, 66, 5])
    bisect = [0, 16, 8, 4, 12, 2, 6, 10, 14, 1, 3, 5, 7, 9, 11, 13, 15]
    assert idx[0].tolist() == bisect and idx[1].tolist() == bisect
    assert rad[0][0] == np.inf and rad[0][1:].tolist() == [256.0, 64.0, 16.0, 16.0] + [4.0] * 4 + [1.0] * 8
    assert idx[2].tolist() == [66] + [i for i in range(70) if i != 66] and (rad[2][1:] == 0).all() and rad[2][0] == np.inf
    assert idx[3].tolist() == [5, 16, 0] and rad[3][1:].tolist() == [121.0, 25.0]
    # a [B,n,3] tensor with one m gives [B,m] tensors; None is point 0
    both = R.farthest_point_sample(dev(np.stack([line, line[::-1]])), 3, return_radius=True)
    assert both[0].shape == (2, 3) and both[1].shape == (2, 3) and both[0].dtype == torch.int32
    assert both[0].cpu().tolist() == [[0, 16, 8], [0, 16, 8]]
    assert R.farthest_point_sample(dev(line[None]), 2).cpu().tolist() == [[0, 16]]
    assert R.check_status() == 0


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_greedy_properties_without_the_oracle(dtype):
    """Distinct indices; radius2[0] = +inf; radius2[k] = min over earlier picks of d2, evaluated directly; radius2
    non-increasing from k = 1; and every point not taken is within radius2[k] of the first k picks (the greedy choice)."""
    sizes = [(300, 300), (2000, 128), (9000, 64)]
    clouds = [O.clouds("random", n, 5 * n, dtype) for n, _ in sizes]
    idx, rad = sample(clouds, [m for _, m in sizes], first=[0, 1999, 4500])
    for (n, m), P, i, r in zip(sizes, clouds, idx, rad):
        P = P.astype(np.float64)
        assert len(set(i.tolist())) == m and i.min() >= 0 and i.max() < n
        assert r[0] == np.inf and (np.diff(r[1:]) <= 0).all()
        S = P[i]
        d = S[:, None, :] - S[None, :, :]
        D = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        for k in range(1, m):
            assert r[k] == D[k, :k].min(), (n, k)
        k = m // 2
        e = P[:, None, :] - S[None, :k, :]
        cover = ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).min(axis=1)
        assert cover.max() == r[k]


# 5 ---------------------------------------------------------------------------------------------------------------
def raw_fps(pts, rows, status=None):
    """dpc_fps itself on a packed device buffer and a table of (start, count, first, out_start, samples) rows."""
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 5))
    desc_d = dev(desc)
    total = int(desc[-1, 3] + desc[-1, 4])
    indices = torch.full((total,), -7, dtype=torch.int32, device="cuda")
    radius2 = torch.full((total,), -7.0, dtype=torch.float64, device="cuda")
    rc = _native.lib().dpc_fps(_native.ptr(pts), int(pts.shape[0]), int(pts.dtype == torch.float64), _native.ptr(desc_d),
                               desc.ctypes.data_as(ctypes.c_void_p), len(desc), _native.ptr(indices), _native.ptr(radius2),
                               _native.ptr(status), _native.stream_ptr(pts.device))
    assert rc == 0
    return indices.cpu().numpy(), radius2.cpu().numpy()


def test_reproducible_and_independent_of_batching():
    """A ragged batch of fp32 and fp64 clouds of every size class: the same bits in a second run, with the clouds in
    reverse order, and one cloud per call (an fp32 cloud alone runs the fp32 kernels, in the batch the fp64 ones)."""
    sizes = [(1, 1), (64, 64), (300, 100), (1025, 64), (5000, 48), (9000, 32)]
    clouds = [O.clouds("lattice" if n == 300 else "random", n, 90 + n, DTYPES[k % 2]) for k, (n, _) in enumerate(sizes)]
    ms = [m for _, m in sizes]
    first, second = sample(clouds, ms), sample(clouds, ms)
    rev = sample(clouds[::-1], ms[::-1])
    for k in range(len(sizes)):
        one = (first[0][k], first[1][k])
        same((second[0][k], second[1][k]), one, "second run, cloud %d" % k)
        same((rev[0][-1 - k], rev[1][-1 - k]), one, "reversed, cloud %d" % k)
        alone = sample([clouds[k]], ms[k])
        same((alone[0][0], alone[1][0]), one, "alone, cloud %d" % k)
        same(one, O.fps(clouds[k], ms[k]), "oracle, cloud %d" % k)


def test_clouds_may_share_input_rows():
    """The same rows listed twice with different `first`, and a sub-range of them: each equals the oracle on its rows."""
    P = O.clouds("random", 1500, 3, np.float32)
    rows = [(0, 1500, 0, 0, 40), (0, 1500, 777, 40, 40), (200, 1000, 5, 85, 30)]   # a gap in the output at 80..84
    idx, rad = raw_fps(dev(P), rows)
    for start, count, first, out0, m in rows:
        same((idx[out0:out0 + m], rad[out0:out0 + m]), O.fps(P[start:start + count], m, first), "row %d" % out0)
    assert (idx[80:85] == -7).all() and (rad[80:85] == -7.0).all()   # rows of no cloud are left alone


# 6 ---------------------------------------------------------------------------------------------------------------
def test_nonfinite_clouds_are_flagged_and_their_neighbours_unaffected():
    a, b, c = (O.clouds("random", n, 60 + n, np.float32) for n in (500, 1500, 700))
    nan, inf = b.copy(), c.copy()
    nan[1234, 1] = np.nan
    inf[3, 2] = -np.inf
    R.check_status()   # clean slate
    idx, rad = sample([a, nan, b, inf], [50, 60, 70, 80])
    assert R.check_status() == _native.DPC_STATUS_NONFINITE and R.check_status() == 0
    assert (idx[1] == -1).all() and np.isnan(rad[1]).all() and len(idx[1]) == 60
    assert (idx[3] == -1).all() and np.isnan(rad[3]).all() and len(idx[3]) == 80
    same((idx[0], rad[0]), O.fps(a, 50), "neighbour 0")
    same((idx[2], rad[2]), O.fps(b, 70), "neighbour 2")


def test_a_device_table_that_differs_from_the_host_table_is_not_run():
    """The guard of the header: a device row outside the buffer, or of a size class the host table did not announce, sets
    DPC_STATUS_BAD_INDEX and writes nothing; the other rows are unaffected."""
    P = O.clouds("random", 600, 8, np.float32)
    host = np.array([(0, 600, 0, 0, 16), (0, 300, 0, 16, 16), (100, 500, 0, 32, 16)], dtype=np.int32)
    bad = host.copy()
    bad[0, 1] = 700        # beyond the buffer
    bad[2, 1] = 5000       # inside no buffer either, and of another size class
    pts, desc_d, status = dev(P), dev(bad), torch.zeros(1, dtype=torch.int32, device="cuda")
    indices = torch.full((48,), -7, dtype=torch.int32, device="cuda")
    radius2 = torch.full((48,), -7.0, dtype=torch.float64, device="cuda")
    rc = _native.lib().dpc_fps(_native.ptr(pts), 600, 0, _native.ptr(desc_d), host.ctypes.data_as(ctypes.c_void_p), 3,
                               _native.ptr(indices), _native.ptr(radius2), _native.ptr(status), _native.stream_ptr(pts.device))
    assert rc == 0
    assert status.item() == _native.DPC_STATUS_BAD_INDEX
    idx, rad = indices.cpu().numpy(), radius2.cpu().numpy()
    assert (idx[:16] == -7).all() and (idx[32:] == -7).all() and (rad[:16] == -7.0).all() and (rad[32:] == -7.0).all()
    same((idx[16:32], rad[16:32]), O.fps(P[:300], 16), "the valid row")


# 7 ---------------------------------------------------------------------------------------------------------------
def test_emd_of_split_with_fps_equals_emd_loss_on_the_same_samples():
    """Three models, two views, a reference rotation, one model with truncated views: sampling="fps" equals emd_loss on
    clouds gathered with farthest_point_sample(first=0); sampling="random" equals the value through subsample_indices."""
    from dpc.render._split import _host_unit_quaternion, _rotate

    rng = np.random.default_rng(12)
    M, V, N, K = 3, 2, 300, 64
    preds = [(rng.random((V, N, 3)).astype(np.float32) - 0.5, np.array([250, 300]) if m == 1 else None) for m in range(M)]
    gts = [rng.random((310 + m, 3)) - 0.5 for m in range(M)]
    q = np.array([[0.9, 0.1, -0.3, 0.2]])
    R.check_status()
    got = R.emd_of_split(preds, gts, reference_rotation=q, num_points=K, seed=4, eps=1e-6, models_per_call=2, sampling="fps")
    assert got.shape == (M, V) and got.dtype == np.float64
    assert got.tobytes() == R.emd_of_split(preds, gts, reference_rotation=q, num_points=K, seed=99, eps=1e-6,
                                           sampling="fps").tobytes()   # no seed, no grouping in the result
    qn = _host_unit_quaternion(q)
    counts = [[N if nums is None else int(nums[i]) for i in range(V)] for _, nums in preds]
    views, targets = [], []
    for m in range(M):
        rot = _rotate(torch.from_numpy(preds[m][0]), qn, torch.device("cuda"))
        g = dev(gts[m])
        gi = R.farthest_point_sample([g], K, first=0)[0]
        for i in range(V):
            v = rot[i][:counts[m][i]]
            views.append(v[R.farthest_point_sample([v], K)[0].long()])
            targets.append(g[gi.long()])
    want = R.emd_loss(views, targets, eps=1e-6).cpu().numpy().reshape(M, V)
    assert got.tobytes() == want.tobytes() and (got > 0).all()
    # the default is the random draw, exactly as before
    rand = R.emd_of_split(preds, gts, reference_rotation=q, num_points=K, seed=4, eps=1e-6)
    assert rand.tobytes() == R.emd_of_split(preds, gts, reference_rotation=q, num_points=K, seed=4, eps=1e-6,
                                            sampling="random").tobytes()
    picks = R.emd.subsample_indices([(len(g), c) for g, c in zip(gts, counts)], K, 4)
    views, targets = [], []
    for m in range(M):
        rot = _rotate(torch.from_numpy(preds[m][0]), qn, torch.device("cuda"))
        for i in range(V):
            views.append(rot[i][dev(picks[m][1][i])])
            targets.append(dev(gts[m])[dev(picks[m][0])])
    assert rand.tobytes() == R.emd_loss(views, targets, eps=1e-6).cpu().numpy().reshape(M, V).tobytes()
    assert rand.tobytes() != got.tobytes()
    bad = [g.copy() for g in gts]
    bad[2][17, 0] = np.nan
    with pytest.raises(RuntimeError, match="GT cloud of model 2 holds a NaN or infinite coordinate"):
        R.emd_of_split(preds, bad, num_points=K, eps=1e-6, sampling="fps")
    assert R.check_status() == 0   # the split's failure was raised with names; the shared status word stays clean


# 8 ---------------------------------------------------------------------------------------------------------------
def test_sampled_clouds_carry_gradient_to_the_sampled_rows_only():
    """emd_loss(pred[idx], gt[jdx]) back-propagates to pred with non-zero rows exactly at idx."""
    pred = dev(O.clouds("random", 900, 21, np.float32)).requires_grad_(True)
    gt = dev(O.clouds("random", 1300, 22, np.float64))
    idx, jdx = R.farthest_point_sample([pred, gt], 128)
    assert not idx.requires_grad
    R.emd_loss([pred[idx.long()]], [gt[jdx.long()]], eps=1e-6).sum().backward()
    rows = (pred.grad != 0).any(dim=1).nonzero().flatten().cpu().numpy()
    assert rows.tolist() == sorted(idx.cpu().tolist()) and len(rows) == 128
