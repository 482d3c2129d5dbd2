"""CPU side of the Chamfer loss (no GPU): the closed-form gradient of tests/chamfer_grad_oracle.py against the reference's
own autograd (F19, tests/golden/make_golden_chamfer_grad.py), against torch-CPU autograd of a brute-force restatement on
fresh seeds (both modes), and against central finite differences; the d = 0 rule; and the argument checks of
dpc_nearest_batched_bwd's C ABI, which return before anything touches a device.

The bound of every comparison is the one the GPU tests use, per component of a point's gradient:
    |got - ref| <= (n + 8) * u * sum |contribution|,   u = 2^-53 here,
n the number of contributions the point receives: each term carries a handful of roundings (difference, distance, divide,
weight, multiply) and any summation order of n terms adds at most (n - 1) u sum |c|."""
import ctypes

import numpy as np
import pytest
import torch

from chamfer_grad_oracle import chamfer_grad, nearest_brute

U64 = 2.0 ** -53


def within(got, ref, abs_sum, count, u):
    bound = (count[:, None] + 8) * u * abs_sum
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert np.isfinite(got).all()
    assert (err <= bound).all(), "worst error / bound %.3f" % float((err / np.maximum(bound, 1e-300)).max())
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def torch_loss(pts, pairs, a, b, squared):
    """sum_p a[p] * mean_p + sum_i b[i] * v[i] with torch ops autograd can differentiate (v: distances or their squares)."""
    loss, o = pts.sum() * 0.0, 0
    for p, (s0, ns, t0, nt) in enumerate(pairs):
        if ns == 0:
            continue
        s, t = pts[s0:s0 + ns], pts[t0:t0 + nt]
        dist = torch.sqrt(((t[None, :, :] - s[:, None, :]) ** 2).sum(2))
        v = dist[torch.arange(ns), torch.argmin(dist, dim=1)]
        v = v * v if squared else v
        loss = loss + a[p] * v.mean() + (torch.from_numpy(b[o:o + ns]) * v).sum()
        o += ns
    return loss


@pytest.fixture(scope="module")
def f19(golden):
    return golden("f19_chamfer_grad.npz")


def f19_problem(f19):
    pts = np.concatenate([f19["tgt"], f19["src0"], f19["src1"], f19["src2"]])
    pairs = np.array([[300, 257, 0, 300], [557, 64, 0, 300], [621, 5, 0, 300]])
    ref = np.concatenate([f19["grad_tgt"], f19["grad_src0"], f19["grad_src1"], f19["grad_src2"]])
    return pts, pairs, ref


def test_oracle_matches_f19(f19):
    pts, pairs, ref = f19_problem(f19)
    assert pts.dtype == np.float64 and np.isfinite(ref).all()
    dist, idx = nearest_brute(pts, pairs)
    assert np.array_equal(idx, f19["idx"])
    assert np.allclose(dist, f19["min_dist"], rtol=4 * U64, atol=0)
    grad, abs_sum, count = chamfer_grad(pts, pairs, f19["idx"], f19["a"], f19["b"])
    assert count[:300].max() > 3 and (count[:300] == 0).any()       # shared targets, and targets nobody chose
    within(ref, grad, abs_sum, count, U64)


def ragged_problem(seed):
    """Clouds of 40, 1, 23, 64 and 9 points; shared targets, both directions, a one-point target, an empty source."""
    rng = np.random.default_rng(seed)
    sizes = [40, 1, 23, 64, 9]
    start = np.cumsum([0] + sizes)
    pts = rng.random((start[-1], 3)) - 0.5
    r = lambda i: (start[i], sizes[i])
    pairs = np.array([r(0) + r(3), r(3) + r(0), r(2) + r(3), r(3) + r(2), r(4) + r(1), r(1) + r(4), (start[2], 0) + r(0),
                      r(4) + r(3)])
    a = rng.standard_normal(len(pairs))
    b = rng.standard_normal(int(pairs[:, 1].sum()))
    return pts, pairs, a, b


@pytest.mark.parametrize("squared", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_matches_torch_autograd(seed, squared):
    pts, pairs, a, b = ragged_problem(seed)
    leaf = torch.from_numpy(pts).requires_grad_(True)
    torch_loss(leaf, pairs, a, b, squared).backward()
    _, idx = nearest_brute(pts, pairs)
    for gm, gd in ((a, b), (a, None), (None, b)):
        grad, abs_sum, count = chamfer_grad(pts, pairs, idx, gm, gd, squared)
        if gm is not None and gd is not None:
            within(leaf.grad.numpy(), grad, abs_sum, count, U64)
        else:   # the loss is linear in (a, b): the two halves add up to the whole
            other = chamfer_grad(pts, pairs, idx, None if gm is not None else a, None if gd is not None else b, squared)
            within(leaf.grad.numpy(), grad + other[0], abs_sum + other[1], count + other[2], U64)


@pytest.mark.parametrize("squared", [False, True])
def test_oracle_matches_finite_differences(squared):
    """ns = 5, nt = 7, every source 0.2 or 0.3 from its own target and >= 0.7 from any other: no nearest neighbour changes
    within the step (asserted for both directions).  Central differences with h = 1e-5: truncation
    h^2 / 6 |f'''| <= 1e-10 / 6 * 3 |w| / d^2 ~ 1e-9 |w|, rounding 2^-53 |loss| / h ~ 1e-10; the bound below is ten times
    their sum for sum |w| ~ 10."""
    rng = np.random.default_rng(7)
    tgt = np.array([[i, 0.0, 0.0] for i in range(7)]) + 0.02 * rng.standard_normal((7, 3))
    dirs = rng.standard_normal((5, 3))
    src = tgt[[5, 0, 3, 3, 6]] + np.array([[0.3], [0.3], [0.3], [0.2], [0.3]]) * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    pts = np.concatenate([src, tgt])
    pairs = np.array([[0, 5, 5, 7], [5, 7, 0, 5]])
    a, b = rng.standard_normal(2), rng.standard_normal(12)
    _, idx = nearest_brute(pts, pairs)
    assert list(idx[:5]) == [5, 0, 3, 3, 6]
    for s0, ns, t0, nt in pairs:   # in both directions the runner-up is at least 1e-2 behind: far more than the step
        d = np.sort(np.linalg.norm(pts[t0:t0 + nt][None] - pts[s0:s0 + ns][:, None], axis=2), axis=1)
        assert (d[:, 1] - d[:, 0]).min() > 1e-2 and d[:, 0].min() > 0.15
    grad, _, _ = chamfer_grad(pts, pairs, idx, a, b, squared)
    f = lambda x: float(torch_loss(torch.from_numpy(x), pairs, a, b, squared))
    h = 1e-5
    fd = np.zeros_like(pts)
    for i in range(len(pts)):
        for k in range(3):
            e = np.zeros_like(pts)
            e[i, k] = h
            fd[i, k] = (f(pts + e) - f(pts - e)) / (2 * h)
    assert np.abs(fd - grad).max() <= 1e-7, np.abs(fd - grad).max()


@pytest.mark.parametrize("squared", [False, True])
def test_coincident_points_give_exact_zeros(squared):
    rng = np.random.default_rng(3)
    pts = rng.random((30, 3))
    pairs = np.array([[0, 30, 0, 30]])
    dist, idx = nearest_brute(pts, pairs)
    assert (dist == 0).all() and np.array_equal(idx, np.arange(30))
    grad, abs_sum, count = chamfer_grad(pts, pairs, idx, np.array([1.5]), rng.standard_normal(30), squared)
    assert (grad == 0).all() and (abs_sum == 0).all() and (count == 2).all()


def _c(a, dtype=np.int32):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_new_symbols_are_bound():
    from dpc.render import _native

    L = _native.lib()
    for name in ("dpc_chamfer_bwd_workspace_bytes", "dpc_nearest_batched_bwd", "dpc_chamfer_pair_means"):
        assert name in _native.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert L.dpc_chamfer_bwd_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.dpc_nearest_batched_bwd.argtypes) == 14


def test_bwd_workspace_bytes():
    from dpc.render import _native

    L = _native.lib()
    d, pd = _c([[0, 300, 300, 20000], [300, 20000, 0, 300], [0, 0, 300, 5]])
    n64, n32 = L.dpc_chamfer_bwd_workspace_bytes(3, pd, 1), L.dpc_chamfer_bwd_workspace_bytes(3, pd, 0)
    # a term per source point, a sum per (pair, target), three components each, and the prefixes
    assert n64 >= (20300 + 20305) * 3 * 8 + 4 * 4 * 4
    assert n32 < n64 and n32 % 16 == 0 and n64 % 16 == 0
    assert L.dpc_chamfer_bwd_workspace_bytes(0, pd, 1) == 0
    assert L.dpc_chamfer_bwd_workspace_bytes(3, None, 1) == 0
    for bad in ([[0, -1, 0, 5]], [[-1, 1, 0, 5]], [[0, 1, -2, 5]], [[0, 1, 0, -5]], [[0, 4, 0, 0]],
                [[0, 2 ** 31 - 1, 0, 1], [0, 1, 0, 1]], [[0, 1, 0, 2 ** 31 - 1], [0, 1, 0, 1]]):
        b, pb = _c(bad)
        assert L.dpc_chamfer_bwd_workspace_bytes(len(bad), pb, 1) == 0, bad


@pytest.mark.parametrize("case", ["ok", "empty_source", "pairs_neg", "n_pts_neg", "neg_count", "neg_start", "neg_tgt_start",
                                  "neg_tgt_count", "src_range", "tgt_range", "empty_target", "too_many_points",
                                  "too_many_targets"])
def test_bwd_argument_checks_come_before_any_launch(case):
    """The table rules of dpc_nearest_batched (tests/test_chamfer_host.py) hold for its backward, and the target points of
    all pairs must fit int32 as well.  With NULL device pointers a valid call gets as far as DPC_ERR_NULL."""
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
    elif case == "too_many_targets":
        desc = [[0, 1, 0, 2 ** 30], [0, 1, 0, 2 ** 30]]
        n_pts, pairs = 2 ** 30, 2
    d, pd = _c(desc)
    for squared in (0, 1):
        rc = L.dpc_nearest_batched_bwd(None, n_pts, 1, None, pd, pairs, None, None, None, None, squared, None, None, None)
        assert rc == (_native.DPC_ERR_NULL if case in ("ok", "empty_source") else _native.DPC_ERR_SHAPE)
    assert L.dpc_nearest_batched_bwd(None, 0, 1, None, None, 0, None, None, None, None, 0, None, None, None) == 0
    rc = L.dpc_chamfer_pair_means(None, 1, None, pd, pairs, None, None, None)
    if case in ("ok", "empty_source", "n_pts_neg", "src_range", "tgt_range", "too_many_targets"):
        assert rc == _native.DPC_ERR_NULL     # only the signs, the counts and the empty-target rule apply to the means
    else:
        assert rc == _native.DPC_ERR_SHAPE


def test_chamfer_loss_refuses_bad_arguments_without_a_device():
    from dpc.render import chamfer_loss, nearest_batched

    a = np.zeros((4, 3))
    with pytest.raises(ValueError):
        chamfer_loss([a], [np.zeros((0, 3))])
    with pytest.raises(ValueError):
        chamfer_loss([a, a], [a], gt_of=[0, 1])
    with pytest.raises(ValueError):
        chamfer_loss([a, a], [a])
    with pytest.raises(ValueError):
        chamfer_loss(torch.zeros(2, 4, 2), [a, a])
    with pytest.raises(ValueError):
        chamfer_loss([np.zeros((4, 2))], [a])
    with pytest.raises(ValueError):
        nearest_batched(torch.zeros(10, 3, requires_grad=True), [[0, 5, 5, 0]])      # empty target
    with pytest.raises(ValueError):
        nearest_batched(torch.zeros(10, 3, requires_grad=True), [[0, 5, 6, 5]], squared=True)
