"""The Earth Mover's Distance on the GPU (csrc/dpc_emd.hip) against the numpy restatement of its auction
(tests/emd_oracle.py), scipy's optima stored in tests/golden/f24_emd.npz, and optima known in closed form.

The optimality bound (`bound`), for a pair of n points with optimum opt and largest cost cmax:

    pi is a permutation and inverse is its inverse;
    |emd - mean_i c[i, pi(i)]| <= 4 n u |.|        u = 2^-53: both sides are fixed-order fp64 sums of the same n
                                                    non-negative terms (error at most (n - 1) u each) and one divide;
    opt - slack <= n * emd <= opt + n * eps + slack,  slack = 64 n u max(1, cmax).

The middle inequality is the auction's guarantee: the final phase ends with every bidder within eps of its best value at
the final prices, so the total is within n * eps of the optimum.  The slack: each of the two compared values (n * emd and
the stored optimum) carries a handful of fp64 roundings of quantities bounded by a few times cmax (the cost itself: the
differences, squares, two additions, the root; then a sum of n terms, the divide and the multiply by n), and 64 n u cmax
covers them with room.  It is a few 1e-12 at n = 1000 against n * eps = 1e-3.

The gradient bound, per component: |got - ref| <= 8 u |ref|, u of the dtype the gradient is stored in; ref is the closed
form on the device's own matching, evaluated in extended precision.  The device evaluates in fp64: the difference (1
rounding), d = sqrt of a sum of three squares (at most 3.5 u), the divide, w = upstream / n and the multiply, at most
7.5 u of fp64 in all, then one rounding to the stored type.

Round counts seen on the device are printed by every case (run with -s) and recorded in profiles/LAB_NOTES.md."""
import os

import numpy as np
import pytest
import torch

import dpc.render as R
import emd_oracle as O
from dpc.render import _native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
DTYPES = [np.float32, np.float64]
T = np.array([0.05, -0.03, 0.02])


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "f24_emd.npz")) as f:
        return {k: f[k] for k in f.files}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def match(pairs, squared, eps, max_rounds=None):
    """emd_match on numpy pairs [(P, G), ...] -> numpy (emd [P], assignments, inverses, rounds [P])."""
    emd, asg, inv, rounds = R.emd_match([dev(p) for p, _ in pairs], [dev(g) for _, g in pairs], squared=squared, eps=eps,
                                        max_rounds=max_rounds)
    assert emd.dtype == torch.float64 and rounds.dtype == torch.int32 and all(a.dtype == torch.int32 for a in asg + inv)
    return emd.cpu().numpy(), [a.cpu().numpy() for a in asg], [a.cpu().numpy() for a in inv], rounds.cpu().numpy()


def bound(P, G, squared, eps, emd, pi, inv, opt, what):
    n = len(P)
    assert sorted(pi.tolist()) == list(range(n)), what
    assert (inv[pi] == np.arange(n)).all(), what
    C = O.cost_matrix(P, G, squared)
    mean = C[np.arange(n), pi].sum() / n
    slack = 64 * n * U64 * max(1.0, C.max())
    print("%s: n %d emd %.17g recomputed %.17g n*emd - opt %.3e (n*eps %.3e, slack %.3e)"
          % (what, n, emd, mean, n * emd - opt, n * eps, slack))
    assert abs(emd - mean) <= 4 * n * U64 * abs(mean), what
    assert opt - slack <= n * emd <= opt + n * eps + slack, what


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("kind", ["random", "lattice"])
def test_exact_parity_with_the_oracle(kind, dtype):
    """squared = True, eps = 1e-6, n in {1, 2, 63, 64, 65, 257}: assignment, inverse and round count equal the oracle's
    exactly; so does emd, whose summation order the oracle restates."""
    sizes = (1, 2, 63, 64, 65, 257)
    pairs = [O.clouds(kind, n, 100 + n, dtype) for n in sizes]
    emd, asg, inv, rounds = match(pairs, True, 1e-6)
    for k, (P, G) in enumerate(pairs):
        ref = O.emd(P, G, True, 1e-6)
        print("parity %s %s n %d: rounds device %d oracle %d" % (kind, np.dtype(dtype).name, len(P), rounds[k], ref["rounds"]))
        assert ref["converged"]
        assert rounds[k] == ref["rounds"]
        assert (asg[k] == ref["assignment"]).all() and (inv[k] == ref["inverse"]).all()
        assert emd[k] == ref["emd"]


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("squared", [True, False], ids=["sq", "l2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_optimality_bound_against_scipy(fixture, dtype, squared):
    """n in {1, 2, 64, 257, 1000}, eps = 1e-6, optima from the fixture: `bound` of the module docstring."""
    name = np.dtype(dtype).name
    cases = [("random", n, name, squared) for n in (1, 2, 64, 257, 1000)]
    pairs = [O.clouds("random", c[1], int(fixture[O.case_key(*c) + "/seed"]), dtype) for c in cases]
    emd, asg, inv, rounds = match(pairs, squared, 1e-6)
    for k, c in enumerate(cases):
        key = O.case_key(*c)
        assert O.checksum(*pairs[k]) == str(fixture[key + "/checksum"])
        print("rounds %s: %d" % (key, rounds[k]))
        bound(pairs[k][0], pairs[k][1], squared, 1e-6, emd[k], asg[k], inv[k], float(fixture[key + "/optimum"]), key)


# 3 ---------------------------------------------------------------------------------------------------------------
def test_exact_optimum_on_integer_costs(fixture):
    """Lattice clouds, squared cost, n = 300 and 1000, eps = 1 / (128 n): costs are multiples of 1/64 and n * eps < 1/64,
    so the matching is optimal and every sum is exact: the cost of pi equals scipy's total and n * emd equals it too,
    bit for bit."""
    cases = [("lattice", n, "float64", True) for n in (300, 1000)]
    for c in cases:   # one call each: eps differs
        key, n = O.case_key(*c), c[1]
        P, G = O.clouds("lattice", n, int(fixture[key + "/seed"]))
        assert O.checksum(P, G) == str(fixture[key + "/checksum"])
        emd, asg, inv, rounds = match([(P, G)], True, 1.0 / (128 * n))
        opt = float(fixture[key + "/optimum"])
        print("rounds %s: %d; n*emd %.17g opt %.17g" % (key, rounds[0], n * emd[0], opt))
        assert sorted(asg[0].tolist()) == list(range(n)) and (inv[0][asg[0]] == np.arange(n)).all()
        assert O.cost_matrix(P, G, True)[np.arange(n), asg[0]].sum() == opt
        assert n * emd[0] == opt


@pytest.mark.parametrize("squared", [True, False], ids=["sq", "l2"])
def test_a_permuted_copy_has_emd_exactly_zero(squared):
    rng = np.random.default_rng(3)
    pairs, eps = [], 1e-6
    for dtype in DTYPES:
        P = O.clouds("random", 257, 31, dtype)[0]
        pairs.append((P, P[rng.permutation(257)]))
    L = O.clouds("lattice", 300, 32)[0]   # coincident points among them: any matching of cost 0 will do
    pairs.append((L, L[rng.permutation(300)]))
    emd, asg, inv, rounds = match(pairs, squared, eps)
    print("rounds permuted copies:", rounds.tolist())
    for k, (P, G) in enumerate(pairs):
        assert emd[k] == 0.0 and (G[asg[k]] == P).all() and (inv[k][asg[k]] == np.arange(len(P))).all()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025, _native.DPC_EMD_MAX_POINTS])
def test_known_optimum_at_the_size_limit(n):
    """gt = (pred + t) shuffled, t = (0.05, -0.03, 0.02).  The identity is optimal in both modes: with the squared cost
    sum |x_i - x_s(i) - t|^2 = sum |x_i - x_s(i)|^2 + n |t|^2 (the cross term telescopes over a permutation), with the plain
    cost by the triangle inequality (sum of the vectors x_s(i) + t - x_i is n t).  So opt = n |t|^2 or n |t|; rounding
    pred + t to fp64 moves it by less than n u.  `bound` with eps = 1e-4."""
    rng = np.random.default_rng(n)
    P = O.clouds("random", n, 40 + n)[0]
    G = (P + T)[rng.permutation(n)]
    for squared in (True, False):
        emd, asg, inv, rounds = match([(P, G)], squared, 1e-4)
        print("rounds shift n %d %s: %d" % (n, "sq" if squared else "l2", rounds[0]))
        opt = n * (T @ T if squared else np.sqrt(T @ T))
        bound(P, G, squared, 1e-4, emd[0], asg[0], inv[0], opt, "shift n %d" % n)


def test_known_optimum_with_mixed_input_types():
    """The same construction with an fp32 prediction and an fp64 GT in one pair (gt = pred + t formed in fp64)."""
    n = 1025
    rng = np.random.default_rng(9)
    P32 = O.clouds("random", n, 77, np.float32)[0]
    G = (P32.astype(np.float64) + T)[rng.permutation(n)]
    emd, asg, inv, rounds = match([(P32, G)], True, 1e-4)
    bound(P32, G, True, 1e-4, emd[0], asg[0], inv[0], n * (T @ T), "mixed types")


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [8, 257])
def test_degenerate_inputs_terminate(n, dtype):
    """All pred points identical and all gt points identical: every cost is the same number c, every matching is optimal
    with total n c, and every bid of a round is a tie.  `bound` with eps = 1e-6, both modes."""
    P = np.tile(np.array([[0.25, -0.125, 0.0625]], dtype=dtype), (n, 1))
    G = np.tile(np.array([[-0.3, 0.2, 0.1]], dtype=dtype), (n, 1))
    for squared in (True, False):
        emd, asg, inv, rounds = match([(P, G)], squared, 1e-6)
        print("rounds degenerate n %d %s %s: %d" % (n, np.dtype(dtype).name, "sq" if squared else "l2", rounds[0]))
        c = O.cost_matrix(P[:1], G[:1], squared)[0, 0]
        bound(P, G, squared, 1e-6, emd[0], asg[0], inv[0], n * c, "degenerate n %d" % n)


def test_identical_bidders_terminate():
    """All pred points identical, gt random: every bidder wants the same object in every round, and every matching has the
    same total sum_j c(p, g_j), which is the optimum.  `bound` with eps = 1e-6, both modes."""
    n = 257
    P = np.tile(np.array([[0.25, -0.125, 0.0625]]), (n, 1))
    G = O.clouds("random", n, 55)[1]
    for squared in (True, False):
        emd, asg, inv, rounds = match([(P, G)], squared, 1e-6)
        print("rounds identical bidders n %d %s: %d" % (n, "sq" if squared else "l2", rounds[0]))
        bound(P, G, squared, 1e-6, emd[0], asg[0], inv[0], O.cost_matrix(P[:1], G, squared).sum(), "identical bidders")


# 6 ---------------------------------------------------------------------------------------------------------------
def test_round_cap():
    """n = 8, all pred points identical, max_rounds = 1: one round assigns one point, so the pair cannot converge.  Its emd
    is NaN, its unmatched entries are -1, its gradient is zero and the status bit is set; the other pairs of the call
    (one that converges in its single round, one that is cut off too) equal their results alone, bit for bit."""
    rng = np.random.default_rng(6)
    stuck = (np.zeros((8, 3)), rng.random((8, 3)) - 0.5)
    single = O.clouds("random", 1, 61)
    cut = O.clouds("random", 64, 62)
    R.check_status()   # clean slate
    preds = [dev(p).requires_grad_(True) for p, _ in (stuck, single, cut)]
    gts = [dev(g).requires_grad_(True) for _, g in (stuck, single, cut)]
    emd, asg, inv, rounds = R.emd_match(preds, gts, squared=True, eps=1e-6, max_rounds=1)
    (emd * dev(np.array([1.0, 2.0, 3.0]))).sum().backward()
    bits = R.check_status()
    assert bits & _native.DPC_STATUS_EMD_NOT_CONVERGED and not bits & ~_native.DPC_STATUS_EMD_NOT_CONVERGED
    assert R.check_status() == 0
    e = emd.detach().cpu().numpy()
    assert np.isnan(e[0]) and np.isnan(e[2]) and rounds.cpu().tolist() == [1, 1, 1]
    ref = O.emd(stuck[0], stuck[1], True, 1e-6, max_rounds=1)
    assert (asg[0].cpu().numpy() == ref["assignment"]).all() and (inv[0].cpu().numpy() == ref["inverse"]).all()
    assert (asg[0] >= 0).sum().item() == 1 and (asg[0] == -1).sum().item() == 7
    assert (preds[0].grad == 0).all() and (gts[0].grad == 0).all() and (preds[2].grad == 0).all()
    assert e[1] == O.emd(single[0], single[1], True, 1e-6)["emd"]
    assert gts[1].grad.abs().max().item() > 0 and (preds[1].grad == -gts[1].grad).all()
    for k, pair in enumerate((stuck, single, cut)):
        alone = match([pair], True, 1e-6, max_rounds=1)
        assert np.array_equal(alone[0], e[k:k + 1], equal_nan=True) and alone[3][0] == 1
        assert (alone[1][0] == asg[k].cpu().numpy()).all() and (alone[2][0] == inv[k].cpu().numpy()).all()
    assert R.check_status() == _native.DPC_STATUS_EMD_NOT_CONVERGED   # the runs alone flagged theirs; cleared again


# 7 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("squared", [True, False], ids=["sq", "l2"])
def test_reproducible_and_independent_of_batching(squared):
    """A ragged batch of fp32 and fp64 pairs: every output is the same bits in a second run, with the pairs in another
    order, and with one pair per call."""
    sizes = (1, 2, 63, 64, 65, 257, 300)
    pairs = [O.clouds("lattice" if n == 300 else "random", n, 70 + n, DTYPES[k % 2]) for k, n in enumerate(sizes)]

    def same(a, b, ka, kb):
        assert a[0][ka].tobytes() == b[0][kb].tobytes() and a[3][ka] == b[3][kb]
        assert (a[1][ka] == b[1][kb]).all() and (a[2][ka] == b[2][kb]).all()

    first, second = match(pairs, squared, 1e-6), match(pairs, squared, 1e-6)
    order = [4, 0, 6, 2, 5, 1, 3]
    shuffled = match([pairs[k] for k in order], squared, 1e-6)
    for k in range(len(pairs)):
        same(first, second, k, k)
        same(first, shuffled, k, order.index(k))
        same(first, match([pairs[k]], squared, 1e-6), k, 0)
    assert not np.isnan(first[0]).any()


# 8 ---------------------------------------------------------------------------------------------------------------
def closed_form(P, G, pi, up, squared):
    """(dpred, dgt) of up * emd on the matching pi, in extended precision."""
    P, G = P.astype(np.longdouble), G.astype(np.longdouble)
    n = len(P)
    diff = P - G[pi]
    if squared:
        c = 2 * diff / n * np.longdouble(up)
    else:
        d = np.sqrt((diff * diff).sum(axis=1, keepdims=True))
        c = np.where(d == 0, 0, diff / np.where(d == 0, 1, d) / n * np.longdouble(up))
    dgt = np.zeros_like(c)
    dgt[pi] = -c
    return c, dgt


@pytest.mark.parametrize("squared", [True, False], ids=["sq", "l2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_gradient_is_the_closed_form_on_the_device_matching(dtype, squared):
    """emd.sum().backward() and a random upstream vector, for pred and gt: `the gradient bound` of the module docstring."""
    rng = np.random.default_rng(8)
    sizes = (1, 64, 257)
    pairs = [O.clouds("random", n, 80 + n, dtype) for n in sizes] + [O.clouds("lattice", 65, 81, dtype)]
    for up in (np.ones(len(pairs)), rng.standard_normal(len(pairs))):
        preds = [dev(p).requires_grad_(True) for p, _ in pairs]
        gts = [dev(g).requires_grad_(True) for _, g in pairs]
        emd, asg = R.emd_loss(preds, gts, squared=squared, eps=1e-6, return_assignment=True)
        assert emd.requires_grad and not asg[0].requires_grad
        if (up == 1).all():
            emd.sum().backward()
        else:
            emd.backward(dev(up))
        worst = 0.0
        for k, (P, G) in enumerate(pairs):
            pi = asg[k].cpu().numpy()
            rp, rg = closed_form(P, G, pi, up[k], squared)
            for got, ref in ((preds[k].grad, rp), (gts[k].grad, rg)):
                assert got.dtype == preds[k].dtype and got.shape == preds[k].shape
                err = np.abs(got.cpu().numpy().astype(np.longdouble) - ref)
                assert (err <= 8 * U[dtype] * np.abs(ref)).all()
                worst = max(worst, float((err / np.maximum(np.abs(ref), 1e-300)).max() / U[dtype]))
        print("gradient %s %s: worst error %.2f u" % (np.dtype(dtype).name, "sq" if squared else "l2", worst))


@pytest.mark.parametrize("squared", [True, False], ids=["sq", "l2"])
def test_gradient_of_coincident_couples_and_of_inputs_without_grad(squared):
    rng = np.random.default_rng(5)
    P = O.clouds("random", 65, 90, np.float32)[0]
    pred, gt = dev(P).requires_grad_(True), dev(P[rng.permutation(65)]).requires_grad_(True)
    R.emd_loss([pred], [gt], squared=squared, eps=1e-6).sum().backward()
    assert (pred.grad == 0).all() and (gt.grad == 0).all()   # every couple coincides: exactly zero, not NaN
    P, G = O.clouds("random", 64, 91, np.float64)
    pred, gt = dev(P[None]).requires_grad_(True), dev(G[None])
    emd, asg = R.emd_loss(pred, gt, squared=squared, eps=1e-6, return_assignment=True)
    assert asg.shape == (1, 64) and asg.dtype == torch.int32
    emd.sum().backward()
    assert gt.grad is None and pred.grad.abs().max().item() > 0
    with torch.no_grad():
        assert not R.emd_loss(pred, gt, squared=squared, eps=1e-6).requires_grad


# 9 ---------------------------------------------------------------------------------------------------------------
def test_emd_of_split_equals_emd_loss_on_the_same_subsamples():
    """Three models, two views, a reference rotation, one model with truncated views."""
    from dpc.render._split import _host_unit_quaternion, _rotate

    rng = np.random.default_rng(12)
    M, V, N, K = 3, 2, 200, 128
    preds = [(rng.random((V, N, 3)).astype(np.float32) - 0.5, np.array([150, 200]) if m == 1 else None) for m in range(M)]
    gts = [rng.random((300 + m, 3)) - 0.5 for m in range(M)]
    q = np.array([[0.9, 0.1, -0.3, 0.2]])
    R.check_status()
    got = R.emd_of_split(preds, gts, reference_rotation=q, num_points=K, seed=4, eps=1e-6, models_per_call=2)
    assert got.shape == (M, V) and got.dtype == np.float64
    picks = R.emd.subsample_indices([(len(g), [N if nums is None else int(nums[i]) for i in range(V)])
                                     for (_, nums), g in zip(preds, gts)], K, 4)
    qn = _host_unit_quaternion(q)
    views, targets = [], []
    for m in range(M):
        rot = _rotate(torch.from_numpy(preds[m][0]), qn, torch.device("cuda"))
        for i in range(V):
            views.append(rot[i][dev(picks[m][1][i])])
            targets.append(dev(gts[m])[dev(picks[m][0])])
    want = R.emd_loss(views, targets, eps=1e-6).cpu().numpy().reshape(M, V)
    assert got.tobytes() == want.tobytes() and (got > 0).all()
    sq = R.emd_of_split(preds, gts, reference_rotation=q, num_points=K, seed=4, eps=1e-6, squared=True)
    assert sq.tobytes() == R.emd_loss(views, targets, eps=1e-6, squared=True).cpu().numpy().reshape(M, V).tobytes()
    with pytest.raises(RuntimeError, match="model 0, view 0 did not converge"):
        R.emd_of_split(preds, gts, num_points=K, eps=1e-6, max_rounds=2)
    assert R.check_status() == 0   # the split's failure was raised with names; the shared status word stays clean


# 10 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampling", ["random", "fps"])
def test_emd_of_split_does_not_depend_on_models_per_call(sampling):
    """Three models (the last group is short at 2 per call), two views of 24 points, one view truncated to 16, a rotation."""
    rng = np.random.default_rng(21)
    preds = [((rng.random((2, 24, 3)) * 0.6 - 0.3).astype(np.float32), np.array([24, 16]) if m == 1 else None) for m in range(3)]
    gts = [rng.random((20 + m, 3)) - 0.5 for m in range(3)]
    q = np.array([[0.9, 0.1, -0.3, 0.2]])
    got = [R.emd_of_split(preds, gts, reference_rotation=q, num_points=16, seed=3, eps=1e-6, models_per_call=step,
                          sampling=sampling) for step in (1, 2, 256)]
    assert got[0].shape == (3, 2) and got[0].dtype == np.float64 and (got[0] > 0).all()
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()
