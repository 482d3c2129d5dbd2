"""Host-side checks of the Earth Mover's Distance (no GPU): the numpy oracle of the auction (tests/emd_oracle.py) against
scipy's optima in the fixture and against brute force, the argument refusals of dpc_emd_fwd / emd_loss before any launch,
and the subsampling rule of emd_of_split."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import emd_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "f24_emd.npz")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def fixture():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def case_eps(kind, n):
    return 1.0 / (128 * n) if kind == "lattice" else 1e-6


@pytest.mark.parametrize("case", O.FIXTURE_CASES, ids=lambda c: O.case_key(*c))
def test_oracle_reaches_the_fixture_optimum_within_n_eps(fixture, case):
    """The clouds a seed regenerates are the ones scipy solved (checksum), and the oracle's matching is a permutation whose
    total is within n * eps of scipy's optimum (plus the slack of tests/test_emd_gpu.py for the two summations)."""
    kind, n, dt, squared = case
    key = O.case_key(*case)
    seed = int(fixture[key + "/seed"])
    assert seed == O.FIXTURE_CASES.index(case)
    P, G = O.clouds(kind, n, seed, np.dtype(dt))
    assert O.checksum(P, G) == str(fixture[key + "/checksum"])
    eps, opt = case_eps(kind, n), float(fixture[key + "/optimum"])
    C = O.cost_matrix(P, G, squared)
    assert C.max() == float(fixture[key + "/max_cost"])
    out = O.emd(P, G, squared, eps)
    assert out["converged"]
    assert sorted(out["assignment"]) == list(range(n))
    assert (out["inverse"][out["assignment"]] == np.arange(n)).all()
    slack = 64 * n * U * max(1.0, C.max())
    assert opt - slack <= out["total"] <= opt + n * eps + slack
    if kind == "lattice":   # costs are multiples of 1/64 and n * eps < 1/64: the auction's result is optimal, every sum exact
        assert out["total"] == opt and n * out["emd"] == opt


@pytest.mark.parametrize("squared", [True, False])
@pytest.mark.parametrize("kind", ["random", "lattice"])
def test_oracle_against_brute_force(kind, squared):
    """Every permutation for n <= 6: total <= best + n * eps, and equal to the best when eps is below the gap."""
    for n in range(1, 7):
        for seed in range(4):
            P, G = O.clouds(kind, n, 1000 + 10 * n + seed)
            C = O.cost_matrix(P, G, squared)
            totals = sorted(sum(C[i, s[i]] for i in range(n)) for s in itertools.permutations(range(n)))
            eps = 1e-9
            out = O.emd(P, G, squared, eps)
            assert out["converged"] and sorted(out["assignment"]) == list(range(n))
            assert totals[0] - 1e-14 <= out["total"] <= totals[0] + n * eps + 1e-14
            gap = next((t - totals[0] for t in totals if t - totals[0] > 1e-12), None)
            if gap is not None and gap > n * eps + 1e-12:
                assert abs(out["total"] - totals[0]) <= 1e-14


def test_oracle_round_cap_and_single_point():
    P = np.zeros((8, 3))
    G = O.clouds("random", 8, 5)[1]
    out = O.emd(P, G, True, 1e-6, max_rounds=1)   # identical bidders: one round assigns one of them
    assert not out["converged"] and out["rounds"] == 1 and np.isnan(out["emd"])
    assert (out["assignment"] >= 0).sum() == 1 and (out["inverse"] >= 0).sum() == 1
    one = O.emd(P[:1], G[:1], False, 1e-6, max_rounds=1)
    assert one["converged"] and one["rounds"] == 1 and one["assignment"][0] == 0


def _table(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 4))


def _dry(rows, n_pred, n_gt, eps=1e-6, max_rounds=100):
    from dpc.render import _native

    t = _table(rows)
    return _native.lib().dpc_emd_fwd(None, n_pred, None, n_gt, 0, None, t.ctypes.data_as(ctypes.c_void_p), len(t), 0, eps,
                                     max_rounds, None, None, None, None, None, None)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """dpc_emd_fwd and dpc_emd_bwd with the real host table and NULL device pointers: DPC_ERR_SHAPE for what the header
    lists, DPC_ERR_NULL (nothing launched) for a valid table."""
    from dpc.render import _native

    N, SHAPE, NUL = _native.DPC_EMD_MAX_POINTS, _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL
    assert _dry([(0, 5, 0, 5), (5, N, 5, N)], 5 + N, 5 + N) == NUL
    assert _dry([], 0, 0) == 0                                        # no pairs: nothing to do
    assert _dry([(0, 5, 0, 4)], 5, 5) == SHAPE                        # unequal sizes within a pair
    assert _dry([(0, 0, 0, 0)], 0, 0) == SHAPE                        # n = 0
    assert _dry([(0, N + 1, 0, N + 1)], N + 1, N + 1) == SHAPE        # beyond the limit
    assert _dry([(0, 5, 0, 5)], 4, 5) == SHAPE and _dry([(0, 5, 1, 5)], 5, 5) == SHAPE   # outside a buffer
    assert _dry([(-1, 5, 0, 5)], 5, 5) == SHAPE
    assert _dry([(0, 5, 0, 5), (4, 5, 5, 5)], 10, 10) == SHAPE        # overlapping ranges
    assert _dry([(5, 5, 5, 5), (0, 5, 0, 5)], 10, 10) == SHAPE        # descending ranges
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert _dry([(0, 5, 0, 5)], 5, 5, eps=eps) == SHAPE
    assert _dry([(0, 5, 0, 5)], 5, 5, max_rounds=0) == SHAPE
    L = _native.lib()
    t = _table([(0, 5, 0, 4)])
    assert L.dpc_emd_bwd(None, 5, None, 5, 0, None, t.ctypes.data_as(ctypes.c_void_p), 1, 0, *([None] * 7)) == SHAPE
    t = _table([(0, 5, 0, 5)])
    assert L.dpc_emd_bwd(None, 5, None, 5, 0, None, t.ctypes.data_as(ctypes.c_void_p), 1, 0, *([None] * 7)) == NUL


def test_limit_and_status_bit_match_the_header():
    from dpc.render import _native, emd

    header = open(os.path.join(ROOT, "include", "dpc_render.h")).read()
    assert "#define DPC_EMD_MAX_POINTS %d" % _native.DPC_EMD_MAX_POINTS in header
    assert int(re.search(r"DPC_STATUS_EMD_NOT_CONVERGED = (\d+)", header).group(1)) == _native.DPC_STATUS_EMD_NOT_CONVERGED
    bits = [int(v) for v in re.findall(r"DPC_STATUS_[A-Z_]+ = (\d+)", header)]
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 for b in bits)
    L = _native.lib()
    assert _native.DPC_EMD_MAX_POINTS >= 2048 and emd.MAX_POINTS == _native.DPC_EMD_MAX_POINTS
    assert 0 < L.dpc_emd_lds_bytes(_native.DPC_EMD_MAX_POINTS) <= 160 * 1024
    assert L.dpc_emd_lds_bytes(0) == 0 and L.dpc_emd_lds_bytes(_native.DPC_EMD_MAX_POINTS + 1) == 0
    assert L.dpc_emd_lds_bytes(1) % 8 == 0 and L.dpc_emd_lds_bytes(63) == L.dpc_emd_lds_bytes(64)


def test_emd_loss_names_the_offending_pair():
    """Every refusal comes before a device is looked for (this machine may have none), as ValueError naming the pair."""
    import dpc.render as R

    ok = np.zeros((4, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="pair 1 has 4 prediction points and 5 GT points"):
        R.emd_loss([ok, ok], [ok, np.zeros((5, 3), dtype=np.float32)], eps=1e-6)
    with pytest.raises(ValueError, match=r"pair 1 has %d points" % (R.emd.MAX_POINTS + 1)):
        big = np.zeros((R.emd.MAX_POINTS + 1, 3), dtype=np.float32)
        R.emd_loss([ok, big], [ok, big], eps=1e-6)
    with pytest.raises(ValueError, match="pair 0 is empty"):
        R.emd_loss([ok[:0]], [ok[:0]], eps=1e-6)
    with pytest.raises(ValueError, match=r"gts\[1\] must be \[n,3\]"):
        R.emd_loss([ok, ok], [ok, np.zeros((4, 2), dtype=np.float32)], eps=1e-6)
    with pytest.raises(ValueError, match=r"preds\[0\] must be \[n,3\]"):
        R.emd_match([np.zeros(3)], [ok], eps=1e-6)
    for eps in (0.0, -1e-6, float("nan")):
        with pytest.raises(ValueError, match="eps must be a positive finite cost"):
            R.emd_loss([ok], [ok], eps=eps)
    with pytest.raises(ValueError, match="max_rounds"):
        R.emd_loss([ok], [ok], eps=1e-6, max_rounds=0)
    with pytest.raises(ValueError, match="2 predictions and 1 GT clouds"):
        R.emd_loss([ok, ok], [ok], eps=1e-6)
    with pytest.raises(RuntimeError, match="MI355X only"):
        R.emd_loss(torch.zeros(2, 4, 3), torch.zeros(2, 4, 3), eps=1e-6)
    assert R.emd.default_max_rounds(100) == 100 * R.emd.ROUNDS_PER_POINT


def test_subsampling_rule_of_emd_of_split():
    """One default_rng(seed) for the split; per model the GT cloud's draw, then its views' draws in order."""
    import dpc.render as R

    counts = [(300, [200, 150]), (128, [128, 400]), (500, [129, 130])]
    got = R.emd.subsample_indices(counts, 128, 7)
    rng = np.random.default_rng(7)
    for (gn, views), (gi, vi) in zip(counts, got):
        assert (gi == rng.choice(gn, 128, replace=False)).all()
        for vn, idx in zip(views, vi):
            assert (idx == rng.choice(vn, 128, replace=False)).all()
            assert len(set(idx.tolist())) == 128 and idx.max() < vn
    assert (got[1][0] != np.arange(128)).any()   # a cloud of exactly num_points points is permuted, not copied
    with pytest.raises(ValueError, match="GT cloud of model 1 has 127 points"):
        R.emd.subsample_indices([(300, [200]), (127, [200])], 128, 0)
    with pytest.raises(ValueError, match="view 1 of model 2 has 100 points"):
        R.emd.subsample_indices([(300, [200, 200])] * 2 + [(300, [200, 100])], 128, 0)
    # the public call makes the same refusals before it looks for a device, truncation by num_points included
    pts = np.zeros((2, 200, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="view 1 of model 0 has 100 points"):
        R.emd_of_split([(pts, np.array([200, 100]))], [np.zeros((300, 3), dtype=np.float32)], num_points=128)
    with pytest.raises(ValueError, match="num_points must be in"):
        R.emd_of_split([(pts, None)], [np.zeros((300, 3), dtype=np.float32)], num_points=4096)
