"""The Chamfer loss on the GPU (csrc/dpc_chamfer_bwd.hip): the gradient of dpc_nearest_batched against the closed form of
tests/chamfer_grad_oracle.py on one ragged batch built to reach every edge of the kernels, against the reference's own
autograd (F19), run-to-run and batching independence, the squared mode's values and means, chamfer_loss and the
differentiable point_cloud_distance.

The bound of every gradient comparison, per component:  |got - ref| <= (n + 8) * u * sum |contribution|,  u = 2^-53 (fp64)
or 2^-24 (fp32), n the contributions the point receives: each term carries at most about 6 roundings (the difference, the
stored distance, the divide, the weight, the multiply) and a fixed-order sum of n terms adds (n - 1) u sum |c|.  The oracle
is fed the device's own idx (pinned by F11 / F16), so ties and near ties leave no case out."""
import json
import os

import numpy as np
import pytest
import torch

import dpc.render as R
from chamfer_grad_oracle import chamfer_grad, nearest_brute
from test_chamfer_loss_host import f19_problem, torch_loss, within

pytestmark = pytest.mark.gpu

U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
RATIOS = {}   # (dtype, mode) -> worst observed error / bound


def _cloud(rng, n, dtype):
    return (rng.random((n, 3)) - 0.5).astype(dtype)


def ragged(dtype):
    """Source counts 0, 1, 255, 256, 257, 700 (and 1000), target counts 1, 255, 256, 257, 1000; a one-point target (one
    700-long segment, across three source blocks); a 1000-point target of a single source (999 targets nobody chooses); an
    empty source; a GT shared by three views, both directions; a pair whose source and target are the same range (every
    d = 0); two lattice clouds (exact ties, some coincident points); ten points in no pair."""
    rng = np.random.default_rng(19)
    names = ["one", "a", "b", "c", "d", "g", "lat1", "lat2", "unused"]
    sizes = dict(one=1, a=255, b=256, c=257, d=700, g=1000, lat1=300, lat2=280, unused=10)
    clouds = {k: _cloud(rng, sizes[k], dtype) for k in names}
    for k in ("lat1", "lat2"):
        clouds[k] = (np.round(clouds[k] * 8) / 8).astype(dtype)
    start = dict(zip(names, np.cumsum([0] + [sizes[k] for k in names])))
    r = lambda k: (int(start[k]), sizes[k])
    pairs = [r("d") + r("one"), r("one") + r("g"), r("a") + r("b"), r("b") + r("a"), r("c") + r("g"), r("g") + r("c"),
             r("d") + r("c"), (int(start["a"]), 0) + r("a")]
    for v in ("a", "b", "d"):
        pairs += [r(v) + r("g"), r("g") + r(v)]
    pairs += [r("c") + r("c"), r("lat1") + r("lat2"), r("lat2") + r("lat1"), r("b") + r("c")]
    return np.concatenate([clouds[k] for k in names]), np.array(pairs, dtype=np.int64), start, sizes


def device_grad(pts_np, pairs, gm, gd, squared):
    """(grad of sum gm * mean + sum gd * value, mean, value, idx) from the device, as numpy."""
    pts = torch.from_numpy(pts_np).cuda().requires_grad_(True)
    mean, val, idx = R.nearest_batched(pts, pairs, return_distances=True, squared=squared)
    assert mean.requires_grad and val.requires_grad and not idx.requires_grad
    outs, grads = [], []
    if gm is not None:
        outs.append(mean)
        grads.append(torch.from_numpy(gm).cuda())
    if gd is not None:
        outs.append(val)
        grads.append(torch.from_numpy(gd).cuda())
    torch.autograd.backward(outs, grads)
    assert pts.grad.dtype == pts.dtype and pts.grad.shape == pts.shape
    return pts.grad.cpu().numpy(), mean.detach().cpu().numpy(), val.detach().cpu().numpy(), idx.cpu().numpy()


@pytest.fixture(scope="module")
def batches():
    return {dt: ragged(dt) for dt in (np.float32, np.float64)}


@pytest.mark.parametrize("which", ["gmean", "gdist", "both"])
@pytest.mark.parametrize("squared", [False, True], ids=["distance", "squared"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_gradient_vs_closed_form(batches, dtype, squared, which):
    pts, pairs, start, sizes = batches[dtype]
    rng = np.random.default_rng(23)
    gm = rng.standard_normal(len(pairs)) if which != "gdist" else None
    gd = rng.standard_normal(int(pairs[:, 1].sum())).astype(dtype) if which != "gmean" else None
    got, mean, val, idx = device_grad(pts, pairs, gm, gd, squared)
    # the forward: what it is without a gradient, the squares rounded once, their means in numpy's order
    plain = R.nearest_batched(torch.from_numpy(pts).cuda(), pairs, return_distances=True)
    dist = plain[1].cpu().numpy()
    assert np.array_equal(idx, plain[2].cpu().numpy())
    assert val.tobytes() == ((dist * dist) if squared else dist).tobytes()
    o = 0
    for p, (s0, ns, t0, nt) in enumerate(pairs):
        want = np.mean(val[o:o + ns].astype(np.float64)) if ns else np.nan
        assert np.float64(mean[p]).tobytes() == np.float64(want).tobytes() or (ns == 0 and np.isnan(mean[p])), p
        o += ns
    ref, abs_sum, count = chamfer_grad(pts, pairs, idx, gm, gd, squared)
    ratio = within(got, ref, abs_sum, count, U[dtype])
    key = "%s %s" % ("f32" if dtype == np.float32 else "f64", "squared" if squared else "distance")
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    u0 = int(start["unused"])
    assert (got[u0:u0 + sizes["unused"]] == 0).all()         # points in no pair: written, and zero


@pytest.mark.parametrize("squared", [False, True], ids=["distance", "squared"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_coincident_points_give_exact_finite_zeros(batches, dtype, squared):
    """A cloud against itself: every d = 0.  The reference's autograd gives NaN; here every gradient is exactly zero."""
    pts, _, start, sizes = batches[dtype]
    c0, n = int(start["c"]), sizes["c"]
    rng = np.random.default_rng(29)
    got, mean, val, idx = device_grad(pts, np.array([[c0, n, c0, n]]), rng.standard_normal(1),
                                      rng.standard_normal(n).astype(dtype), squared)
    assert (val == 0).all() and mean[0] == 0 and np.array_equal(idx, np.arange(n))
    assert np.isfinite(got).all() and (got == 0).all()


def test_empty_source_pair():
    rng = np.random.default_rng(31)
    pts = _cloud(rng, 300, np.float64)
    got, mean, val, idx = device_grad(pts, np.array([[0, 0, 0, 300], [0, 40, 40, 260]]), np.array([2.0, 0.0]), None, False)
    assert np.isnan(mean[0]) and len(val) == 40
    assert (got == 0).all()


def test_f19_reference_autograd(golden):
    f19 = golden("f19_chamfer_grad.npz")
    pts, pairs, ref = f19_problem(f19)
    got, mean, val, idx = device_grad(pts, pairs, f19["a"], f19["b"], False)
    assert np.array_equal(idx, f19["idx"])
    assert np.allclose(val, f19["min_dist"], rtol=4 * U[np.float64], atol=0)
    _, abs_sum, count = chamfer_grad(pts, pairs, idx, f19["a"], f19["b"])
    within(got, ref, abs_sum, count, U[np.float64])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_reproducible_and_independent_of_the_other_pairs(batches, dtype):
    pts, pairs, start, sizes = batches[dtype]
    rng = np.random.default_rng(37)
    gm = rng.standard_normal(len(pairs))
    gd = rng.standard_normal(int(pairs[:, 1].sum())).astype(dtype)
    first = device_grad(pts, pairs, gm, gd, False)[0]
    again = device_grad(pts, pairs, gm, gd, False)[0]
    assert first.tobytes() == again.tobytes()
    # pair 5 (g -> c, 1000 sources over four blocks, shared targets) alone, and inside the batch with zero upstream
    # gradient for every other pair: the other pairs add exact zeros
    k = 5
    o = int(pairs[:k, 1].sum())
    n = int(pairs[k, 1])
    alone = device_grad(pts, pairs[k:k + 1], gm[k:k + 1], gd[o:o + n], False)[0]
    gm0, gd0 = np.zeros_like(gm), np.zeros_like(gd)
    gm0[k], gd0[o:o + n] = gm[k], gd[o:o + n]
    inside = device_grad(pts, pairs, gm0, gd0, False)[0]
    assert np.array_equal(alone, inside)
    assert (alone != 0).any()


def test_backward_runs_the_native_kernels():
    from dpc.render import _native

    rng = np.random.default_rng(41)
    pts = torch.from_numpy(_cloud(rng, 600, np.float32)).cuda().requires_grad_(True)
    ids = _native.launched_instantiations(lambda: R.nearest_batched(pts, [[0, 300, 300, 300]]).sum().backward(),
                                          torch.device("cuda"))
    for k in ("k_chamfer_bwd_scan", "k_chamfer_bwd_terms", "k_chamfer_bwd_targets", "k_chamfer_bwd_gather"):
        assert any(i.startswith(k) for i in ids), (k, sorted(ids))


def test_backward_in_a_replayed_graph(batches):
    """dpc_nearest_batched_bwd makes no host synchronisation and no host -> device copy: captured into a HIP graph and
    replayed on new upstream gradients it gives the eager call's bits."""
    import ctypes

    from dpc.render import _native as N

    pts_np, pairs, _, _ = batches[np.float32]
    d = torch.device("cuda")
    pts = torch.from_numpy(pts_np).to(d)
    _, dist, idx = R.nearest_batched(pts, pairs, return_distances=True)
    desc = np.ascontiguousarray(pairs, dtype=np.int32)
    host = desc.ctypes.data_as(ctypes.c_void_p)
    desc_d = torch.from_numpy(desc).to(d)
    P, n = len(desc), len(pts_np)
    L = N.lib()
    ws = torch.empty((L.dpc_chamfer_bwd_workspace_bytes(P, host, 0),), dtype=torch.uint8, device=d)
    gm = torch.zeros((P,), dtype=torch.float64, device=d)
    gd = torch.zeros((dist.shape[0],), dtype=torch.float32, device=d)
    out = torch.empty_like(pts)

    def call():
        return L.dpc_nearest_batched_bwd(N.ptr(pts), n, 0, N.ptr(desc_d), host, P, N.ptr(dist), N.ptr(idx), N.ptr(gm), N.ptr(gd),
                                         0, N.ptr(out), N.ptr(ws), N.stream_ptr(d))

    assert call() == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert call() == 0
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        gm.copy_(torch.from_numpy(rng.standard_normal(P)))
        gd.copy_(torch.from_numpy(rng.standard_normal(dist.shape[0]).astype(np.float32)))
        g.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        out.zero_()
        assert call() == 0
        torch.cuda.synchronize()
        assert torch.equal(replayed, out) and bool((out != 0).any())


def _separated(rng):
    """5 predictions, each 0.2 - 0.3 from its own one of 7 GT points that are 1 apart (no nearest neighbour changes under a
    finite-difference step)."""
    gt = np.array([[i, 0.0, 0.0] for i in range(7)]) + 0.02 * rng.standard_normal((7, 3))
    dirs = rng.standard_normal((5, 3))
    pred = gt[[5, 0, 3, 3, 6]] + np.array([[0.3], [0.3], [0.3], [0.2], [0.3]]) * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    return pred, gt


@pytest.mark.parametrize("squared", [False, True], ids=["distance", "squared"])
def test_chamfer_loss_gradcheck(squared):
    pred, gt = _separated(np.random.default_rng(7))
    p = torch.from_numpy(pred).cuda().requires_grad_(True)
    g = torch.from_numpy(gt).cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: R.chamfer_loss([a], [b], squared=squared), (p, g))


@pytest.mark.parametrize("squared", [False, True], ids=["distance", "squared"])
def test_chamfer_loss_reaches_every_input(squared):
    """Three views in one [3,N,3] tensor sharing GT 0, and a list-style fourth prediction with a GT of its own: gradients
    reach the tensor, the list entry and both GT clouds, and the shared GT's gradient sums over its views."""
    rng = np.random.default_rng(43)
    views = torch.from_numpy(rng.random((3, 200, 3)) - 0.5).cuda().requires_grad_(True)
    extra = torch.from_numpy(rng.random((130, 3)) - 0.5).cuda().requires_grad_(True)
    gt0 = torch.from_numpy(rng.random((300, 3)) - 0.5).cuda().requires_grad_(True)
    gt1 = torch.from_numpy(rng.random((90, 3)) - 0.5).cuda().requires_grad_(True)
    w = rng.standard_normal((4, 2))
    shared = R.chamfer_loss(views, [gt0], gt_of=[0, 0, 0], squared=squared)
    own = R.chamfer_loss([extra], [gt1], squared=squared)
    assert shared.shape == (3, 2) and own.shape == (1, 2) and shared.dtype == torch.float64
    ((torch.cat([shared, own]) * torch.from_numpy(w).cuda()).sum()).backward()
    if not squared:
        plain = R.chamfer_batched(list(views.detach()), [gt0.detach()], gt_of=[0, 0, 0])
        assert torch.equal(plain, shared.detach())
    # the same problem for the oracle: one packed buffer, pairs (view -> gt0, gt0 -> view) and (extra -> gt1, gt1 -> extra)
    clouds = [gt0, gt1, views[0], views[1], views[2], extra]
    pts = np.concatenate([c.detach().cpu().numpy() for c in clouds])
    st = np.cumsum([0] + [len(c) for c in clouds])
    pairs = []
    for v in range(3):
        pairs += [(st[2 + v], 200, 0, 300), (0, 300, st[2 + v], 200)]
    pairs += [(st[5], 130, st[1], 90), (st[1], 90, st[5], 130)]
    pairs = np.array(pairs)
    _, idx = nearest_brute(pts, pairs)
    ref, abs_sum, count = chamfer_grad(pts, pairs, idx, w.reshape(-1), None, squared)
    got = np.concatenate([gt0.grad.cpu().numpy(), gt1.grad.cpu().numpy(), views.grad.cpu().numpy().reshape(-1, 3),
                          extra.grad.cpu().numpy()])
    within(got, ref, abs_sum, count, U[np.float64])
    assert count[:300].min() >= 3         # every point of the shared GT is a source in each of its three views' pairs


def test_chamfer_loss_mixed_precision_rows_keep_their_order():
    """fp32-only pairs and fp64 pairs go through two native calls; the rows come back in the order of preds, each equal to
    chamfer_batched's, and every gradient arrives in its input's dtype."""
    rng = np.random.default_rng(47)
    preds = [torch.from_numpy(_cloud(rng, 100, dt)).cuda().requires_grad_(True) for dt in (np.float64, np.float32, np.float64)]
    gts = [torch.from_numpy(_cloud(rng, 150, dt)).cuda().requires_grad_(True) for dt in (np.float32, np.float32, np.float64)]
    out = R.chamfer_loss(preds, gts)
    assert torch.equal(out.detach(), R.chamfer_batched([p.detach() for p in preds], [g.detach() for g in gts]))
    out.sum().backward()
    for t in preds + gts:
        assert t.grad is not None and t.grad.dtype == t.dtype and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any())


def test_point_cloud_distance_differentiates():
    rng = np.random.default_rng(53)
    vs_np, vt_np = _cloud(rng, 50, np.float64), _cloud(rng, 60, np.float64)
    b = rng.standard_normal(50)
    vs = torch.from_numpy(vs_np).cuda().requires_grad_(True)
    vt = torch.from_numpy(vt_np).cuda().requires_grad_(True)
    proj, dist, idx = R.point_cloud_distance(vs, vt)
    assert proj.requires_grad and dist.requires_grad and not idx.requires_grad
    detached = R.point_cloud_distance(vs.detach(), vt.detach())
    assert not detached[0].requires_grad and not detached[1].requires_grad
    for x, y in zip((proj, dist, idx), detached):       # the values are what they are without a gradient
        assert x.dtype == y.dtype and x.detach().cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
    ((dist * torch.from_numpy(b).cuda()).sum() + 0.3 * proj.sum()).backward()
    # the reference's formulation in CPU torch
    cs, ct = torch.from_numpy(vs_np).requires_grad_(True), torch.from_numpy(vt_np).requires_grad_(True)
    d = torch.sqrt(((ct[None] - cs[:, None]) ** 2).sum(2))
    j = torch.argmin(d, dim=1)
    assert np.array_equal(j.numpy(), idx.cpu().numpy())
    ((d[torch.arange(50), j] * torch.from_numpy(b)).sum() + 0.3 * ct[j].sum()).backward()
    # bound: the distance terms as everywhere, plus 0.3 per choosing source on the targets (proj's adjoint)
    pts = np.concatenate([vt_np, vs_np])
    _, abs_sum, count = chamfer_grad(pts, [[60, 50, 0, 60]], j.numpy(), None, b)
    chosen = np.bincount(j.numpy(), minlength=60)
    abs_sum[:60] += 0.3 * chosen[:, None]
    count[:60] += chosen
    got = np.concatenate([vt.grad.cpu().numpy(), vs.grad.cpu().numpy()])
    within(got, np.concatenate([ct.grad.numpy(), cs.grad.numpy()]), abs_sum, count, U[np.float64])


def test_bad_table_raises_before_any_launch():
    from dpc.render import _native

    pts = torch.zeros(10, 3, device="cuda", requires_grad=True)
    for bad in ([[0, 5, 5, 0]], [[0, 5, 6, 5]], [[-1, 5, 5, 5]]):
        ids = set()

        def call():
            with pytest.raises(ValueError):
                R.nearest_batched(pts, bad)

        ids = _native.launched_instantiations(call, torch.device("cuda"))
        assert not ids, sorted(ids)
    with pytest.raises(ValueError):
        R.chamfer_loss([pts], [torch.zeros(0, 3, device="cuda")])


def test_zz_parity_report():
    """Not a check: writes the worst observed error / bound ratio per dtype and mode (profiles/chamfer_loss_parity.json,
    or the file DPC_CHAMFER_LOSS_PARITY names)."""
    assert len(RATIOS) == 4 and all(0.0 <= r <= 1.0 for r in RATIOS.values()), RATIOS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.environ.get("DPC_CHAMFER_LOSS_PARITY") or os.path.join(root, "profiles", "chamfer_loss_parity.json")
    with open(path, "w") as fh:
        json.dump({"bound": "(n + 8) * u * sum |contribution| per component, u = 2^-24 (f32) / 2^-53 (f64)",
                   "worst_error_over_bound": dict(sorted(RATIOS.items()))}, fh, indent=1)
        fh.write("\n")
