"""The Earth Mover's Distance between point clouds of equal size, batched on the GPU: metric, loss and gradient.

The EMD of two clouds of n points is the mean cost of the cheapest one-to-one matching between them.  Where Chamfer
(dpc/render/chamfer.py) lets every point pick its nearest neighbour, EMD makes the clouds pay for uneven density and
collapsed regions.  The reference has no EMD; the exact answer is scipy.optimize.linear_sum_assignment on the host, one
pair at a time, cubic in n and without a gradient.  Here all pairs of a call go into one launch (csrc/dpc_emd.hip: one
workgroup per pair, a deterministic auction with eps-scaling held in LDS), and the result is within a chosen eps of the
optimum, bit-reproducible, and differentiable.

    emd_match     the metric with everything the matching produced: (emd [P], assignments, inverses, rounds [P])
    emd_loss      emd [P] as a differentiable loss (dpc_emd_bwd), optionally with the assignments
    emd_of_split  the [M,V] table of a split, next to chamfer_of_split; clouds are brought to a common size by a seeded
                  random draw, or by farthest-point sampling on the device (dpc/render/sampling.py)

The schedule, the tie rules and the summation order are in include/dpc_render.h (dpc_emd_fwd).
"""
import numpy as np
import torch

from . import _batch, _native, _split
from . import sampling as _sampling
from ._ops import status_word

_WHAT = "dpc.render EMD"
MAX_POINTS = _native.DPC_EMD_MAX_POINTS
DEFAULT_EPS = 1e-6
ROUNDS_PER_POINT = 1024


def default_max_rounds(n):
    """The round cap emd_loss / emd_match use when none is given, for a call whose largest pair has n points:
    ROUNDS_PER_POINT * n.  The most any measured input needed was 36 rounds per point (profiles/LAB_NOTES.md, section 15)."""
    return ROUNDS_PER_POINT * max(int(n), 1)


def _clouds(x, what, fn):
    """x as a list of [n,3] float32 / float64 tensors that keep their autograd history: a [B,n,3] tensor gives its B
    rows, a list gives its entries (arrays wrapped; other dtypes converted to float32)."""
    if isinstance(x, torch.Tensor) and x.dim() == 3:
        x = x.unbind(0)
    out = []
    for i, c in enumerate(x):
        t = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c))
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("%s: %s[%d] must be [n,3], got %s" % (fn, what, i, tuple(t.shape)))
        out.append(t if t.dtype in (torch.float32, torch.float64) else t.to(torch.float32))
    return out


def _check(preds, gts, eps, max_rounds, fn):
    """The argument checks of a call, before anything touches a device: the pair lists, eps and max_rounds as
    (P_list, G_list, host table, eps, max_rounds).  Every refusal the native entry point makes is made here first with
    the pair's index in the message; the entry point's own dry run follows."""
    P_list, G_list = _clouds(preds, "preds", fn), _clouds(gts, "gts", fn)
    if len(P_list) != len(G_list):
        raise ValueError("%s: %d predictions and %d GT clouds" % (fn, len(P_list), len(G_list)))
    eps = DEFAULT_EPS if eps is None else float(eps)
    if not (eps > 0.0 and np.isfinite(eps)):
        raise ValueError("%s: eps must be a positive finite cost, got %r" % (fn, eps))
    for i, (p, g) in enumerate(zip(P_list, G_list)):
        if len(p) != len(g):
            raise ValueError("%s: pair %d has %d prediction points and %d GT points; EMD matches clouds of equal size "
                             "one to one" % (fn, i, len(p), len(g)))
        if len(p) == 0:
            raise ValueError("%s: pair %d is empty (n = 0)" % (fn, i))
        if len(p) > MAX_POINTS:
            raise ValueError("%s: pair %d has %d points, the limit is DPC_EMD_MAX_POINTS = %d (a pair lives in one CU's "
                             "LDS)" % (fn, i, len(p), MAX_POINTS))
    counts = [len(p) for p in P_list]
    if max_rounds is None:
        max_rounds = default_max_rounds(max(counts, default=1))
    if int(max_rounds) != max_rounds or not 1 <= int(max_rounds) <= _batch.INT32_MAX:
        raise ValueError("%s: max_rounds must be an integer in [1, 2^31 - 1], got %r" % (fn, max_rounds))
    start = np.cumsum([0] + counts)
    if start[-1] > _batch.INT32_MAX:
        raise ValueError("%s: more than 2^31 - 1 points in one call" % fn)
    desc = _batch.table([(start[i], counts[i], start[i], counts[i]) for i in range(len(counts))], 4,
                        "%s: pair table entries must fit int32" % fn)
    total = int(start[-1])
    rc = _native.lib().dpc_emd_fwd(None, total, None, total, 0, None, desc.ctypes.data, len(counts), 0,
                                   eps, int(max_rounds), None, None, None, None, None, None)
    _batch.dry_run(rc, "%s: dpc_emd_fwd refused the pair table" % fn)
    return P_list, G_list, desc, eps, int(max_rounds)


def _forward(pred, gt, desc, squared, eps, max_rounds, status):
    """One dpc_emd_fwd call on the packed clouds: (emd [P] float64, assignment [N] int32, inverse [N] int32,
    rounds [P] int32, the device table)."""
    dev, P, total = pred.device, desc.shape[0], int(pred.shape[0])
    emd = torch.empty((P,), dtype=torch.float64, device=dev)
    assignment = torch.empty((total,), dtype=torch.int32, device=dev)
    inverse = torch.empty((total,), dtype=torch.int32, device=dev)
    rounds = torch.empty((P,), dtype=torch.int32, device=dev)
    desc_d = None
    if P:
        desc_d = _batch.on_device(desc, dev)
        _native.call(dev, "dpc_emd_fwd", _native.ptr(pred), total, _native.ptr(gt), total, int(pred.dtype == torch.float64),
                     _native.ptr(desc_d), desc.ctypes.data, P, int(squared), eps, max_rounds, _native.ptr(emd),
                     _native.ptr(assignment), _native.ptr(inverse), _native.ptr(rounds), _native.ptr(status))
    return emd, assignment, inverse, rounds, desc_d


class _Emd(torch.autograd.Function):
    """dpc_emd_fwd with a gradient: the forward keeps the packed clouds and its own matching, the backward is one
    dpc_emd_bwd call."""

    @staticmethod
    def forward(ctx, pred, gt, desc, squared, eps, max_rounds, status):
        p, g = pred.detach().contiguous(), gt.detach().contiguous()
        emd, assignment, inverse, rounds, desc_d = _forward(p, g, desc, squared, eps, max_rounds, status)
        ctx.save_for_backward(p, g, emd, assignment, inverse)
        ctx.desc, ctx.desc_d, ctx.squared = desc, desc_d, bool(squared)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(assignment, inverse, rounds)
        return emd, assignment, inverse, rounds

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gemd, _ga, _gi, _gr):
        p, g, emd, assignment, inverse = ctx.saved_tensors
        want_p, want_g = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        desc, dev, P, total = ctx.desc, p.device, ctx.desc.shape[0], int(p.shape[0])
        if gemd is None or P == 0:
            return (torch.zeros_like(p) if want_p else None, torch.zeros_like(g) if want_g else None) + (None,) * 5
        gemd = gemd.to(device=dev, dtype=torch.float64).contiguous()
        dpred = torch.empty_like(p) if want_p else None
        dgt = torch.empty_like(g) if want_g else None
        _native.call(dev, "dpc_emd_bwd", _native.ptr(p), total, _native.ptr(g), total, int(p.dtype == torch.float64),
                     _native.ptr(ctx.desc_d), desc.ctypes.data, P, int(ctx.squared), _native.ptr(emd), _native.ptr(assignment),
                     _native.ptr(inverse), _native.ptr(gemd), _native.ptr(dpred), _native.ptr(dgt))
        return (dpred, dgt) + (None,) * 5


def _run(preds, gts, squared, eps, max_rounds, fn, status=None):
    P_list, G_list, desc, eps, max_rounds = _check(preds, gts, eps, max_rounds, fn)
    _batch.refuse_cpu(preds, gts)
    dev = _batch.device(_WHAT, P_list, G_list)
    counts = [len(p) for p in P_list]
    if not counts:
        empty = torch.empty((0,), dtype=torch.float64, device=dev)
        return empty, [], [], torch.empty((0,), dtype=torch.int32, device=dev)
    dtype = _batch.widest(P_list + G_list)    # one fp64 pair makes the whole call fp64 without changing a bit
    pred = torch.cat([c.to(device=dev, dtype=dtype) for c in P_list])
    gt = torch.cat([c.to(device=dev, dtype=dtype) for c in G_list])
    status = status_word(dev) if status is None else status
    emd, assignment, inverse, rounds = _Emd.apply(pred, gt, desc, bool(squared), eps, max_rounds, status)
    return emd, list(assignment.split(counts)), list(inverse.split(counts)), rounds


def emd_match(preds, gts, squared=False, eps=None, max_rounds=None):
    """emd_loss with everything the matching produced: (emd [P] float64, assignments, inverses, rounds [P] int32), all
    on the device.  assignments[p][i] is the gt point matched to prediction point i of pair p, inverses[p][j] the
    prediction point matched to gt point j (int32; -1 where a pair that did not converge left a point unmatched),
    rounds[p] the bidding rounds the pair ran.  Arguments, refusals and gradient as emd_loss."""
    return _run(preds, gts, squared, eps, max_rounds, "emd_match")


def emd_loss(preds, gts, squared=False, eps=None, max_rounds=None, return_assignment=False):
    """The Earth Mover's Distance of P pairs of clouds: emd[p] = mean_i c(pred_p[i], gt_p[pi(i)]) for a one-to-one
    matching pi whose total cost is within n_p * eps of the optimum, [P] float64 on the device, carrying gradient to
    every prediction and GT cloud that requires it.  With return_assignment: (emd, assignments), assignments[p] the
    [n_p] int32 indices pi (a list, or a [B,n] tensor when preds was a [B,n,3] tensor).

    preds, gts: [B,n,3] tensors, or lists of [n_p,3] tensors or arrays; sizes may differ between pairs, not within one,
    and 1 <= n_p <= DPC_EMD_MAX_POINTS (2048).  c is the distance, or with squared the squared distance, evaluated in
    fp64 whatever the input dtype.  eps, in cost units, bounds the excess of emd over the optimal mean; default 1e-6.
    Smaller values cost rounds (about log5(cost range / eps) phases), and an eps below 1 / n_p of the smallest
    difference between two matchings' totals makes the result exactly optimal.  max_rounds: the cap on a pair's bidding
    rounds, default 1024 * the call's largest n_p (default_max_rounds; more than twenty times what any measured input
    needed).  A pair that reaches it has emd NaN, a zero gradient and -1 for its unmatched points, and sets
    DPC_STATUS_EMD_NOT_CONVERGED in the device status word, which check_status() returns; the other pairs are
    unaffected.  NaN coordinates end the same way.

    The matching is a deterministic auction (include/dpc_render.h, dpc_emd_fwd): results are bit-identical from run to
    run and do not depend on which pairs share a call.  The gradient is that of the matching found: (p - g) / (|p - g| n),
    or 2 (p - g) / n with squared, and exactly zero for a coincident couple (chamfer_loss's rule).  No host
    synchronisation.  ValueError, before anything is launched and naming the pair, for unequal sizes within a pair, an
    empty pair, more than DPC_EMD_MAX_POINTS points, a shape that is not [n,3], and eps <= 0; CPU tensors are refused."""
    emd, assignments, _, _ = _run(preds, gts, squared, eps, max_rounds, "emd_loss")
    if not return_assignment:
        return emd
    if isinstance(preds, torch.Tensor) and preds.dim() == 3 and assignments:
        return emd, torch.stack(assignments)
    return emd, assignments


def subsample_indices(counts, num_points, seed):
    """The subsampling rule of emd_of_split: one np.random.default_rng(seed) for the whole split, and for model m in
    order first its GT cloud, then its views 0 .. V-1, each drawing rng.choice(count, num_points, replace=False).
    counts: per model (gt_count, [view counts]).  Returns per model (gt_idx, [view_idx ...]), int64 arrays in the drawn
    order.  ValueError naming the model when a cloud has fewer than num_points points."""
    rng = np.random.default_rng(seed)
    out = []
    for m, (gn, views) in enumerate(counts):
        if gn < num_points:
            raise ValueError("emd_of_split: GT cloud of model %d has %d points, fewer than num_points = %d" % (m, gn, num_points))
        for v, vn in enumerate(views):
            if vn < num_points:
                raise ValueError("emd_of_split: view %d of model %d has %d points, fewer than num_points = %d"
                                 % (v, m, vn, num_points))
        out.append((rng.choice(gn, num_points, replace=False), [rng.choice(vn, num_points, replace=False) for vn in views]))
    return out


def _fps_counts(counts, num_points):
    """The refusals of emd_of_split(sampling="fps") for counts as subsample_indices takes them: ValueError naming the
    model for a cloud with fewer than num_points points or more than DPC_FPS_MAX_POINTS."""
    for m, (gn, views) in enumerate(counts):
        for what, n in [("GT cloud of model %d" % m, gn)] + [("view %d of model %d" % (v, m), vn) for v, vn in enumerate(views)]:
            if n < num_points:
                raise ValueError("emd_of_split: %s has %d points, fewer than num_points = %d" % (what, n, num_points))
            if n > _sampling.MAX_POINTS:
                raise ValueError("emd_of_split: %s has %d points, sampling=\"fps\" takes at most DPC_FPS_MAX_POINTS = %d"
                                 % (what, n, _sampling.MAX_POINTS))


def emd_of_split(predictions, gt_clouds, reference_rotation=None, num_points=1024, seed=0, squared=False, eps=None,
                 max_rounds=None, models_per_call=64, sampling="random"):
    """The EMD table of a split, [M,V] float64 numpy: every view's prediction against its model's GT cloud, next to
    chamfer_of_split and with its arguments: predictions per model (points [V,N,3], num_points [V] | None) or
    load_predictions' triples, view i truncated to its first num_points[i] points; gt_clouds per model [n,3];
    reference_rotation a [1,4] quaternion applied to every view first.

    EMD needs clouds of equal size, so each view (after truncation and rotation) and each model's GT cloud are
    subsampled to num_points points without replacement by subsample_indices(…, num_points, seed): one generator for
    the split; per model the GT cloud first, then its views in order.  The result does not depend on models_per_call.
    A cloud with fewer than num_points points raises ValueError naming the model; a pair that did not converge (or
    holds a NaN coordinate) raises RuntimeError naming model and view.  squared, eps, max_rounds as emd_loss.

    sampling="fps" replaces the random draw by farthest-point sampling on the device (farthest_point_sample with
    first = 0): each model's GT cloud once, and each of its views after truncation and rotation.  The subsample is
    deterministic and covers the cloud evenly; seed is ignored.  A cloud with more than DPC_FPS_MAX_POINTS points raises
    ValueError naming the model, a cloud with a NaN or infinite coordinate RuntimeError naming it.  Any other value of
    sampling raises ValueError."""
    split = _split.Split("emd_of_split", predictions, gt_clouds, reference_rotation, models_per_call)
    num_points = int(num_points)
    if not 1 <= num_points <= MAX_POINTS:
        raise ValueError("emd_of_split: num_points must be in [1, DPC_EMD_MAX_POINTS = %d], got %d" % (MAX_POINTS, num_points))
    counts = [(len(g), n) for g, n in zip(split.gts, split.counts)]
    if sampling not in ("random", "fps"):
        raise ValueError("emd_of_split: sampling must be \"random\" or \"fps\", got %r" % (sampling,))
    fps = sampling == "fps"
    if fps:
        _fps_counts(counts, num_points)
    else:
        picks = subsample_indices(counts, num_points, seed)
    V = split.V
    out = np.zeros((split.M, V), dtype=np.float64)
    if split.empty:
        return out
    dev = _batch.device(_WHAT, *split.tensors())
    status = torch.zeros(1, dtype=torch.int32, device=dev)  # its own word: the failure is raised here, with names
    for group in split.groups:
        a = group[0]
        view_list, gt_list = [], []
        for m in group:
            views = split.model(m, dev, on_device=True)
            g = split.gts[m].to(dev)
            if fps:
                view_list.extend(views)
                gt_list.append(g)
                continue
            g = g[torch.from_numpy(picks[m][0]).to(dev)]
            for v, idx in zip(views, picks[m][1]):
                view_list.append(v[torch.from_numpy(idx).to(dev)])
                gt_list.append(g)
        if fps:   # one call for the group's GT clouds, one for its views; the full clouds give way to their samples
            g_idx = _sampling._sample(gt_list, num_points, 0, status)[0]
            v_idx = _sampling._sample(view_list, num_points, 0, status)[0]
            sampled = torch.stack([i[0] for i in g_idx + v_idx])   # -1: that cloud holds a non-finite coordinate
            gt_list = [g[i.long()] for g, i in zip(gt_list, g_idx) for _ in range(V)]
            view_list = [v[i.long()] for v, i in zip(view_list, v_idx)]
        with torch.no_grad():
            emd = _run(view_list, gt_list, squared, eps, max_rounds, "emd_of_split", status)[0]
        res = split.store(out, group, emd)
        if fps and bool((sampled < 0).any()):
            k = int(np.argmax(sampled.cpu().numpy() < 0))
            G = len(group)
            what = "GT cloud of model %d" % (a + k) if k < G else "view %d of model %d" % ((k - G) % V, a + (k - G) // V)
            raise RuntimeError("emd_of_split: %s holds a NaN or infinite coordinate" % what)
        if np.isnan(res).any():
            j, i = np.argwhere(np.isnan(res))[0]
            raise RuntimeError("emd_of_split: model %d, view %d did not converge within max_rounds (or holds a NaN "
                               "coordinate)" % (a + j, i))
    return out
