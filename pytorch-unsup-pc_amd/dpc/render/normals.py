"""Batched k-nearest neighbours, PCA surface normals and the normal-consistency metric of a whole split.

Chamfer, EMD, IoU and F-score are position metrics: a cloud that sits on the surface but is locally scrambled (noisy
sheets, doubled layers, fuzz) scores like a clean one.  Normal consistency compares which way the surfaces face.

    knn_batched                  the thin wrapper over dpc_knn_batched: packed points, a [R,4] row table, idx [Q,k] int32
    estimate_normals             per cloud, the unit normal of every point from the covariance of its k nearest neighbours
    normal_consistency           (pred -> GT, GT -> pred, their mean) of |n . n'| over nearest neighbours, [P,3] float64
    normal_consistency_of_split  the same for loaded predictions and GT clouds of M models, [M,V,3] numpy

The rules of the search and of the normals (ties, padding, the sign, the accuracy) are stated in include/dpc_render.h
(dpc_knn_batched, dpc_pca_normals) and defined by tests/normals_oracle.py; the kernels are csrc/dpc_knn.hip.
"""
import numpy as np
import torch

from . import _batch, _native, _split
from ._ops import status_word
from .chamfer import nearest_batched
from .closest import _ClosestPlan
from .pointmesh import _index_map

_WHAT = "dpc.render normal estimation"
MAX_K, TILE = _native.DPC_KNN_MAX_K, _native.DPC_KNN_TILE


def _check_k(k, fn):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
        raise ValueError("%s: k must be an integer in [1, %d], got %r" % (fn, MAX_K, k))
    return int(k)


def _refuse_nonfinite(clouds, names, fn, host_only):
    """ValueError naming the first cloud with a NaN or inf coordinate; host_only: look at host clouds alone (before a
    device is looked for), otherwise at all of them."""
    for c, name in zip(clouds, names):
        if (not host_only or not c.is_cuda) and c.numel() and not bool(torch.isfinite(c).all()):
            raise ValueError("%s: %s holds a NaN or inf coordinate" % (fn, name))


def _packed_finite(packed, clouds, names, fn):
    """One device reduction over the packed buffer; the clouds are looked at one by one only when it fails."""
    if packed.numel() and not bool(torch.isfinite(packed).all()):
        _refuse_nonfinite(clouds, names, fn, False)


def _row_table(rows, fn):
    desc = rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    if desc.ndim != 2 or desc.shape[1] != 4 or not (np.issubdtype(desc.dtype, np.integer) or desc.size == 0):
        raise ValueError("%s: rows must be an integer [R,4] table (q_start, q_count, r_start, r_count), got %s %s"
                         % (fn, desc.dtype, tuple(desc.shape)))
    return _batch.table(desc, 4, "%s: row table entries must fit int32" % fn)


def _dry_run(desc, n_pts, k, fn):
    rc = _native.lib().dpc_knn_batched(None, n_pts, 0, None, desc.ctypes.data, len(desc), k, None, None, None, None)
    _batch.dry_run(rc, "%s: invalid row table (a negative start or count, a range outside the %d points, or more than "
                       "2^31 - 1 output slots)" % (fn, n_pts))


def _knn(pts, desc, k, dev, want_d2):
    """One dpc_knn_batched call on pts (on dev, float32 or float64, contiguous): (idx [Q,k] int32, d2 [Q,k] | None, the
    device table)."""
    Q = int(desc[:, 1].astype(np.int64).sum()) if len(desc) else 0
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((Q, k), dtype=pts.dtype, device=dev) if want_d2 else None
    desc_d = _batch.on_device(desc, dev) if len(desc) else None
    if Q:
        _native.call(dev, "dpc_knn_batched", _native.ptr(pts), int(pts.shape[0]), int(pts.dtype == torch.float64),
                     _native.ptr(desc_d), desc.ctypes.data, len(desc), k, _native.ptr(idx), _native.ptr(d2),
                     _native.ptr(status_word(dev)))
    return idx, d2, desc_d


def _pca(pts, desc, desc_d, k, idx, viewpoints, dev, want_eigenvalues):
    """One dpc_pca_normals call over what _knn returned: (normals [Q,3] float64, eigenvalues [Q,3] | None)."""
    Q = idx.shape[0]
    normals = torch.empty((Q, 3), dtype=torch.float64, device=dev)
    evals = torch.empty((Q, 3), dtype=torch.float64, device=dev) if want_eigenvalues else None
    if Q:
        _native.call(dev, "dpc_pca_normals", _native.ptr(pts), int(pts.shape[0]), int(pts.dtype == torch.float64),
                     _native.ptr(desc_d), desc.ctypes.data, len(desc), k, _native.ptr(idx), _native.ptr(viewpoints),
                     _native.ptr(normals), _native.ptr(evals), _native.ptr(status_word(dev)))
    return normals, evals


def knn_batched(points, rows, k, return_distances=False):
    """The k nearest references of every query, for R rows over one packed cloud buffer: idx [Q,k] int32 on the device, Q
    the sum of the rows' q_count, the rows' queries packed in row order; with return_distances (idx, d2 [Q,k]) with the
    squared distances in the compute type.

    points: [n,3] tensor (or array) holding every cloud; rows: [R,4] integer rows (q_start, q_count, r_start, r_count)
    indexing it, so a cloud against itself is one row and several rows may share a reference range.  fp64 arithmetic
    when points is fp64, fp32 otherwise.  A query's neighbours are the k references smallest by (squared distance, index),
    in that order; the query itself is not excluded; idx is relative to r_start; slots beyond r_count hold -1 and +inf.
    1 <= k <= 64.  Bit-identical from run to run and however the rows are ordered or batched; no host synchronisation
    but one finiteness check.  ValueError before a device is looked for: k, the shapes, a bad table, and (for host
    input) a NaN or inf coordinate."""
    fn = "knn_batched"
    k = _check_k(k, fn)
    desc = _row_table(rows, fn)
    pts = _batch.cloud(points, "%s: points" % fn)
    n_pts = int(pts.shape[0])
    if n_pts > _batch.INT32_MAX:
        raise ValueError("%s: more than 2^31 - 1 points" % fn)
    _dry_run(desc, n_pts, k, fn)
    _refuse_nonfinite([pts], ["points"], fn, True)
    dev = _batch.device(_WHAT, [pts])
    pts = pts.to(device=dev).contiguous()
    _packed_finite(pts, [pts], ["points"], fn)
    idx, d2, _ = _knn(pts, desc, k, dev, return_distances)
    return (idx, d2) if return_distances else idx


def _viewpoints(viewpoints, n, fn):
    if viewpoints is None:
        return None
    try:
        vp = np.asarray(viewpoints.detach().cpu() if isinstance(viewpoints, torch.Tensor) else viewpoints, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: viewpoints must be [%d,3] numbers, one camera location per cloud" % (fn, n))
    if vp.shape != (n, 3) or not np.isfinite(vp).all():
        raise ValueError("%s: viewpoints must be [%d,3] finite numbers, one camera location per cloud, got %s"
                         % (fn, n, tuple(vp.shape)))
    return np.ascontiguousarray(vp)


class _NormalsPlan:
    """A checked estimate_normals call: the clouds, split by precision, with the table of each group."""

    def __init__(self, clouds, k, viewpoints, fn, name="clouds", indices=None):
        self.fn, self.k = fn, _check_k(k, fn)
        self.names = ["%s[%d]" % (name, i if indices is None else indices[i]) for i in range(len(clouds))]
        self.clouds = [_batch.cloud(c, "%s: %s" % (fn, n)) for c, n in zip(clouds, self.names)]
        self.vp = _viewpoints(viewpoints, len(self.clouds), fn)
        self.groups = []
        for dtype in (torch.float32, torch.float64):
            sel = [i for i, c in enumerate(self.clouds) if c.dtype == dtype]
            if not sel:
                continue
            start = np.cumsum([0] + [len(self.clouds[i]) for i in sel])
            if start[-1] > _batch.INT32_MAX:
                raise ValueError("%s: more than 2^31 - 1 points in one call" % fn)
            rows = [(start[j], len(self.clouds[i]), start[j], len(self.clouds[i])) for j, i in enumerate(sel)]
            desc = _batch.table(np.asarray(rows, dtype=np.int64), 4, "%s: table entries must fit int32" % fn)
            _dry_run(desc, int(start[-1]), self.k, fn)
            self.groups.append((dtype, sel, desc))
        _refuse_nonfinite(self.clouds, self.names, fn, True)

    def run(self, dev, want_eigenvalues):
        """(normals, eigenvalues | None): lists of [n_i,3] float64 device tensors in cloud order; one k-NN call and one PCA
        call per precision."""
        normals, evals = [None] * len(self.clouds), [None] * len(self.clouds)
        for dtype, sel, desc in self.groups:
            group = [self.clouds[i] for i in sel]
            packed, _ = _batch.pack(group, dev, dtype)
            _packed_finite(packed, group, [self.names[i] for i in sel], self.fn)
            idx, _, desc_d = _knn(packed, desc, self.k, dev, False)
            vp = None if self.vp is None else torch.from_numpy(self.vp[sel]).to(dev)
            n, w = _pca(packed, desc, desc_d, self.k, idx, vp, dev, want_eigenvalues)
            sizes = [len(c) for c in group]
            for i, part in zip(sel, torch.split(n, sizes)):
                normals[i] = part
            if want_eigenvalues:
                for i, part in zip(sel, torch.split(w, sizes)):
                    evals[i] = part
        return normals, (evals if want_eigenvalues else None)


def estimate_normals(clouds, k=16, viewpoints=None, return_eigenvalues=False):
    """The unit surface normal of every point of every cloud: a list of [n,3] float64 device tensors; with
    return_eigenvalues (normals, eigenvalues), the second a list of [n,3] ascending eigenvalues of the covariance.

    clouds: a list of [n,3] float32 / float64 tensors or arrays.  Each cloud is searched against itself for the k nearest
    neighbours of every point (the point included) in its own precision; the normal is the eigenvector of the smallest
    eigenvalue of the neighbours' covariance, in fp64.  viewpoints: [len(clouds),3], one camera location per cloud: the
    normals are flipped to face it (n . (viewpoint - p) >= 0, open3d's orient_normals_towards_camera_location); without,
    the component of largest magnitude is made positive, which is deterministic but not a consistent orientation (the
    consistency metric takes |n . n'| and does not need one).  A cloud of fewer than 3 points gets zero normals.  The
    clouds of each precision go into one k-NN call and one PCA call; the result does not depend on the batching.  Every
    argument is checked before a device is looked for; ValueError for a NaN or inf coordinate, naming the cloud."""
    plan = _NormalsPlan(clouds, k, viewpoints, "estimate_normals")
    dev = _batch.device(_WHAT, plan.clouds)
    normals, evals = plan.run(dev, return_eigenvalues)
    return (normals, evals) if return_eigenvalues else normals


def _given_normals(normals, clouds, fn, name, cloud_name):
    """normals (None, or one [n_i,3] per cloud) as detached float64 tensors; ValueError naming the mismatch."""
    if normals is None:
        return None
    normals = list(normals)
    if len(normals) != len(clouds):
        raise ValueError("%s: %d %s for %d %s" % (fn, len(normals), name, len(clouds), cloud_name))
    out = []
    for i, (n, c) in enumerate(zip(normals, clouds)):
        t = _batch.cloud(n, "%s: %s[%d]" % (fn, name, i), cast=torch.float64)
        if len(t) != len(c):
            raise ValueError("%s: %s[%d] has %d normals for the %d points of %s[%d]" % (fn, name, i, len(t), len(c), cloud_name, i))
        out.append(t)
    return out


def _check_gt_meshes(gt_meshes, gt_normals, gts, fn):
    """gt_meshes stands in for gt_normals, one mesh per GT cloud."""
    if gt_normals is not None:
        raise ValueError("%s: give gt_normals or gt_meshes, not both" % fn)
    if len(gt_meshes) != len(gts):
        raise ValueError("%s: %d GT clouds and %d GT meshes" % (fn, len(gts), len(gt_meshes)))


def _dot_abs(a, b):
    """|a . b| per row, elementwise in fp64 in a fixed order: the value of a point does not depend on its neighbours in
    the batch."""
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]).abs()


class _ConsistencyPlan:
    """Every host check of a normal_consistency call."""

    def __init__(self, preds, gts, gt_of, k, pred_normals, gt_normals, fn, gt_meshes=None):
        self.fn, self.k = fn, _check_k(k, fn)
        self.preds = [_batch.cloud(p, "%s: preds[%d]" % (fn, i)) for i, p in enumerate(preds)]
        self.gts = [_batch.cloud(g, "%s: gts[%d]" % (fn, i)) for i, g in enumerate(gts)]
        self.gt_of = _index_map(gt_of, len(self.preds), len(self.gts), fn, "gt_of", "predictions", "GT clouds")
        for i, j in enumerate(self.gt_of):
            if len(self.gts[j]) == 0 and len(self.preds[i]) > 0:
                raise ValueError("%s: GT cloud %d is empty but prediction %d is not (argmin of an empty set)" % (fn, j, i))
        self.pred_normals = _given_normals(pred_normals, self.preds, fn, "pred_normals", "preds")
        self.gt_normals = _given_normals(gt_normals, self.gts, fn, "gt_normals", "gts")
        self.used = sorted(set(self.gt_of))
        self.pred_plan = self.gt_plan = self.mesh_plan = None
        self.meshes = gt_meshes
        if gt_meshes is not None:
            _check_gt_meshes(gt_meshes, gt_normals, self.gts, fn)
            self.mesh_plan = _ClosestPlan(self.gts, gt_meshes, None, fn, "gts")   # face_normals_at(gts, gt_meshes), checked
        if self.pred_normals is None:
            self.pred_plan = _NormalsPlan(self.preds, self.k, None, fn, "preds")
        else:
            _refuse_nonfinite(self.preds, ["preds[%d]" % i for i in range(len(self.preds))], fn, True)
        if self.gt_normals is None and self.mesh_plan is None:   # once per GT cloud that a prediction names, not once per view
            self.gt_plan = _NormalsPlan([self.gts[j] for j in self.used], self.k, None, fn, "gts", self.used)
        else:
            _refuse_nonfinite(self.gts, ["gts[%d]" % i for i in range(len(self.gts))], fn, True)

    def tensors(self):
        return [self.preds, self.gts, self.pred_normals or [], self.gt_normals or [],
                [] if self.meshes is None else [x for m in self.meshes for x in m[:2]]]

    def run(self, dev):
        P = len(self.preds)
        out = torch.full((P, 3), float("nan"), dtype=torch.float64, device=dev)
        if P == 0:
            return out
        n_pred = self.pred_normals if self.pred_plan is None else self.pred_plan.run(dev, False)[0]
        if self.mesh_plan is not None:   # face_normals_at(gts, gt_meshes): the normal of the face each GT sample lies on
            n_gt = dict(enumerate(self.mesh_plan.split(self.mesh_plan.closest(dev, True)[4])))
        elif self.gt_plan is None:
            n_gt = {j: self.gt_normals[j] for j in self.used}
        else:
            n_gt = dict(zip(self.used, self.gt_plan.run(dev, False)[0]))
        f64 = [self.preds[i].dtype == torch.float64 or self.gts[j].dtype == torch.float64 for i, j in enumerate(self.gt_of)]
        for want in (False, True):   # an empty prediction has no pair: its row stays NaN
            sel = [i for i in range(P) if f64[i] == want and len(self.preds[i]) > 0]
            if sel:
                out[sel] = self._group(sel, n_pred, n_gt, dev, torch.float64 if want else torch.float32)
        return out

    def _group(self, sel, n_pred, n_gt, dev, dtype):
        """The rows of the predictions `sel`: the GT clouds they use, then the predictions, in one packed buffer with the
        normals packed alike; pairs (p -> g, g -> p) interleaved; one nearest_batched call and one
        dpc_chamfer_pair_means call."""
        used = sorted({self.gt_of[i] for i in sel})
        clouds = [self.gts[j] for j in used] + [self.preds[i] for i in sel]
        names = ["gts[%d]" % j for j in used] + ["preds[%d]" % i for i in sel]
        packed, start = _batch.pack(clouds, dev, dtype)
        if start[-1] > _batch.INT32_MAX:
            raise ValueError("%s: more than 2^31 - 1 points in one call" % self.fn)
        _packed_finite(packed, clouds, names, self.fn)
        normals = torch.cat([n_gt[j].to(device=dev, dtype=torch.float64) for j in used]
                            + [n_pred[i].to(device=dev, dtype=torch.float64) for i in sel])
        slot = {j: s for s, j in enumerate(used)}
        desc = np.zeros((2 * len(sel), 4), dtype=np.int64)
        for s, i in enumerate(sel):
            ps, pn = start[len(used) + s], len(self.preds[i])
            gs, gn = start[slot[self.gt_of[i]]], len(self.gts[self.gt_of[i]])
            desc[2 * s] = (ps, pn, gs, gn)
            desc[2 * s + 1] = (gs, gn, ps, pn)
        _, _, idx = nearest_batched(packed, desc, return_distances=True)
        counts = torch.from_numpy(desc[:, 1].copy()).to(dev)
        total = int(desc[:, 1].sum())
        pair = torch.repeat_interleave(torch.arange(len(desc), device=dev), counts, output_size=total)
        first = torch.cumsum(counts, 0) - counts                      # the first output point of each pair
        src = torch.from_numpy(desc[:, 0].copy()).to(dev)[pair] + (torch.arange(total, device=dev) - first[pair])
        tgt = torch.from_numpy(desc[:, 2].copy()).to(dev)[pair] + idx
        values = _dot_abs(normals[src], normals[tgt]).contiguous()
        table = _batch.table(desc, 4, "%s: table entries must fit int32" % self.fn)
        table_d = _batch.on_device(table, dev)
        mean = torch.empty((len(table),), dtype=torch.float64, device=dev)
        ws = _batch.workspace(_native.lib().dpc_chamfer_workspace_bytes(len(table), table.ctypes.data, 1), dev)
        _native.call(dev, "dpc_chamfer_pair_means", _native.ptr(values), 1, _native.ptr(table_d), table.ctypes.data, len(table),
                     _native.ptr(mean), _native.ptr(ws))
        ab = mean.view(len(sel), 2)
        return torch.cat([ab, ((ab[:, 0] + ab[:, 1]) / 2.0)[:, None]], dim=1)


def normal_consistency(preds, gts, gt_of=None, k=16, pred_normals=None, gt_normals=None, gt_meshes=None):
    """The normal consistency of every prediction against its ground truth: [P,3] float64 on the device, (a, b, (a + b) / 2)
    per prediction, each in [0, 1], 1 where the surfaces face the same way up to sign.

    a = the mean over the prediction's points of |Np[j] . Ng[nearest GT point of P_j]|, b = the mean over the GT cloud's
    points of |Ng[l] . Np[nearest predicted point of G_l]|.  preds, gts: lists of [n,3] tensors or arrays; gt_of: the GT
    index of each prediction (default i -> i), as in chamfer_batched, whose precision rule applies to the nearest-neighbour
    searches (nearest_batched's).  pred_normals / gt_normals: one [n,3] array of normals per prediction / per GT cloud;
    those not supplied are estimated with estimate_normals(k) -- the GT's once per GT cloud, not once per view.
    gt_meshes: one (V, F, ...) per GT cloud, as point_mesh_distance takes them -- the GT normals are then
    face_normals_at(gts, gt_meshes), the unit normal of the mesh face nearest to each GT point (for a cloud sampled from
    its mesh, the face it lies on), as published single-view reconstruction numbers take them, instead of the PCA
    estimate; giving both gt_normals and gt_meshes is a ValueError.  The means
    are dpc_chamfer_pair_means over the packed |dot| values, so they are bit-reproducible and do not depend on how the
    predictions are grouped.  A zero normal contributes 0; an empty prediction gives NaN.  Every argument is checked
    before a device is looked for; ValueError for a NaN or inf coordinate, naming the cloud."""
    plan = _ConsistencyPlan(preds, gts, gt_of, k, pred_normals, gt_normals, "normal_consistency", gt_meshes)
    return plan.run(_batch.device(_WHAT, *plan.tensors()))


def normal_consistency_of_split(predictions, gt_clouds, gt_normals=None, k=16, reference_rotation=None, models_per_call=256,
                                gt_meshes=None):
    """normal_consistency for every view of M models: [M,V,3] float64 numpy.

    predictions, gt_clouds, reference_rotation and models_per_call as in fscore_of_split (view i is truncated to its first
    num_points[i] points, the rotation is applied to every view first); gt_normals: one [n,3] array per model, estimated
    with k when not given, once per model; gt_meshes: one mesh per model instead, as in normal_consistency (the GT normals
    are the mesh faces').  The predictions' normals are always estimated with k.  The result does not
    depend on the grouping.  Every argument is checked before anything is launched."""
    fn = "normal_consistency_of_split"
    split = _split.Split(fn, predictions, gt_clouds, reference_rotation, models_per_call, gt_label=fn + ": gt_clouds[%d]",
                         refuse_empty_gt=True)
    k = _check_k(k, fn)
    gts = split.gts
    given = _given_normals(gt_normals, gts, fn, "gt_normals", "gt_clouds")
    _refuse_nonfinite([p for p, _ in split.preds], ["predictions[%d]" % m for m in range(split.M)], fn, True)
    _refuse_nonfinite(gts, ["gt_clouds[%d]" % m for m in range(split.M)], fn, True)
    if gt_meshes is not None:
        # The meshes' own checks and the dry run of every group's table.  normal_consistency builds the same plan again
        # for each group; building them here first is what makes every refusal come before the first group is launched.
        _check_gt_meshes(gt_meshes, gt_normals, gts, fn)
        for g in split.groups:
            _ClosestPlan([gts[m] for m in g], [gt_meshes[m] for m in g], None, fn, "gt_clouds")
    out = np.zeros((split.M, split.V, 3), dtype=np.float64)
    if split.empty:
        return out
    dev = _batch.device(_WHAT, *split.tensors(), [] if gt_meshes is None else [x for m in gt_meshes for x in m[:2]])
    for group in split.groups:
        views_list, gt_of = split.views(group, dev)
        split.store(out, group, normal_consistency(views_list, [gts[m] for m in group], gt_of, k, None,
                                                   None if given is None else [given[m] for m in group],
                                                   None if gt_meshes is None else [gt_meshes[m] for m in group]))
    return out
