"""What the evaluations of a whole split share, next to _batch.py: the checked arguments of the *_of_split functions
(chamfer, emd, voxels, meshvoxels, pointmesh, normals, voxeldist) with their walk over groups of models, and the walk over a
split by model name (densify_split, render_training_views, render_split, downsample_split, eval_chamfer).

    Split      predictions, per-model targets, rotation and models_per_call, checked before a device is looked for; per
               group of models the views rotated, truncated and detached, and the write-back of a group's result
    batches    model names -> batches of at most `step` loaded (name, item) pairs
    isolate    a batched call, and after a MeshError each of its models alone
"""
import numpy as np
import torch

from . import _batch
from . import densify as _densify    # for MeshError, read when isolate runs: densify imports this module too


def _host_unit_quaternion(q):
    """The reference's q / |q| (util/quaternion.py quaternion_rotate), evaluated in CPU torch where its evaluation ran:
    a device norm of four numbers is not guaranteed to round the same way."""
    qt = q.detach().cpu() if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q))
    if qt.dim() != 2 or qt.shape != (1, 4):
        raise ValueError("reference_rotation must be a [1,4] quaternion, got %s" % (tuple(qt.shape),))
    return torch.div(qt, qt.norm(p=2, dim=-1).reshape(qt.shape[0], 1))


def _rotate(points, qn, dev):
    """quaternion_rotate(points [V,N,3], q) with q already normalised: q * p * conj(q), the reference's products in its
    order, in the promoted dtype (float64 for a float64 quaternion; no cast back, as eval_chamfer_to.py:116-120)."""
    from . import quaternion_conjugate, quaternion_multiply

    pc = points.to(dev).reshape(1, -1, 3)
    q = qn.to(dev).reshape(1, 1, 4)
    wxyz = quaternion_multiply(quaternion_multiply(q, pc), quaternion_conjugate(q))
    return wxyz[:, :, 1:4].reshape(points.shape[0], points.shape[1], 3)


def _prediction(entry, m):
    if not isinstance(entry, (tuple, list)) or len(entry) not in (2, 3):
        raise ValueError("predictions[%d] must be (points, num_points) or load_predictions' (points, camera_pose, num_points)" % m)
    pts, nums = entry[0], entry[-1]
    pts = pts if isinstance(pts, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pts))
    if pts.dim() != 3 or pts.shape[2] != 3:
        raise ValueError("predictions[%d] points must be [V,N,3], got %s" % (m, tuple(pts.shape)))
    if nums is not None:
        nums = np.asarray(nums.detach().cpu() if isinstance(nums, torch.Tensor) else nums).reshape(-1)
        if (len(nums) != pts.shape[0] or not np.issubdtype(nums.dtype, np.integer) or (nums < 0).any()
                or (nums > pts.shape[1]).any()):
            raise ValueError("predictions[%d] num_points must be %d integers in [0, %d], got %r"
                             % (m, pts.shape[0], pts.shape[1], nums))
    return pts, nums


def checked_step(fn, models_per_call):
    """models_per_call as an int >= 1."""
    step = int(models_per_call)
    if step < 1:
        raise ValueError("%s: models_per_call must be >= 1" % fn)
    return step


class Split:
    """The arguments every *_of_split function takes, checked on the host (ValueError naming `fn`):

        M, V     models, views per model
        preds    per model (points [V,N,3] tensor, num_points [V] array | None)
        counts   per model the V point counts of its views after truncation
        gts      per model the detached [n,3] GT cloud; [] when the targets are not clouds (gt_label None)
        qn       the unit quaternion on the host, or None
        groups   the ranges of models that go into one call, models_per_call each

    noun names the targets in the length message; gt_label % m names a GT cloud; refuse_empty_gt refuses an empty GT cloud
    under a non-empty view."""

    def __init__(self, fn, predictions, targets, reference_rotation, models_per_call, noun="GT clouds",
                 gt_label="gt_clouds[%d]", refuse_empty_gt=False):
        if len(predictions) != len(targets):
            raise ValueError("%s: %d predictions and %d %s" % (fn, len(predictions), len(targets), noun))
        step = checked_step(fn, models_per_call)
        self.preds = [_prediction(e, m) for m, e in enumerate(predictions)]
        self.gts = [] if gt_label is None else [_batch.cloud(g, gt_label % m) for m, g in enumerate(targets)]
        views = {p.shape[0] for p, _ in self.preds}
        if len(views) > 1:
            raise ValueError("%s: every model needs the same number of views, got %s" % (fn, sorted(views)))
        self.M, self.V = len(self.preds), views.pop() if views else 0
        for m, ((p, nums), g) in enumerate(zip(self.preds, self.gts)):
            if refuse_empty_gt and len(g) == 0 and (p.shape[1] if nums is None else nums.max(initial=0)) > 0:
                raise ValueError("%s: GT cloud %d is empty" % (fn, m))
        self.counts = [[int(p.shape[1]) if nums is None else int(nums[i]) for i in range(self.V)] for p, nums in self.preds]
        self.qn = None if reference_rotation is None else _host_unit_quaternion(reference_rotation)
        self.groups = [range(a, min(self.M, a + step)) for a in range(0, self.M, step)]

    @property
    def empty(self):
        """No view to evaluate: the caller returns its pre-filled output without looking for a device."""
        return self.M == 0 or self.V == 0

    def tensors(self):
        """What the device is chosen from, in this order (_batch.device): the predictions' points, the GT clouds."""
        return [p for p, _ in self.preds], self.gts

    def model(self, m, dev, on_device=False):
        """The V views of model m: rotated on dev when there is a rotation (the result stays in the promoted dtype),
        truncated to their counts and detached.  Without a rotation they are views of the input where it lives, or with
        on_device of its copy on dev."""
        pts = self.preds[m][0].detach()
        if self.qn is not None:
            pts = _rotate(pts, self.qn, dev)
        elif on_device:
            pts = pts.to(dev)
        if self.preds[m][1] is None:
            return list(pts)
        return [pts[i, :n] for i, n in enumerate(self.counts[m])]

    def views(self, group, dev):
        """(views_list, gt_of) of a group for a batched call: every view of every model of the group, model-major, and the
        position within the group of the model each belongs to."""
        views_list = [v for m in group for v in self.model(m, dev)]
        return views_list, [j for j in range(len(group)) for _ in range(self.V)]

    def store(self, out, group, res):
        """out[group] = the device result res of a group, [len(group) * V, ...] reshaped to (len(group), V, ...); returns
        the host array written."""
        host = res.cpu().numpy().reshape((len(group), self.V) + out.shape[2:])
        out[group[0]:group[-1] + 1] = host
        return host


def batches(model_names, load, step, errors=None, catch=()):
    """Walks a split by model name: yields lists of at most `step` (name, item) pairs, item = load(name, i) with i the
    position the item takes in the pending batch; a model whose item is None is skipped.  An exception of one of the types
    `catch` raised by load is raised again as the same type with the model's name in front, or with an `errors` dict
    recorded there (errors[name] = message) and the model skipped; any other exception propagates untouched."""
    batch = []
    for name in model_names:
        try:
            item = load(name, len(batch))
        except catch as exc:
            if errors is None:
                raise type(exc)("model %r: %s" % (name, exc)) from exc
            errors[name] = str(exc)
            continue
        if item is None:
            continue
        batch.append((name, item))
        if len(batch) >= step:
            yield batch
            batch = []
    if batch:
        yield batch


def isolate(run, items, names, errors):
    """run(items), one result per item; when a batch raises MeshError (a status bit is batch-wide), each of its models
    alone, so the error names the model, or, with an `errors` dict, is recorded there and that model's result is None."""
    try:
        return run(items)
    except _densify.MeshError as exc:
        if len(items) == 1:
            if errors is None:
                raise _densify.MeshError("model %r: %s" % (names[0], exc)) from exc
            errors[names[0]] = str(exc)
            return [None]
    return [r for it, name in zip(items, names) for r in isolate(run, [it], [name], errors)]
