"""Voxel-grid evaluation on the GPU: the reference's dpc/util/voxel.py (evaluate_voxel_prediction, voxel2pc) and the
voxel IoU that voxel baselines (PTN, DRC) are compared in, batched.

    voxelise                   clouds -> bool occupancy grids (the nearest node of the renderer's node-centred grid)
    voxel_stats, voxel_iou     the five counts of evaluate_voxel_prediction / intersection over union, per pair
    evaluate_voxel_prediction  the reference's function on [B,2,D,H,W] arrays
    voxel2pc                   the reference's function; voxels2pc_batched: a batch of grids in one pass
    iou_of_split               voxel IoU of every view of every model against its ground-truth cloud
    render_voxels              voxel2pc, then render_point_clouds

Clouds and float grids become bit grids (csrc/dpc_voxels.hip); everything downstream is bit-OR and popcount, so every
output has one right answer.  The conventions -- grid layout, the voxelisation rule, the bit layout, which threshold is
inclusive, voxel2pc's axis order -- are in include/dpc_render.h (dpc_voxelise).
"""
import numpy as np
import torch

from . import _batch, _native, _split
from ._ops import status_word

_WHAT = "dpc.render voxel evaluation"
MAX_SIDE = _native.DPC_VOXEL_MAX_SIDE
_GRID_DTYPES = {torch.float32: 0, torch.float64: 1, torch.bool: 2, torch.uint8: 2}


def _side(v, name, fn):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s: %s must be an integer, got %r" % (fn, name, v))
    return int(v)


def _shape_of(vox_size, vox_size_z, fn):
    """(D, H, W) of the config's vox_size / vox_size_z (-1: vox_size)."""
    G, Gz = _side(vox_size, "vox_size", fn), _side(vox_size_z, "vox_size_z", fn)
    return _check_shape((G if Gz == -1 else Gz, G, G), fn)


def _check_shape(shape, fn):
    shape = tuple(int(s) for s in shape)
    if any(s < 1 for s in shape):
        raise ValueError("%s: a grid of %s has an empty side" % (fn, shape))
    if any(s > MAX_SIDE for s in shape):
        raise ValueError("%s: a grid of %s has a side above DPC_VOXEL_MAX_SIDE = %d" % (fn, shape, MAX_SIDE))
    return shape


def _words(shape):
    return (shape[0] * shape[1] * shape[2] + 31) // 32


def _is_grid(x):
    return isinstance(x, (torch.Tensor, np.ndarray)) and x.ndim == 4


class _Clouds(list):
    """A list of [n,3] tensors; `stacked`: the [B,n,3] device tensor they are the rows of (it needs no packing), or None."""
    stacked = None


def _clouds(x, name, fn):
    """x (a list of [n,3] clouds, or a [B,n,3] tensor) as a list of detached [n,3] float32 / float64 tensors."""
    stacked = None
    if isinstance(x, (torch.Tensor, np.ndarray)):
        if x.ndim != 3:
            raise ValueError("%s: %s must be a list of [n,3] clouds, a [B,n,3] tensor or [B,D,H,W] grids, got %s"
                             % (fn, name, tuple(x.shape)))
        if isinstance(x, torch.Tensor) and x.is_cuda and x.shape[2] == 3 and x.dtype in (torch.float32, torch.float64):
            stacked = x.detach().contiguous()
        x = list(x)
    out = _Clouds(_batch.cloud(c, "%s: %s[%d]" % (fn, name, i)) for i, c in enumerate(x))
    out.stacked = stacked
    return out


def _grid_tensor(x, name, fn, kinds):
    """x ([B,D,H,W], tensor or array) as a detached tensor of one of the dtypes `kinds`; its shape is checked."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype not in kinds:
        raise ValueError("%s: %s must be a %s grid, got %s" % (fn, name, " / ".join(str(k).replace("torch.", "") for k in kinds), t.dtype))
    _check_shape(t.shape[1:], fn)
    return t.detach()


def _bits_of_clouds(clouds, shape, dev, fn, status=None):
    """(bit grids int32 [C, words], dropped int32 [C]) of a list of [n,3] tensors: one dpc_voxelise call."""
    C = len(clouds)
    counts = [len(c) for c in clouds]
    start = np.cumsum([0] + counts)
    if start[-1] > _batch.INT32_MAX:
        raise ValueError("%s: more than 2^31 - 1 points in one call" % fn)
    desc = _batch.table(np.stack([start[:-1], counts], axis=1) if C else np.zeros((0, 2)), 2, "%s: cloud table entries must fit int32" % fn)
    bits = torch.empty((C, _words(shape)), dtype=torch.int32, device=dev)
    dropped = torch.empty((C,), dtype=torch.int32, device=dev)
    if C:
        stacked = getattr(clouds, "stacked", None)
        if stacked is not None:
            pts, dtype = stacked.view(-1, 3), stacked.dtype
        else:
            dtype = _batch.widest(clouds)
            pts, _ = _batch.pack(clouds, dev, dtype)
        desc_d = _batch.on_device(desc, dev)
        status = status_word(dev) if status is None else status
        _native.call(dev, "dpc_voxelise", _native.ptr(pts) if len(pts) else None, int(pts.shape[0]), int(dtype == torch.float64),
                     _native.ptr(desc_d), desc.ctypes.data, C, shape[0], shape[1], shape[2], _native.ptr(bits),
                     _native.ptr(dropped), _native.ptr(status))
    return bits, dropped


def _bits_of_grids(grids, threshold, inclusive, dev):
    """Bit grids int32 [B, words] of a [B,D,H,W] float32 / float64 (thresholded) or bool / uint8 (non-zero) tensor."""
    g = grids.to(dev).contiguous()
    B, shape = g.shape[0], tuple(g.shape[1:])
    bits = torch.empty((B, _words(shape)), dtype=torch.int32, device=dev)
    if B:
        _native.call(dev, "dpc_voxel_threshold", _native.ptr(g), _GRID_DTYPES[g.dtype], B, shape[0], shape[1], shape[2],
                     float(threshold), int(bool(inclusive)), _native.ptr(bits))
    return bits


def _unpack(bits, shape):
    """Bit grids -> bool [B,D,H,W]."""
    B = bits.shape[0]
    out = torch.empty((B,) + tuple(shape), dtype=torch.bool, device=bits.device)
    if B:
        _native.call(bits.device, "dpc_voxel_unpack", _native.ptr(bits), B, shape[0], shape[1], shape[2], _native.ptr(out))
    return out


def _pair_stats(pred_bits, gt_bits, pairs, shape, status=None):
    """int64 [P,5] for the [P,2] host table `pairs` of (pred grid, gt grid) indices."""
    dev = pred_bits.device
    P = len(pairs)
    stats = torch.zeros((P, 5), dtype=torch.int64, device=dev)
    if P:
        pairs_d = _batch.on_device(pairs, dev)
        status = status_word(dev) if status is None else status
        _native.call(dev, "dpc_voxel_stats", _native.ptr(pred_bits), int(pred_bits.shape[0]), _native.ptr(gt_bits),
                     int(gt_bits.shape[0]), shape[0], shape[1], shape[2], _native.ptr(pairs_d), pairs.ctypes.data, P,
                     _native.ptr(stats), _native.ptr(status))
    return stats


def voxelise(clouds, vox_size, vox_size_z=-1, return_dropped=False):
    """Occupancy grids of clouds: a bool [C,D,H,W] device tensor, D = vox_size_z (vox_size when -1), H = W = vox_size.

    clouds: a list of [n_i,3] float32 / float64 tensors or arrays (n_i may be 0), or a [B,n,3] tensor.  Point column c
    goes to grid axis c.  A point with -0.5 <= p_c <= 0.5 on all axes marks the node floor((p_c + 0.5) * (G_c - 1) + 0.5),
    evaluated in fp64, so an fp32 cloud and its fp64 copy give the same grid; every other point is dropped.  With
    return_dropped: (grids, int32 [C] dropped points per cloud).  A NaN or infinite coordinate is dropped too and sets
    DPC_STATUS_NONFINITE in the status word that check_status() returns.  No host synchronisation.  ValueError before
    anything is launched for a cloud that is not [n,3] or a side outside [1, DPC_VOXEL_MAX_SIDE]."""
    fn = "voxelise"
    shape = _shape_of(vox_size, vox_size_z, fn)
    cl = _clouds(clouds, "clouds", fn)
    _batch.refuse_cpu(clouds)
    dev = _batch.device(_WHAT, cl)
    bits, dropped = _bits_of_clouds(cl, shape, dev, fn)
    grids = _unpack(bits, shape)
    return (grids, dropped) if return_dropped else grids


def _sources(preds, gts, gt_of, vox_size, vox_size_z, fn):
    """The argument checks of voxel_stats, before anything touches a device: (pred source, gt source, pair table, shape);
    a source is ("clouds", list) or ("grids", tensor)."""
    if _is_grid(preds):
        pred = ("grids", _grid_tensor(preds, "preds", fn, (torch.float32, torch.float64)))
    else:
        pred = ("clouds", _clouds(preds, "preds", fn))
    if _is_grid(gts):
        gt = ("grids", _grid_tensor(gts, "gts", fn, (torch.bool, torch.uint8)))
    else:
        gt = ("clouds", _clouds(gts, "gts", fn))
    shapes = {tuple(s[1].shape[1:]) for s in (pred, gt) if s[0] == "grids"}
    if len(shapes) > 1:
        raise ValueError("%s: preds are grids of %s and gts grids of %s" % (fn, tuple(pred[1].shape[1:]), tuple(gt[1].shape[1:])))
    if vox_size is not None:
        asked = _shape_of(vox_size, vox_size_z, fn)
        if shapes and shapes != {asked}:
            raise ValueError("%s: vox_size / vox_size_z ask for grids of %s, the grids given are %s" % (fn, asked, shapes.pop()))
        shape = asked
    elif shapes:
        shape = shapes.pop()
    else:
        raise ValueError("%s: clouds on both sides need vox_size" % fn)
    P, Q = len(pred[1]), len(gt[1])
    if gt_of is None:
        if P != Q:
            raise ValueError("%s: %d predictions and %d ground truths need gt_of" % (fn, P, Q))
        gt_of = range(P)
    gt_of = list(gt_of.tolist() if isinstance(gt_of, (torch.Tensor, np.ndarray)) else gt_of)
    if len(gt_of) != P or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 0 or k >= Q for k in gt_of):
        raise ValueError("%s: gt_of must map each of the %d predictions to one of %d ground truths" % (fn, P, Q))
    pairs = _batch.table(np.stack([np.arange(P), np.asarray(gt_of, dtype=np.int64)], axis=1) if P else np.zeros((0, 2)), 2,
                         "%s: pair table entries must fit int32" % fn)
    rc = _native.lib().dpc_voxel_stats(None, P, None, Q, shape[0], shape[1], shape[2], None, pairs.ctypes.data, P, None, None, None)
    _batch.dry_run(rc, "%s: dpc_voxel_stats refused the pair table" % fn)
    return pred, gt, pairs, shape


def _source_bits(source, shape, threshold, inclusive, dev, fn):
    kind, data = source
    if kind == "grids":
        return _bits_of_grids(data, threshold, inclusive, dev), None
    return _bits_of_clouds(data, shape, dev, fn)


def _stats(preds, gts, gt_of, vox_size, vox_size_z, threshold, fn):
    pred, gt, pairs, shape = _sources(preds, gts, gt_of, vox_size, vox_size_z, fn)
    threshold = float(threshold)
    given = [x for x in (preds, gts) if isinstance(x, torch.Tensor)]
    given += [c for x in (preds, gts) if isinstance(x, (list, tuple)) for c in x if isinstance(c, torch.Tensor)]
    _native.require_device(*given)
    dev = _batch.device(_WHAT, given)
    pb, _ = _source_bits(pred, shape, threshold, True, dev, fn)
    gb, _ = _source_bits(gt, shape, 0.0, True, dev, fn)
    return _pair_stats(pb, gb, pairs, shape)


def voxel_stats(preds, gts, gt_of=None, vox_size=None, vox_size_z=-1, threshold=0.5):
    """The five counts of evaluate_voxel_prediction for P (prediction, ground truth) pairs: int64 [P,5] on the device, in
    its order (diff, intersection, union, num_fp, num_fn), num_fp = |pred & ~gt| and num_fn = |~pred & gt|.

    preds: a list of clouds (or a [P,n,3] tensor), voxelised like voxelise, or float32 / float64 grids [P,D,H,W], occupied
    where v >= threshold (compared in the grid's dtype; a NaN voxel is unoccupied).  gts: a list of clouds, or bool (uint8:
    non-zero) grids [Q,D,H,W].  gt_of[i]: the ground truth of prediction i (None: Q == P, pair i with i), so the views of
    one model share one grid.  vox_size / vox_size_z: the grid of the clouds; not needed beside a grid, whose shape it
    must equal when given.  No host synchronisation.  ValueError before anything is launched for grids of different
    shapes, a bad gt_of, clouds on both sides without vox_size, a side above DPC_VOXEL_MAX_SIDE, a prediction grid that
    is not float32 / float64 or a ground-truth grid that is not bool / uint8."""
    return _stats(preds, gts, gt_of, vox_size, vox_size_z, threshold, "voxel_stats")


def _iou(stats):
    inter, union = stats[..., 1].double(), stats[..., 2].double()
    return torch.where(union > 0, inter / union, torch.full_like(union, float("nan")))


def voxel_iou(preds, gts, gt_of=None, vox_size=None, vox_size_z=-1, threshold=0.5):
    """intersection / union of voxel_stats (the same arguments): float64 [P] on the device, NaN where the union is 0."""
    return _iou(_stats(preds, gts, gt_of, vox_size, vox_size_z, threshold, "voxel_iou"))


def _as_float_grid(x, name, fn):
    """A tensor or array as a detached tensor that compares like numpy: float32 / float64 as they are, integers and bool as
    float64 (numpy compares them with a Python float in float64)."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    t = t.detach()
    if t.dtype in (torch.float32, torch.float64):
        return t
    if t.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
        return t.to(torch.float64)
    raise ValueError("%s: %s must be float32, float64, integer or bool, got %s" % (fn, name, t.dtype))


def evaluate_voxel_prediction(preds, gt, thresh):
    """The reference's evaluate_voxel_prediction (util/voxel.py:4-11) on the GPU: preds and gt are [B,2,D,H,W] arrays or
    tensors; with occ = preds[:,1] >= thresh and gt's channels taken as logical (non-zero), the int64 numpy array
    [sum(occ ^ gt1), sum(occ & gt1), sum(occ | gt1), sum(occ & gt0), sum(~occ & gt1)], equal to the reference's."""
    fn = "evaluate_voxel_prediction"
    p, g = _as_float_grid(preds, "preds", fn), _as_float_grid(gt, "gt", fn)
    if p.dim() != 5 or p.shape[1] != 2 or tuple(g.shape) != tuple(p.shape):
        raise ValueError("%s: preds and gt must both be [B,2,D,H,W], got %s and %s" % (fn, tuple(p.shape), tuple(g.shape)))
    shape = _check_shape(p.shape[2:], fn)
    B = p.shape[0]
    given = [x for x in (preds, gt) if isinstance(x, torch.Tensor)]
    _native.require_device(*given)
    dev = _batch.device(_WHAT, given)
    pb = _bits_of_grids(p[:, 1], float(thresh), True, dev)
    g = g.to(dev)
    gb = _bits_of_grids(torch.cat([g[:, 1] != 0, g[:, 0] != 0]), 0.0, True, dev)    # gt1 of every item, then gt0
    idx = np.arange(B)
    pairs = _batch.table(np.concatenate([np.stack([idx, idx], axis=1), np.stack([idx, B + idx], axis=1)]), 2, fn)
    s = _pair_stats(pb, gb, pairs, shape).cpu().numpy()
    with_gt1, with_gt0 = s[:B].sum(axis=0), s[B:].sum(axis=0)
    return np.array([with_gt1[0], with_gt1[1], with_gt1[2], with_gt0[1], with_gt1[4]], dtype=np.int64)


def _cubic(shape, fn):
    if len(shape) != 3 or len(set(shape)) != 1:
        raise ValueError("%s: voxels must squeeze to a cubic [G,G,G] grid, got %s (the reference raises for others)" % (fn, tuple(shape)))
    if shape[0] < 2:
        raise ValueError("%s: G = %d: np.linspace over one node has no spacing (the reference raises)" % (fn, shape[0]))
    return _check_shape(shape, fn)


def _points_of_bits(bits, G, dev):
    """(xyz float64 [n,3], counts list) of bit grids [B, words] of G^3 voxels: a count call, one read of the counts, a write call."""
    B = bits.shape[0]
    counts_d = torch.empty((B,), dtype=torch.int32, device=dev)
    if B:
        _native.call(dev, "dpc_voxel_count", _native.ptr(bits), B, G, G, G, _native.ptr(counts_d))
    counts = counts_d.cpu().numpy().astype(np.int64)      # the one host synchronisation: the output is sized by it
    start = np.cumsum(np.concatenate([[0], counts]))
    total = int(start[-1])
    if total > _batch.INT32_MAX:
        raise ValueError("voxels2pc_batched: more than 2^31 - 1 occupied voxels in one call")
    xyz = torch.empty((total, 3), dtype=torch.float64, device=dev)
    if B:
        desc = _batch.table(np.stack([start[:-1], counts], axis=1), 2, "voxel2pc: table entries must fit int32")
        desc_d = _batch.on_device(desc, dev)
        _native.call(dev, "dpc_voxel2pc", _native.ptr(bits), B, G, _native.ptr(desc_d), desc.ctypes.data, total,
                     _native.ptr(xyz) if total else None, _native.ptr(status_word(dev)))
    return xyz, [int(c) for c in counts]


def voxels2pc_batched(voxels, threshold):
    """voxel2pc for a batch: voxels [B,G,G,G] (float32 / float64 tensor or array; integers and bool compare as float64) ->
    a list of B [n_i,3] float64 device tensors, the points of the voxels > threshold in ascending flat index, voxel
    (i,j,k) at (x[j], x[i], x[k]) with x = np.linspace(-0.5, 0.5, G).  One count call, one read of the counts (the only
    host synchronisation) and one write call.  ValueError for grids that are not cubic or have G < 2."""
    fn = "voxels2pc_batched"
    if not isinstance(voxels, (torch.Tensor, np.ndarray)) or voxels.ndim != 4:
        raise ValueError("%s: voxels must be [B,G,G,G], got %s" % (fn, tuple(getattr(voxels, "shape", ()))))
    v = _as_float_grid(voxels, "voxels", fn)
    G = _cubic(tuple(v.shape[1:]), fn)[0]
    given = [voxels] if isinstance(voxels, torch.Tensor) else []
    _native.require_device(*given)
    dev = _batch.device(_WHAT, given)
    xyz, counts = _points_of_bits(_bits_of_grids(v, float(threshold), False, dev), G, dev)
    return list(xyz.split(counts))


def voxel2pc(voxels, threshold):
    """The reference's voxel2pc (util/voxel.py:61-77): (xyz [n,3] float64, occupancies [G^3] bool) of a grid whose
    singleton dimensions are squeezed; numpy arrays for numpy input, device tensors for a tensor.  occupancies is
    (voxels > threshold) flattened; xyz its points in ascending flat index, voxel (i,j,k) at (x[j], x[i], x[k]) with
    x = np.linspace(-0.5, 0.5, G): the reference's 'xy' meshgrid swaps the first two axes, so voxelising xyz gives the mask
    with its first two axes transposed.  ValueError for a grid that is not cubic or has G < 2 (the reference raises)."""
    fn = "voxel2pc"
    is_tensor = isinstance(voxels, torch.Tensor)
    v = _as_float_grid(voxels if is_tensor else np.asarray(voxels), "voxels", fn).squeeze()
    G = _cubic(tuple(v.shape), fn)[0]
    given = [voxels] if is_tensor else []
    _native.require_device(*given)
    dev = _batch.device(_WHAT, given)
    bits = _bits_of_grids(v[None], float(threshold), False, dev)
    xyz, _ = _points_of_bits(bits, G, dev)
    occ = _unpack(bits, (G, G, G)).reshape(-1)
    return (xyz, occ) if is_tensor else (xyz.cpu().numpy(), occ.cpu().numpy())


def iou_of_split(predictions, gt_clouds, reference_rotation=None, vox_size=64, vox_size_z=-1, models_per_call=256):
    """Voxel IoU of every view of M models against the model's ground-truth cloud, both voxelised like voxelise:
    {"stats": [M,V,5] int64, "iou": [M,V] float64 (NaN where the union is empty), "dropped": [M,V] int64 (points of the
    view outside the unit cube, or not finite)}, numpy.

    predictions, gt_clouds, reference_rotation and models_per_call as in chamfer_of_split: per model (points [V,N,3],
    num_points [V] | None), view i truncated to its first num_points[i] points and rotated by the quaternion first; the
    result does not depend on the grouping.  A non-finite coordinate is dropped and sets DPC_STATUS_NONFINITE in the
    status word.  Every argument is checked before anything is launched."""
    fn = "iou_of_split"
    shape = _shape_of(vox_size, vox_size_z, fn)
    split = _split.Split(fn, predictions, gt_clouds, reference_rotation, models_per_call)
    M, V = split.M, split.V
    out = {"stats": np.zeros((M, V, 5), dtype=np.int64), "iou": np.full((M, V), np.nan), "dropped": np.zeros((M, V), dtype=np.int64)}
    if split.empty:
        return out
    dev = _batch.device(_WHAT, *split.tensors())
    for group in split.groups:
        pb, dropped, pairs = _view_bits(split, group, shape, dev, fn)
        gb, _ = _bits_of_clouds([split.gts[m] for m in group], shape, dev, fn)
        stats = _pair_stats(pb, gb, pairs, shape)
        split.store(out["stats"], group, stats)
        split.store(out["iou"], group, _iou(stats))
        split.store(out["dropped"], group, dropped)
    return out


def _view_bits(split, group, shape, dev, fn):
    """(bit grids, dropped, the [P,2] host table of (view, its model's position in the group)) of a group's views."""
    views_list, gt_of = split.views(group, dev)
    pb, dropped = _bits_of_clouds([_batch.cloud(v, fn) for v in views_list], shape, dev, fn)
    return pb, dropped, _batch.table(np.stack([np.arange(len(gt_of)), np.asarray(gt_of)], axis=1), 2, fn)


def render_voxels(voxels, threshold, **kw):
    """The reference's --voxels mode (render_point_cloud_blender.py:199-227): the points of voxel2pc(voxels, threshold)
    drawn by render_point_clouds(**kw): a [S,S,3] image on the device."""
    from .visualise import render_point_clouds

    fn = "render_voxels"
    v = _as_float_grid(voxels if isinstance(voxels, torch.Tensor) else np.asarray(voxels), "voxels", fn).squeeze()
    _cubic(tuple(v.shape), fn)
    xyz, _ = voxel2pc(v if v.is_cuda else v.to(_batch.device(_WHAT, [])), threshold)   # the points stay on the device
    return render_point_clouds([xyz], **kw)[0]
