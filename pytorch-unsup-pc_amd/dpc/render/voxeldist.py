"""Distances on voxel grids: exact Euclidean distance transforms, signed distance fields, surface shells and an F-score
of occupancy grids, batched on the GPU (csrc/dpc_voxel_edt.hip).

    voxel_distance_transform   squared (int32) or plain (float64) distance of every voxel to the nearest occupied / empty one
    voxel_signed_distance      + distance to the nearest occupied voxel outside, - distance to the nearest empty one inside
    voxel_shell                the occupied voxels with a clear (or missing) face neighbour
    voxel_surface_stats        per (prediction, ground truth) pair and direction: voxels, reached, sum of squares, counts
                               within each threshold
    voxel_fscore               precision, recall and F of those counts
    voxel_fscore_of_split      voxel_fscore of every view of every model against its ground-truth cloud

Where voxel IoU treats every miss alike, these say how far off a voxel is.  Distances are in index units (voxel spacing 1
on every axis) and squared distances are integers, so every count has one right answer; only the square roots and the
ratios are floating point.  The conventions are in include/dpc_render.h (dpc_voxel_edt); sources, thresholding and pairing
are those of voxel_stats (voxels.py).
"""
import numpy as np
import torch

from . import _batch, _native, _split
from ._ops import status_word
from .voxels import _bits_of_clouds, _bits_of_grids, _grid_tensor, _shape_of, _source_bits, _sources, _unpack, _view_bits

_WHAT = "dpc.render voxel distances"
NONE = _native.DPC_VOXEL_EDT_NONE
MAX_THRESHOLDS = _native.DPC_VOXEL_EDT_MAX_THRESHOLDS
_KINDS = (torch.float32, torch.float64, torch.bool, torch.uint8)


def _grids(grids, fn):
    """grids ([B,D,H,W] float32 / float64 / bool / uint8, tensor or array) as a detached tensor; CPU tensors are refused."""
    if not isinstance(grids, (torch.Tensor, np.ndarray)) or grids.ndim != 4:
        raise ValueError("%s: grids must be [B,D,H,W], got %s" % (fn, tuple(getattr(grids, "shape", ()))))
    return _grid_tensor(grids, "grids", fn, _KINDS)


def _threshold(threshold, fn):
    try:
        t = float(threshold)
    except (TypeError, ValueError):
        raise ValueError("%s: threshold must be a number, got %r" % (fn, threshold))
    if t != t:
        raise ValueError("%s: threshold must not be NaN" % fn)
    return t


def _thresholds_sq(thresholds, fn):
    """floor(tau^2), evaluated in fp64, of at most MAX_THRESHOLDS non-negative finite distances in voxel units, as int32.
    A value beyond every possible squared distance is stored as NONE - 1: it counts every reached voxel either way."""
    msg = "%s: thresholds must be a non-empty sequence of at most %d non-negative finite numbers, got %r" % (fn, MAX_THRESHOLDS, thresholds)
    try:
        thr = np.asarray(list(thresholds), dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(msg)
    if thr.size == 0 or thr.size > MAX_THRESHOLDS or not np.isfinite(thr).all() or not (thr >= 0).all():
        raise ValueError(msg)
    return np.ascontiguousarray(np.minimum(np.floor(thr * thr), float(NONE - 1)).astype(np.int32))


def _edt(bits, shape, of_clear):
    """int32 [B,D,H,W]: the squared distance of every voxel of bit grids [B, words] to the nearest set (clear) voxel."""
    B = bits.shape[0]
    sq = torch.empty((B,) + tuple(shape), dtype=torch.int32, device=bits.device)
    if B:
        _native.call(bits.device, "dpc_voxel_edt", _native.ptr(bits), B, shape[0], shape[1], shape[2], int(bool(of_clear)),
                     _native.ptr(sq))
    return sq


def _shell_bits(bits, shape):
    out = torch.empty_like(bits)
    if bits.shape[0]:
        _native.call(bits.device, "dpc_voxel_shell", _native.ptr(bits), int(bits.shape[0]), shape[0], shape[1], shape[2],
                     _native.ptr(out))
    return out


def _field_stats(sq, bits, pairs, shape, thr_sq, out, status=None):
    """dpc_voxel_edt_stats for the host table `pairs` [P,2] of (field, bit grid) into out [P, 3+K] int64."""
    dev = bits.device
    P = len(pairs)
    if P:
        pairs_d = _batch.on_device(pairs, dev)
        status = status_word(dev) if status is None else status
        _native.call(dev, "dpc_voxel_edt_stats", _native.ptr(sq), int(sq.shape[0]), _native.ptr(bits), int(bits.shape[0]),
                     shape[0], shape[1], shape[2], _native.ptr(pairs_d), pairs.ctypes.data, P,
                     thr_sq.ctypes.data if len(thr_sq) else None, len(thr_sq), _native.ptr(out), _native.ptr(status))
    return out


def _grid_bits(grids, threshold, fn):
    """(bit grids, shape) of the grids argument of the single-grid functions: float grids are occupied where
    v >= threshold, as voxel_stats thresholds predictions; bool / uint8 where non-zero."""
    g = _grids(grids, fn)
    thr = _threshold(threshold, fn)
    given = [grids] if isinstance(grids, torch.Tensor) else []
    _native.require_device(*given)
    dev = _batch.device(_WHAT, given)
    return _bits_of_grids(g, thr, True, dev), tuple(g.shape[1:])


def _sqrt(sq):
    """float64 square roots of squared distances, +inf where there was no seed."""
    return torch.where(sq == NONE, torch.full((), float("inf"), dtype=torch.float64, device=sq.device), torch.sqrt(sq.double()))


def voxel_distance_transform(grids, threshold=0.5, to="occupied", squared=True):
    """The exact Euclidean distance of every voxel to the nearest occupied (to="occupied") or empty (to="empty") voxel of
    its grid, in index units: int32 [B,D,H,W] squared distances on the device, DPC_VOXEL_EDT_NONE (2^31 - 1) throughout a
    grid that has no such voxel; with squared=False their float64 square roots, +inf for NONE.

    grids: float32 / float64 [B,D,H,W], occupied where v >= threshold (compared in the grid's dtype, a NaN voxel is empty:
    as voxel_stats thresholds predictions), or bool / uint8, occupied where non-zero.  No host synchronisation.  ValueError
    before a device is looked for when grids are not [B,D,H,W] of those dtypes, a side is outside
    [1, DPC_VOXEL_MAX_SIDE] or `to` is neither word; CPU tensors are refused."""
    fn = "voxel_distance_transform"
    if to not in ("occupied", "empty"):
        raise ValueError("%s: to must be \"occupied\" or \"empty\", got %r" % (fn, to))
    bits, shape = _grid_bits(grids, threshold, fn)
    sq = _edt(bits, shape, to == "empty")
    return sq if squared else _sqrt(sq)


def voxel_signed_distance(grids, threshold=0.5):
    """The signed distance field of occupancy grids, float64 [B,D,H,W] in index units: at an empty voxel + the distance to
    the nearest occupied voxel, at an occupied voxel - the distance to the nearest empty one, with no half-voxel offset
    (so no value lies in (-1, 1)).  An all-empty grid is +inf throughout, an all-full one -inf.  grids, threshold and the
    checks as in voxel_distance_transform."""
    bits, shape = _grid_bits(grids, threshold, "voxel_signed_distance")
    outside, inside = _edt(bits, shape, False), _edt(bits, shape, True)
    return torch.where(outside == 0, -_sqrt(inside), _sqrt(outside))


def voxel_shell(grids, threshold=0.5):
    """The surface shell of occupancy grids, bool [B,D,H,W]: the occupied voxels with at least one of their six face
    neighbours empty or outside the grid.  grids, threshold and the checks as in voxel_distance_transform."""
    bits, shape = _grid_bits(grids, threshold, "voxel_shell")
    return _unpack(_shell_bits(bits, shape), shape)


def _surface_stats(pb, gb, pairs, shape, thr_sq, surface):
    """int64 [P,2,3+K] of prediction bit grids pb, ground-truth bit grids gb and the [P,2] host table of (pred, gt): every
    distinct grid is transformed once, however many pairs it is in."""
    dev = pb.device
    P, C = len(pairs), 3 + len(thr_sq)
    out = torch.zeros((2, P, C), dtype=torch.int64, device=dev)
    if P:
        if surface:
            pb, gb = _shell_bits(pb, shape), _shell_bits(gb, shape)
        to_pred, to_gt = _edt(pb, shape, False), _edt(gb, shape, False)
        _field_stats(to_gt, pb, np.ascontiguousarray(pairs[:, ::-1]), shape, thr_sq, out[0])   # the prediction's voxels in the GT's field
        _field_stats(to_pred, gb, pairs, shape, thr_sq, out[1])                                 # the GT's voxels in the prediction's
    return out.permute(1, 0, 2).contiguous()


def _fscore_of(stats):
    """float64 [P,K,3] (precision, recall, F) of surface stats [P,2,3+K]: a side's share of voxels within the threshold;
    0 / 0 = NaN for an empty side, F = 2 P R / (P + R) and 0 where P + R = 0 (fscore's conventions, pointmesh.py)."""
    n = stats[:, :, 0:1].to(torch.float64)
    share = stats[:, :, 3:].to(torch.float64) / n
    prec, rec = share[:, 0], share[:, 1]
    total = prec + rec
    f = torch.where(total == 0, torch.zeros_like(total), 2.0 * prec * rec / total)
    return torch.stack([prec, rec, f], dim=-1)


def _stats(preds, gts, thresholds, gt_of, vox_size, vox_size_z, threshold, surface, fn):
    pred, gt, pairs, shape = _sources(preds, gts, gt_of, vox_size, vox_size_z, fn)
    thr_sq = _thresholds_sq(thresholds, fn)
    threshold = _threshold(threshold, fn)
    given = [x for x in (preds, gts) if isinstance(x, torch.Tensor)]
    given += [c for x in (preds, gts) if isinstance(x, (list, tuple)) for c in x if isinstance(c, torch.Tensor)]
    _native.require_device(*given)
    dev = _batch.device(_WHAT, given)
    pb, _ = _source_bits(pred, shape, threshold, True, dev, fn)
    gb, _ = _source_bits(gt, shape, 0.0, True, dev, fn)
    return _surface_stats(pb, gb, pairs, shape, thr_sq, bool(surface))


def voxel_surface_stats(preds, gts, thresholds, gt_of=None, vox_size=None, vox_size_z=-1, threshold=0.5, surface=True):
    """What a distance-aware comparison of P (prediction, ground truth) pairs of voxel grids is made of: int64 [P,2,3+K] on
    the device.  Row 0 measures the prediction's voxels in the distance field of the ground truth, row 1 the ground
    truth's voxels in the field of the prediction; the columns are (n, reached, sum_sq, within_1 .. within_K): the voxels
    measured, those of them that have a seed to reach (all or none: none when the other side is empty), the sum of their
    squared distances, and per threshold how many lie within it, sq <= floor(tau_k^2), i.e. distance <= tau_k.  A mean
    surface distance is sqrt-free only as the root mean square, sqrt(sum_sq / reached).

    preds, gts, gt_of, vox_size, vox_size_z and threshold: the sources and the pairing of voxel_stats, exactly (clouds or
    grids on either side, the views of a model sharing a ground truth through gt_of).  surface=True: both the seeds and
    the measured voxels are the grids' shells (voxel_shell); False: all occupied voxels.  thresholds: a non-empty sequence
    of at most 8 non-negative finite distances in voxel units (index spacing; distances ignore vox_size_z's anisotropy).
    Every distinct grid is transformed once, not once per pair; the fields take 4 bytes per voxel per distinct grid.  No
    host synchronisation.  Every argument is checked, with ValueError, before a device is looked for."""
    return _stats(preds, gts, thresholds, gt_of, vox_size, vox_size_z, threshold, surface, "voxel_surface_stats")


def voxel_fscore(preds, gts, thresholds, gt_of=None, vox_size=None, vox_size_z=-1, threshold=0.5, surface=True):
    """Precision, recall and F-score of voxel grids at distance thresholds: float64 [P,K,3] on the device, (precision,
    recall, F) per threshold, from voxel_surface_stats (the same arguments).

    precision[tau] is the share of the prediction's (shell) voxels within tau of the ground truth's, recall[tau] the share
    of the ground truth's within tau of the prediction's, F = 2 P R / (P + R), 0 where P + R = 0.  The empty sides follow
    fscore (pointmesh.py): an empty prediction has precision NaN (0 / 0), and so has its F; a non-empty side measured
    against an empty one reaches nothing and scores 0 (there is nothing to refuse here: the field of an empty grid is
    DPC_VOXEL_EDT_NONE, not an argmin of an empty set).  tau = 0 asks for the same voxel; one voxel off is tau = 1."""
    return _fscore_of(_stats(preds, gts, thresholds, gt_of, vox_size, vox_size_z, threshold, surface, "voxel_fscore"))


def voxel_fscore_of_split(predictions, gt_clouds, thresholds, reference_rotation=None, vox_size=64, vox_size_z=-1,
                          models_per_call=256, surface=True):
    """voxel_fscore of every view of M models against the model's ground-truth cloud, both voxelised like voxelise:
    {"stats": [M,V,2,3+K] int64, "fscore": [M,V,K,3] float64, "dropped": [M,V] int64 (points of the view outside the unit
    cube, or not finite)}, numpy.

    predictions, gt_clouds, reference_rotation, vox_size, vox_size_z and models_per_call as in iou_of_split, with its
    checks; thresholds and surface as in voxel_fscore.  The result does not depend on models_per_call.  A group of models
    needs 4 bytes per voxel per distinct grid for its distance fields: models_per_call * (V + 1) grids, 1.5 GiB at the
    defaults with 5 views of 64^3.  Every argument is checked before anything is launched."""
    fn = "voxel_fscore_of_split"
    shape = _shape_of(vox_size, vox_size_z, fn)
    thr_sq = _thresholds_sq(thresholds, fn)
    split = _split.Split(fn, predictions, gt_clouds, reference_rotation, models_per_call)
    M, V, K = split.M, split.V, len(thr_sq)
    out = {"stats": np.zeros((M, V, 2, 3 + K), dtype=np.int64), "fscore": np.full((M, V, K, 3), np.nan),
           "dropped": np.zeros((M, V), dtype=np.int64)}
    if split.empty:
        return out
    dev = _batch.device(_WHAT, *split.tensors())
    for group in split.groups:
        pb, dropped, pairs = _view_bits(split, group, shape, dev, fn)
        gb, _ = _bits_of_clouds([split.gts[m] for m in group], shape, dev, fn)
        stats = _surface_stats(pb, gb, pairs, shape, thr_sq, bool(surface))
        split.store(out["stats"], group, stats)
        split.store(out["fscore"], group, _fscore_of(stats))
        split.store(out["dropped"], group, dropped)
    return out
