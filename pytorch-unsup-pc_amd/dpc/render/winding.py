"""Generalized winding numbers: which side of a mesh a point is on, for the triangle soups this project is used on.

point_mesh_distance says how far a point is from a mesh; this says whether it is inside (csrc/dpc_winding.hip).  The
winding number w(P) = (1 / 4 pi) sum_f Omega_f(P) is 1 inside and 0 outside a closed mesh wound outward and a smooth "how
much inside" for open, self-intersecting and inconsistently closed meshes; it needs no connectivity.

    winding_numbers             per cloud, w of every point (and the int64 sums it is formed from)
    points_inside_meshes        per cloud, bool: w above a threshold, compared in integers -- occupancy labels
    signed_point_mesh_distance  point_mesh_distance, negated inside
    winding_voxels              bool [M,D,H,W]: the grid nodes whose centre is inside, a third solid fill

The rules (the term of one face, its quantisation to 2^-40 and the int64 sum that makes every result independent of the
batching) are stated in include/dpc_render.h (dpc_mesh_winding) and defined by tests/winding_oracle.py.
"""
import math

import numpy as np
import torch

from . import _batch, _native
from ._ops import status_word
from .meshvoxels import _bits_of_meshes, _checked_meshes, _mesh_shape
from .pointmesh import _Plan
from .voxels import _unpack, _words

_WHAT = "dpc.render winding numbers"
FRAC_BITS = _native.DPC_WINDING_FRAC_BITS
QUANTUM = 2.0 ** -FRAC_BITS


def _threshold_q(threshold, fn):
    """llrint(threshold 2^40): what the int64 sums are compared with."""
    try:
        thr = float(threshold)
    except (TypeError, ValueError):
        thr = math.nan
    if not math.isfinite(thr) or not -2.0 ** 20 < thr < 2.0 ** 20:
        raise ValueError("%s: threshold must be a finite number in (-2^20, 2^20), got %r" % (fn, threshold))
    return int(np.rint(thr * 2.0 ** FRAC_BITS))


class _WindingPlan(_Plan):
    """A checked dpc_mesh_winding call: point_mesh_distance's checks, and the entry point's own dry run."""

    def __init__(self, clouds, meshes, mesh_of, fn):
        super().__init__(clouds, meshes, mesh_of, fn)
        n_pts, n_verts, n_faces = self.sizes
        rc = _native.lib().dpc_mesh_winding(None, n_pts, 0, None, n_verts, 0, None, n_faces, None, self.desc.ctypes.data,
                                            len(self.desc), None, None, None, None, None)
        _batch.dry_run(rc, "%s: dpc_mesh_winding refused the table (a mesh of more than 2^22 faces, or too many points, work "
                           "items or workspace slots in one call)" % fn)

    def sums(self, dev, args, winding):
        """(sums [n] int64, w [n] float64 | None) packed in cloud order on dev for packed()'s args: one native call."""
        n = self.sizes[0]
        sums = torch.empty((n,), dtype=torch.int64, device=dev)
        w = torch.empty((n,), dtype=torch.float64, device=dev) if winding else None
        ws = _batch.workspace(_native.lib().dpc_mesh_winding_workspace_bytes(self.desc.ctypes.data, len(self.desc)), dev)
        _native.call(dev, "dpc_mesh_winding", *args, _native.ptr(sums), _native.ptr(w), _native.ptr(ws), _native.ptr(status_word(dev)))
        return sums, w


def winding_numbers(clouds, meshes, mesh_of=None, return_sums=False):
    """The generalized winding number of every point of every cloud about its mesh: a list of float64 device tensors [n_i],
    one per cloud; with return_sums (that list, the list of int64 [n_i] sums), w = sums * 2^-40 exactly.

    clouds, meshes and mesh_of as in point_mesh_distance, with its checks, its exceptions (ValueError and MeshError
    before a device is looked for) and its one finiteness check of the points.  A face contributes
    atan2(det, den) / 2 pi for a = V0 - P, b = V1 - P, c = V2 - P, det = a . (b x c),
    den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|, and 0 when det == 0 (P in its plane or on a vertex, a zero-area face),
    rounded to a multiple of 2^-40; the terms are added as integers, so no result depends on how the clouds are batched
    or ordered.  The faces' winding is the caller's: a closed mesh wound inward gives -1 inside.  A face with a NaN or
    infinite vertex is skipped and sets DPC_STATUS_NONFINITE in the status word that check_status() returns.  All clouds
    go into one native call; the arithmetic is fp64 whatever the inputs are."""
    plan = _WindingPlan(clouds, meshes, mesh_of, "winding_numbers")
    dev = _batch.device(_WHAT, *plan.tensors())
    if plan.sizes[0] == 0:
        sums, w = torch.empty((0,), dtype=torch.int64, device=dev), torch.empty((0,), dtype=torch.float64, device=dev)
    else:
        keep, args = plan.packed(dev)
        sums, w = plan.sums(dev, args, True)
    if not plan.clouds:
        return ([], []) if return_sums else []
    return (plan.split(w), plan.split(sums)) if return_sums else plan.split(w)


def points_inside_meshes(clouds, meshes, mesh_of=None, threshold=0.5):
    """Whether every point of every cloud is inside its mesh: a list of bool device tensors [n_i].  A point is inside when
    its winding sum exceeds llrint(threshold 2^40), an integer compare, so the labels too are independent of the
    batching.  clouds, meshes, mesh_of and every check as in winding_numbers; threshold must be finite and lie in
    (-2^20, 2^20) (ValueError): 0.5 for closed meshes, lower to count the half-enclosed space of an open one."""
    fn = "points_inside_meshes"
    tq = _threshold_q(threshold, fn)
    plan = _WindingPlan(clouds, meshes, mesh_of, fn)
    dev = _batch.device(_WHAT, *plan.tensors())
    if plan.sizes[0] == 0:
        return [torch.empty((0,), dtype=torch.bool, device=dev) for _ in plan.clouds]
    keep, args = plan.packed(dev)
    sums, _ = plan.sums(dev, args, False)
    return plan.split(sums > tq)


def signed_point_mesh_distance(clouds, meshes, mesh_of=None, threshold=0.5, squared=False):
    """point_mesh_distance with a sign: a list of float64 device tensors [n_i], the distance to the mesh's surface negated
    where points_inside_meshes(..., threshold) holds.  The magnitude is point_mesh_distance's bit for bit (the same native
    call on the same packed arguments); +inf (a mesh with no usable face) and NaN pass through as that function gives
    them.  squared: the signed squared distances.  Every check as in points_inside_meshes."""
    fn = "signed_point_mesh_distance"
    tq = _threshold_q(threshold, fn)
    plan = _WindingPlan(clouds, meshes, mesh_of, fn)
    dev = _batch.device(_WHAT, *plan.tensors())
    if plan.sizes[0] == 0:
        return [torch.empty((0,), dtype=torch.float64, device=dev) for _ in plan.clouds]
    keep, args = plan.packed(dev)
    d2 = plan.distance(dev, args)
    sums, _ = plan.sums(dev, args, False)
    mag = d2 if squared else torch.sqrt(d2)
    return plan.split(torch.where((sums > tq) & torch.isfinite(mag), -mag, mag))


def winding_voxels(meshes, vox_size, vox_size_z=-1, threshold=0.5, surface=True):
    """Solid occupancy grids of triangle meshes by their winding numbers: a bool [M,D,H,W] device tensor, the nodes whose
    centre has a winding sum above llrint(threshold 2^40).  Exact for closed meshes like fill "parity", and it neither
    leaks through holes nor fills the concavities "carve" fills.

    meshes, vox_size, vox_size_z, the checks and the frame are voxelise_meshes': node n of an axis of G nodes sits at
    n / (G - 1) - 1/2.  The node centres are formed in the kernel; no [M D H W, 3] tensor exists.  surface: the result is
    OR-ed, on the packed words, with voxelise_meshes(fill="none"), so parts thinner than a voxel survive.  A mesh without
    faces gives an empty grid.  The result feeds voxel_stats / voxel_iou as it is.  threshold as in points_inside_meshes.
    No host synchronisation."""
    fn = "winding_voxels"
    tq = _threshold_q(threshold, fn)
    shape = _mesh_shape(vox_size, vox_size_z, fn)
    items, desc = _checked_meshes(meshes, shape, _native.DPC_MESH_FILL_NONE, fn)
    n_verts, n_faces, M = sum(len(V) for V, _ in items), sum(len(F) for _, F in items), len(items)
    rc = _native.lib().dpc_mesh_winding_voxels(None, n_verts, 0, None, n_faces, None, desc.ctypes.data, M, shape[0], shape[1], shape[2],
                                               tq, None, None, None, None)
    _batch.dry_run(rc, "%s: dpc_mesh_winding_voxels refused the mesh table or the grid %s (a mesh of more than 2^22 faces, or "
                       "too many nodes in one call)" % (fn, (shape,)))
    dev = _batch.device(_WHAT, [x for m in meshes for x in m[:2]])
    bits = torch.empty((M, _words(shape)), dtype=torch.int32, device=dev)
    if M:
        dtype = _batch.widest(V for V, _ in items)
        verts, _ = _batch.pack([V for V, _ in items], dev, dtype)
        faces = torch.from_numpy(np.concatenate([F for _, F in items]).reshape(-1, 3)).to(dev)
        desc_d = _batch.on_device(desc, dev)
        ws = _batch.workspace(_native.lib().dpc_mesh_winding_voxels_workspace_bytes(desc.ctypes.data, M, shape[0], shape[1], shape[2]), dev)
        _native.call(dev, "dpc_mesh_winding_voxels", _native.ptr(verts) if len(verts) else None, n_verts, int(dtype == torch.float64),
                     _native.ptr(faces) if len(faces) else None, n_faces, _native.ptr(desc_d), desc.ctypes.data, M, shape[0], shape[1],
                     shape[2], tq, _native.ptr(bits), _native.ptr(ws), _native.ptr(status_word(dev)))
        if surface:
            bits |= _bits_of_meshes(items, desc, shape, _native.DPC_MESH_FILL_NONE, dev)[0]
    return _unpack(bits, shape)
