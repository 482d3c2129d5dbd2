"""Closest points on meshes: the nearest face of every point, the closest surface point, a surface loss, mesh normals.

point_mesh_distance says how far a point is from a mesh; this says where the nearest surface point is
(csrc/dpc_closest.hip).  With it the GT meshes can supervise a predicted cloud, not only score it, and a cloud sampled from
a mesh can take its normals from the faces it lies on.

    closest_points_on_meshes  per cloud (d2, face, point, weights[, normal]): the squared distance, the nearest face, the
                              closest point Q of it, Q's weights on the face's vertices, the face's unit normal
    point_surface_loss        [P] float64, the mean squared point-to-surface distance of each cloud; differentiable with
                              respect to the clouds: the gradient of |P - Q|^2 is 2 (P - Q)
    face_normals_at           per cloud, the unit normal of every point's nearest face

The rules (ties between faces, zero-area and non-finite faces, the order of the weights) are stated in
include/dpc_render.h (dpc_point_mesh_closest) and defined by tests/closest_oracle.py.
"""
import collections

import numpy as np
import torch

from . import _batch, _native
from ._ops import status_word
from .pointmesh import _Plan

_WHAT = "dpc.render closest points on meshes"

ClosestPoints = collections.namedtuple("ClosestPoints", "d2 face point weights")
ClosestPointsNormals = collections.namedtuple("ClosestPointsNormals", "d2 face point weights normal")


class _ClosestPlan(_Plan):
    """A checked dpc_point_mesh_closest call: point_mesh_distance's checks, and the entry point's own dry run."""

    def __init__(self, clouds, meshes, mesh_of, fn, cloud_name="clouds", map_name="mesh_of"):
        super().__init__(clouds, meshes, mesh_of, fn, cloud_name, map_name)
        n_pts, n_verts, n_faces = self.sizes
        rc = _native.lib().dpc_point_mesh_closest(None, n_pts, 0, None, n_verts, 0, None, n_faces, None, self.desc.ctypes.data,
                                                  len(self.desc), None, None, None, None, None, None, None, None)
        _batch.dry_run(rc, "%s: dpc_point_mesh_closest refused the table (too many points, work items or workspace slots in "
                           "one call)" % fn)

    def closest(self, dev, normals):
        """(d2 [n], face [n] int32, point [n,3], weights [n,3], normal [n,3] | None) packed in cloud order on dev, float64:
        one native call."""
        n = self.sizes[0]
        d2 = torch.empty((n,), dtype=torch.float64, device=dev)
        face = torch.empty((n,), dtype=torch.int32, device=dev)
        point, weights = (torch.empty((n, 3), dtype=torch.float64, device=dev) for _ in range(2))
        normal = torch.empty((n, 3), dtype=torch.float64, device=dev) if normals else None
        if n:
            keep, args = self.packed(dev)
            ws = _batch.workspace(_native.lib().dpc_point_mesh_closest_workspace_bytes(self.desc.ctypes.data, len(self.desc)), dev)
            _native.call(dev, "dpc_point_mesh_closest", *args, _native.ptr(d2), _native.ptr(face), _native.ptr(point),
                         _native.ptr(weights), _native.ptr(normal), _native.ptr(ws), _native.ptr(status_word(dev)))
        return d2, face, point, weights, normal


def closest_points_on_meshes(clouds, meshes, mesh_of=None, normals=False):
    """The closest surface point of every point of every cloud: one record per cloud, (d2 [n], face [n] int32, point [n,3],
    weights [n,3]) and with normals a fifth field normal [n,3]; float64 device tensors.

    clouds, meshes and mesh_of as in point_mesh_distance, with its checks, its exceptions (ValueError and MeshError
    before a device is looked for) and its one finiteness check of the points.  d2 equals
    point_mesh_distance(..., squared=True).  face indexes the mesh's F as passed; among faces at bit-equal distance the
    lowest index wins.  point is Q, the nearest point of that face; weights are non-negative, sum to 1 and weigh F[face]'s
    three vertices in the order F lists them: Q = sum_k weights[k] V[F[face][k]].  normal is the unit normal
    (V1 - V0) x (V2 - V0) of F[face] in that winding, zeros for a zero-area face.  A mesh with no usable face (every face
    has a NaN or infinite vertex) gives d2 = +inf, face = -1, NaN point and weights, zero normal, and sets
    DPC_STATUS_NONFINITE in the status word that check_status() returns.  All clouds go into one native call; no result
    depends on how they are batched or ordered."""
    plan = _ClosestPlan(clouds, meshes, mesh_of, "closest_points_on_meshes")
    dev = _batch.device(_WHAT, *plan.tensors())
    out = [plan.split(t) for t in plan.closest(dev, normals) if t is not None]
    return [(ClosestPointsNormals if normals else ClosestPoints)(*rec) for rec in zip(*out)]


def face_normals_at(clouds, meshes, mesh_of=None):
    """The unit normal of the mesh face nearest to every point of every cloud: a list of [n,3] float64 device tensors,
    closest_points_on_meshes' normal alone.  For a cloud sampled from its mesh these are the normals of the faces the
    samples lie on, which published normal-consistency numbers use for the ground truth."""
    plan = _ClosestPlan(clouds, meshes, mesh_of, "face_normals_at")
    dev = _batch.device(_WHAT, *plan.tensors())
    return plan.split(plan.closest(dev, True)[4])


def _pair_means(values, counts, dev, fn):
    """np.mean of each of the len(counts) runs of the packed fp64 values, by dpc_chamfer_pair_means: NaN for an empty run,
    the same bits however the runs are grouped into calls."""
    start = np.cumsum([0] + list(counts))
    table = _batch.table(np.asarray([(start[i], n, start[i], n) for i, n in enumerate(counts)], dtype=np.int64), 4,
                         "%s: table entries must fit int32" % fn)
    mean = torch.empty((len(table),), dtype=torch.float64, device=dev)
    ws = _batch.workspace(_native.lib().dpc_chamfer_workspace_bytes(len(table), table.ctypes.data, 1), dev)
    _native.call(dev, "dpc_chamfer_pair_means", _native.ptr(values), 1, _native.ptr(_batch.on_device(table, dev)), table.ctypes.data,
                 len(table), _native.ptr(mean), _native.ptr(ws))
    return mean


class _SurfaceLoss(torch.autograd.Function):
    """mean_j |P_j - Q_j|^2 per cloud; d / dP_j = 2 (P_j - Q_j) / n.  Q moves within the surface as P moves, which changes
    the squared distance only to second order, so Q counts as constant."""

    @staticmethod
    def forward(ctx, plan, dev, *clouds):
        d2, _, q, _, _ = plan.closest(dev, False)
        counts = [len(c) for c in plan.clouds]
        loss = _pair_means(d2.contiguous(), counts, dev, plan.fn)
        if any(ctx.needs_input_grad[2:]):
            ctx.save_for_backward(torch.cat([c.to(device=dev, dtype=torch.float64) for c in plan.clouds]) - q,
                                  torch.tensor(counts, dtype=torch.int64, device=dev))
        ctx.counts = counts
        ctx.like = [(c.dtype, c.device) if isinstance(c, torch.Tensor) else None for c in clouds]
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        resid, counts = ctx.saved_tensors
        # one packed product, elementwise in fp64: (P - Q) * (2 g / n); a point's gradient does not depend on the batch
        scale = torch.repeat_interleave(2.0 * g / counts, counts, output_size=resid.shape[0])
        packed = resid * scale[:, None]
        parts, grads = {}, []
        for i, (like, needed) in enumerate(zip(ctx.like, ctx.needs_input_grad[2:])):
            if like is None or not needed:
                grads.append(None)
                continue
            dtype, device = like
            if dtype not in parts:                       # rounded once to the clouds' dtype, all such clouds at once
                parts[dtype] = torch.split(packed.to(dtype), ctx.counts)
            grads.append(parts[dtype][i].to(device))
        return (None, None) + tuple(grads)


def point_surface_loss(clouds, meshes, mesh_of=None):
    """The mean squared distance from each cloud's points to its mesh's surface: [P] float64 on the device, carrying
    gradient to every cloud tensor that requires it.

    clouds, meshes, mesh_of and every check as in closest_points_on_meshes.  The value of cloud i is the mean of
    point_mesh_distance(..., squared=True)[i], taken by dpc_chamfer_pair_means: bit-reproducible and independent of how
    the clouds are grouped into calls; an empty cloud gives NaN.  backward: the gradient of point P is
    g[i] * 2 (P - Q) / n_i with Q its closest surface point, formed in fp64 and returned in the cloud's dtype.  The meshes
    get no gradient: fine-tune the network that predicts the clouds, with the GT meshes fixed."""
    clouds = list(clouds)
    plan = _ClosestPlan(clouds, meshes, mesh_of, "point_surface_loss")
    dev = _batch.device(_WHAT, *plan.tensors())
    if not plan.clouds:
        return torch.empty((0,), dtype=torch.float64, device=dev)
    given = [c if isinstance(c, torch.Tensor) and c.dtype in (torch.float32, torch.float64) else None for c in clouds]
    return _SurfaceLoss.apply(plan, dev, *given)
