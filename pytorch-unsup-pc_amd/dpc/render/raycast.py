"""Ray-mesh intersection: what a ray hits first, how many faces it crosses, and which surface samples a viewpoint sees.

point_mesh_distance, closest_points_on_meshes and winding_numbers answer questions about points; this answers "what does
a ray from here hit" (csrc/dpc_raycast.hip): the occlusion test between a camera and ground-truth samples, partial scans
of a mesh by arbitrary ray bundles, a crossing count along any direction, and the face, weights and normal where a ray lands.

    ray_mesh_intersect  per bundle (t, face, weights, hits[, normal]): the first hit of every ray and the faces it crosses
    rays_hit_points     per bundle, the hit points O + t D, NaN for a miss
    visible_points      per cloud, bool: no face between the viewpoint and the point

A ray is O + t D with D NOT normalised: t is in units of |D|, t = 1 is the point O + D.  The rules (the Moeller-Trumbore
test with a division-free decision, inclusive ends, the lowest face index among bit-equal t) are stated in
include/dpc_render.h (dpc_ray_mesh_intersect) and defined by tests/raycast_oracle.py.  The test is not watertight along
shared edges: a ray exactly through an edge may report both faces or neither.
"""
import collections
import math

import numpy as np
import torch

from . import _batch, _native
from ._ops import status_word
from .pointmesh import _Plan

_WHAT = "dpc.render ray-mesh intersection"

RayHits = collections.namedtuple("RayHits", "t face weights hits")
RayHitsNormals = collections.namedtuple("RayHitsNormals", "t face weights hits normal")


def _t_range(t_min, t_max, fn):
    try:
        lo, hi = float(t_min), float(t_max)
    except (TypeError, ValueError):
        lo = hi = math.nan
    if not lo <= hi:
        raise ValueError("%s: t_min and t_max must be numbers with t_min <= t_max, got %r and %r" % (fn, t_min, t_max))
    return lo, hi


class _RayPlan(_Plan):
    """A checked dpc_ray_mesh_intersect call: point_mesh_distance's checks with the origins for clouds (a mesh without
    faces is allowed, every ray misses it), the directions' own, and the entry point's dry run."""

    def __init__(self, origins, directions, meshes, mesh_of, t_min, t_max, fn, names=("origins", "directions")):
        super().__init__(origins, meshes, mesh_of, fn, names[0], empty_ok=True)
        self.t_range = _t_range(t_min, t_max, fn)
        self.dirs = [_batch.cloud(d, "%s: %s[%d]" % (fn, names[1], i)) for i, d in enumerate(directions)]
        if len(self.dirs) != len(self.clouds):
            raise ValueError("%s: %d %s and %d %s" % (fn, len(self.clouds), names[0], len(self.dirs), names[1]))
        for i, (o, d) in enumerate(zip(self.clouds, self.dirs)):
            if o.shape != d.shape or o.dtype != d.dtype:
                raise ValueError("%s: %s[%d] is %s %s but %s[%d] is %s %s" % (fn, names[0], i, tuple(o.shape), o.dtype, names[1], i,
                                                                             tuple(d.shape), d.dtype))
        n_rays, n_verts, n_faces = self.sizes
        rc = _native.lib().dpc_ray_mesh_intersect(None, None, n_rays, 0, None, n_verts, 0, None, n_faces, None, self.desc.ctypes.data,
                                                  len(self.desc), self.t_range[0], self.t_range[1], 0, None, None, None, None, None,
                                                  None, None, None)
        _batch.dry_run(rc, "%s: dpc_ray_mesh_intersect refused the table (too many rays, work items or workspace slots in one "
                           "call)" % fn)

    def tensors(self):
        return self.clouds, self.dirs, [V for V, _ in self.items]

    def intersect(self, dev, cull_backfaces, normals, rays=None):
        """(t [n], face [n] int32, weights [n,3], hits [n] int32, normal [n,3] | None) packed in bundle order on dev: one
        native call.  rays: (origins, directions) already packed on dev in one dtype, instead of this plan's bundles."""
        n = self.sizes[0]
        t = torch.empty((n,), dtype=torch.float64, device=dev)
        face, hits = (torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(2))
        weights = torch.empty((n, 3), dtype=torch.float64, device=dev)
        normal = torch.empty((n, 3), dtype=torch.float64, device=dev) if normals else None
        if n:
            if rays is None:
                dtype = _batch.widest(self.clouds)
                rays = _batch.pack(self.clouds, dev, dtype)[0], _batch.pack(self.dirs, dev, dtype)[0]
            keep, args = self.packed(dev, pts=rays[0])
            ws = _batch.workspace(_native.lib().dpc_ray_mesh_workspace_bytes(self.desc.ctypes.data, len(self.desc)), dev)
            _native.call(dev, "dpc_ray_mesh_intersect", args[0], _native.ptr(rays[1]), args[1], args[2], *args[3:], self.t_range[0],
                         self.t_range[1], int(bool(cull_backfaces)), _native.ptr(t), _native.ptr(face), _native.ptr(weights),
                         _native.ptr(hits), _native.ptr(normal), _native.ptr(ws), _native.ptr(status_word(dev)))
        return t, face, weights, hits, normal


def ray_mesh_intersect(origins, directions, meshes, mesh_of=None, t_min=0.0, t_max=math.inf, cull_backfaces=False, normals=False):
    """The first hit of every ray of every bundle with its mesh: one record per bundle, RayHits(t [n], face [n] int32,
    weights [n,3], hits [n] int32) and with normals a fifth field normal [n,3]; device tensors, float64 but for the ints.

    origins, directions: lists of [n,3] float32 / float64 tensors or arrays, origins[i] and directions[i] of one shape and
    dtype; meshes and mesh_of as in point_mesh_distance, except that a mesh without faces is allowed: every ray misses it.
    A ray is O + t D; D is not normalised, so t counts in units of |D|.  A face is hit when the ray's line meets the closed
    triangle and t_min <= t <= t_max (both inclusive; t_max may be inf).  t is the smallest hit parameter, face its index
    in the mesh's F as passed (the lowest among faces with bit-equal t), weights the hit's weights on F[face]'s three
    vertices in the order F lists them, hits the number of faces hit, normal the unit normal (V1 - V0) x (V2 - V0) of
    F[face].  A miss gives t = +inf, face = -1, NaN weights and a zero normal.  cull_backfaces: faces the ray meets from
    behind (D . normal > 0) are no hits.  A zero D misses everything.  Rays exactly through a shared edge or vertex may
    report both faces or neither: the test is not watertight.

    A ray with a NaN or infinite component gives t = NaN, face = -1, hits = 0 and sets DPC_STATUS_NONFINITE in the status
    word that check_status() returns, as does a face with such a vertex, which is skipped.  All bundles go into one native
    call; no result depends on how they are batched or ordered, and there is no host synchronisation.  ValueError or
    MeshError, naming the input, before a device is looked for."""
    plan = _RayPlan(origins, directions, meshes, mesh_of, t_min, t_max, "ray_mesh_intersect")
    dev = _batch.device(_WHAT, *plan.tensors())
    out = [plan.split(x) for x in plan.intersect(dev, cull_backfaces, normals) if x is not None]
    return [(RayHitsNormals if normals else RayHits)(*rec) for rec in zip(*out)]


def rays_hit_points(origins, directions, hits):
    """The points the rays land on, O + t D per bundle: a list of [n,3] float64 tensors on the device of hits[i].t, one
    multiplication and one addition per coordinate in fp64; NaN for a miss and for a ray that was not finite.
    hits: what ray_mesh_intersect returned for these origins and directions (or any sequence of records with a field t)."""
    fn = "rays_hit_points"
    origins, directions, hits = list(origins), list(directions), list(hits)
    if not len(origins) == len(directions) == len(hits):
        raise ValueError("%s: %d origins, %d directions and %d records" % (fn, len(origins), len(directions), len(hits)))
    O = [_batch.cloud(o, "%s: origins[%d]" % (fn, i)) for i, o in enumerate(origins)]
    D = [_batch.cloud(d, "%s: directions[%d]" % (fn, i)) for i, d in enumerate(directions)]
    out = []
    for i, (o, d, h) in enumerate(zip(O, D, hits)):
        t = h.t
        if not isinstance(t, torch.Tensor) or o.shape != d.shape or t.shape != (len(o),):
            raise ValueError("%s: origins[%d], directions[%d] and hits[%d].t do not describe the same rays" % (fn, i, i, i))
        o, d = (x.to(device=t.device, dtype=torch.float64) for x in (o, d))
        hit = torch.isfinite(t)
        p = o + torch.where(hit, t, torch.zeros_like(t))[:, None] * d
        out.append(torch.where(hit[:, None], p, torch.full_like(p, math.nan)))
    return out


def _viewpoints(viewpoints, n, fn):
    """[n,3] float64 on the host from one [3] for all clouds or one per cloud."""
    try:
        if isinstance(viewpoints, torch.Tensor):
            v = viewpoints.detach().cpu().numpy()
        else:
            v = np.asarray([x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x for x in viewpoints])
        v = v.astype(np.float64)
    except (TypeError, ValueError):
        v = np.zeros(0)
    if v.shape == (3,):
        v = np.broadcast_to(v, (n, 3))
    if v.shape != (n, 3) or not np.isfinite(v).all():
        raise ValueError("%s: viewpoints must be one finite [3] for all clouds or one per cloud (%d)" % (fn, n))
    return np.array(v)   # a writable copy: torch.from_numpy warns about a broadcast view


def visible_points(clouds, meshes, viewpoints, eps, mesh_of=None):
    """Which points of every cloud its viewpoint sees: a list of bool device tensors [n_i].  Point P is visible from the
    viewpoint C iff the ray O = C, D = P - C (formed in fp64) hits no face of the cloud's mesh with t in [0, 1 - eps].

    clouds, meshes, mesh_of as in ray_mesh_intersect (a cloud's points are the rays' targets); viewpoints: one [3] per
    cloud, or a single [3] for all.  eps is required and has no default: it is the relative slack that keeps the face a
    sample lies on from occluding it, and must exceed the samples' own distance from their faces divided by |P - C| --
    about 1e-6 for float32 samples of unit-size meshes, smaller for float64 ones; 0 <= eps < 1.  A point equal to its
    viewpoint is visible (a zero D hits nothing); a point with a NaN or infinite coordinate is not, and sets
    DPC_STATUS_NONFINITE.  For the ground-truth samples a training view can see, pass that view's camera position.  One
    native call; ValueError or MeshError before a device is looked for."""
    fn = "visible_points"
    try:
        slack = float(eps)
    except (TypeError, ValueError):
        slack = math.nan
    if not 0.0 <= slack < 1.0:
        raise ValueError("%s: eps must be a number in [0, 1), got %r" % (fn, eps))
    clouds = list(clouds)
    plan = _RayPlan(clouds, clouds, meshes, mesh_of, 0.0, 1.0 - slack, fn, names=("clouds", "clouds"))
    view = _viewpoints(viewpoints, len(plan.clouds), fn)
    dev = _batch.device(_WHAT, *plan.tensors())
    if plan.sizes[0] == 0:
        return [torch.empty((0,), dtype=torch.bool, device=dev) for _ in plan.clouds]
    target = _batch.pack(plan.clouds, dev, torch.float64)[0]
    counts = torch.tensor([len(c) for c in plan.clouds], dtype=torch.int64, device=dev)
    origin = torch.repeat_interleave(torch.from_numpy(view).to(dev), counts, dim=0, output_size=len(target))
    t = plan.intersect(dev, False, False, rays=(origin.contiguous(), (target - origin).contiguous()))[0]
    return plan.split(t == math.inf)
