"""Exact point-to-mesh distance and the F-score of a whole split in batched GPU calls.

Every other distance of the evaluation is measured against sampled ground truth (densify_gt.py, then downsample_gt.py at
voxel size 0.01), so a predicted point lying exactly on the surface still gets a distance of the order of the sample
spacing -- the size of the thresholds an F-score is reported at.  point_mesh_distance measures against the triangles
themselves (csrc/dpc_point_mesh.hip), and fscore can take its precision half from it.

    point_mesh_distance   per cloud, the distance of every point to the nearest point of its mesh's surface
    fscore                precision, recall and their harmonic mean at distance thresholds, [P,T,3] float64
    fscore_of_split       the same for loaded predictions and GT clouds of M models, [M,V,T,3] numpy

The rules of the distance (zero-area faces, non-finite vertices) are stated in include/dpc_render.h
(dpc_point_mesh_distance) and defined by tests/point_mesh_oracle.py.
"""
import numpy as np
import torch

from . import _batch, _native, _split
from ._ops import status_word
from .chamfer import nearest_batched
from .densify import MeshError
from .meshvoxels import _mesh

_WHAT = "dpc.render point-to-mesh distance"
BLOCK, FACE_TILE, CHUNK_TILES = _native.DPC_PM_BLOCK, _native.DPC_PM_FACE_TILE, _native.DPC_PM_CHUNK_TILES


def _index_map(of, n_src, n_tgt, fn, name, src, tgt):
    """of (None: i -> i) as a list of n_src indices into n_tgt items."""
    if of is None:
        if n_src != n_tgt:
            raise ValueError("%s: %d %s and %d %s need %s" % (fn, n_src, src, n_tgt, tgt, name))
        return list(range(n_src))
    of = list(of)
    if len(of) != n_src or any(not isinstance(k, (int, np.integer)) or k < 0 or k >= n_tgt for k in of):
        raise ValueError("%s: %s must map each of the %d %s to one of %d %s" % (fn, name, n_src, src, n_tgt, tgt))
    return [int(k) for k in of]


class _Plan:
    """A checked dpc_point_mesh_distance call: the clouds, the meshes it uses, and the host table.  empty_ok: a mesh
    without faces may serve a cloud with points (an entry point that defines its answer over no faces, which then makes
    its own dry run: dpc_point_mesh_distance refuses such a table)."""

    def __init__(self, clouds, meshes, mesh_of, fn, cloud_name="clouds", map_name="mesh_of", empty_ok=False):
        self.fn, self.cloud_name = fn, cloud_name
        self.clouds = [_batch.cloud(c, "%s: %s[%d]" % (fn, cloud_name, i)) for i, c in enumerate(clouds)]
        items = [_mesh(m, i, fn) for i, m in enumerate(meshes)]
        self.mesh_of = _index_map(mesh_of, len(self.clouds), len(items), fn, map_name, cloud_name, "meshes")
        for i, k in enumerate(self.mesh_of):
            if len(items[k][1]) == 0 and len(self.clouds[i]) > 0 and not empty_ok:
                raise MeshError("%s: mesh %d has no faces but %s[%d] has points (the minimum over an empty set)"
                                % (fn, k, cloud_name, i))
        used = sorted(set(self.mesh_of))
        self.items = [items[k] for k in used]
        slot = {k: j for j, k in enumerate(used)}
        npts = [len(c) for c in self.clouds]
        nv, nf = [len(V) for V, _ in self.items], [len(F) for _, F in self.items]
        ps, vs, fs = np.cumsum([0] + npts), np.cumsum([0] + nv), np.cumsum([0] + nf)
        if max(ps[-1], vs[-1], fs[-1]) > _batch.INT32_MAX:
            raise ValueError("%s: more than 2^31 - 1 points, vertices or faces in one call" % fn)
        rows = [(ps[i], npts[i], vs[slot[k]], nv[slot[k]], fs[slot[k]], nf[slot[k]]) for i, k in enumerate(self.mesh_of)]
        self.desc = _batch.table(np.asarray(rows, dtype=np.int64) if rows else np.zeros((0, 6)), 6,
                                 "%s: table entries must fit int32" % fn)
        self.sizes = (int(ps[-1]), int(vs[-1]), int(fs[-1]))
        if empty_ok:
            return
        rc = _native.lib().dpc_point_mesh_distance(None, self.sizes[0], 0, None, self.sizes[1], 0, None, self.sizes[2], None,
                                                   self.desc.ctypes.data, len(rows), None, None, None, None)
        _batch.dry_run(rc, "%s: dpc_point_mesh_distance refused the table (too many points or work items in one call)" % fn)

    def tensors(self):
        return self.clouds, [V for V, _ in self.items]

    def packed(self, dev, pts=None):
        """The leading arguments both point-to-mesh entry points take, points to n_pairs, on dev (the tuple keeps the
        packed tensors alive), after the one finiteness check of the points.  Needs at least one point.  pts: the packed
        points [sum n_i, 3] on dev when the caller has packed them itself; they are then not checked for finiteness."""
        n_pts, n_verts, n_faces = self.sizes
        pdt, vdt = _batch.widest(self.clouds) if pts is None else pts.dtype, _batch.widest(V for V, _ in self.items)
        check = pts is None
        if pts is None:
            pts, _ = _batch.pack(self.clouds, dev, pdt)
        if check and not bool(torch.isfinite(pts).all()):
            for i, c in enumerate(self.clouds):
                if not bool(torch.isfinite(c).all()):
                    raise ValueError("%s: %s[%d] holds a NaN or inf coordinate" % (self.fn, self.cloud_name, i))
        verts, _ = _batch.pack([V for V, _ in self.items], dev, vdt)
        faces = torch.from_numpy(np.concatenate([F for _, F in self.items]).reshape(-1, 3)).to(dev)
        desc_d = _batch.on_device(self.desc, dev)
        keep = (pts, verts, faces, desc_d)
        return keep, (_native.ptr(pts), n_pts, int(pdt == torch.float64), _native.ptr(verts), n_verts, int(vdt == torch.float64),
                      _native.ptr(faces), n_faces, _native.ptr(desc_d), self.desc.ctypes.data, len(self.desc))

    def distance(self, dev, args):
        """The packed squared distances [sum n_i] float64 on dev, in cloud order, for packed()'s args: one native call."""
        d2 = torch.empty((self.sizes[0],), dtype=torch.float64, device=dev)
        ws = _batch.workspace(_native.lib().dpc_point_mesh_workspace_bytes(len(self.desc)), dev)
        _native.call(dev, "dpc_point_mesh_distance", *args, _native.ptr(d2), _native.ptr(ws), _native.ptr(status_word(dev)))
        return d2

    def run(self, dev):
        """distance() on arguments packed here; an empty tensor when there is no point."""
        if self.sizes[0] == 0:
            return torch.empty((0,), dtype=torch.float64, device=dev)
        keep, args = self.packed(dev)
        return self.distance(dev, args)

    def split(self, t):
        """The packed tensor t as one tensor per cloud."""
        return list(torch.split(t, [len(c) for c in self.clouds]))


def point_mesh_distance(clouds, meshes, mesh_of=None, squared=False):
    """The distance from every point of every cloud to the nearest point of its mesh's surface (the union of the closed
    triangles): a list of float64 device tensors [n_i], one per cloud.

    clouds: a list of [n,3] float32 / float64 tensors or arrays; meshes: a list of (V [n,3], F [f,3] integers, ...) as
    voxelise_meshes takes them, so load_obj_mesh's (V, E, F)[::2] and load_obj_scene's result work as they are; mesh_of: the
    mesh index of each cloud (default i -> i), so the views of one model share one mesh copy.  All clouds go into one
    native call; the arithmetic is fp64 whatever the inputs are.  squared: the squared distances, as the kernel writes
    them; otherwise torch.sqrt of those.

    A zero-area face counts as the segment or point it degenerates to.  A face with a NaN or infinite vertex is skipped
    and sets DPC_STATUS_NONFINITE in the status word that check_status() returns; a cloud whose mesh has no face left gets
    +inf.  No host synchronisation except one finiteness check of the points.  ValueError, naming the input, before a
    device is looked for: clouds, V or F of the wrong shape, a bad mesh_of; MeshError for a face index out of range, or a
    mesh without faces for a cloud with points.  ValueError for a NaN or inf point coordinate, naming the cloud."""
    plan = _Plan(clouds, meshes, mesh_of, "point_mesh_distance")
    dev = _batch.device(_WHAT, *plan.tensors())
    d2 = plan.run(dev)
    out = d2 if squared else torch.sqrt(d2)
    return list(torch.split(out, [len(c) for c in plan.clouds])) if plan.clouds else []


def _thresholds(thresholds, fn):
    try:
        thr = np.asarray(list(thresholds), dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError("%s: thresholds must be a non-empty sequence of positive finite numbers, got %r" % (fn, thresholds))
    if thr.size == 0 or not np.isfinite(thr).all() or not (thr > 0).all():
        raise ValueError("%s: thresholds must be a non-empty sequence of positive finite numbers, got %r" % (fn, thresholds))
    return thr


def _counts_below(dist, counts, thr_d, dev):
    """[len(counts), T] int64: how many of each owner's distances (packed in owner order) lie below each threshold."""
    n = torch.from_numpy(np.asarray(counts, dtype=np.int64)).to(dev)
    owner = torch.repeat_interleave(torch.arange(len(counts), device=dev), n, output_size=int(np.sum(counts)))
    out = torch.zeros((len(counts), thr_d.shape[0]), dtype=torch.int64, device=dev)
    return out.index_add_(0, owner, (dist.to(torch.float64)[:, None] < thr_d[None, :]).to(torch.int64))


def _cloud_counts(srcs, tgts, names, dev, thr_d, fn):
    """Counts below the thresholds of the nearest-neighbour distances srcs[i] -> tgts[i], [len(srcs), T] int64: one
    nearest_batched call per precision (a pair is fp64 when either side is, chamfer_batched's rule).  An empty target is
    at distance +inf: its pair counts nothing and is not issued."""
    out = torch.zeros((len(srcs), thr_d.shape[0]), dtype=torch.int64, device=dev)
    f64 = [s.dtype == torch.float64 or t.dtype == torch.float64 for s, t in zip(srcs, tgts)]
    for want in (False, True):
        sel = [i for i in range(len(srcs)) if f64[i] == want and len(tgts[i]) > 0]
        if not sel:
            continue
        clouds, start, slot = [], [0], {}
        for i in sel:
            for c, name in ((srcs[i], names[i][0]), (tgts[i], names[i][1])):
                if id(c) not in slot:
                    slot[id(c)] = (len(clouds), name)
                    clouds.append(c)
                    start.append(start[-1] + len(c))
        if start[-1] > _batch.INT32_MAX:
            raise ValueError("%s: more than 2^31 - 1 points in one call" % fn)
        packed, _ = _batch.pack(clouds, dev, torch.float64 if want else torch.float32)
        if packed.numel() and not bool(torch.isfinite(packed).all()):
            for c, (_, name) in zip(clouds, slot.values()):
                if not bool(torch.isfinite(c).all()):
                    raise ValueError("%s: %s holds a NaN or inf coordinate" % (fn, name))
        desc = np.asarray([(start[slot[id(srcs[i])][0]], len(srcs[i]), start[slot[id(tgts[i])][0]], len(tgts[i])) for i in sel],
                          dtype=np.int64)
        _, dist, _ = nearest_batched(packed, desc, return_distances=True)
        out[sel] = _counts_below(dist, [len(srcs[i]) for i in sel], thr_d, dev)
    return out


class _FscorePlan:
    """Every host check of an fscore call."""

    def __init__(self, preds, gts, thresholds, gt_of, gt_meshes, fn):
        self.fn = fn
        self.thr = _thresholds(thresholds, fn)
        self.preds = [_batch.cloud(p, "%s: preds[%d]" % (fn, i)) for i, p in enumerate(preds)]
        self.gts = [_batch.cloud(g, "%s: gts[%d]" % (fn, i)) for i, g in enumerate(gts)]
        self.gt_of = _index_map(gt_of, len(self.preds), len(self.gts), fn, "gt_of", "predictions", "GT clouds")
        for i, k in enumerate(self.gt_of):
            if len(self.gts[k]) == 0 and len(self.preds[i]) > 0:
                raise ValueError("%s: GT cloud %d is empty but prediction %d is not (argmin of an empty set)" % (fn, k, i))
        self.mesh = None
        self.meshes = gt_meshes
        if gt_meshes is not None:
            if len(gt_meshes) != len(self.gts):
                raise ValueError("%s: %d GT clouds and %d GT meshes" % (fn, len(self.gts), len(gt_meshes)))
            self.mesh = _Plan(self.preds, gt_meshes, self.gt_of, fn, "preds", "gt_of")

    def tensors(self):
        return [self.preds, self.gts] + ([] if self.meshes is None else [[x for m in self.meshes for x in m[:2]]])

    def run(self, dev):
        P, T = len(self.preds), len(self.thr)
        out = torch.empty((P, T, 3), dtype=torch.float64, device=dev)
        if P == 0:
            return out
        thr_d = torch.from_numpy(self.thr).to(dev)
        gts = [self.gts[k] for k in self.gt_of]
        names = [("preds[%d]" % i, "gts[%d]" % k) for i, k in enumerate(self.gt_of)]
        hit_r = _cloud_counts(gts, self.preds, [(b, a) for a, b in names], dev, thr_d, self.fn)
        if self.mesh is None:
            hit_p = _cloud_counts(self.preds, gts, names, dev, thr_d, self.fn)
        else:
            hit_p = _counts_below(torch.sqrt(self.mesh.run(dev)), [len(p) for p in self.preds], thr_d, dev)
        n_p = torch.tensor([len(p) for p in self.preds], dtype=torch.float64, device=dev)[:, None]
        n_g = torch.tensor([len(g) for g in gts], dtype=torch.float64, device=dev)[:, None]
        prec, rec = hit_p.to(torch.float64) / n_p, hit_r.to(torch.float64) / n_g
        total = prec + rec
        out[:, :, 0], out[:, :, 1] = prec, rec
        out[:, :, 2] = torch.where(total == 0, torch.zeros_like(total), 2.0 * prec * rec / total)
        return out


def fscore(preds, gts, thresholds, gt_of=None, gt_meshes=None):
    """Precision, recall and F-score of every prediction against its ground truth at distance thresholds: [P,T,3] float64
    on the device, (precision, recall, F) for each of the T thresholds.

    precision[tau] is the share of the prediction's points with distance < tau (strictly) to the ground truth, recall[tau]
    the share of the GT cloud's points with distance < tau to the prediction, F = 2 P R / (P + R), 0 where P + R = 0.  An
    empty prediction has precision NaN (0 / 0, as nearest_batched's mean), and so has its F.

    preds, gts: lists of [n,3] tensors or arrays; gt_of: the GT index of each prediction (default i -> i), as in
    chamfer_batched, whose precision rule and finiteness check also apply: the distances are nearest_batched's.
    gt_meshes: one (V, F, ...) per GT cloud, as point_mesh_distance takes them -- the precision side is then measured
    against the meshes' surfaces (exactly, in fp64) instead of the sampled clouds; the recall side stays on the clouds.
    thresholds: a non-empty sequence of positive finite numbers, required: there is no default (the cube has side 1, so
    0.01 is the customary 1 % of the side).  The counts are device reductions over the packed distances; nothing
    synchronises with the host but the finiteness checks.  Every argument is checked before a device is looked for."""
    plan = _FscorePlan(preds, gts, thresholds, gt_of, gt_meshes, "fscore")
    return plan.run(_batch.device(_WHAT, *plan.tensors()))


def fscore_of_split(predictions, gt_clouds, thresholds, reference_rotation=None, gt_meshes=None, models_per_call=256):
    """fscore for every view of M models: [M,V,T,3] float64 numpy.

    predictions, gt_clouds, reference_rotation and models_per_call as in chamfer_of_split (view i is truncated to its first
    num_points[i] points, the rotation is applied to every view first); thresholds and gt_meshes (one mesh per model) as in
    fscore.  The result does not depend on the grouping.  Every argument is checked before anything is launched."""
    fn = "fscore_of_split"
    split = _split.Split(fn, predictions, gt_clouds, reference_rotation, models_per_call, gt_label=fn + ": gt_clouds[%d]",
                         refuse_empty_gt=True)
    if gt_meshes is not None and len(gt_meshes) != len(gt_clouds):
        raise ValueError("%s: %d GT clouds and %d GT meshes" % (fn, len(gt_clouds), len(gt_meshes)))
    thr = _thresholds(thresholds, fn)
    if gt_meshes is not None:   # the meshes' own checks, and the table of every group with the views' sizes
        for g in split.groups:
            sizes = [torch.empty((n, 3), device="meta") for m in g for n in split.counts[m]]
            _Plan(sizes, [gt_meshes[m] for m in g], [j for j in range(len(g)) for _ in range(split.V)], fn, "views", "gt_of")
    out = np.zeros((split.M, split.V, len(thr), 3), dtype=np.float64)
    if split.empty:
        return out
    dev = _batch.device(_WHAT, *split.tensors(), [] if gt_meshes is None else [x for m in gt_meshes for x in m[:2]])
    for group in split.groups:
        views_list, gt_of = split.views(group, dev)
        split.store(out, group, fscore(views_list, [split.gts[m] for m in group], thr, gt_of,
                                       None if gt_meshes is None else [gt_meshes[m] for m in group]))
    return out
