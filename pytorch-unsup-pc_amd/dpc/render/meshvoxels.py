"""Solid ground-truth occupancy grids from triangle meshes on the GPU: the `Volume` arrays the reference expects
ready-made (dpc/run/create_tf_records.py:104-115, made off-line with binvox), and the volumetric IoU of solid grids that
PTN, DRC and 3D-R2N2 report.

    voxelise_meshes      meshes -> bool [M,D,H,W]: the nodes whose cube meets a face, filled ("carve", "parity") or not
    carve_voxels         the "carve" fill for any bool grids, e.g. the shell of a predicted cloud
    solid_iou_of_split   iou_of_split against the models' meshes instead of their clouds, both sides filled

The rules (the surface test, the two fills, the counts) are this library's own; they are stated in
include/dpc_render.h (dpc_voxelise_meshes) and defined by tests/mesh_voxels_oracle.py.  Grid, axis order and bit layout
are those of voxelise, so the grid of a mesh and the grid of a cloud of the same model line up.
"""
import numpy as np
import torch

from . import _batch, _native, _split
from ._ops import status_word
from .densify import MeshError
from .voxels import MAX_SIDE, _bits_of_grids, _grid_tensor, _iou, _pair_stats, _shape_of, _unpack, _view_bits, _words

_WHAT = "dpc.render mesh voxelisation"
FILLS = {"none": _native.DPC_MESH_FILL_NONE, "carve": _native.DPC_MESH_FILL_CARVE, "parity": _native.DPC_MESH_FILL_PARITY}


def _fill(fill, fn):
    if not isinstance(fill, str) or fill not in FILLS:
        raise ValueError("%s: fill must be one of %s, got %r" % (fn, ", ".join(repr(k) for k in FILLS), fill))
    return FILLS[fill]


def _mesh_shape(vox_size, vox_size_z, fn):
    shape = _shape_of(vox_size, vox_size_z, fn)
    if any(s < 2 for s in shape):
        raise ValueError("%s: a grid of %s has a side below 2 (sides are 2 .. DPC_VOXEL_MAX_SIDE = %d)" % (fn, shape, MAX_SIDE))
    return shape


def _mesh(mesh, i, fn):
    """(V [n,3] float32 / float64 tensor, F [f,3] int32 host array) of mesh i; only its first two entries are read."""
    if not isinstance(mesh, (tuple, list)) or len(mesh) < 2:
        raise ValueError("%s: mesh %d must be (V [n,3], F [f,3], ...)" % (fn, i))
    V = _batch.cloud(mesh[0], "%s: mesh %d: V" % (fn, i))
    F = mesh[1]
    F = F.detach().cpu().numpy() if isinstance(F, torch.Tensor) else np.asarray(F)
    if F.size == 0:
        F = F.reshape(-1, 3)
    if F.ndim != 2 or F.shape[1] != 3:
        raise ValueError("%s: mesh %d: F must be [f,3], got %s" % (fn, i, tuple(F.shape)))
    if F.dtype.kind not in "iu" and F.size:
        raise ValueError("%s: mesh %d: F must hold integers, got %s" % (fn, i, F.dtype))
    if F.size and (F.min() < 0 or F.max() >= len(V)):
        raise MeshError("%s: mesh %d: F holds a vertex index outside [0, %d)" % (fn, i, len(V)))
    return V, np.ascontiguousarray(F, dtype=np.int32)


def _checked_meshes(meshes, shape, fill, fn):
    """Every argument check of a dpc_voxelise_meshes call, the library's own included, before a device is looked for:
    (items, host table [M,4])."""
    items = [_mesh(m, i, fn) for i, m in enumerate(meshes)]
    nv, nf = [len(V) for V, _ in items], [len(F) for _, F in items]
    vs, fs = np.cumsum([0] + nv), np.cumsum([0] + nf)
    if vs[-1] > _batch.INT32_MAX or fs[-1] > _batch.INT32_MAX:
        raise ValueError("%s: more than 2^31 - 1 vertices or faces in one call" % fn)
    desc = _batch.table(np.stack([vs[:-1], nv, fs[:-1], nf], axis=1) if items else np.zeros((0, 4)), 4,
                        "%s: mesh table entries must fit int32" % fn)
    rc = _native.lib().dpc_voxelise_meshes(None, int(vs[-1]), 0, None, int(fs[-1]), None, desc.ctypes.data,
                                           len(items), shape[0], shape[1], shape[2], fill, None, None, None, None, None)
    _batch.dry_run(rc, "%s: dpc_voxelise_meshes refused the mesh table or the grid %s" % (fn, (shape,)))
    return items, desc


def _bits_of_meshes(items, desc, shape, fill, dev, status=None):
    """(bit grids int32 [M, words], info int32 [M,2]) of checked meshes: one dpc_voxelise_meshes call."""
    M = len(items)
    bits = torch.empty((M, _words(shape)), dtype=torch.int32, device=dev)
    info = torch.zeros((M, 2), dtype=torch.int32, device=dev)
    if M:
        dtype = _batch.widest(V for V, _ in items)
        verts, _ = _batch.pack([V for V, _ in items], dev, dtype)
        faces = torch.from_numpy(np.concatenate([F for _, F in items]).reshape(-1, 3)).to(dev)
        scratch = torch.empty_like(bits) if fill == _native.DPC_MESH_FILL_CARVE else None
        desc_d = _batch.on_device(desc, dev)
        status = status_word(dev) if status is None else status
        _native.call(dev, "dpc_voxelise_meshes", _native.ptr(verts) if len(verts) else None, int(verts.shape[0]),
                     int(dtype == torch.float64), _native.ptr(faces) if len(faces) else None, int(faces.shape[0]), _native.ptr(desc_d),
                     desc.ctypes.data, M, shape[0], shape[1], shape[2], fill, _native.ptr(bits), _native.ptr(scratch),
                     _native.ptr(info), _native.ptr(status))
    return bits, info


def _carved(bits, shape):
    """The "carve" fill of bit grids [B, words]: a new tensor."""
    out = torch.empty_like(bits)
    if bits.shape[0]:
        _native.call(bits.device, "dpc_voxel_carve", _native.ptr(bits), int(bits.shape[0]), shape[0], shape[1], shape[2],
                     _native.ptr(out))
    return out


def voxelise_meshes(meshes, vox_size, vox_size_z=-1, fill="carve", return_info=False):
    """Occupancy grids of triangle meshes: a bool [M,D,H,W] device tensor, D = vox_size_z (vox_size when -1), H = W = vox_size.

    meshes: a list of (V [n,3] float32 / float64, F [f,3] integers, ...), tensors or arrays; only the first two entries
    are read, so what load_obj_scene and load_obj_mesh's (V, E, F)[::2] return works as it is.  Vertex column c goes to grid
    axis c, over [-1/2, 1/2]^3 like voxelise.  A node is set when its cube [n - 1/2, n + 1/2]^3 (in grid units) meets a
    face; fill "none" leaves that surface, "carve" (the default) adds every node that none of the six axis directions
    sees past the surface (robust to open and self-intersecting meshes), "parity" adds the nodes an odd number of faces
    lie below along grid axis 0 (exact for closed meshes, leaks through holes).  A mesh without faces gives an empty grid.
    With return_info: (grids, int32 [M,2] on the device: faces with a vertex outside the cube, columns crossed an odd number
    of times -- 0 unless fill is "parity").  A face with a NaN or infinite vertex is skipped and sets DPC_STATUS_NONFINITE
    in the status word that check_status() returns.  No host synchronisation.  ValueError (MeshError for a face index out
    of range), naming the mesh, before anything is launched for V or F of the wrong shape, a bad fill, or a side outside
    [2, DPC_VOXEL_MAX_SIDE]."""
    fn = "voxelise_meshes"
    code = _fill(fill, fn)
    shape = _mesh_shape(vox_size, vox_size_z, fn)
    items, desc = _checked_meshes(meshes, shape, code, fn)
    dev = _batch.device(_WHAT, [x for m in meshes for x in m[:2]])     # meshes may live on the host, as for densify_meshes
    bits, info = _bits_of_meshes(items, desc, shape, code, dev)
    grids = _unpack(bits, shape)
    return (grids, info) if return_info else grids


def carve_voxels(grids):
    """The "carve" fill of voxelise_meshes for any occupancy grids: bool or uint8 (non-zero) [B,D,H,W], tensor or array ->
    bool [B,D,H,W] on the device.  A voxel is kept or added iff each of the three grid lines through it has an occupied
    voxel at an index <= its own and one at an index >= its own; the input is a subset of the result and carving twice
    changes nothing.  ValueError before anything is launched for grids that are not 4-D bool / uint8 or have a side above
    DPC_VOXEL_MAX_SIDE."""
    fn = "carve_voxels"
    if not isinstance(grids, (torch.Tensor, np.ndarray)) or grids.ndim != 4:
        raise ValueError("%s: grids must be [B,D,H,W], got %s" % (fn, tuple(getattr(grids, "shape", ()))))
    g = _grid_tensor(grids, "grids", fn, (torch.bool, torch.uint8))
    given = [grids] if isinstance(grids, torch.Tensor) else []
    _native.require_device(*given)
    dev = _batch.device(_WHAT, given)
    shape = tuple(int(s) for s in g.shape[1:])
    return _unpack(_carved(_bits_of_grids(g, 0.0, True, dev), shape), shape)


def solid_iou_of_split(predictions, meshes, reference_rotation=None, vox_size=32, vox_size_z=-1, fill="carve", carve_predictions=True,
                       models_per_call=256):
    """Volumetric IoU of every view of M models against the model's mesh: the view's cloud voxelised like voxelise and,
    with carve_predictions, filled like carve_voxels; the mesh voxelised and filled like voxelise_meshes(fill=fill).
    Returns iou_of_split's dict -- {"stats": [M,V,5] int64, "iou": [M,V] float64 (NaN where the union is empty),
    "dropped": [M,V] int64} -- plus "info": [M,2] int64, voxelise_meshes' counts per mesh; numpy.

    predictions, reference_rotation and models_per_call as in iou_of_split; meshes as in voxelise_meshes, one per model.
    The result does not depend on the grouping.  Every argument is checked before anything is launched."""
    fn = "solid_iou_of_split"
    code = _fill(fill, fn)
    shape = _mesh_shape(vox_size, vox_size_z, fn)
    split = _split.Split(fn, predictions, meshes, reference_rotation, models_per_call, noun="meshes", gt_label=None)
    checked = [_checked_meshes([meshes[m] for m in g], shape, code, fn) for g in split.groups]
    M, V = split.M, split.V
    out = {"stats": np.zeros((M, V, 5), dtype=np.int64), "iou": np.full((M, V), np.nan), "dropped": np.zeros((M, V), dtype=np.int64),
           "info": np.zeros((M, 2), dtype=np.int64)}
    if M == 0:
        return out
    dev = _batch.device(_WHAT, *split.tensors(), [x for m in meshes for x in m[:2]])
    for group, (items, desc) in zip(split.groups, checked):
        gb, info = _bits_of_meshes(items, desc, shape, code, dev)
        out["info"][group[0]:group[-1] + 1] = info.cpu().numpy()
        if V == 0:
            continue
        pb, dropped, pairs = _view_bits(split, group, shape, dev, fn)
        if carve_predictions:
            pb = _carved(pb, shape)
        stats = _pair_stats(pb, gb, pairs, shape)
        split.store(out["stats"], group, stats)
        split.store(out["iou"], group, _iou(stats))
        split.store(out["dropped"], group, dropped)
    return out
