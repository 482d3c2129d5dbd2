"""Iso-surface extraction on the GPU: occupancy grids to triangle meshes, batched -- the reference's extract_surface and
augment_mesh (dpc/util/voxel.py:80-96), whose marching cubes are skimage's.

    extract_surfaces   grids -> a list of (V float64 [n,3], F int64 [m,3]) device tensors, one count call, one read of
                       the counts and one write call per chunk of grids
    extract_surface    the reference's function: the surface vertices of one grid (with dense: plus the edge midpoints)
    augment_mesh       the reference's helper: vertices followed by the faces' edge midpoints
    save_obj           a mesh as a Wavefront OBJ

The surface rule -- which nodes are inside, where a vertex lies, the order of vertices and faces, how a cell is
triangulated -- is in include/dpc_render.h (dpc_surface_count); every output has one right answer
(tests/surface_oracle.py restates it in numpy).  The meshes are in the form voxelise_meshes, point_mesh_distance,
fscore(gt_meshes=) and render_mesh_views take.
"""
import numpy as np
import torch

from . import _batch, _native
from ._ops import status_word

_WHAT = "dpc.render surface extraction"
MAX_SIDE = _native.DPC_VOXEL_MAX_SIDE
MAX_TRIANGLES = 5                                   # of a cell (csrc/dpc_surface_table.h)
_NODES_PER_CALL = _batch.INT32_MAX // MAX_TRIANGLES   # 3 vertex rows and fewer than 5 face rows a node: both totals fit int32


def _grid(g, name, fn, ranks):
    """One tensor or array of grids, checked: detached, float32 / float64 (bool is cast to float32)."""
    if not isinstance(g, (torch.Tensor, np.ndarray)):
        raise ValueError("%s: %s must be a tensor or an array, got %s" % (fn, name, type(g).__name__))
    if g.ndim not in ranks:
        want = "[D,H,W]" if ranks == (3,) else "[B,D,H,W], [D,H,W] or a list of [D,H,W] grids"
        raise ValueError("%s: %s must be %s, got %s" % (fn, name, want, tuple(g.shape)))
    if isinstance(g, torch.Tensor) and not g.is_cuda:
        raise ValueError("%s: %s must be on a HIP device, got a %s tensor (arrays are copied there)" % (fn, name, g.device))
    t = g if isinstance(g, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(g))
    if t.dtype == torch.bool:
        t = t.to(torch.float32)
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError("%s: %s must be float32, float64 or bool, got %s" % (fn, name, t.dtype))
    sides = tuple(int(s) for s in t.shape[-3:])
    if any(s < 1 for s in sides):
        raise ValueError("%s: %s: a grid of %s has an empty side" % (fn, name, sides))
    if any(s > MAX_SIDE for s in sides):
        raise ValueError("%s: %s: a grid of %s has a side above DPC_VOXEL_MAX_SIDE = %d" % (fn, name, sides, MAX_SIDE))
    return t.detach()


def _grid_list(voxels, fn):
    """voxels as (list of [D,H,W] float32 / float64 tensors, the [B,D,H,W] tensor they are the rows of | None)."""
    if isinstance(voxels, (list, tuple)):
        return [_grid(g, "voxels[%d]" % i, fn, (3,)) for i, g in enumerate(voxels)], None
    t = _grid(voxels, "voxels", fn, (3, 4))
    whole = t[None] if t.dim() == 3 else t
    return list(whole), whole


def _levels(iso_level, B, fn):
    iso = iso_level.detach().cpu().numpy() if isinstance(iso_level, torch.Tensor) else np.asarray(iso_level)
    if iso.dtype == bool or iso.dtype.kind not in "fiu":
        raise ValueError("%s: iso_level must be a number or one number per grid, got %s" % (fn, iso.dtype))
    iso = iso.astype(np.float64)
    if iso.ndim == 0:
        return np.full(B, float(iso))
    if iso.shape != (B,):
        raise ValueError("%s: iso_level must be a number or one number per grid: %d grids, got %s" % (fn, B, iso.shape))
    return np.ascontiguousarray(iso)


def _chunks(grids, grids_per_call):
    """Ranges [a, b) of consecutive grids whose nodes together fit a call."""
    out, a, nodes = [], 0, 0
    for i, g in enumerate(grids):
        n = g.numel()
        if i > a and (nodes + n > _NODES_PER_CALL or (grids_per_call is not None and i - a >= grids_per_call)):
            out.append((a, i))
            a, nodes = i, 0
        nodes += n
    if len(grids) > a:
        out.append((a, len(grids)))
    return out


def _extract_call(grids, packed, iso, dev):
    """One dpc_surface_count + dpc_surface_extract over `grids` (their nodes in `packed`): [(V, F int64)]."""
    B = len(grids)
    sizes = [g.numel() for g in grids]
    start = np.cumsum([0] + sizes)
    desc = _batch.table([(start[i],) + tuple(g.shape) for i, g in enumerate(grids)], 4, "extract_surfaces: table entries must fit int32")
    n_values = int(start[-1])
    L = _native.lib()
    nbytes = L.dpc_surface_workspace_bytes(desc.ctypes.data, B, n_values)
    desc_d = _batch.on_device(desc, dev)
    iso_d = torch.from_numpy(iso).to(dev)
    work = _batch.workspace(nbytes, dev)
    counts_d = torch.empty((B, 2), dtype=torch.int32, device=dev)
    status = status_word(dev)
    f64 = int(packed.dtype == torch.float64)
    _native.call(dev, "dpc_surface_count", _native.ptr(packed), n_values, f64, _native.ptr(desc_d), desc.ctypes.data, B,
                 _native.ptr(iso_d), _native.ptr(counts_d), _native.ptr(work), _native.ptr(status))
    counts = counts_d.cpu().numpy().astype(np.int64)       # the one host synchronisation: the outputs are sized by it
    v0, f0 = np.cumsum(np.concatenate([[0], counts[:, 0]])), np.cumsum(np.concatenate([[0], counts[:, 1]]))
    n_verts, n_faces = int(v0[-1]), int(f0[-1])
    out = _batch.table(np.stack([v0[:-1], counts[:, 0], f0[:-1], counts[:, 1]], axis=1), 4,
                       "extract_surfaces: more than 2^31 - 1 vertices or faces in one call")
    out_d = _batch.on_device(out, dev)
    verts = torch.empty((n_verts, 3), dtype=torch.float64, device=dev)
    faces = torch.empty((n_faces, 3), dtype=torch.int32, device=dev)
    _native.call(dev, "dpc_surface_extract", _native.ptr(packed), n_values, f64, _native.ptr(desc_d), desc.ctypes.data, B,
                 _native.ptr(iso_d), _native.ptr(out_d), out.ctypes.data, n_verts, n_faces, _native.ptr(verts) if n_verts else None,
                 _native.ptr(faces) if n_faces else None, _native.ptr(work), _native.ptr(status))
    faces = faces.long()       # one conversion for the call, not one per mesh
    return list(zip(verts.split([int(c) for c in counts[:, 0]]), faces.split([int(c) for c in counts[:, 1]])))


def extract_surfaces(voxels, iso_level, unit_cube=False, grids_per_call=None):
    """The iso-surfaces of a batch of grids: a list of (V float64 [n,3], F int64 [m,3]) device tensors, one per grid, in
    the form voxelise_meshes, point_mesh_distance, fscore(gt_meshes=) and render_mesh_views take.

    voxels: [B,D,H,W] or [D,H,W] (a list of one mesh comes back), float32 / float64 on the device, or a list of [D,H,W]
    grids of any shapes (they share the calls); arrays are copied to the device.  A bool grid is cast to float32: its
    natural level is 0.5.  iso_level: a number, or one per grid.  A node is inside iff v > iso_level (a NaN is outside);
    every grid edge with exactly one end inside carries one vertex, linearly interpolated in fp64, in index units (node i
    at i, column c is grid axis c), so an fp32 grid and its fp64 copy give the same mesh; faces are wound so that their
    normals point toward lower values; the surface is open at the grid's border; a grid with a side of 1 has vertices and
    no faces.  The full rule, with the order of vertices and faces, is in include/dpc_render.h (dpc_surface_count).

    unit_cube: column c becomes V_c / (G_c - 1) - 0.5 (torch, fp64): the node grid of voxelise, so the mesh lines up with
    clouds in the cube [-1/2, 1/2]^3; needs sides >= 2.  grids_per_call: at most that many grids share a call (default:
    as many as keep a call's vertex and face totals inside int32); the result does not depend on it.  One host
    synchronisation per call (the outputs are sized by the counts).  A crossed edge with a NaN or infinite end sets
    DPC_STATUS_NONFINITE in the status word that check_status() returns.  ValueError, naming the input, before anything
    is launched for a wrong rank, dtype, device or side."""
    fn = "extract_surfaces"
    grids, whole = _grid_list(voxels, fn)
    iso = _levels(iso_level, len(grids), fn)
    if grids_per_call is not None:
        if isinstance(grids_per_call, bool) or not isinstance(grids_per_call, (int, np.integer)) or grids_per_call < 1:
            raise ValueError("%s: grids_per_call must be an integer >= 1, got %r" % (fn, grids_per_call))
        grids_per_call = int(grids_per_call)
    if unit_cube and any(min(g.shape) < 2 for g in grids):
        raise ValueError("%s: unit_cube needs sides >= 2 (one node has no spacing)" % fn)
    if not grids:
        return []
    dev = _batch.device(_WHAT, grids)
    dtype = _batch.widest(grids)
    meshes = []
    for a, b in _chunks(grids, grids_per_call):
        if whole is not None:
            packed = whole[a:b].to(dev).contiguous().reshape(-1)          # rows of one tensor: no copy
        else:
            packed = torch.cat([g.to(device=dev, dtype=dtype).reshape(-1) for g in grids[a:b]])
        meshes += _extract_call(grids[a:b], packed, iso[a:b], dev)
    out = []
    for g, (V, F) in zip(grids, meshes):
        if unit_cube:
            V = V / torch.tensor([s - 1 for s in g.shape], dtype=torch.float64, device=dev) - 0.5
        out.append((V, F))
    return out


def _as_tensor(x):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))


def augment_mesh(verts, faces):
    """The reference's augment_mesh (util/voxel.py:80-87): the vertices followed by the midpoints 0.5 * (v[i1] + v[i2])
    of every face's corners (0,1), then of every face's (1,2), then (0,2); an edge shared by two faces appears twice.
    Tensors in (any device), a tensor out; arrays in, an array out."""
    V, F = _as_tensor(verts), _as_tensor(faces)
    if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
        raise ValueError("augment_mesh: verts and faces must be [n,3] and [m,3], got %s and %s" % (tuple(V.shape), tuple(F.shape)))
    F = F.to(device=V.device, dtype=torch.int64)
    blocks = [V] + [0.5 * (V.index_select(0, F[:, k1]) + V.index_select(0, F[:, k2])) for k1, k2 in ((0, 1), (1, 2), (0, 2))]
    out = torch.cat(blocks, dim=0)
    return out if isinstance(verts, torch.Tensor) else out.numpy()


def extract_surface(voxels, iso_level, dense=False):
    """The reference's extract_surface (util/voxel.py:90-96): the surface vertices of one [D,H,W] grid as a float64 numpy
    array [n,3]; with dense, followed by the edge midpoints in augment_mesh's order.

    Against skimage's Lewiner marching cubes, which the reference calls: the same cube-edge vertices (one per grid edge
    that crosses the level, linearly interpolated, in index units), in this library's order (ascending 3 * flat node index
    + axis) and in float64 where skimage returns float32; none of the interior vertices Lewiner's tables add to some
    cells; the faces, which only `dense` reads, follow this library's table."""
    fn = "extract_surface"
    if not isinstance(voxels, (torch.Tensor, np.ndarray)) or voxels.ndim != 3:
        raise ValueError("%s: voxels must be one [D,H,W] grid, got %s" % (fn, tuple(getattr(voxels, "shape", ()))))
    V, F = extract_surfaces(voxels, iso_level)[0]
    return (augment_mesh(V, F) if dense else V).cpu().numpy()


def save_obj(path, verts, faces):
    """A mesh as a Wavefront OBJ: `v` lines with %.17g (a float64 reads back exactly), then 1-based `f` lines."""
    V = np.asarray(verts.detach().cpu().numpy() if isinstance(verts, torch.Tensor) else verts, dtype=np.float64)
    F = np.asarray(faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else faces)
    if V.ndim != 2 or V.shape[1] != 3 or F.ndim != 2 or F.shape[1] != 3:
        raise ValueError("save_obj: verts and faces must be [n,3] and [m,3], got %s and %s" % (V.shape, F.shape))
    with open(path, "w") as f:
        f.write("".join("v %.17g %.17g %.17g\n" % tuple(v) for v in V.tolist()))
        f.write("".join("f %d %d %d\n" % (a + 1, b + 1, c + 1) for a, b, c in F.astype(np.int64).tolist()))
