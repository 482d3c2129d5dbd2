"""Mesh densification of ground-truth models on the GPU (densify/densify_single.py with densify/utils.py).

The reference parses each ShapeNet model.obj, then splits its longest edge densifyN = 100 000 times, one Python step
each, and saves the parsed vertices followed by the midpoints as "points".  Here the parsing stays on the host
(load_obj_mesh: the edge order is a CPython set's iteration order, which only the host can reproduce) and the splits of
a whole group of models run in one dpc_densify job (csrc/dpc_densify.hip), in rounds of many splits each.  Every output
point equals the reference's, in the reference's order, bit for bit.

    load_obj_mesh    parseObj + removeWeirdDuplicate: (V [n,3] float64, E [e,2], F [f,3]) in the reference's orders
    densify_meshes   the splits for many meshes: a list of [n + num_points, 3] float64 numpy arrays
    densify_split    densify_single.py's per-model work for a list of names, models_per_call models per job

Reading .obj files and writing .mat files stays with the caller (load_mesh, save), as everywhere in this package.
"""
import numbers

import numpy as np
import torch

from . import _batch, _native, _split

ROUNDS_PER_SYNC = 8  # rounds enqueued between two reads of the "models left" counter


class MeshError(ValueError):
    """A model the library refused or could not densify as the reference would (a status bit of its job)."""


def load_obj_mesh(path):
    """The reference's parseObj(path) followed by removeWeirdDuplicate(F) (densify/utils.py), in numpy.

    Vertices are the lines whose first split(" ") token is "v"; faces the first three "/"-fields of the "f" lines, kept
    when np.linalg.matrix_rank of their three vertices is 3 (so faces in a plane through the origin are dropped too);
    edges the (min, max) pairs of the kept faces, in the iteration order of a CPython set of tuples filled in face order.
    Then every face's indices are sorted, the faces sorted, and adjacent duplicates dropped, with the reference's quirk:
    its first step compares F[0] with F[-1], so a file whose faces are all one triangle ends with no faces (its three
    edges stay).  Returns (V [n,3] float64, E [e,2] int64, F [f,3] int64).

    Malformed input raises where the reference raises (ValueError or IndexError).  One divergence: a face index <= 0 in
    the file (negative after the reference's "- 1") raises ValueError; the reference would wrap it around the vertex
    array with numpy's negative indexing, which no OBJ reader means by it."""
    verts = []
    for rest in _obj_records(path, "v", " "):
        if len(rest) < 3:
            raise IndexError("load_obj_mesh: %s: a vertex line with %d coordinates" % (path, len(rest)))
        verts.append([float(x) for x in rest[:3]])
    V = np.array(verts, dtype=np.float64).reshape(-1, 3)
    corners = []
    for rest in _obj_records(path, "f", None):
        if len(rest) < 3:
            raise IndexError("load_obj_mesh: %s: a face line with %d indices" % (path, len(rest)))
        corners.append([int(field.split("/", 1)[0]) - 1 for field in rest[:3]])  # vertex field; a quad's 4th is unused
    F = np.array(corners, dtype=np.int64).reshape(-1, 3)
    if len(F) and F.min() < 0:
        raise ValueError("load_obj_mesh: %s: face index %d <= 0 (relative OBJ indices are refused)" % (path, F.min() + 1))
    if len(F) and F.max() >= len(V):
        raise IndexError("load_obj_mesh: %s: face index %d beyond the %d vertices" % (path, F.max() + 1, len(V)))
    F = F[np.linalg.matrix_rank(V[F]) == 3] if len(F) else F  # the per-face rank test, on a [F,3,3] stack
    if len(F) == 0:  # the reference fails on its empty face array
        raise ValueError("load_obj_mesh: %s has no face of rank 3" % path)
    pairs = np.sort(F[:, [[0, 1], [0, 2], [1, 2]]], axis=2).reshape(-1, 2)  # face by face: (0,1), (0,2), (1,2)
    edges = set(map(tuple, pairs.tolist()))  # filled in that order; its iteration order is the reference's edge order
    E = np.array(list(edges), dtype=np.int64).reshape(-1, 2)
    return V, E, _unique_faces(F)


def _obj_records(path, tag, sep):
    """The fields after the first of every line of `path` whose first field is `tag`, the stripped line split on sep."""
    with open(path) as fh:
        for text in fh:
            fields = text.strip().split(sep)
            if fields and fields[0] == tag:
                yield fields[1:]


def _unique_faces(F):
    """Faces with sorted indices, sorted and without repeats; when they are all one face, none (the reference compares
    its first face with its last one as well)."""
    uniq = np.unique(np.sort(F, axis=1), axis=0)
    return uniq[:0] if len(uniq) == 1 else uniq


def _budget(num_points):
    if isinstance(num_points, bool) or not isinstance(num_points, numbers.Integral):
        raise ValueError("densify: num_points must be an integer, got %r" % (num_points,))
    n = int(num_points)
    if n < 0:
        raise ValueError("densify: num_points must be >= 0, got %d" % n)
    return n


def _mesh(mesh, i):
    """(V, E, F) -> (V float64 [n,3], E int32 [e,2], F int32 [f,3], face_edges int32 [f,3], most faces on an edge)."""
    V, E, F = mesh
    V = np.ascontiguousarray(V, dtype=np.float64)
    E, F = np.asarray(E), np.asarray(F)
    if V.ndim != 2 or V.shape[1] != 3:
        raise ValueError("densify: mesh %d: V must be [n,3], got %s" % (i, V.shape))
    E = E.reshape(-1, 2) if E.size == 0 else E
    F = F.reshape(-1, 3) if F.size == 0 else F
    if E.ndim != 2 or E.shape[1] != 2 or F.ndim != 2 or F.shape[1] != 3:
        raise ValueError("densify: mesh %d: E must be [e,2] and F [f,3], got %s and %s" % (i, E.shape, F.shape))
    if len(E) == 0:
        raise ValueError("densify: mesh %d has no edges" % i)
    if not np.isfinite(V).all():
        raise ValueError("densify: mesh %d holds a NaN or inf vertex coordinate" % i)
    n = len(V)
    for name, a in (("E", E), ("F", F)):
        if a.size and (a.min() < 0 or a.max() >= n):
            raise ValueError("densify: mesh %d: %s holds a vertex index outside [0, %d)" % (i, name, n))
    if (E[:, 0] == E[:, 1]).any():
        raise ValueError("densify: mesh %d: an edge joins a vertex to itself" % i)
    lo, hi = np.minimum(E[:, 0], E[:, 1]).astype(np.int64), np.maximum(E[:, 0], E[:, 1]).astype(np.int64)
    keys = lo * n + hi
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    if (sk[1:] == sk[:-1]).any():
        raise ValueError("densify: mesh %d: E holds an edge twice" % i)
    F64 = F.astype(np.int64)
    ends = F64[:, [[1, 2], [0, 2], [0, 1]]]  # the two vertices of the edge opposite vertex j
    want = np.minimum(ends[..., 0], ends[..., 1]) * n + np.maximum(ends[..., 0], ends[..., 1])
    pos = np.minimum(np.searchsorted(sk, want), len(sk) - 1)
    if len(F) and not (sk[pos] == want).all():
        f, j = np.argwhere(sk[pos] != want)[0]
        raise ValueError("densify: mesh %d: face %d's edge (%d, %d) is not in E" % (i, f, ends[f, j, 0], ends[f, j, 1]))
    fe = order[pos].astype(np.int32).reshape(F.shape)
    most = int(np.bincount(fe.ravel(), minlength=len(E)).max()) if len(F) else 0
    return V, E.astype(np.int32), F.astype(np.int32), fe, most


def _densify_packed(meshes, n, rounds_per_sync=ROUNDS_PER_SYNC):
    """One dpc_densify job.  Returns (out [sum(v_i + n), 3] float64 on the device, [v_i + n] rows per model, rounds)."""
    C = len(meshes)
    desc_rows = []
    vo = eo = fo = 0
    for V, E, F, _, _ in meshes:
        desc_rows.append((vo, len(V), eo, len(E), fo, len(F), n))
        vo, eo, fo = vo + len(V), eo + len(E), fo + len(F)
    desc = _batch.table(desc_rows, 7,
                        "densify: more than 2^31 - 1 vertices, edges or faces, or num_points %d, in one job" % n)
    most = max(mm[4] for mm in meshes)
    L = _native.lib()
    host_desc = desc.ctypes.data
    _batch.dry_run(L.dpc_densify(None, vo, None, eo, None, None, fo, None, host_desc, C, most, 1, 0, None, None, None,
                                 None, None),
                   "densify: refused by dpc_densify (%d models, num_points %d: an id would pass 2^31 - 1)" % (C, n),
                   MeshError)
    dev = _batch.device("dpc.render densification")
    cat = lambda k, dt, w: torch.from_numpy(np.concatenate([mm[k] for mm in meshes]).astype(dt).reshape(-1, w)).to(dev)
    verts, edges, faces, face_edges = cat(0, np.float64, 3), cat(1, np.int32, 2), cat(2, np.int32, 3), cat(3, np.int32, 3)
    rows = [len(mm[0]) + n for mm in meshes]
    out = torch.empty((max(sum(rows), 1), 3), dtype=torch.float64, device=dev)
    info = torch.zeros((2,), dtype=torch.int32, device=dev)  # status, models with splits left
    desc_d = _batch.on_device(desc, dev)
    ws = _batch.workspace(L.dpc_densify_workspace_bytes(C, eo, fo, C * n, most), dev)
    rounds, begin = 0, 1
    while True:
        _native.call(dev, "dpc_densify", _native.ptr(verts), vo, _native.ptr(edges), eo, _native.ptr(faces),
                     _native.ptr(face_edges), fo, _native.ptr(desc_d), host_desc, C, most, begin, rounds_per_sync,
                     _native.ptr(out), _native.ptr(info[:1]), _native.ptr(info[1:]), _native.ptr(ws))
        rounds += rounds_per_sync
        begin = 0
        status, left = (int(x) for x in info.cpu().tolist())  # one synchronisation per rounds_per_sync rounds
        if status or left == 0:
            break
        if rounds > n + rounds_per_sync:  # every round splits at least one edge of every model with splits left
            raise RuntimeError("dpc_densify: %d rounds and %d models still unfinished" % (rounds, left))
    _batch.raise_status(status, [
        (_native.DPC_STATUS_NONFINITE, "densify: a vertex, edge length or midpoint is not finite"),
        (_native.DPC_STATUS_BAD_INDEX, "densify: dpc_densify found an inconsistent mesh"),
        (_native.DPC_STATUS_DENSIFY_ORDER, "densify: a new edge was longer than 0.87 x its round's longest edge; the round "
         "order does not hold for this mesh and the output would not be the reference's")], MeshError)
    return out, rows, rounds


def _groups(items, n, step, workspace_limit):
    """Consecutive index ranges of items, each at most `step` models and, unless it is one model, at most
    workspace_limit bytes of dpc_densify workspace: the bound grows with the batch's largest face count per edge, so one
    strongly non-manifold model does not inflate a whole batch."""
    L = _native.lib()
    start, e, f, most = 0, 0, 0, 0
    for k, it in enumerate(items):
        e2, f2, most2 = e + len(it[1]), f + len(it[2]), max(most, it[4])
        if k > start and (k - start >= step or L.dpc_densify_workspace_bytes(k - start + 1, e2, f2, (k - start + 1) * n,
                                                                             most2) > workspace_limit):
            yield start, k
            start, e2, f2, most2 = k, len(it[1]), len(it[2]), it[4]
        e, f, most = e2, f2, most2
    if start < len(items):
        yield start, len(items)


def _densify_group(items, n, rounds_per_sync=ROUNDS_PER_SYNC):
    out, rows, _ = _densify_packed(items, n, rounds_per_sync)
    host = out.cpu().numpy()
    res, o = [], 0
    for r in rows:
        res.append(host[o:o + r].copy())
        o += r
    return res


WORKSPACE_LIMIT = 32 << 30  # bytes of dpc_densify workspace per job (a single model may need more)


def densify_meshes(meshes, num_points=100000, rounds_per_sync=ROUNDS_PER_SYNC, workspace_limit=WORKSPACE_LIMIT):
    """densify_single.py's points for every mesh: a list of [n_i + num_points, 3] float64 numpy arrays.

    meshes: a list of (V [n,3], E [e,2], F [f,3]) as load_obj_mesh returns them (E in the order the reference lists its
    edges, F after removeWeirdDuplicate).  Row i < n_i is V[i]; row n_i + s is the midpoint made by split s.  The meshes
    run in as few jobs as workspace_limit allows.  ValueError, before anything touches a device, for a negative
    num_points, a mesh without edges, non-finite coordinates, indices out of range or a face whose edges are not in E.
    num_points = 0 returns the vertices once; the reference's V[-0:] would save them twice."""
    n = _budget(num_points)
    items = [_mesh(m, i) for i, m in enumerate(meshes)]
    res = []
    for a, b in _groups(items, n, len(items), workspace_limit):
        res += _split.isolate(lambda group: _densify_group(group, n, rounds_per_sync), items[a:b],
                              ["mesh %d" % k for k in range(a, b)], None)
    return res


def densify_split(model_names, load_mesh, num_points=100000, save=None, models_per_call=256, errors=None, keep=True,
                  workspace_limit=WORKSPACE_LIMIT):
    """densify_single.py over model_names, at most models_per_call models (and workspace_limit bytes of workspace) per
    dpc_densify job.

    load_mesh(name) -> (V, E, F) (load_obj_mesh(path), say), or None to skip the model; save(name, points) is called with
    each [n + num_points, 3] float64 result (scipy.io.savemat(path, {"points": points}), say).  Returns {name: points},
    or {} with keep=False (results then only go to save).  The result does not depend on the batching.  A model whose
    loading or densification fails raises an error that names it; with an `errors` dict it is recorded there
    (errors[name] = message) and skipped instead, and the other models go on."""
    n = _budget(num_points)
    step = _split.checked_step("densify_split", models_per_call)
    result = {}

    def load(name, i):
        mesh = load_mesh(name)
        return None if mesh is None else _mesh(mesh, i)

    for batch in _split.batches(model_names, load, step, errors, (ValueError, IndexError, OSError)):
        names, items = [name for name, _ in batch], [item for _, item in batch]
        for a, b in _groups(items, n, step, workspace_limit):
            for name, pts in zip(names[a:b], _split.isolate(lambda group: _densify_group(group, n), items[a:b], names[a:b], errors)):
                if pts is None:
                    continue
                if keep:
                    result[name] = pts
                if save is not None:
                    save(name, pts)
    return result
