"""Host-side checks of the closest points on meshes (no GPU): the numpy oracle (tests/closest_oracle.py) against the exact
values of the fixture f31_closest.npz within the recorded ratios, closed forms for the seven regions and the zero-area
faces, every refusal of the Python functions and of the entry point before a device is needed, and the exported symbols."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import closest_oracle as C
import mesh_voxels_oracle as MV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def f31(golden):
    return golden("f31_closest.npz")


@pytest.fixture(scope="module")
def f28(golden):
    return golden("f28_point_mesh.npz")


def geometry(f28, f31, name):
    src = f31 if name + "_P" in f31 else f28
    return src[name + "_P"], src[name + "_V"], src[name + "_F"]


class _DeviceLookedFor(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """Valid arguments get as far as looking for a device, and no further, whatever this machine has."""
    from dpc.render import _batch

    def device(*a, **k):
        raise _DeviceLookedFor()

    monkeypatch.setattr(_batch, "device", device)


def test_oracle_meets_the_fixture_within_the_recorded_ratios(f28, f31):
    """mesh_closest (Ericson's region walk in fp64) against the exact closest points, case by case: q, and sum w V rebuilt
    exactly from its weights, no further from the exact Q than the generator recorded; the face among the exact
    near-minimisers; the exact distances those of f28."""
    cap = 16.0                                                       # make_golden_closest.py's CAP, explained there
    assert 0 < float(f31["max_ratio_q"]) <= cap and 0 < float(f31["max_ratio_wv"]) <= cap and float(f31["sliver_ratio_q"]) <= cap
    assert "sliver" in f31["cases"] and "sliver" not in f31["well_shaped"] and len(f31["well_shaped"]) == len(f31["cases"]) - 1
    for name in f31["cases"]:
        P, V, F = geometry(f28, f31, name)
        d2, face, q, w, status = C.mesh_closest(P, V, F)
        want_q, near, unit = f31[name + "_q"], f31[name + "_near"], C.unit_len(P, V)
        fin = np.isfinite(f31[name + "_d2"])
        assert (np.isfinite(d2) == fin).all() and (face[~fin] == -1).all() and np.isnan(q[~fin]).all() and np.isnan(w[~fin]).all(), name
        if name in f31["well_shaped"]:
            assert float(f31[name + "_ratio_q"]) <= float(f31["max_ratio_q"]) and float(f31[name + "_ratio_wv"]) <= float(f31["max_ratio_wv"])
        if name + "_d2" in f28:
            assert np.array_equal(f31[name + "_d2"], f28[name + "_d2"]), name
        v64 = np.asarray(V).astype(np.float64)
        for i in np.nonzero(fin)[0]:
            assert face[i] in near[i] and face[i] >= 0, (name, i)
            assert (w[i] >= 0).all() and abs(w[i].sum() - 1.0) <= 2.0 ** -51, (name, i)
            stored = [Fraction(float(x)) for x in want_q[i]]                     # the ratios were recorded against these
            assert C.point_error(q[i], stored) / unit <= float(f31[name + "_ratio_q"]), (name, i)
            assert C.point_error(C.combine_exact(w[i], v64[F[face[i]]]), stored) / unit <= float(f31[name + "_ratio_wv"]), (name, i)
        assert status == (C.PM.STATUS_NONFINITE if name in ("nan_among", "nan_only") else 0), name


def test_fixture_cases_are_what_they_were_built_for(f28, f31):
    from dpc.render import _native

    T, CH = _native.DPC_PM_FACE_TILE, _native.DPC_PM_FACE_TILE * _native.DPC_PM_CHUNK_TILES
    assert (int(f31["block"]), int(f31["face_tile"]), int(f31["chunk_tiles"])) == (_native.DPC_PM_BLOCK, T, _native.DPC_PM_CHUNK_TILES)
    j = int(f31["dup_j"])
    F = f31["duplicates_F"]
    assert (F[j] == F[j + T]).all() and (F[j] == F[j + CH + 5]).all() and len(F) > j + CH + 5
    assert (f31["duplicates_argmin"] == [j, j + T, j + CH + 5]).all() and (f31["duplicates_near"] == f31["duplicates_argmin"]).all()
    n = len(f31["unique_P"])
    assert f31["unique_argmin"].shape == (n, 1) and (f31["unique_argmin"][:, 0] == np.arange(n)).all()
    assert (f31["unique_near"] == f31["unique_argmin"]).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "f31_closest.npz")) <= os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "f28_point_mesh.npz"))
    assert f31["split_argmin"][:, 0].tolist() == [5, 2 * CH + 7, len(f28["split_F"]) - 1]
    assert np.isnan(f31["nan_only_q"]).all() and (f31["nan_only_argmin"] == -1).all()


def test_exact_and_numpy_definitions_on_closed_forms():
    """Inputs whose answer is known: the seven regions of a triangle, points on it, zero-area faces, the caller's order."""
    tri = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
    want = {(1, 1, 3): ((1, 1, 0), (0.5, 0.25, 0.25)), (1, 1, -3): ((1, 1, 0), (0.5, 0.25, 0.25)), (2, -2, 0): ((2, 0, 0), (0.5, 0.5, 0)),
            (-3, 2, 1): ((0, 2, 0), (0.5, 0, 0.5)), (3, 3, 0): ((2, 2, 0), (0, 0.5, 0.5)), (-1, -1, 2): ((0, 0, 0), (1, 0, 0)),
            (6, -1, 0): ((4, 0, 0), (0, 1, 0)), (-2, 7, 0): ((0, 4, 0), (0, 0, 1)), (2, 2, 0): ((2, 2, 0), (0, 0.5, 0.5))}
    for rot in range(3):                                             # the weights follow the caller's vertex order
        t = tri[rot:] + tri[:rot]
        for p, (q, w) in want.items():
            w = w[rot:] + w[:rot]
            d2 = sum((a - b) ** 2 for a, b in zip(p, q))
            ed2, eq, ew = C.tri_closest_exact(p, *t)
            assert (ed2, eq, ew) == (d2, list(q), [Fraction(x) for x in w]), (rot, p)
            nd2, nq, nw = C.tri_closest(np.array([p], dtype=np.float64), *(np.array([v], dtype=np.float64) for v in t))
            assert nd2[0, 0] == d2 and nq[0, 0].tolist() == list(q) and nw[0, 0].tolist() == list(w), (rot, p)
    a, b, m = (1.0, 1.0, 1.0), (3.0, 1.0, 1.0), (2.0, 1.0, 1.0)
    for faces in ((a, a, a), (a, b, b), (a, b, a), (b, a, a), (a, b, m), (a, m, b)):
        seg = faces != (a, a, a)
        for p, q in (((2.0, 1.0, 3.0), m if seg else a), ((0.0, 1.0, 1.0), a), ((5.0, 2.0, 1.0), b if seg else a), ((1.0, 1.0, 1.0), a)):
            ed2, eq, ew = C.tri_closest_exact(p, *faces)
            assert eq == list(q) and sum(ew) == 1 and min(ew) >= 0, (faces, p)
            assert [sum(ew[k] * Fraction(faces[k][c]) for k in range(3)) for c in range(3)] == list(q), (faces, p)
            nd2, nq, nw = C.tri_closest(np.array([p]), *(np.array([v]) for v in faces))
            assert nq[0, 0].tolist() == list(q) and nd2[0, 0] == ed2 and nw[0, 0].sum() == 1 and nw[0, 0].min() >= 0, (faces, p)
            assert (nw[0, 0] @ np.array(faces)).tolist() == list(q), (faces, p)
    V = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [8, 0, 0]], dtype=np.float64)
    n = C.face_normals(V, [[0, 1, 2], [1, 0, 2], [0, 1, 3], [2, 2, 2]])
    assert n.tolist() == [[0, 0, 1], [0, 0, -1], [0, 0, 0], [0, 0, 0]]
    d2, face, q, w, status = C.mesh_closest([[1, 1, 3]], V, [[0, 1, 3], [0, 1, 2], [1, 2, 0]])
    assert (d2[0], face[0], q[0].tolist(), w[0].tolist(), status) == (9.0, 1, [1, 1, 0], [0.5, 0.25, 0.25], 0)   # the lowest of equals


def test_header_symbols_and_abi():
    from dpc.render import _native
    import dpc.render as R

    header = open(os.path.join(ROOT, "include", "dpc_render.h")).read()
    assert int(re.search(r"#define DPC_ABI_VERSION (\d+)", header).group(1)) == 15 == _native.lib().dpc_abi_version() == _native.ABI_VERSION
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("dpc_point_mesh_closest", "dpc_point_mesh_closest_workspace_bytes"):
        assert name in _native.SYMBOLS and hasattr(lib, name), name
        assert not name.startswith(("dpc_drc_", "dpc_rgb_", "dpc_depth_"))
    assert re.search(r"\bint dpc_point_mesh_closest\(", header) and re.search(r"\bsize_t dpc_point_mesh_closest_workspace_bytes\(", header)
    for name in ("closest_points_on_meshes", "point_surface_loss", "face_normals_at"):
        assert name in R.__all__ and callable(getattr(R, name)), name
    csrc = os.path.join(ROOT, "pytorch-unsup-pc_amd", "csrc")
    for src in ("dpc_point_mesh.hip", "dpc_closest.hip"):             # one per-face arithmetic, shared
        assert '#include "dpc_point_mesh.h"' in open(os.path.join(csrc, src)).read(), src
    shared = open(os.path.join(csrc, "dpc_point_mesh.h")).read()
    assert "pm_stage(" in shared and "pm_d2(" in shared
    assert "pm_d2(" in open(os.path.join(csrc, "dpc_closest.hip")).read() and "atomicMin" not in open(os.path.join(csrc, "dpc_closest.hip")).read()


def _tab(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 6))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """dpc_point_mesh_closest with NULL device pointers returns what dpc_point_mesh_distance returns for the same table:
    DPC_ERR_SHAPE for what the header lists (an oversized table among it), DPC_ERR_NULL (nothing launched) for valid
    arguments, DPC_OK when there is nothing to do; the workspace is sized from the host table."""
    from dpc.render import _native

    L, SHAPE, NUL, N = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL, None

    def both(rows, n_pts=10, n_verts=5, n_faces=3, pairs=None):
        t = _tab(rows)
        tp = t.ctypes.data_as(ctypes.c_void_p) if len(t) else N
        k = len(t) if pairs is None else pairs
        rc = L.dpc_point_mesh_closest(N, n_pts, 0, N, n_verts, 0, N, n_faces, N, tp, k, N, N, N, N, N, N, N, N)
        assert rc == L.dpc_point_mesh_distance(N, n_pts, 0, N, n_verts, 0, N, n_faces, N, tp, k, N, N, N, N), rows
        return rc

    good = (0, 10, 0, 5, 0, 3)
    assert both([good]) == NUL and both([good, (0, 0, 0, 5, 0, 3), (2, 3, 0, 5, 1, 2)]) == NUL
    assert both([]) == 0 and both([(0, 0, 0, 5, 0, 3)]) == 0 and both([(0, 0, 0, 0, 0, 0)]) == 0
    assert L.dpc_point_mesh_closest(N, 10, 0, N, 5, 0, N, 3, N, N, 1, N, N, N, N, N, N, N, N) == NUL
    assert both([good], n_pts=-1) == SHAPE and both([good], n_verts=-1) == SHAPE and both([good], n_faces=-1) == SHAPE
    assert both([], pairs=-1) == SHAPE
    for row in ((0, 11, 0, 5, 0, 3), (1, 10, 0, 5, 0, 3), (-1, 5, 0, 5, 0, 3), (0, -1, 0, 5, 0, 3), (0, 10, 0, 6, 0, 3), (0, 10, 1, 5, 0, 3),
                (0, 10, -1, 5, 0, 3), (0, 10, 0, -1, 0, 3), (0, 10, 0, 5, 0, 4), (0, 10, 0, 5, 1, 3), (0, 10, 0, 5, -1, 3),
                (0, 10, 0, 5, 0, -1), (0, 10, 0, 5, 0, 0), (0, 10, 0, 5, 3, 0)):
        assert both([row]) == SHAPE, row
    big = 2 ** 31 - 1
    assert both([(0, big, 0, 5, 0, 3)], n_pts=big) == NUL                                   # the most one call takes
    oversized = [(0, big, 0, 5, 0, 3), (0, 1, 0, 5, 0, 3)]
    assert both(oversized, n_pts=big) == SHAPE                                               # 2^31 output points
    ws = lambda rows: L.dpc_point_mesh_closest_workspace_bytes(_tab(rows).ctypes.data_as(ctypes.c_void_p), len(rows))
    assert ws(oversized) == 0 and ws([(0, 10, 0, 5, 0, 0)]) == 0
    assert L.dpc_point_mesh_closest_workspace_bytes(N, 1) == 0 and L.dpc_point_mesh_closest_workspace_bytes(_tab([good]).ctypes.data_as(ctypes.c_void_p), 0) == 0
    one = ws([good])                                                                         # one chunk: a slot per point
    assert one >= 3 * 2 * 4 + 10 * 12 and one % 16 == 0
    CH = _native.DPC_PM_FACE_TILE * _native.DPC_PM_CHUNK_TILES
    split = ws([(0, 3, 0, 5, 0, 4 * CH + 1)])                                                # 3 points, 5 chunks of faces
    assert split >= 3 * 2 * 4 + 5 * 3 * 12 and split % 16 == 0 and split > ws([(0, 3, 0, 5, 0, CH)])


def test_refusals_come_before_a_device_is_needed(no_device):
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    good, pts = (V, F), np.zeros((4, 3), dtype=np.float32)
    for fn in (R.closest_points_on_meshes, R.point_surface_loss, R.face_normals_at):
        name = fn.__name__
        with pytest.raises(_DeviceLookedFor):
            fn([pts, pts[:0]], [good], mesh_of=[0, 0])
        with pytest.raises(_DeviceLookedFor):
            fn([pts[:0]], [(V, F[:0])])                                           # no faces, but no points either
        with pytest.raises(ValueError, match=r"%s: clouds\[1\] must be \[n,3\]" % name):
            fn([pts, pts[:, :2]], [good, good])
        with pytest.raises(ValueError, match=r"mesh 1: V must be \[n,3\]"):
            fn([pts, pts], [good, (V[:, :2], F)])
        with pytest.raises(ValueError, match=r"mesh 0: F must be \[f,3\]"):
            fn([pts], [(V, F[:, :2])])
        with pytest.raises(ValueError, match="mesh 0: F must hold integers"):
            fn([pts], [(V, F.astype(np.float32))])
        with pytest.raises(R.MeshError, match=r"mesh 1: F holds a vertex index outside \[0, 12\)"):
            fn([pts, pts], [good, (V, F + 1)])
        with pytest.raises(ValueError, match=r"mesh 0 must be \(V \[n,3\], F \[f,3\], ...\)"):
            fn([pts], [V])
        with pytest.raises(R.MeshError, match=r"mesh 1 has no faces but clouds\[2\] has points"):
            fn([pts, pts, pts], [good, (V, F[:0])], mesh_of=[0, 0, 1])
        with pytest.raises(ValueError, match="2 clouds and 1 meshes need mesh_of"):
            fn([pts, pts], [good])
        for bad in ([0], [0, 1], [0, -1], [0, 0.0]):
            with pytest.raises(ValueError, match="mesh_of must map each of the 2 clouds to one of 1 meshes"):
                fn([pts, pts], [good], mesh_of=bad)
    with pytest.raises(_DeviceLookedFor):
        R.closest_points_on_meshes([pts], [good], normals=True)
    with pytest.raises(_DeviceLookedFor):
        R.point_surface_loss([torch.zeros(4, 3, requires_grad=True)], [good])


def test_a_device_is_needed_after_the_checks():
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    if not torch.cuda.is_available():
        for fn in (R.closest_points_on_meshes, R.point_surface_loss, R.face_normals_at):
            with pytest.raises(RuntimeError, match="MI355X only"):
                fn([np.zeros((4, 3), dtype=np.float32)], [(V, F)])


def test_normal_consistency_gt_meshes_refusals(no_device):
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    p, g = np.zeros((4, 3), dtype=np.float32), np.ones((5, 3))
    pts = np.zeros((2, 10, 3), dtype=np.float32)
    with pytest.raises(_DeviceLookedFor):
        R.normal_consistency([p, p], [g], gt_of=[0, 0], gt_meshes=[(V, F)])
    with pytest.raises(_DeviceLookedFor):
        R.normal_consistency_of_split([(pts, None)], [g], gt_meshes=[(V, F)])
    with pytest.raises(ValueError, match="normal_consistency: give gt_normals or gt_meshes, not both"):
        R.normal_consistency([p], [g], gt_normals=[np.ones((5, 3))], gt_meshes=[(V, F)])
    with pytest.raises(ValueError, match="normal_consistency_of_split: give gt_normals or gt_meshes, not both"):
        R.normal_consistency_of_split([(pts, None)], [g], gt_normals=[np.ones((5, 3))], gt_meshes=[(V, F)])
    with pytest.raises(ValueError, match="1 GT clouds and 2 GT meshes"):
        R.normal_consistency([p], [g], gt_meshes=[(V, F), (V, F)])
    with pytest.raises(ValueError, match="1 GT clouds and 2 GT meshes"):
        R.normal_consistency_of_split([(pts, None)], [g], gt_meshes=[(V, F), (V, F)])
    with pytest.raises(R.MeshError, match="mesh 0: F holds a vertex index outside"):
        R.normal_consistency([p], [g], gt_meshes=[(V, F + 1)])
    with pytest.raises(R.MeshError, match=r"mesh 0 has no faces but gts\[0\] has points"):
        R.normal_consistency([p], [g], gt_meshes=[(V, F[:0])])
    with pytest.raises(R.MeshError, match="mesh 0: F holds a vertex index outside"):           # the second group's mesh
        R.normal_consistency_of_split([(pts, None)] * 2, [g, g], gt_meshes=[(V, F), (V, F + 1)], models_per_call=1)


def test_bench_tool_workloads_and_operation_count():
    """tools/bench_closest_points.py without a device: it takes bench_point_mesh's workloads and states its count."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_closest_points", os.path.join(ROOT, "tools", "bench_closest_points.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.FLOPS_PER_TEST == mod.PM.FLOPS_PER_TEST + 3 == 83
    assert mod.mesh is mod.PM.mesh
