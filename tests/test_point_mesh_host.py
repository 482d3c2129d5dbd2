"""Host-side checks of the point-to-mesh distance and the F-score (no GPU): the numpy oracle (tests/point_mesh_oracle.py)
against the exact values of the fixture f28_point_mesh.npz within the recorded ratios, the F-score rule on hand-made
distances, every refusal of the three Python functions and of the entry point before a device is needed, and the exported
symbol and constants."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import mesh_voxels_oracle as MV
import point_mesh_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("regions", "regions_p32", "on_triangle", "degenerate_only", "degenerate_nearest", "tile_m1", "tile", "tile_p1", "tile_2p1",
         "cross", "blocks", "split", "mm", "sliver", "ico", "nan_without", "nan_among", "nan_only")


@pytest.fixture(scope="module")
def f28(golden):
    return golden("f28_point_mesh.npz")


class _DeviceLookedFor(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """Valid arguments get as far as looking for a device, and no further, whatever this machine has."""
    from dpc.render import _batch

    def device(*a, **k):
        raise _DeviceLookedFor()

    monkeypatch.setattr(_batch, "device", device)


def test_oracle_meets_the_fixture_within_the_recorded_ratios(f28):
    """mesh_d2 (Ericson's region walk in fp64) against the exact values, case by case: no further from them than the
    ratio the generator recorded, all of which are at most 16; +inf exactly where no face is left."""
    assert 0 < float(f28["max_ratio"]) <= 16.0
    for name in CASES:
        P, V, F, want = f28[name + "_P"], f28[name + "_V"], f28[name + "_F"], f28[name + "_d2"]
        got, status = O.mesh_d2(P, V, F)
        fin = np.isfinite(want)
        assert (np.isfinite(got) == fin).all(), name
        assert float(f28[name + "_ratio"]) <= float(f28["max_ratio"])
        if fin.any():
            assert (np.abs(got[fin] - want[fin]) / O.unit(P, V) <= float(f28[name + "_ratio"])).all(), name
        assert status == (O.STATUS_NONFINITE if name in ("nan_among", "nan_only") else 0), name
    for k in range(len(f28["random_T"])):
        P, T = f28["random_P"][k], f28["random_T"][k]
        got, _ = O.mesh_d2(P, T, [[0, 1, 2]])
        assert (np.abs(got - f28["random_d2"][k]) / O.unit(P, T) <= float(f28["random_ratio"])).all(), k


def test_fixture_was_placed_from_the_library_constants(f28):
    from dpc.render import _native

    assert (int(f28["block"]), int(f28["face_tile"]), int(f28["chunk_tiles"])) == (_native.DPC_PM_BLOCK, _native.DPC_PM_FACE_TILE,
                                                                                   _native.DPC_PM_CHUNK_TILES)
    T, C = _native.DPC_PM_FACE_TILE, _native.DPC_PM_FACE_TILE * _native.DPC_PM_CHUNK_TILES
    assert [len(f28[n + "_F"]) for n in ("tile_m1", "tile", "tile_p1", "tile_2p1")] == [T - 1, T, T + 1, 2 * T + 1]
    assert len(f28["blocks_P"]) == _native.DPC_PM_BLOCK + 1 and len(f28["split_F"]) == 4 * C + 1 and len(f28["split_P"]) == 3


def test_exact_and_numpy_definitions_on_closed_forms(f28):
    """The rules on inputs whose answer is known: points on the triangle, the seven regions, zero-area faces."""
    tri = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
    want = {(1, 1, 3): 9, (1, 1, -3): 9, (2, -2, 0): 4, (-3, 2, 1): 10, (3, 3, 0): 2, (-1, -1, 2): 6, (6, -1, 0): 5, (-2, 7, 0): 13,
            (1, 1, 0): 0, (2, 2, 0): 0, (4, 0, 0): 0}
    for p, d2 in want.items():
        assert O.tri_d2_exact(p, *tri) == d2, p
        assert O.tri_d2(np.array([p], dtype=np.float64), *(np.array([v], dtype=np.float64) for v in tri))[0, 0] == d2, p
    a, b = (1.0, 1.0, 1.0), (3.0, 1.0, 1.0)
    for faces in ((a, a, a), (a, b, b), (a, b, a), (b, a, a), (a, b, (2.0, 1.0, 1.0)), (a, (2.0, 1.0, 1.0), b)):
        seg = faces != (a, a, a)
        for p, d2 in (((2.0, 1.0, 3.0), 4 if seg else 5), ((0.0, 1.0, 1.0), 1), ((5.0, 2.0, 1.0), 5 if seg else 17), ((1.0, 1.0, 1.0), 0)):
            assert O.tri_d2_exact(p, *faces) == d2, (faces, p)
            assert O.tri_d2(np.array([p]), *(np.array([v]) for v in faces))[0, 0] == d2, (faces, p)
    assert (f28["on_triangle_d2"][:6] == 0.0).all()
    assert isinstance(O.tri_d2_exact((0.1, 0.2, 0.3), (0, 0, 0), (1, 0, 0), (0, 1, 0)), Fraction)
    V, F = f28["nan_only_V"], f28["nan_only_F"]
    assert np.isinf(O.mesh_d2(f28["nan_only_P"], V, F)[0]).all() and O.mesh_d2_exact(f28["nan_only_P"], V, F) == [None] * 3


def test_fscore_rule_on_hand_made_distances():
    d_pred, d_gt = [0.0, 0.01, 0.02, 0.5], [0.005, 0.01, 0.03]
    got = O.fscore_rule(d_pred, d_gt, [0.01, 0.02, 1.0, 0.001])
    assert got[0].tolist() == [0.25, 1 / 3, 2 * 0.25 * (1 / 3) / (0.25 + 1 / 3)]        # d == tau does not count: strict
    assert got[1, :2].tolist() == [0.5, 2 / 3] and got[2].tolist() == [1.0, 1.0, 1.0]
    assert got[3].tolist() == [0.25, 0.0, 0.0]
    assert O.fscore_rule([0.5], [0.5], [0.1]).tolist() == [[0.0, 0.0, 0.0]]          # P + R = 0 gives 0, not 0 / 0
    empty = O.fscore_rule([], [0.005, 0.5], [0.01])
    assert np.isnan(empty[0, 0]) and empty[0, 1] == 0.5 and np.isnan(empty[0, 2])
    assert (O.nearest_d(np.zeros((2, 3)), np.zeros((0, 3))) == np.inf).all()


def test_header_symbols_constants_and_abi():
    from dpc.render import _native, pointmesh

    header = open(os.path.join(ROOT, "include", "dpc_render.h")).read()
    assert int(re.search(r"#define DPC_ABI_VERSION (\d+)", header).group(1)) == 15 == _native.lib().dpc_abi_version()
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert "dpc_point_mesh_distance" in _native.SYMBOLS and hasattr(lib, "dpc_point_mesh_distance")
    assert "dpc_point_mesh_workspace_bytes" in _native.SYMBOLS and hasattr(lib, "dpc_point_mesh_workspace_bytes")
    assert re.search(r"\bint dpc_point_mesh_distance\(", header) and re.search(r"\bsize_t dpc_point_mesh_workspace_bytes\(", header)
    for name in ("DPC_PM_BLOCK", "DPC_PM_FACE_TILE", "DPC_PM_CHUNK_TILES"):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == getattr(_native, name), name
    assert (pointmesh.BLOCK, pointmesh.FACE_TILE) == (_native.DPC_PM_BLOCK, _native.DPC_PM_FACE_TILE)
    assert _native.DPC_PM_BLOCK % 64 == 0 and 0 < _native.DPC_PM_FACE_TILE <= _native.DPC_PM_BLOCK
    assert float(re.search(r"#define DPC_MESH_VOXEL_MAX_COORD ([0-9.]+)", header).group(1)) == O.MAX_COORD
    import dpc.render as R

    for name in ("point_mesh_distance", "fscore", "fscore_of_split"):
        assert name in R.__all__ and callable(getattr(R, name)), name


def _tab(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 6))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """dpc_point_mesh_distance with NULL device pointers: DPC_ERR_SHAPE for what the header lists, DPC_ERR_NULL (nothing
    launched) for valid arguments, DPC_OK when there is nothing to do."""
    from dpc.render import _native

    L, SHAPE, NUL, N = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL, None

    def pm(rows, n_pts=10, n_verts=5, n_faces=3, pairs=None):
        t = _tab(rows)
        return L.dpc_point_mesh_distance(N, n_pts, 0, N, n_verts, 0, N, n_faces, N, t.ctypes.data_as(ctypes.c_void_p) if len(t) else N,
                                         len(t) if pairs is None else pairs, N, N, N, N)

    good = (0, 10, 0, 5, 0, 3)
    assert pm([good]) == NUL and pm([good, (0, 0, 0, 5, 0, 3), (2, 3, 0, 5, 1, 2)]) == NUL     # shared mesh, an empty row
    assert pm([]) == 0 and pm([(0, 0, 0, 5, 0, 3)]) == 0 and pm([(0, 0, 0, 0, 0, 0)]) == 0      # nothing to write
    assert L.dpc_point_mesh_distance(N, 10, 0, N, 5, 0, N, 3, N, N, 1, N, N, N, N) == NUL
    assert pm([good], n_pts=-1) == SHAPE and pm([good], n_verts=-1) == SHAPE and pm([good], n_faces=-1) == SHAPE
    assert pm([], pairs=-1) == SHAPE
    for row in ((0, 11, 0, 5, 0, 3), (1, 10, 0, 5, 0, 3), (-1, 5, 0, 5, 0, 3), (0, -1, 0, 5, 0, 3), (0, 10, 0, 6, 0, 3), (0, 10, 1, 5, 0, 3),
                (0, 10, -1, 5, 0, 3), (0, 10, 0, -1, 0, 3), (0, 10, 0, 5, 0, 4), (0, 10, 0, 5, 1, 3), (0, 10, 0, 5, -1, 3),
                (0, 10, 0, 5, 0, -1)):
        assert pm([row]) == SHAPE, row
    assert pm([(0, 10, 0, 5, 0, 0)]) == SHAPE and pm([(0, 10, 0, 5, 3, 0)]) == SHAPE    # no faces for a row with points
    big = 2 ** 31 - 1
    assert pm([(0, big, 0, 5, 0, 3), (0, 1, 0, 5, 0, 3)], n_pts=big) == SHAPE            # more than 2^31 - 1 output points
    assert L.dpc_point_mesh_workspace_bytes(0) == 0 and L.dpc_point_mesh_workspace_bytes(-3) == 0
    assert L.dpc_point_mesh_workspace_bytes(5) >= 2 * 6 * 4 and L.dpc_point_mesh_workspace_bytes(5) % 16 == 0


def test_point_mesh_distance_refusals_come_before_a_device_is_needed(no_device):
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    good, pts = (V, F), np.zeros((4, 3), dtype=np.float32)
    with pytest.raises(_DeviceLookedFor):
        R.point_mesh_distance([pts, pts[:0]], [good], mesh_of=[0, 0])
    with pytest.raises(_DeviceLookedFor):
        R.point_mesh_distance([pts[:0]], [(V, F[:0])])                           # no faces, but no points either
    with pytest.raises(ValueError, match=r"clouds\[1\] must be \[n,3\]"):
        R.point_mesh_distance([pts, pts[:, :2]], [good, good])
    with pytest.raises(ValueError, match=r"mesh 1: V must be \[n,3\]"):
        R.point_mesh_distance([pts, pts], [good, (V[:, :2], F)])
    with pytest.raises(ValueError, match=r"mesh 0: F must be \[f,3\]"):
        R.point_mesh_distance([pts], [(V, F[:, :2])])
    with pytest.raises(ValueError, match="mesh 0: F must hold integers"):
        R.point_mesh_distance([pts], [(V, F.astype(np.float32))])
    with pytest.raises(R.MeshError, match=r"mesh 1: F holds a vertex index outside \[0, 12\)"):
        R.point_mesh_distance([pts, pts], [good, (V, F + 1)])
    with pytest.raises(ValueError, match=r"mesh 0 must be \(V \[n,3\], F \[f,3\], ...\)"):
        R.point_mesh_distance([pts], [V])
    with pytest.raises(R.MeshError, match=r"mesh 1 has no faces but clouds\[2\] has points"):
        R.point_mesh_distance([pts, pts, pts], [good, (V, F[:0])], mesh_of=[0, 0, 1])
    with pytest.raises(ValueError, match="2 clouds and 1 meshes need mesh_of"):
        R.point_mesh_distance([pts, pts], [good])
    for bad in ([0], [0, 1], [0, -1], [0, 0.0]):
        with pytest.raises(ValueError, match="mesh_of must map each of the 2 clouds to one of 1 meshes"):
            R.point_mesh_distance([pts, pts], [good], mesh_of=bad)


def test_point_mesh_distance_needs_a_device_after_the_checks():
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="MI355X only"):
            R.point_mesh_distance([np.zeros((4, 3), dtype=np.float32)], [(V, F)])


def test_fscore_refusals_come_before_a_device_is_needed(no_device):
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    p, g = np.zeros((4, 3), dtype=np.float32), np.ones((5, 3))
    with pytest.raises(_DeviceLookedFor):
        R.fscore([p, p[:0]], [g], [0.01, 0.02], gt_of=[0, 0], gt_meshes=[(V, F)])
    with pytest.raises(TypeError):
        R.fscore([p], [g])                                                       # thresholds are required
    for bad in ([], [0.01, 0.0], [-0.01], [float("nan")], [float("inf")], 0.01, ["a"]):
        with pytest.raises(ValueError, match="thresholds must be a non-empty sequence of positive finite numbers"):
            R.fscore([p], [g], bad)
    with pytest.raises(ValueError, match=r"preds\[0\] must be \[n,3\]"):
        R.fscore([p[:, :2]], [g], [0.01])
    with pytest.raises(ValueError, match=r"gts\[0\] must be \[n,3\]"):
        R.fscore([p], [g[0]], [0.01])
    with pytest.raises(ValueError, match="2 predictions and 1 GT clouds need gt_of"):
        R.fscore([p, p], [g], [0.01])
    with pytest.raises(ValueError, match="gt_of must map each of the 2 predictions to one of 1 GT clouds"):
        R.fscore([p, p], [g], [0.01], gt_of=[0, 1])
    with pytest.raises(ValueError, match="GT cloud 0 is empty but prediction 0 is not"):
        R.fscore([p], [g[:0]], [0.01])
    with pytest.raises(ValueError, match="1 GT clouds and 2 GT meshes"):
        R.fscore([p], [g], [0.01], gt_meshes=[(V, F), (V, F)])
    with pytest.raises(R.MeshError, match="mesh 0: F holds a vertex index outside"):
        R.fscore([p], [g], [0.01], gt_meshes=[(V, F + 1)])
    with pytest.raises(R.MeshError, match=r"mesh 0 has no faces but preds\[0\] has points"):
        R.fscore([p], [g], [0.01], gt_meshes=[(V, F[:0])])


def test_fscore_of_split_refusals_come_before_a_device_is_needed(no_device):
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    pts, g = np.zeros((2, 10, 3), dtype=np.float32), np.ones((5, 3))
    with pytest.raises(_DeviceLookedFor):
        R.fscore_of_split([(pts, np.array([10, 0]))], [g], [0.01], gt_meshes=[(V, F)], reference_rotation=np.array([[1.0, 0, 0, 0]]))
    assert R.fscore_of_split([], [], [0.01, 0.02]).shape == (0, 0, 2, 3)
    with pytest.raises(ValueError, match="1 predictions and 2 GT clouds"):
        R.fscore_of_split([(pts, None)], [g, g], [0.01])
    with pytest.raises(ValueError, match="1 GT clouds and 2 GT meshes"):
        R.fscore_of_split([(pts, None)], [g], [0.01], gt_meshes=[(V, F)] * 2)
    with pytest.raises(ValueError, match="models_per_call must be >= 1"):
        R.fscore_of_split([(pts, None)], [g], [0.01], models_per_call=0)
    with pytest.raises(ValueError, match="thresholds must be a non-empty sequence"):
        R.fscore_of_split([(pts, None)], [g], [])
    with pytest.raises(ValueError, match=r"predictions\[0\] points must be \[V,N,3\]"):
        R.fscore_of_split([(pts[0], None)], [g], [0.01])
    with pytest.raises(ValueError, match=r"predictions\[0\] num_points must be 2 integers"):
        R.fscore_of_split([(pts, np.array([11, 0]))], [g], [0.01])
    with pytest.raises(ValueError, match="same number of views"):
        R.fscore_of_split([(pts, None), (pts[:1], None)], [g, g], [0.01])
    with pytest.raises(ValueError, match="GT cloud 0 is empty"):
        R.fscore_of_split([(pts, None)], [g[:0]], [0.01])
    with pytest.raises(ValueError, match="reference_rotation must be a"):
        R.fscore_of_split([(pts, None)], [g], [0.01], reference_rotation=np.ones(4))
    with pytest.raises(R.MeshError, match="mesh 1: F holds a vertex index outside"):
        R.fscore_of_split([(pts, None)] * 2, [g, g], [0.01], gt_meshes=[(V, F), (V, F + 1)], models_per_call=2)
    with pytest.raises(R.MeshError, match="mesh 0: F holds a vertex index outside"):           # the second group's mesh
        R.fscore_of_split([(pts, None)] * 2, [g, g], [0.01], gt_meshes=[(V, F), (V, F + 1)], models_per_call=1)
    with pytest.raises(R.MeshError, match=r"mesh 0 has no faces but views\[0\] has points"):
        R.fscore_of_split([(pts, None)], [g], [0.01], gt_meshes=[(V, F[:0])])


def test_bench_tool_counts_and_arguments():
    """tools/bench_point_mesh.py without a device: its workload sizes and the operation count it states."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_point_mesh", os.path.join(ROOT, "tools", "bench_point_mesh.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.FLOPS_PER_TEST == 80
    src = open(os.path.join(ROOT, "pytorch-unsup-pc_amd", "csrc", "dpc_point_mesh.hip")).read()
    assert "%d fp64 operations" % mod.FLOPS_PER_TEST in src
    V, F = mod.mesh("soup", 1000, 3)
    assert len(F) == 1000 and V.shape == (3000, 3)
    V, F = mod.mesh("icosphere", 20480, 0)
    assert len(F) == 20480
