"""Host-side checks of the generalized winding numbers (no GPU): the numpy oracle (tests/winding_oracle.py) against the
50-digit sums of the fixture f32_winding.npz within the recorded bound, closed forms, the clearance every compared query
keeps, every refusal of the Python functions and of the two entry points before a device is needed, and the header's
prototypes against the ctypes bindings."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import mesh_voxels_oracle as MV
import point_mesh_oracle as PM
import winding_oracle as WO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << WO.FRAC_BITS


@pytest.fixture(scope="module")
def f32(golden):
    return golden("f32_winding.npz")


class _DeviceLookedFor(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """Valid arguments get as far as looking for a device, and no further, whatever this machine has."""
    from dpc.render import _batch

    def device(*a, **k):
        raise _DeviceLookedFor()

    monkeypatch.setattr(_batch, "device", device)


def _extent(V):
    v = np.asarray(V).astype(np.float64)
    return float((v.max(axis=0) - v.min(axis=0)).max())


def test_oracle_meets_the_fixture_within_the_bound(f32):
    """numpy against mpmath: within one quantum per usable face where the points keep the clearance, bit for bit on the
    guard cases (a point on a vertex or in a face's plane), whose zero terms do not depend on rounding."""
    assert int(f32["frac_bits"]) == WO.FRAC_BITS == 40 and float(f32["clearance"]) == WO.CLEARANCE == 1e-3
    assert sorted(f32["cases"]) == sorted(list(f32["clear"]) + list(f32["exact"]))
    for name in f32["cases"]:
        P, V, F = f32[name + "_P"], f32[name + "_V"], f32[name + "_F"]
        sums, status = WO.mesh_sums(P, V, F)
        assert status == 0 and sums.dtype == np.int64 and int(f32[name + "_bound"]) == WO.bound(V, F) == len(F), name
        worst = int(np.abs(sums - f32[name + "_sums"]).max())
        assert worst <= (int(f32[name + "_bound"]) if name in f32["clear"] else 0), (name, worst)
        assert np.array_equal(WO.mesh_winding(P, V, F)[0], sums * 2.0 ** -40), name


def test_every_compared_query_keeps_the_clearance(f32):
    """The bound holds away from the surface only: every point of a clear case lies at least 1e-3 of the mesh's extent
    from it, by point_mesh_oracle; so does every node centre of the grid tests' meshes."""
    for name in f32["clear"]:
        P, V, F = f32[name + "_P"], f32[name + "_V"], f32[name + "_F"]
        d2, _ = PM.mesh_d2(P, V, F)
        assert np.sqrt(d2.min()) >= WO.CLEARANCE * _extent(V), name
        assert float(f32[name + "_clearance"]) >= WO.CLEARANCE, name
    for name in f32["exact"]:
        assert float(f32[name + "_clearance"]) < 1e-12, name               # on the surface on purpose
    for name, (V, F) in WO.voxel_cases().items():
        for shape in WO.VOX_SHAPES:
            d2, _ = PM.mesh_d2(WO.node_centres(shape), V, F)
            assert np.sqrt(d2.min()) >= WO.CLEARANCE * _extent(V), (name, shape)
            # and no sum is near a threshold the tests use: far more than the bound away
            sums, _ = WO.voxel_sums(V, F, shape)
            for thr in (0.5, 0.25):
                assert np.abs(sums - WO.threshold_q(thr)).min() > 1000 * len(F), (name, shape, thr)


def test_fixture_cases_are_what_they_were_built_for(f32):
    F = f32["soup64_F"]
    assert F.shape == (97, 3) and f32["soup64_P"].shape == (60, 3) and f32["soup64_P"].dtype == np.float64
    assert sum(len(set(f)) < 3 for f in F.tolist()) >= 4                                        # repeated-index faces
    assert f32["soup32_P"].dtype == np.float32 and f32["soup32_V"].dtype == np.float32 and np.array_equal(f32["soup32_F"], F)
    assert np.array_equal(f32["soup32_V"], f32["soup64_V"].astype(np.float32))
    for name in ("cube", "tetra"):
        n = len(f32[name + "_F"])
        assert np.array_equal(f32[name + "_in_F"], f32[name + "_F"][:, ::-1]) and np.array_equal(f32[name + "_in_P"], f32[name + "_P"])
        out, inw = f32[name + "_sums"], f32[name + "_in_sums"]
        inside = np.abs(out - ONE) <= n
        assert 5 <= inside.sum() <= len(out) - 5 and (np.abs(out[~inside]) <= n).all(), name     # w = 1 or 0
        assert (np.abs(inw[inside] + ONE) <= n).all() and (np.abs(inw[~inside]) <= n).all(), name  # w = -1 or 0
    # a cube seen from its corner fills an octant, from a point inside a side half the space, from an edge a quarter
    assert (np.abs(f32["on_vertex_sums"] - ONE // 8) <= 12).all()
    assert (np.abs(f32["in_plane_sums"] - np.array([ONE // 2] * 4 + [0, 0, ONE // 4])) <= 12).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "f32_winding.npz")) < 64 * 1024


def test_numpy_and_mpmath_definitions_on_closed_forms():
    """Inputs whose answer is known."""
    tri = np.eye(3)
    for P, want in (((0, 0, 0), 0.125), ((-1e-3, -1e-3, -1e-3), None), ((1, 1, 1), None)):
        t = WO.face_terms([P], tri[:1], tri[1:2], tri[2:])
        exact = float(WO.face_term_mp(P, *tri))
        assert abs(t[0, 0] - exact) <= 2.0 ** -52, P
        if want is not None:                                                  # the octant's triangle from the origin
            assert abs(exact - want) <= 2.0 ** -53 and WO.quantise(t)[0, 0] == ONE // 8
    assert abs(WO.face_terms([(0, 0, 0)], tri[:1], tri[2:], tri[1:2])[0, 0] + 0.125) <= 2.0 ** -52            # the other winding
    # det == 0: in the plane (inside the face too), on a vertex, zero-area faces; never a NaN, never the sign of a zero
    for P in ((0.25, 0.25, 0.5), (2.0, -0.5, -0.5), (1, 0, 0), (0.5, 0.5, 0)):
        assert WO.face_terms([P], tri[:1], tri[1:2], tri[2:])[0, 0] == 0.0 and WO.face_term_mp(P, *tri) == 0, P
    for faces in ((tri[0], tri[0], tri[1]), (tri[0], tri[0], tri[0]), (tri[0], tri[1], 0.5 * (tri[0] + tri[1]))):
        assert WO.quantise(WO.face_terms([(0.1, 0.2, 0.3)], *(np.array([v]) for v in faces)))[0, 0] == 0
        assert WO.face_term_mp((0.1, 0.2, 0.3), *faces) == 0
    V, F = WO.cube((-1, -1, -1), (1, 1, 1))
    sums, status = WO.mesh_sums([(0, 0, 0), (0.3, -0.2, 0.9), (3, 0, 0), (np.nan, 0, 0), (0, np.inf, 0)], V, F)
    assert (np.abs(sums - np.array([ONE, ONE, 0, 0, 0])) <= 12).all() and sums[3:].tolist() == [0, 0] and status == WO.STATUS_NONFINITE
    w, _ = WO.mesh_winding([(0, 0, 0), (np.nan, 0, 0)], V, F)
    assert abs(w[0] - 1.0) <= 12 * 2.0 ** -40 and np.isnan(w[1])
    Vn = V.copy()
    Vn[7, 1] = np.nan
    kept, status = WO.kept_faces(Vn, F)
    assert status == WO.STATUS_NONFINITE and len(kept) == len(F) - int((F == 7).any(axis=1).sum()) == WO.bound(Vn, F)
    Fb = F.copy()
    Fb[3, 1] = 8
    kept, status = WO.kept_faces(V, Fb)
    assert status == WO.STATUS_BAD_INDEX and len(kept) == 11
    assert abs(WO.mesh_sums([(0, 0, 0)], V, Fb)[0][0] - (ONE - ONE // 12)) <= 12                  # one of twelve equal faces
    # grids: the frame, the compare, the open box
    c = WO.node_centres((3, 2, 5))
    assert c.shape == (30, 3) and c[0].tolist() == [-0.5, -0.5, -0.5] and c[-1].tolist() == [0.5, 0.5, 0.5] and c[1].tolist() == [-0.5, -0.5, -0.25]
    Vc, Fc = WO.voxel_cases(np.float64)["cube"]
    g = WO.winding_grid(Vc, Fc, (8, 8, 8))
    cs = WO.node_centres((8, 8, 8)).reshape(8, 8, 8, 3)
    assert np.array_equal(g, ((cs > WO.VOX_LO) & (cs < WO.VOX_HI)).all(axis=-1)) and g.any()
    Vo, Fo = WO.voxel_cases(np.float64)["open_box"]
    assert len(Fo) == 10 and WO.winding_grid(Vo, Fo, (8, 8, 8), 0.25).sum() > WO.winding_grid(Vo, Fo, (8, 8, 8), 0.5).sum() > 0
    assert not WO.winding_grid(Vc, Fc[:0], (8, 8, 8), -1.0).any()
    assert WO.threshold_q(0.5) == ONE // 2 and WO.threshold_q(-0.25) == -ONE // 4


_C_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}


def test_header_prototypes_match_the_bindings():
    from dpc.render import _native
    import dpc.render as R

    header = open(os.path.join(ROOT, "include", "dpc_render.h")).read()
    assert int(re.search(r"#define DPC_ABI_VERSION (\d+)", header).group(1)) == 15 == _native.lib().dpc_abi_version() == _native.ABI_VERSION
    assert int(re.search(r"#define DPC_WINDING_FRAC_BITS (\d+)", header).group(1)) == 40 == _native.DPC_WINDING_FRAC_BITS
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {name: (res, args) for name, res, args in _native._FUNCTIONS}
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("dpc_mesh_winding", "dpc_mesh_winding_workspace_bytes", "dpc_mesh_winding_voxels", "dpc_mesh_winding_voxels_workspace_bytes"):
        m = re.search(r"\b(\w+)\s+%s\(([^)]*)\);" % name, code)
        assert m and hasattr(lib, name) and name in _native.SYMBOLS, name
        want = []
        for arg in m.group(2).split(","):
            arg = " ".join(arg.split())
            want.append(ctypes.c_void_p if "*" in arg else _C_TYPES[arg.rsplit(" ", 1)[0]])
        assert bound[name] == (_C_TYPES[m.group(1)], want), name
    proto = re.search(r"int dpc_mesh_winding\(([^)]*)\)", code).group(1)
    dist = re.search(r"int dpc_point_mesh_distance\(([^)]*)\)", code).group(1)
    lead = lambda s: [" ".join(a.split()) for a in s.split(",")][:11]
    assert lead(proto) == lead(dist) and lead(proto)[-1] == "int n_pairs"               # the same leading arguments
    for name in ("winding_numbers", "points_inside_meshes", "signed_point_mesh_distance", "winding_voxels"):
        assert name in R.__all__ and callable(getattr(R, name)), name
    src = open(os.path.join(ROOT, "pytorch-unsup-pc_amd", "csrc", "dpc_winding.hip")).read()
    assert '#include "dpc_point_mesh.h"' in src and "atomicAdd" not in src and "pm_plan(" in src
    shared = open(os.path.join(ROOT, "pytorch-unsup-pc_amd", "csrc", "dpc_point_mesh.h")).read()
    assert "pm_geometry(" in shared[shared.index("inline int pm_plan("):]          # the distance's geometry, through the shared plan


def _tab(rows, width=6):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, width))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """dpc_mesh_winding with NULL device pointers returns what dpc_point_mesh_distance returns for the same table:
    DPC_ERR_SHAPE for what the header lists, DPC_ERR_NULL (nothing launched) for valid arguments, DPC_OK when there is
    nothing to do; besides, a row of more than 2^22 faces is refused; the workspace is sized from the host table."""
    from dpc.render import _native

    L, SHAPE, NUL, N = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL, None

    def both(rows, n_pts=10, n_verts=5, n_faces=3, pairs=None, same=True):
        t = _tab(rows)
        tp = t.ctypes.data_as(ctypes.c_void_p) if len(t) else N
        k = len(t) if pairs is None else pairs
        rc = L.dpc_mesh_winding(N, n_pts, 0, N, n_verts, 0, N, n_faces, N, tp, k, N, N, N, N, N)
        if same:
            assert rc == L.dpc_point_mesh_distance(N, n_pts, 0, N, n_verts, 0, N, n_faces, N, tp, k, N, N, N, N), rows
        return rc

    good = (0, 10, 0, 5, 0, 3)
    assert both([good]) == NUL and both([good, (0, 0, 0, 5, 0, 3), (2, 3, 0, 5, 1, 2)]) == NUL
    assert both([]) == 0 and both([(0, 0, 0, 5, 0, 3)]) == 0 and both([(0, 0, 0, 0, 0, 0)]) == 0
    assert L.dpc_mesh_winding(N, 10, 0, N, 5, 0, N, 3, N, N, 1, N, N, N, N, N) == NUL
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
    most = 2 ** 22                                                                           # |q| <= 2^39: the sum cannot wrap
    assert both([(0, 10, 0, 5, 0, most)], n_faces=most) == NUL
    assert both([(0, 10, 0, 5, 0, most + 1)], n_faces=most + 1, same=False) == SHAPE
    assert both([(0, 0, 0, 5, 0, most + 1)], n_faces=most + 1, same=False) == SHAPE
    ws = lambda rows: L.dpc_mesh_winding_workspace_bytes(_tab(rows).ctypes.data_as(ctypes.c_void_p), len(rows))
    assert ws(oversized) == 0 and ws([(0, 10, 0, 5, 0, 0)]) == 0 and ws([(0, 10, 0, 5, 0, most + 1)]) == 0
    assert L.dpc_mesh_winding_workspace_bytes(N, 1) == 0 and L.dpc_mesh_winding_workspace_bytes(_tab([good]).ctypes.data_as(ctypes.c_void_p), 0) == 0
    one = ws([good])                                                                         # one chunk: a slot per point
    assert one >= 3 * 2 * 4 + 10 * 8 and one % 16 == 0
    CH = _native.DPC_PM_FACE_TILE * _native.DPC_PM_CHUNK_TILES
    split = ws([(0, 3, 0, 5, 0, 4 * CH + 1)])                                                # 3 points, 5 chunks of faces
    assert split >= 3 * 2 * 4 + 5 * 3 * 8 and split % 16 == 0 and split > ws([(0, 3, 0, 5, 0, CH)])


def test_voxel_entry_point_refuses_bad_arguments_before_any_launch():
    from dpc.render import _native

    L, SHAPE, NUL, N = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL, None

    def run(rows, n_verts=8, n_faces=12, shape=(8, 8, 8), meshes=None, tq=1 << 39):
        t = _tab(rows, 4)
        tp = t.ctypes.data_as(ctypes.c_void_p) if len(t) else N
        k = len(t) if meshes is None else meshes
        return L.dpc_mesh_winding_voxels(N, n_verts, 0, N, n_faces, N, tp, k, shape[0], shape[1], shape[2], tq, N, N, N, N)

    good = (0, 8, 0, 12)
    assert run([good]) == NUL and run([good, (0, 8, 0, 0), (4, 4, 6, 6)]) == NUL and run([good], tq=-5) == NUL
    assert run([]) == 0 and run([], meshes=-1) == SHAPE
    assert L.dpc_mesh_winding_voxels(N, 8, 0, N, 12, N, N, 1, 8, 8, 8, 0, N, N, N, N) == NUL
    assert run([good], n_verts=-1) == SHAPE and run([good], n_faces=-1) == SHAPE
    for shape in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8), (129, 8, 8), (8, 129, 8), (8, 8, 129), (-1, 8, 8)):
        assert run([good], shape=shape) == SHAPE, shape
        assert run([], shape=shape) == SHAPE, shape
    assert run([good], shape=(2, 2, 2)) == NUL and run([good], shape=(128, 128, 128)) == NUL and run([good], shape=(16, 8, 8)) == NUL
    for row in ((0, 9, 0, 12), (1, 8, 0, 12), (-1, 8, 0, 12), (0, -1, 0, 12), (0, 8, 0, 13), (0, 8, 1, 12), (0, 8, -1, 12), (0, 8, 0, -1)):
        assert run([row]) == SHAPE, row
    most = 2 ** 22
    assert run([(0, 8, 0, most)], n_faces=most) == NUL and run([(0, 8, 0, most + 1)], n_faces=most + 1) == SHAPE
    assert run([good] * 1024, shape=(128, 128, 128)) == SHAPE                                # 2^31 slots
    ws = lambda rows, shape=(8, 8, 8): L.dpc_mesh_winding_voxels_workspace_bytes(_tab(rows, 4).ctypes.data_as(ctypes.c_void_p), len(rows), *shape)
    assert ws([good]) >= 512 * 8 and ws([good, good]) >= 2 * 512 * 8 and ws([good], (1, 8, 8)) == 0 and ws([(0, 8, 0, most + 1)]) == 0
    assert L.dpc_mesh_winding_voxels_workspace_bytes(N, 1, 8, 8, 8) == 0
    CH = _native.DPC_PM_FACE_TILE * _native.DPC_PM_CHUNK_TILES
    assert ws([(0, 8, 0, 2 * CH + 1)]) >= 3 * 512 * 8                                        # two node blocks: the faces are cut
    assert ws([(0, 8, 0, 2 * CH + 1)] * 32, (32, 32, 32)) < 2 * 32 * 32 ** 3 * 8             # the node blocks fill the device: one chunk


def test_refusals_come_before_a_device_is_needed(no_device):
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    good, pts = (V, F), np.zeros((4, 3), dtype=np.float32)
    for fn in (R.winding_numbers, R.points_inside_meshes, R.signed_point_mesh_distance):
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
        R.winding_numbers([pts], [good], return_sums=True)
    for fn in (R.points_inside_meshes, R.signed_point_mesh_distance):
        for ok in (0.5, 0, -3.25, 2.0 ** 20 - 1, np.float32(0.25)):
            with pytest.raises(_DeviceLookedFor):
                fn([pts], [good], threshold=ok)
        for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20, 1e9, "half", None):
            with pytest.raises(ValueError, match=r"%s: threshold must be a finite number in \(-2\^20, 2\^20\)" % fn.__name__):
                fn([pts], [good], threshold=bad)
    with pytest.raises(_DeviceLookedFor):
        R.signed_point_mesh_distance([pts], [good], squared=True)


def test_winding_voxels_refusals_come_before_a_device_is_needed(no_device):
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    good = (0.4 * V, F)
    for kw in ({}, {"vox_size_z": 16}, {"threshold": 0.25}, {"surface": False}):
        with pytest.raises(_DeviceLookedFor):
            R.winding_voxels([good, (V, F[:0])], 8, **kw)
    with pytest.raises(_DeviceLookedFor):
        R.winding_voxels([], 8)
    for bad in (np.nan, np.inf, 2.0 ** 20, -2.0 ** 20, "half"):
        with pytest.raises(ValueError, match=r"winding_voxels: threshold must be a finite number in \(-2\^20, 2\^20\)"):
            R.winding_voxels([good], 8, threshold=bad)
    with pytest.raises(ValueError, match="winding_voxels: a grid of .* has a side below 2"):
        R.winding_voxels([good], 1)
    with pytest.raises(ValueError, match="winding_voxels: a grid of .* has a side below 2"):
        R.winding_voxels([good], 8, vox_size_z=1)
    with pytest.raises(ValueError, match="winding_voxels: a grid of .* has a side above DPC_VOXEL_MAX_SIDE"):
        R.winding_voxels([good], 129)
    with pytest.raises(ValueError, match=r"winding_voxels: mesh 1: V must be \[n,3\]"):
        R.winding_voxels([good, (V[:, :2], F)], 8)
    with pytest.raises(ValueError, match=r"winding_voxels: mesh 0: F must be \[f,3\]"):
        R.winding_voxels([(V, F[:, :2])], 8)
    with pytest.raises(R.MeshError, match="winding_voxels: mesh 0: F holds a vertex index outside"):
        R.winding_voxels([(V, F + 1)], 8)
    with pytest.raises(ValueError, match=r"winding_voxels: mesh 0 must be \(V \[n,3\], F \[f,3\], ...\)"):
        R.winding_voxels([V], 8)


def test_a_device_is_needed_after_the_checks():
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    if not torch.cuda.is_available():
        for fn in (R.winding_numbers, R.points_inside_meshes, R.signed_point_mesh_distance):
            with pytest.raises(RuntimeError, match="MI355X only"):
                fn([np.zeros((4, 3), dtype=np.float32)], [(V, F)])
        with pytest.raises(RuntimeError, match="MI355X only"):
            R.winding_voxels([(V, F)], 8)


def test_bench_tool_states_its_shapes():
    """tools/bench_winding.py without a device: the two shapes the numbers in DESIGN.md were taken at."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_winding", os.path.join(ROOT, "tools", "bench_winding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.POINTS_SHAPE == (100000, 20000) and mod.VOXELS_SHAPE == (32, 32)
    V, F = mod.mesh(20000)
    assert F.shape == (20000, 3) and V.dtype == np.float32 and F.max() < len(V)
