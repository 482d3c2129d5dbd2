"""Host-side checks of the mesh voxeliser (no GPU): the numpy oracle (tests/mesh_voxels_oracle.py, the definition of the
rules) against its recorded results (fixture f26_mesh_voxels.npz, byte for byte) and against closed forms, the properties
of the two fills, the point rule of voxelise inside the surface rule, every refusal of the Python layer and of the two
entry points before any launch, and the exported symbols."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import mesh_voxels_oracle as O
import voxels_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "f26_mesh_voxels.npz")
ENTRY_POINTS = ("dpc_voxelise_meshes", "dpc_voxel_carve")


def test_oracle_equals_the_fixture_byte_for_byte():
    f = np.load(GOLDEN)
    cases = list(O.golden_cases())
    assert len(cases) == 8 and {c[1] for c in cases} >= {(2, 2, 2), (5, 5, 5), (8, 9, 9), (12, 16, 16), (33, 33, 33)}
    for key, shape, V, F in cases:
        assert f[key + "/inputs"].tolist() == [VO.digest(V), VO.digest(F)], key
        for fill in O.FILLS:
            grid, info, status = O.voxelise_mesh(V, F, shape, fill)
            assert O.pack_bits(grid).tobytes() == f["%s/%s/bits" % (key, fill)].tobytes(), (key, fill)
            assert info.tolist() == f["%s/%s/info" % (key, fill)].tolist() and status == int(f["%s/%s/status" % (key, fill)]), (key, fill)


def test_the_cube_through_node_centres():
    """Faces through the node centres 2 and 8 of an 11^3 grid: a shell one node thick, half-open parity intervals."""
    shape = (11, 11, 11)
    V, F = O.node_box((2, 2, 2), (8, 8, 8), shape)
    s, status, outside = O.surface(V, F, shape)
    assert status == 0 and outside == 0 and s.sum() == 7 ** 3 - 5 ** 3
    full = np.zeros(shape, dtype=bool)
    full[2:9, 2:9, 2:9] = True
    inner = np.zeros(shape, dtype=bool)
    inner[3:8, 3:8, 3:8] = True
    assert (s == (full & ~inner)).all() and (O.carve(s) == full).all()
    par, opened = O.parity(V, F, shape)
    assert opened == 0 and par.sum() == 6 ** 3
    lo = np.argwhere(par).min(axis=0)
    assert (np.argwhere(par).max(axis=0) - lo == 5).all() and lo[0] == 2        # toggles at ceil(2) and ceil(8): planes 2 .. 7
    grid, info, _ = O.voxelise_mesh(V, F, shape, "parity")
    assert grid.sum() == 343 and info.tolist() == [0, 0]


def test_an_off_centre_box_in_closed_form():
    shape = (9, 12, 10)
    lo, hi = np.array([-0.31, -0.23, -0.17]), np.array([0.27, 0.33, 0.41])
    V, F = O.box(lo, hi)
    a, b = O.grid_coordinates(lo, shape)[0], O.grid_coordinates(hi, shape)[0]
    outer = [[n for n in range(shape[c]) if n + 0.5 >= a[c] and n - 0.5 <= b[c]] for c in range(3)]
    inner = [[n for n in range(shape[c]) if n - 0.5 > a[c] and n + 0.5 < b[c]] for c in range(3)]
    s, _, _ = O.surface(V, F, shape)
    want = np.zeros(shape, dtype=bool)
    want[np.ix_(*outer)] = True
    assert (O.carve(s) == want).all()
    want[np.ix_(*inner)] = False
    assert (s == want).all() and s.sum() == math.prod(map(len, outer)) - math.prod(map(len, inner))
    par, opened = O.parity(V, F, shape)
    cols = [range(math.ceil(a[c]), math.floor(b[c]) + 1) for c in (1, 2)]       # no vertex on a column: closed intervals
    want = np.zeros(shape, dtype=bool)
    want[np.ix_(range(math.ceil(a[0]), math.ceil(b[0])), *cols)] = True
    assert opened == 0 and (par == want).all()


def test_single_faces_in_closed_form():
    shape = (6, 7, 9)
    z = 3 / 5 - 0.5                                                            # node plane 3 of axis 0, exactly: 0.1 * 5 = 0.5
    assert O.grid_coordinates([[0.1, 0, 0]], shape)[0, 0] == 3.0
    span = np.array([[0.1, -3.0, -3.0], [0.1, 4.0, -3.0], [0.1, -3.0, 4.0]])
    F = np.array([[0, 1, 2]])
    for fill, planes in (("none", [3]), ("carve", [3]), ("parity", [3, 4, 5])):
        grid, info, status = O.voxelise_mesh(span, F, shape, fill)
        want = np.zeros(shape, dtype=bool)
        want[planes] = True
        assert (grid == want).all() and status == 0, fill
        assert info.tolist() == [1, 7 * 9 if fill == "parity" else 0], fill     # its vertices are outside; every column is open
    far = np.array([[0.7, 0.7, 0.7], [0.9, 0.7, 0.8], [0.8, 0.9, 0.7]])
    for fill in O.FILLS:
        grid, info, status = O.voxelise_mesh(far, F, shape, fill)
        assert not grid.any() and info.tolist() == [1, 0] and status == 0
        grid, info, status = O.voxelise_mesh(far, np.zeros((0, 3), dtype=np.int32), shape, fill)
        assert not grid.any() and info.tolist() == [0, 0] and status == 0
    # zero area: a segment marks what it touches, a point its node (or the 2, 4 or 8 nodes whose cubes share it)
    seg = np.array([[-0.5, -0.5, -0.5], [0.5, -0.5, -0.5], [0.0, 0.0, 0.0]])
    grid, info, status = O.voxelise_mesh(seg, np.array([[0, 1, 1]]), shape, "none")
    assert sorted(map(tuple, np.argwhere(grid))) == [(k, 0, 0) for k in range(6)]
    grid, _, _ = O.voxelise_mesh(seg, np.array([[2, 2, 2]]), (5, 5, 5), "none")
    assert sorted(map(tuple, np.argwhere(grid))) == [(2, 2, 2)]
    grid, _, _ = O.voxelise_mesh(seg, np.array([[2, 2, 2]]), (6, 5, 5), "none")     # u_0 = 2.5: two cubes touch it
    assert sorted(map(tuple, np.argwhere(grid))) == [(2, 2, 2), (3, 2, 2)]
    # guards: a NaN vertex skips its face only; so does an index outside the mesh
    nan = np.array([[0.1, 0.1, 0.1], [np.nan, 0.2, 0.2], [0.3, 0.1, 0.2], [-0.3, -0.3, -0.3], [-0.1, -0.3, -0.2], [-0.2, -0.1, -0.3]])
    both, _, status = O.voxelise_mesh(nan, np.array([[0, 1, 2], [3, 4, 5]]), shape, "none")
    good, _, _ = O.voxelise_mesh(nan, np.array([[3, 4, 5]]), shape, "none")
    assert status == O.STATUS_NONFINITE and (both == good).all() and good.any()
    both, _, status = O.voxelise_mesh(nan, np.array([[3, 4, 6], [3, 4, 5], [-1, 4, 5]]), shape, "none")
    assert status == O.STATUS_BAD_INDEX and (both == good).all()


MESHES = {
    "ico2": lambda: (O.icosphere(2, 0.41, (0.02, 0.01, -0.03), np.float32), True),
    "ico1_f64": lambda: (O.icosphere(1, 0.43, (0.01, -0.02, 0.03), np.float64), True),
    "box": lambda: (O.box((-0.31, -0.23, -0.17), (0.27, 0.33, 0.41), np.float32), True),
    "two_boxes": lambda: (O.join(O.box((-0.41, -0.37, -0.43), (0.03, 0.11, 0.19)), O.box((-0.13, -0.21, -0.29), (0.39, 0.31, 0.36))), True),
    "hemi2": lambda: (O.hemisphere(2, 0.42, np.float32), False),
    "soup": lambda: (O.soup(80, 3, 0.25), False),
}


@pytest.mark.parametrize("name", sorted(MESHES))
@pytest.mark.parametrize("shape", [(5, 5, 5), (12, 16, 16), (33, 33, 33)], ids=lambda s: "x".join(map(str, s)))
def test_properties_of_the_fills(name, shape):
    (V, F), closed = MESHES[name]()
    s, status, _ = O.surface(V, F, shape)
    c = O.carve(s)
    assert status == 0 and s.any() and not (s & ~c).any()                    # S is a subset of carve(S)
    assert (O.carve(c) == c).all()                                            # idempotent
    par, opened = O.parity(V, F, shape)
    if closed:
        assert opened == 0 and not (par & ~c).any()                           # parity inside carve
    if name == "hemi2":
        assert opened > 0                                                     # parity leaks through the open rim
        assert shape[0] < 12 or (par[-1] & ~c[-1]).any()                      # ... to the last plane; carve does not leak
    # a snapped copy (every vertex on a node: every shared edge and vertex lies on columns) still counts each column once
    if closed:
        g1 = np.array(shape, dtype=np.float64) - 1
        Vs = np.round((V.astype(np.float64) + 0.5) * g1) / g1 - 0.5
        assert O.parity(Vs, F, shape)[1] == 0


POINT_RULE = [("ico2", (33, 33, 33), 1), ("two_boxes", (16, 16, 16), 2), ("soup", (12, 16, 16), 3), ("hemi2", (64, 64, 64), 4)]


@pytest.mark.parametrize("name,shape,seed", POINT_RULE, ids=[p[0] for p in POINT_RULE])
def test_points_on_the_faces_fall_inside_the_surface(name, shape, seed):
    """voxelise's nearest node of a point on a face is a node whose cube meets the face: zero misses for these meshes and
    seeds (tests/test_mesh_voxels_gpu.py runs the same ones on the GPU)."""
    (V, F), _ = MESHES[name]()
    pts = O.face_points(V, F, 8, seed)
    cloud, _ = VO.voxelise(pts, shape)
    s, _, _ = O.surface(V, F, shape)
    assert cloud.any() and not (cloud & ~s).any()


def _tab(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 4))


def _p(t):
    return t.ctypes.data_as(ctypes.c_void_p)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Both entry points with NULL device pointers: DPC_ERR_SHAPE for what the header lists, DPC_ERR_NULL (nothing
    launched) for valid arguments, DPC_OK for zero items."""
    from dpc.render import _native

    L, SHAPE, NUL, S = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL, _native.DPC_VOXEL_MAX_SIDE
    N = None

    def vox(rows, n_verts, n_faces, D=4, H=4, W=4, fill=1, meshes=None):
        return L.dpc_voxelise_meshes(N, n_verts, 0, N, n_faces, N, _p(_tab(rows)) if len(rows) else N,
                                     len(rows) if meshes is None else meshes, D, H, W, fill, N, N, N, N, N)

    assert vox([(0, 5, 0, 3), (5, 0, 3, 0), (5, 4, 3, 2)], 9, 5) == NUL          # an empty mesh among others
    assert vox([(0, 5, 0, 3)], 5, 3, S, S, S) == NUL and vox([(0, 5, 0, 3)], 5, 3, 2, 2, 2) == NUL
    for fill in (0, 1, 2):
        assert vox([(0, 5, 0, 3)], 5, 3, fill=fill) == NUL
    assert vox([], 0, 0) == 0
    assert L.dpc_voxelise_meshes(N, 5, 0, N, 3, N, N, 1, 4, 4, 4, 0, N, N, N, N, N) == NUL
    assert vox([(0, 5, 0, 3)], 5, 3, fill=3) == SHAPE and vox([(0, 5, 0, 3)], 5, 3, fill=-1) == SHAPE
    assert vox([(0, 5, 0, 3)], -1, 3) == SHAPE and vox([(0, 5, 0, 3)], 5, -1) == SHAPE and vox([], 0, 0, meshes=-1) == SHAPE
    for row in ((0, 6, 0, 3), (1, 5, 0, 3), (-1, 5, 0, 3), (0, -1, 0, 3), (0, 5, 0, 4), (0, 5, 1, 3), (0, 5, -1, 3), (0, 5, 0, -1)):
        assert vox([row], 5, 3) == SHAPE, row
    for bad in ((1, 4, 4), (4, 1, 4), (4, 4, 1), (0, 4, 4), (S + 1, 4, 4), (4, S + 1, 4), (4, 4, S + 1), (-1, 4, 4)):
        assert vox([(0, 5, 0, 3)], 5, 3, *bad) == SHAPE, bad
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (S + 1, 4, 4), (4, S + 1, 4), (4, 4, S + 1), (-1, 4, 4)):
        assert L.dpc_voxel_carve(N, 2, bad[0], bad[1], bad[2], N, N) == SHAPE, bad
    assert L.dpc_voxel_carve(N, 2, 4, 4, 4, N, N) == NUL and L.dpc_voxel_carve(N, 2, 1, 1, 1, N, N) == NUL
    assert L.dpc_voxel_carve(N, 2, S, S, S, N, N) == NUL and L.dpc_voxel_carve(N, 2, S, 65, 65, N, N) == NUL
    assert L.dpc_voxel_carve(N, 0, 4, 4, 4, N, N) == 0 and L.dpc_voxel_carve(N, -1, 4, 4, 4, N, N) == SHAPE
    words = np.zeros(4, dtype=np.uint32)
    assert L.dpc_voxel_carve(_p(words), 1, 4, 4, 4, _p(words), N) == SHAPE      # in place: refused, nothing launched


def test_header_symbols_and_abi():
    from dpc.render import _native, meshvoxels

    header = open(os.path.join(ROOT, "include", "dpc_render.h")).read()
    assert int(re.search(r"#define DPC_ABI_VERSION (\d+)", header).group(1)) == 15 == _native.lib().dpc_abi_version()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _native.SYMBOLS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, header), name
    for name, value in (("NONE", 0), ("CARVE", 1), ("PARITY", 2)):
        assert "#define DPC_MESH_FILL_%s %d" % (name, value) in header and getattr(_native, "DPC_MESH_FILL_" + name) == value
    assert meshvoxels.FILLS == {"none": 0, "carve": 1, "parity": 2} and tuple(meshvoxels.FILLS) == O.FILLS
    assert float(re.search(r"#define DPC_MESH_VOXEL_MAX_COORD ([0-9.]+)", header).group(1)) == O.MAX_COORD


def test_public_names():
    import dpc.render as R

    for name in ("voxelise_meshes", "carve_voxels", "solid_iou_of_split"):
        assert name in R.__all__ and callable(getattr(R, name)), name


def test_built_instantiations_are_the_class_table():
    """The kernels of dpc_mesh_voxels.o are the instantiations the GPU sweep (tests/test_mesh_voxels_gpu.py) must launch."""
    from test_abi_and_host import device_object_output

    out = device_object_output("dpc_mesh_voxels.o", ["llvm-readelf", "-sW"])
    got = re.findall(r"_ZN12_GLOBAL__N_112k_mv_surfaceILi(\d+)ELi(\d+)ELi(\d+)EEEv", out)
    assert {tuple(map(int, v)) for v in got} == {(f, w, t) for f in (0, 1) for w, t in ((1024, 256), (8192, 512), (16384, 512))}
    got = re.findall(r"_ZN12_GLOBAL__N_111k_mv_parityILi(\d+)ELi(\d+)EEEv", out)
    assert {tuple(map(int, v)) for v in got} == {(f, t) for f in (0, 1) for t in (256, 1024)}
    assert {int(t) for t in re.findall(r"_ZN12_GLOBAL__N_110k_mv_carveILi(\d+)EEEv", out)} == {256, 1024}


def test_python_refusals_come_before_any_launch():
    """Every refusal is a ValueError (MeshError for an index) raised before a device is looked for (this machine may have
    none), and names the mesh."""
    import dpc.render as R

    V, F = O.icosphere(0, dtype=np.float32)
    good = (V, F)
    big = R.voxels.MAX_SIDE + 1
    for fn in (lambda m, **kw: R.voxelise_meshes(m, kw.pop("vox_size", 8), **kw),
               lambda m, **kw: R.solid_iou_of_split([(np.zeros((2, 10, 3), dtype=np.float32), None)] * len(m), m, **kw)):
        with pytest.raises(ValueError, match=r"mesh 1: V must be \[n,3\]"):
            fn([good, (V[:, :2], F)])
        with pytest.raises(ValueError, match=r"mesh 1: F must be \[f,3\]"):
            fn([good, (V, F[:, :2])])
        with pytest.raises(ValueError, match="mesh 0: F must hold integers"):
            fn([(V, F.astype(np.float32))])
        with pytest.raises(R.MeshError, match=r"mesh 1: F holds a vertex index outside \[0, 12\)"):
            fn([good, (V, F + 1)])
        with pytest.raises(R.MeshError, match=r"mesh 0: F holds a vertex index outside"):
            fn([(V, F - 1)])
        with pytest.raises(ValueError, match=r"mesh 0 must be \(V \[n,3\], F \[f,3\], ...\)"):
            fn([V])
        with pytest.raises(ValueError, match="fill must be one of 'none', 'carve', 'parity'"):
            fn([good], fill="flood")
        with pytest.raises(ValueError, match="fill must be one of"):
            fn([good], fill=1)
        with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
            fn([good], vox_size=big)
        with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
            fn([good], vox_size=8, vox_size_z=big)
        with pytest.raises(ValueError, match="a side below 2"):
            fn([good], vox_size=1)
        with pytest.raises(ValueError, match="a side below 2"):
            fn([good], vox_size=8, vox_size_z=1)
        with pytest.raises(ValueError, match="vox_size must be an integer"):
            fn([good], vox_size=8.5)
    assert issubclass(R.MeshError, ValueError)
    pts = np.zeros((2, 10, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="1 predictions and 2 meshes"):
        R.solid_iou_of_split([(pts, None)], [good, good])
    with pytest.raises(ValueError, match="models_per_call must be >= 1"):
        R.solid_iou_of_split([(pts, None)], [good], models_per_call=0)
    with pytest.raises(ValueError, match="same number of views"):
        R.solid_iou_of_split([(pts, None), (pts[:1], None)], [good, good])
    with pytest.raises(ValueError, match=r"grids must be \[B,D,H,W\]"):
        R.carve_voxels(np.zeros((4, 4, 4), dtype=bool))
    with pytest.raises(ValueError, match="grids must be a bool / uint8 grid, got torch.float32"):
        R.carve_voxels(np.zeros((1, 4, 4, 4), dtype=np.float32))
    with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
        R.carve_voxels(np.zeros((1, 2, 2, big), dtype=bool))
    with pytest.raises(RuntimeError, match="MI355X only"):                    # a CPU tensor, after the argument checks
        R.carve_voxels(torch.zeros(1, 4, 4, 4, dtype=torch.bool))


def test_voxelise_gt_tool_arguments():
    import importlib.util

    spec = importlib.util.spec_from_file_location("voxelise_gt", os.path.join(ROOT, "tools", "voxelise_gt.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = mod.parse_arguments(["--shapenet_path=a", "--synth_set=03001627", "--output_dir=b"])
    assert cfg.vox_size == 32 and cfg.fill == "carve" and cfg.subset == "val" and cfg.models_per_call == 256
    cfg = mod.parse_arguments(["--shapenet_path=a", "--synth_set=03001627", "--output_dir=b", "--vox_size=64", "--fill=parity"])
    assert cfg.vox_size == 64 and cfg.fill == "parity"
    with pytest.raises(SystemExit):
        mod.parse_arguments(["--shapenet_path=a", "--synth_set=03001627", "--output_dir=b", "--fill=flood"])
