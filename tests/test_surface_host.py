"""Host-side checks of the iso-surface extraction (no GPU): the oracle's triangulation table (tests/surface_oracle.py)
against the fixture, the committed header and the generator's fresh output; the invariants the rule promises (closed,
manifold single cases, outward winding, Euler characteristic); every refusal of the dpc_surface_* entry points and of the
Python layer before any launch; the exported symbols; and the Python helpers that need no device."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import surface_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "f29_surface.npz")
HEADER = os.path.join(ROOT, "pytorch-unsup-pc_amd", "csrc", "dpc_surface_table.h")
ENTRY_POINTS = ("dpc_surface_workspace_bytes", "dpc_surface_count", "dpc_surface_extract")
KERNELS = {"k_surface_tiles<0>", "k_surface_tiles<1>", "k_surface_scan", "k_surface_verts<0>", "k_surface_verts<1>", "k_surface_faces"}


def generator():
    spec = importlib.util.spec_from_file_location("gen_surface_table", os.path.join(ROOT, "tools", "gen_surface_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def header_table():
    rows = re.findall(r"^\s*\{([-\d,\s]+)\},", open(HEADER).read(), flags=re.M)
    return np.array([[int(x) for x in r.split(",")] for r in rows], dtype=np.int8)


# 1 the table ---------------------------------------------------------------------------------------------------------
def test_oracle_table_equals_the_fixture_the_header_and_the_generator():
    T = O.table()
    assert T.shape == (256, 16) and T.dtype == np.int8
    assert np.array_equal(T, np.load(GOLDEN)["table"])
    assert np.array_equal(T, header_table())
    gen = generator()
    assert np.array_equal(T, np.array(gen.table(), dtype=np.int8))
    assert open(HEADER).read() == gen.header_text()            # the committed header is the generator's output, as text


@pytest.fixture(scope="module")
def committed_table():
    """The table the kernels compile, parsed from the committed header: what the invariants below are about.  It must be the
    oracle's own, which extracts the meshes they look at."""
    T = header_table()
    assert T.shape == (256, 16) and np.array_equal(T, O.table())
    return T


def test_table_row_counts_and_edges(committed_table):
    T = committed_table.astype(int)
    assert T[:, 0].max() == 5 and T[:, 0].sum() == 820 and T[0, 0] == 0 and T[255, 0] == 0
    assert (T[1:255, 0] >= 1).all()
    for case in range(256):
        n = T[case, 0]
        used = T[case, 1:1 + 3 * n]
        assert (T[case, 1 + 3 * n:] == -1).all() and (used >= 0).all() and (used < 12).all()
        crossing = set()
        for e in range(12):
            off, a = O.edge_owner(e)
            lo = 4 * off[0] + 2 * off[1] + off[2]
            hi = lo + (4, 2, 1)[a]
            if (case >> lo & 1) != (case >> hi & 1):
                crossing.add(e)
        assert set(used.tolist()) == crossing, case            # only the case's crossing edges, and each of them


# 2 invariants of the oracle ------------------------------------------------------------------------------------------
def test_every_case_in_a_padded_grid_is_closed_manifold_and_wound_outward(committed_table):
    for case in range(1, 256):
        g = np.zeros((4, 4, 4), dtype=np.float32)
        for k in range(8):
            if case >> k & 1:
                g[1 + (k >> 2 & 1), 1 + (k >> 1 & 1), 1 + (k & 1)] = 1
        verts, faces, nonfinite = O.extract(g, 0.5)
        assert not nonfinite and len(faces)
        counts = O.directed_edge_counts(faces)
        assert all(n == 1 and counts.get((b, a), 0) == 1 for (a, b), n in counts.items()), case
        assert sorted(set(faces.reshape(-1).tolist())) == list(range(len(verts))), case     # every vertex is used
        assert O.signed_volume(verts, faces) > 0, case
    verts, faces, _ = O.extract(np.zeros((4, 4, 4), dtype=np.float32), 0.5)
    assert verts.shape == (0, 3) and faces.shape == (0, 3)


def test_noise_grid_is_closed(committed_table):
    verts, faces, _ = O.extract(O.noise((9, 9, 9), 3), 0.5)
    counts = O.directed_edge_counts(faces)
    assert len(faces) > 300 and all(counts.get((b, a), 0) == n for (a, b), n in counts.items())


def test_ball_has_euler_characteristic_two(committed_table):
    verts, faces, _ = O.extract(O.ball((12, 12, 12)), 0.5)
    assert O.euler_characteristic(verts, faces) == 2 and O.signed_volume(verts, faces) > 0


def test_oracle_closed_forms_and_fixture_meshes():
    # one inside node in the middle of 3^3: six vertices at distance t = 0.5 / 1, an octahedron
    g = np.zeros((3, 3, 3))
    g[1, 1, 1] = 1
    verts, faces, _ = O.extract(g, 0.25)
    assert verts.tolist() == [[0.25, 1, 1], [1, 0.25, 1], [1, 1, 0.25], [1.75, 1, 1], [1, 1.75, 1], [1, 1, 1.75]] and len(faces) == 8
    # a node exactly at the level is outside: the vertex of an edge to it lies on it
    g = np.zeros((2, 2, 2))
    g[0, 0, 0], g[0, 0, 1] = 1.0, 0.5
    verts, faces, _ = O.extract(g, 0.5)
    assert verts.tolist() == [[0.5, 0, 0], [0, 0.5, 0], [0, 0, 1]] and faces.tolist() == [[0, 1, 2]]
    # a side of 1: vertices along the line, no faces; fp32 and fp64 copies agree
    f = np.load(GOLDEN)
    for name in ("ball", "noise", "line"):
        verts, faces, _ = O.extract(f[name + "/grid"], float(f[name + "/iso"]))
        assert verts.tobytes() == f[name + "/verts"].tobytes() and np.array_equal(faces, f[name + "/faces"]), name
        assert faces.dtype == np.int32 and verts.dtype == np.float64
    assert len(f["line/faces"]) == 0 and len(f["line/verts"]) == 5 and len(f["ball/faces"]) > 0
    b32 = O.ball((7, 6, 5), np.float32)
    a, b = O.extract(b32, 0.4), O.extract(b32.astype(np.float64), 0.4)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    # non-finite ends: flagged, NaN is outside, the faces do not change
    g = O.ball((5, 5, 5), np.float64)
    h = g.copy()
    h[2, 2, 1], h[2, 1, 2] = np.nan, np.inf
    v, fc, nonfinite = O.extract(h, 0.5)
    assert nonfinite and np.isnan(v).any() and fc.max() == len(v) - 1


# 3 header and binding ------------------------------------------------------------------------------------------------
def test_header_symbols_and_abi():
    from dpc.render import _native

    header = open(os.path.join(ROOT, "include", "dpc_render.h")).read()
    assert int(re.search(r"#define DPC_ABI_VERSION (\d+)", header).group(1)) == 15 == _native.lib().dpc_abi_version()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _native.SYMBOLS and hasattr(lib, name) and re.search(r"\b(int|size_t) %s\(" % name, header), name


def test_built_kernels_are_the_ones_the_gpu_suite_must_launch():
    from test_abi_and_host import device_object_output

    out = device_object_output("dpc_surface.o", ["llvm-readelf", "-sW"])
    built = set()
    for line in out.splitlines():
        f = line.split()
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)(\w+)$", f[7]) if len(f) >= 8 and f[3] == "FUNC" else None
        if m:
            n = int(m.group(1))
            name, rest = m.group(2)[:n], m.group(2)[n:]
            targs = re.match(r"I((?:Li-?\d+E)+)E", rest)
            built.add(name + ("<%s>" % ", ".join(re.findall(r"Li(-?\d+)E", targs.group(1))) if targs else ""))
    assert {b for b in built if b.startswith("k_")} == KERNELS


def _tab(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 4))


def _p(t):
    return t.ctypes.data_as(ctypes.c_void_p)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """dpc_surface_count / dpc_surface_extract with NULL device pointers: DPC_ERR_SHAPE for what the header lists,
    DPC_ERR_NULL (nothing launched) for valid arguments, DPC_OK for zero grids."""
    from dpc.render import _native

    L, SHAPE, NUL, S = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL, _native.DPC_VOXEL_MAX_SIDE
    N = None
    count = lambda rows, n, f64=0, B=None: L.dpc_surface_count(N, n, f64, N, _p(_tab(rows)) if len(rows) else N,
                                                               len(rows) if B is None else B, N, N, N, N, N)
    ws = lambda rows, n: L.dpc_surface_workspace_bytes(_p(_tab(rows)), len(rows), n)
    good = [(0, 2, 2, 2), (8, 1, 5, 7), (43, 1, 1, 1), (45, S, S, S)]                # a gap is fine
    n = 45 + S ** 3
    assert count([(0, 2, 2, 2), (7, 2, 2, 2)], 20) == SHAPE and count([(8, 2, 2, 2), (0, 2, 2, 2)], 20) == SHAPE   # overlapping, descending
    assert count(good, n) == NUL and count(good, n, 1) == NUL
    assert count([], 0) == 0 and count([], 5) == 0 and count([], 0, B=-1) == SHAPE
    assert L.dpc_surface_count(N, 8, 0, N, N, 1, N, N, N, N, N) == NUL
    assert count(good, -1) == SHAPE and count(good, n, 2) == SHAPE and count(good, n, -1) == SHAPE
    for bad in ((0, 0, 2, 2), (0, 2, 0, 2), (0, 2, 2, 0), (0, S + 1, 2, 2), (0, 2, S + 1, 2), (0, 2, 2, S + 1), (0, -1, 2, 2), (-1, 2, 2, 2),
                (n - 7, 2, 2, 2)):
        assert count([good[0], bad], n) == SHAPE, bad
        assert ws([good[0], bad], n) == 0
    # the workspace: 8 bytes per tile of 1024 nodes (every grid has the largest grid's tiles), 4 per grid, 4 per node,
    # each piece rounded up to 16 bytes
    r16 = lambda x: (x + 15) // 16 * 16
    tiles = (S ** 3 + 1023) // 1024
    assert ws(good, n) == r16(8 * 4 * tiles) + r16(4 * 4) + r16(4 * n)
    assert ws([(0, 2, 2, 2)], 8) == 16 + 16 + 32 and L.dpc_surface_workspace_bytes(N, 1, 8) == 0

    ext = lambda rows, out, nv, nf, n=35, B=None: L.dpc_surface_extract(
        N, n, 0, N, _p(_tab(rows)) if len(rows) else N, len(rows) if B is None else B, N, N, _p(_tab(out)) if len(out) else N, nv, nf,
        N, N, N, N, N)
    n = 35
    two = [(0, 2, 2, 2), (8, 3, 3, 3)]
    assert ext(two, [(0, 3, 0, 1), (3, 6, 1, 8)], 9, 9) == NUL
    assert ext(two, [(0, 0, 0, 0), (5, 6, 2, 8)], 20, 20) == NUL           # gaps and empty meshes are fine
    assert ext([], [], 0, 0) == 0 and ext([], [], 0, 0, B=-1) == SHAPE
    assert L.dpc_surface_extract(N, 8, 0, N, _p(_tab(two[:1])), 1, N, N, N, 0, 0, N, N, N, N, N) == NUL    # no host out table
    assert ext(two, [(0, 3, 0, 1), (3, 6, 1, 8)], 8, 9) == SHAPE and ext(two, [(0, 3, 0, 1), (3, 6, 1, 8)], 9, 8) == SHAPE   # overrun
    assert ext(two, [(0, 3, 0, 1), (3, 6, 1, 8)], -1, 9) == SHAPE and ext(two, [(0, 3, 0, 1), (3, 6, 1, 8)], 9, -1) == SHAPE
    assert ext(two, [(0, 3, 0, 1), (2, 6, 1, 8)], 20, 20) == SHAPE and ext(two, [(0, 3, 0, 2), (3, 6, 1, 8)], 20, 20) == SHAPE  # overlap
    assert ext(two, [(3, 3, 0, 1), (0, 3, 1, 8)], 20, 20) == SHAPE         # descending
    assert ext(two, [(-1, 3, 0, 1), (3, 6, 1, 8)], 20, 20) == SHAPE and ext(two, [(0, -3, 0, 1), (3, 6, 1, 8)], 20, 20) == SHAPE
    assert ext(two, [(0, 3, -1, 1), (3, 6, 1, 8)], 20, 20) == SHAPE and ext(two, [(0, 3, 0, -1), (3, 6, 1, 8)], 20, 20) == SHAPE
    assert ext(two, [(0, 25, 0, 1), (25, 6, 1, 8)], 40, 20) == SHAPE       # more than 3 vertices a node
    assert ext(two, [(0, 3, 0, 6), (3, 6, 6, 8)], 20, 20) == SHAPE         # more than 5 faces a cell
    assert ext([(0, 1, 5, 7)], [(0, 3, 0, 1)], 20, 20, n=35) == SHAPE      # a grid without cells has no face
    assert ext([(0, 1, 5, 7)], [(0, 3, 0, 0)], 20, 20, n=35) == NUL
    assert ext([two[0], (8, 0, 2, 2)], [(0, 3, 0, 1), (3, 6, 1, 8)], 20, 20) == SHAPE


# 4 the Python layer --------------------------------------------------------------------------------------------------
def test_public_names():
    import dpc.render as R

    for name in ("extract_surfaces", "extract_surface", "augment_mesh", "save_obj"):
        assert name in R.__all__ and callable(getattr(R, name)), name


def test_save_obj_round_trip(tmp_path):
    import dpc.render as R

    f = np.load(GOLDEN)
    verts, faces = f["ball/verts"], f["ball/faces"]
    path = str(tmp_path / "ball.obj")
    R.save_obj(path, torch.from_numpy(verts), torch.from_numpy(faces).long())
    v, fc = [], []
    for line in open(path):
        tok = line.split()
        if tok[0] == "v":
            v.append([float(x) for x in tok[1:]])
        else:
            assert tok[0] == "f"
            fc.append([int(x) for x in tok[1:]])
    assert np.array(v).tobytes() == verts.tobytes()                       # %.17g reads back exactly
    assert np.array_equal(np.array(fc) - 1, faces) and np.array(fc).min() == 1
    with pytest.raises(ValueError, match=r"verts and faces must be \[n,3\] and \[m,3\]"):
        R.save_obj(path, verts[:, :2], faces)


def test_augment_mesh_order_on_a_hand_written_example():
    import dpc.render as R

    V = np.array([[0, 0, 0], [2, 0, 0], [0, 4, 0], [0, 0, 8]], dtype=np.float64)
    F = np.array([[0, 1, 2], [0, 2, 3], [1, 3, 2]])
    want = np.array([[0, 0, 0], [2, 0, 0], [0, 4, 0], [0, 0, 8],
                     [1, 0, 0], [0, 2, 0], [1, 0, 4],          # corners (0,1) of the three faces
                     [1, 2, 0], [0, 2, 4], [0, 2, 4],          # corners (1,2): the edge 2-3 is shared, and kept twice
                     [0, 2, 0], [0, 0, 4], [1, 2, 0]],         # corners (0,2)
                    dtype=np.float64)
    got = R.augment_mesh(V, F)
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(O.augment(V, F), want)
    t = R.augment_mesh(torch.from_numpy(V), torch.from_numpy(F).int())
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), want)
    with pytest.raises(ValueError, match="augment_mesh: verts and faces"):
        R.augment_mesh(V, F[:, :2])


def test_render_mesh_views_takes_a_bare_vertex_face_pair():
    """What extract_surfaces returns is a scene of one grey material: (V, F) tensors or arrays become the host arrays of
    (V, F, material 0 for every face, one Kd row); any other length is still refused."""
    from dpc.render import meshviews

    f = np.load(GOLDEN)
    verts, faces = f["ball/verts"], f["ball/faces"]
    for pair in ((torch.from_numpy(verts), torch.from_numpy(faces).long()), (verts, faces), [verts.astype(np.float32), faces]):
        V, F, mat, Kd = meshviews._scene(pair, 0)
        given = np.asarray(pair[0]).astype(np.float64)            # an fp32 V widens exactly
        assert V.dtype == np.float64 and np.array_equal(V, given) and F.dtype == np.int32 and np.array_equal(F, faces)
        assert mat.dtype == np.int32 and mat.shape == (len(faces),) and not mat.any()
        assert Kd.shape == (1, 3) and np.array_equal(Kd, meshviews._PLAIN_KD)
    full = meshviews._scene((verts, faces, np.zeros(len(faces), dtype=np.int64), np.array([[0.1, 0.2, 0.3]])), 0)
    assert np.array_equal(full[0], verts) and full[3].tolist() == [[0.1, 0.2, 0.3]]
    for bad in ((verts,), (verts, faces, np.zeros(len(faces)))):
        with pytest.raises(ValueError, match=r"scene 3 must be \(V, F, material, Kd"):
            meshviews._scene(bad, 3)
    with pytest.raises(ValueError, match="V, F and Kd must be"):
        meshviews._scene((verts[:, :2], faces), 0)


def test_python_refusals_name_the_input_and_come_before_any_launch():
    """Every refusal is a ValueError raised before a device is looked for (this machine may have none)."""
    import dpc.render as R

    f = lambda *s: np.zeros(s, dtype=np.float32)
    big = R.surface.MAX_SIDE + 1
    with pytest.raises(ValueError, match=r"voxels must be \[B,D,H,W\], \[D,H,W\] or a list of \[D,H,W\] grids, got \(4, 4\)"):
        R.extract_surfaces(f(4, 4), 0.5)
    with pytest.raises(ValueError, match=r"voxels must be \[B,D,H,W\]"):
        R.extract_surfaces(f(1, 1, 4, 4, 4), 0.5)
    with pytest.raises(ValueError, match=r"voxels\[1\] must be \[D,H,W\], got \(2, 4, 4, 4\)"):
        R.extract_surfaces([f(4, 4, 4), f(2, 4, 4, 4)], 0.5)
    with pytest.raises(ValueError, match="voxels must be float32, float64 or bool, got torch.int64"):
        R.extract_surfaces(np.zeros((4, 4, 4), dtype=np.int64), 0.5)
    with pytest.raises(ValueError, match=r"voxels\[0\] must be float32, float64 or bool, got torch.float16"):
        R.extract_surfaces([np.zeros((4, 4, 4), dtype=np.float16)], 0.5)
    with pytest.raises(ValueError, match="voxels must be on a HIP device, got a cpu tensor"):
        R.extract_surfaces(torch.zeros(2, 4, 4, 4), 0.5)
    with pytest.raises(ValueError, match="voxels must be a tensor, an array or a list of them|voxels must be a tensor or an array"):
        R.extract_surfaces("grid", 0.5)
    with pytest.raises(ValueError, match="voxels: a grid of .* has a side above DPC_VOXEL_MAX_SIDE"):
        R.extract_surfaces(f(1, 2, 2, big), 0.5)
    with pytest.raises(ValueError, match="voxels: a grid of .* has an empty side"):
        R.extract_surfaces(f(2, 0, 4, 4), 0.5)
    with pytest.raises(ValueError, match=r"iso_level must be a number or one number per grid: 2 grids, got \(3,\)"):
        R.extract_surfaces(f(2, 4, 4, 4), [0.1, 0.2, 0.3])
    with pytest.raises(ValueError, match="iso_level must be a number"):
        R.extract_surfaces(f(2, 4, 4, 4), "half")
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="grids_per_call must be an integer >= 1"):
            R.extract_surfaces(f(2, 4, 4, 4), 0.5, grids_per_call=bad)
    with pytest.raises(ValueError, match="unit_cube needs sides >= 2"):
        R.extract_surfaces(f(1, 4, 4), 0.5, unit_cube=True)
    with pytest.raises(ValueError, match=r"extract_surface: voxels must be one \[D,H,W\] grid, got \(2, 4, 4, 4\)"):
        R.extract_surface(f(2, 4, 4, 4), 0.5)
    assert R.extract_surfaces([], 0.5) == [] and R.extract_surfaces(f(0, 4, 4, 4), 0.5) == []
    five = [torch.zeros(2, 2, 2)] * 5
    assert R.surface._chunks(five, 2) == [(0, 2), (2, 4), (4, 5)] and R.surface._chunks(five, None) == [(0, 5)]
