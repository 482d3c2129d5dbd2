"""Iso-surface extraction on the GPU (csrc/dpc_surface.hip) against the numpy restatement of its rule
(tests/surface_oracle.py).  Vertices and faces are compared with array_equal: the vertex is one fp64 division and one
addition, nothing fused, and the order of vertices and faces is fixed by the rule, so every output has one right answer.

The kernels cut a grid's flat node indices into tiles of 1024 (one workgroup) taken in rounds of 256 (one node a thread),
and scan a grid's tiles 256 at a time; RAGGED has a grid just below, at and just above 256 and 1024 nodes with each axis
in turn making the difference, and grids of many tiles.  The scan's own edge: SCAN_SHAPES has 255 tiles (just below one
chunk) and 260 (just above: a partial second chunk that carries the first one's totals), each axis in turn making the
difference; the large grids have 256 (64^3, exactly one chunk) and 2048 (128^3, eight).  Those shapes also put tile edges in
the middle of rows and planes.  A call of more than 65535 grids runs the kernels' stride over the grids.  The sweep of
`sweep` runs once per module and is shared."""
import ctypes

import numpy as np
import pytest
import torch

import dpc.render as R
import surface_oracle as O
from dpc.render import _native

pytestmark = pytest.mark.gpu

KERNELS = {"k_surface_tiles<0>", "k_surface_tiles<1>", "k_surface_scan", "k_surface_verts<0>", "k_surface_verts<1>", "k_surface_faces"}
EDGE_SHAPES = [(3, 4, 16), (4, 4, 16), (5, 4, 16), (4, 3, 16), (4, 5, 16), (4, 16, 3), (4, 16, 5),           # 192, 256, 320 nodes
               (3, 5, 17), (1, 2, 128), (3, 43, 2),                                                          # 255, 256, 258
               (7, 8, 16), (8, 8, 16), (9, 8, 16), (8, 7, 16), (8, 9, 16), (8, 16, 7), (8, 16, 9),           # 896, 1024, 1152
               (3, 11, 31), (1, 8, 128), (5, 5, 41)]                                                         # 1023, 1024, 1025


SCAN_SHAPES = [(85, 48, 64), (65, 64, 64), (64, 65, 64), (64, 64, 65)]                                       # 255, 260, 260, 260 tiles


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ragged_grids():
    """(grids fp32, levels): all below, all above, one inside node, a ball, noise; sides of 1; every tile and round edge."""
    grids = [np.zeros((3, 3, 3), np.float32), np.ones((3, 3, 3), np.float32), np.zeros((3, 3, 3), np.float32),
             O.ball((12, 12, 12)), O.noise((5, 7, 9), 11, border=False),
             np.array([[[0.7]]], np.float32), O.noise((1, 5, 7), 12, border=False), O.noise((2, 2, 2), 13, border=False),
             O.noise((5, 7, 9), 14), O.noise((20, 20, 20), 15, border=False), O.ball((9, 31, 17), sigma=0.2)]
    grids[2][1, 1, 1] = 1
    grids += [O.noise(s, 100 + i, border=False) for i, s in enumerate(EDGE_SHAPES)]
    grids += [O.noise(s, 200 + i, border=False) for i, s in enumerate(SCAN_SHAPES)]
    levels = [0.5, 0.5, 0.25, 0.5, 0.37, 0.5, 0.61, 0.45, 0.5, 0.7, 0.3] + [0.3 + 0.02 * i for i in range(len(EDGE_SHAPES))]
    levels += [0.8, 0.85, 0.9, 0.75]                      # sparse, so that the big noise grids stay quick on the host
    return grids, levels


def check_mesh(got, want, what):
    V, F = got
    verts, faces = want[0], want[1]
    assert V.dtype == torch.float64 and F.dtype == torch.int64 and V.is_cuda and F.is_cuda, what
    assert tuple(V.shape) == verts.shape and tuple(F.shape) == faces.shape, (what, tuple(V.shape), verts.shape, tuple(F.shape), faces.shape)
    assert np.array_equal(F.cpu().numpy(), faces), what
    assert np.array_equal(V.cpu().numpy(), verts, equal_nan=True), what


@pytest.fixture(scope="module")
def sweep():
    """Everything the comparisons below need, extracted once, and the instantiations launched on the way."""
    out, launched = {}, set()
    R.check_status()
    grids, levels = ragged_grids()
    cases = {"01": (O.one_cell_cases(), 0.5), "seeded": (O.one_cell_cases("seeded", 5, 0.37), 0.37)}
    large = {G: O.blobs(G, G) for G in (64, 128)}

    def run():
        out["ragged32"] = R.extract_surfaces([dev(g) for g in grids], levels)
        out["ragged64"] = R.extract_surfaces([dev(g.astype(np.float64)) for g in grids], levels)
        for key, (g, iso) in cases.items():
            out["cases_" + key] = R.extract_surfaces(dev(g), iso)
        for G, g in large.items():
            out["large%d" % G] = R.extract_surfaces(dev(g), 0.1)

    launched |= _native.launched_instantiations(run, torch.device("cuda"))
    assert R.check_status() == 0
    out["ragged_want"] = [O.extract(g, iso) for g, iso in zip(grids, levels)]
    return out, launched, (grids, levels, cases, large)


# 1 the whole table on the device -------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["01", "seeded"])
def test_all_256_cases_in_one_call(sweep, key):
    g, iso = sweep[2][2][key]
    got = sweep[0]["cases_" + key]
    assert len(got) == 256
    for c in range(256):
        want = O.extract(g[c], iso)
        assert len(want[1]) == O.table()[c, 0]
        check_mesh(got[c], want, (key, c))


# 2 ragged batches ----------------------------------------------------------------------------------------------------
def test_ragged_batch_equals_the_oracle_for_fp32_and_fp64(sweep):
    grids, levels = sweep[2][0], sweep[2][1]
    want = sweep[0]["ragged_want"]
    for k, g in enumerate(grids):
        check_mesh(sweep[0]["ragged32"][k], want[k], ("f32", k, g.shape))
        check_mesh(sweep[0]["ragged64"][k], want[k], ("f64", k, g.shape))
    n = [(len(v), len(f)) for v, f, _ in want]
    assert n[0] == (0, 0) and n[1] == (0, 0) and n[2] == (6, 8)          # all below, all above, one inside node
    assert n[5] == (0, 0) and n[6][0] > 0 and n[6][1] == 0               # 1x1x1; 1x5x7 has vertices and no faces
    assert all(a > 0 and (b > 0) == (min(g.shape) > 1) for (a, b), g in zip(n[7:], grids[7:]))


# 3 large grids -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [64, 128])
def test_large_smooth_field(sweep, G):
    want = O.extract(sweep[2][3][G], 0.1)
    assert len(want[0]) > (20000 if G == 64 else 80000)
    check_mesh(sweep[0]["large%d" % G][0], want, G)


# 4 edge cases --------------------------------------------------------------------------------------------------------
def test_nodes_exactly_at_the_level_keep_their_degenerate_faces():
    g = O.ball((6, 6, 6), np.float64)
    g[2, 2, 3] = g[3, 3, 3] = g[0, 0, 0] = 0.5          # outside, next to inside nodes: t = 0 where they own the edge
    got = R.extract_surfaces(dev(g), 0.5)[0]
    want = O.extract(g, 0.5)
    check_mesh(got, want, "at the level")
    v0, v1, v2 = (want[0][want[1][:, k]] for k in range(3))
    assert (np.abs(np.cross(v1 - v0, v2 - v0)).sum(axis=1) == 0).any()      # there are degenerate faces, and they are kept
    assert R.check_status() == 0


def test_nonfinite_values_are_flagged_and_do_not_change_counts_or_faces():
    g = O.ball((7, 7, 7), np.float32)
    h = g.copy()
    h[3, 3, 2], h[3, 2, 3], h[0, 0, 0] = np.nan, np.inf, -np.inf
    R.check_status()
    clean = R.extract_surfaces(dev(g), 0.5)
    assert R.check_status() == 0
    got = R.extract_surfaces(dev(h), 0.5)[0]
    assert R.check_status() == _native.DPC_STATUS_NONFINITE and R.check_status() == 0
    want = O.extract(h, 0.5)
    assert want[2] and np.isnan(want[0]).any()
    check_mesh(got, want, "non-finite")
    check_mesh(clean[0], O.extract(g, 0.5), "finite")


def raw_tables(grids):
    sizes = [g.size for g in grids]
    start = np.cumsum([0] + sizes)
    desc = np.ascontiguousarray([(start[i],) + g.shape for i, g in enumerate(grids)], dtype=np.int32)
    return desc, int(start[-1])


def test_a_wrong_out_desc_count_is_flagged_and_leaves_the_outputs_untouched():
    """dpc_surface_extract itself: grid 1's table says one vertex fewer than the grid has -> DPC_STATUS_BAD_INDEX, nothing
    of grid 1 is written, grids 0 and 2 are complete."""
    grids = [O.ball((6, 6, 6)), O.noise((5, 7, 9), 3), O.ball((4, 5, 6))]
    want = [O.extract(g, 0.5) for g in grids]
    desc, n = raw_tables(grids)
    L = _native.lib()
    device = torch.device("cuda")
    packed = dev(np.concatenate([g.reshape(-1) for g in grids]))
    iso = dev(np.full(3, 0.5))
    work = torch.empty(L.dpc_surface_workspace_bytes(desc.ctypes.data, 3, n), dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    counts = torch.full((3, 2), -7, dtype=torch.int32, device="cuda")
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    desc_d = dev(desc)                                   # the device tables stay referenced until the results are read
    rc = L.dpc_surface_count(_native.ptr(packed), n, 0, _native.ptr(desc_d), p(desc), 3, _native.ptr(iso), _native.ptr(counts),
                             _native.ptr(work), _native.ptr(status), _native.stream_ptr(device))
    assert rc == 0 and counts.cpu().numpy().tolist() == [[len(v), len(f)] for v, f, _ in want] and status.item() == 0
    nv, nf = [len(w[0]) for w in want], [len(w[1]) for w in want]
    out = np.array([(0, nv[0], 0, nf[0]), (nv[0], nv[1] - 1, nf[0], nf[1]), (nv[0] + nv[1], nv[2], nf[0] + nf[1], nf[2])], dtype=np.int32)
    verts = torch.full((sum(nv), 3), -7.0, dtype=torch.float64, device="cuda")
    faces = torch.full((sum(nf), 3), -7, dtype=torch.int32, device="cuda")
    out_d = dev(out)
    rc = L.dpc_surface_extract(_native.ptr(packed), n, 0, _native.ptr(desc_d), p(desc), 3, _native.ptr(iso), _native.ptr(out_d),
                               p(out), sum(nv), sum(nf), _native.ptr(verts), _native.ptr(faces), _native.ptr(work), _native.ptr(status),
                               _native.stream_ptr(device))
    assert rc == 0 and status.item() == _native.DPC_STATUS_BAD_INDEX
    V, F = verts.cpu().numpy(), faces.cpu().numpy()
    assert (V[nv[0]:nv[0] + nv[1]] == -7.0).all() and (F[nf[0]:nf[0] + nf[1]] == -7).all()
    assert np.array_equal(V[:nv[0]], want[0][0]) and np.array_equal(F[:nf[0]], want[0][1])
    assert np.array_equal(V[nv[0] + nv[1]:], want[2][0]) and np.array_equal(F[nf[0] + nf[1]:], want[2][1])
    # a device grid row that is not the host's (it overruns the packed buffer) is flagged too, and nothing of it is written
    bad = desc.copy()
    bad[2, 0] = n - 5
    out[1, 1] = nv[1]
    status.zero_()
    verts.fill_(-7.0)
    faces.fill_(-7)
    bad_d, out_d = dev(bad), dev(out)
    rc = L.dpc_surface_extract(_native.ptr(packed), n, 0, _native.ptr(bad_d), p(desc), 3, _native.ptr(iso), _native.ptr(out_d),
                               p(out), sum(nv), sum(nf), _native.ptr(verts), _native.ptr(faces), _native.ptr(work), _native.ptr(status),
                               _native.stream_ptr(device))
    assert rc == 0 and status.item() == _native.DPC_STATUS_BAD_INDEX
    V, F = verts.cpu().numpy(), faces.cpu().numpy()
    assert (V[nv[0] + nv[1]:] == -7.0).all() and (F[nf[0] + nf[1]:] == -7).all()
    assert np.array_equal(V[nv[0]:nv[0] + nv[1]], want[1][0]) and np.array_equal(F[nf[0]:nf[0] + nf[1]], want[1][1])


# 5 unit_cube, dense, chunking ----------------------------------------------------------------------------------------
def test_unit_cube_and_dense_against_the_oracle():
    g = O.ball((9, 12, 7))
    want = O.extract(g, 0.4)
    got = R.extract_surfaces(dev(g), 0.4, unit_cube=True)[0]
    check_mesh(got, (O.unit_cube(want[0], g.shape), want[1]), "unit cube")
    assert got[0].abs().max().item() <= 0.5
    plain = R.extract_surface(g, 0.4)
    assert isinstance(plain, np.ndarray) and plain.dtype == np.float64 and np.array_equal(plain, want[0])
    dense = R.extract_surface(dev(g), 0.4, dense=True)
    assert isinstance(dense, np.ndarray) and np.array_equal(dense, O.augment(want[0], want[1]))
    assert len(dense) == len(want[0]) + 3 * len(want[1])
    b = g > 0.4                                                             # a bool grid at its natural level
    check_mesh(R.extract_surfaces(dev(b), 0.5)[0], O.extract(b.astype(np.float32), 0.5), "bool")


def test_one_grid_per_call_gives_the_same_lists(sweep):
    grids, levels = sweep[2][0][:12], sweep[2][1][:12]
    one = R.extract_surfaces([dev(g) for g in grids], levels, grids_per_call=1)
    three = R.extract_surfaces([dev(g) for g in grids], levels, grids_per_call=3)
    for k in range(len(grids)):
        for got in (one[k], three[k]):
            assert torch.equal(got[0], sweep[0]["ragged32"][k][0]) and torch.equal(got[1], sweep[0]["ragged32"][k][1]), k
    stacked = np.stack([O.ball((6, 5, 4)), O.noise((6, 5, 4), 2)])
    a, b = R.extract_surfaces(dev(stacked), [0.5, 0.4]), R.extract_surfaces(dev(stacked), [0.5, 0.4], grids_per_call=1)
    for k in range(2):
        check_mesh(a[k], O.extract(stacked[k], [0.5, 0.4][k]), k)
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1])


def test_more_grids_than_the_launch_has_rows():
    """65792 grids of 2^3 in one call: the launches have 65535 rows of workgroups, so the kernels' stride over the grids
    takes the rest.  Grid b is case b % 256 of the table; the packed outputs equal the oracle's meshes repeated."""
    cases = O.one_cell_cases()
    reps = 257
    want = [O.extract(cases[c], 0.5) for c in range(256)]
    got = R.extract_surfaces(dev(np.tile(cases, (reps, 1, 1, 1))), 0.5)
    assert len(got) == 256 * reps > 65535
    assert [(len(v), len(f)) for v, f in got] == [(len(w[0]), len(w[1])) for w in want] * reps
    V, F = torch.cat([v for v, _ in got]).cpu().numpy(), torch.cat([f for _, f in got]).cpu().numpy()
    assert np.array_equal(V, np.tile(np.concatenate([w[0] for w in want]), (reps, 1)))
    assert np.array_equal(F, np.tile(np.concatenate([w[1] for w in want]), (reps, 1)))
    assert R.check_status() == 0


# 6 composition -------------------------------------------------------------------------------------------------------
def test_the_mesh_goes_straight_into_the_other_mesh_functions():
    G = 12
    mesh = R.extract_surfaces(dev(O.ball((G, G, G))), 0.5, unit_cube=True)[0]
    d = R.point_mesh_distance([mesh[0]], [mesh])[0]
    # a vertex lies on its own surface; half a cell is the geometric bound, not a measured one
    assert d.dtype == torch.float64 and torch.isfinite(d).all() and d.max().item() < 0.5 / (G - 1)
    vox = R.voxelise_meshes([mesh], G)
    assert tuple(vox.shape) == (1, G, G, G) and vox.any() and not vox.all()
    rgba, depth = R.render_mesh_views([mesh], [[[1.2, 1.0, 0.8]]], image_size=32, supersample=1)
    assert tuple(rgba.shape) == (1, 32, 32, 4) and rgba[..., 3].any() and not rgba[..., 3].all()


def test_extract_surfaces_tool_writes_one_obj_per_model(tmp_path):
    """tools/extract_surfaces.py: a saved cloud goes through pointcloud2voxels and the extraction, a saved grid through the
    extraction alone; each OBJ holds the mesh extract_surfaces returns; a second run skips what is there."""
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("extract_surfaces_tool", os.path.join(root, "tools", "extract_surfaces.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    inp, out = tmp_path / "pred", tmp_path / "meshes"
    inp.mkdir()
    rng = np.random.default_rng(4)
    d = rng.normal(size=(2, 500, 3))
    shift = np.array([0.3, -0.2, 0.0])
    cloud = (0.4 * d / np.linalg.norm(d, axis=2, keepdims=True) + shift).astype(np.float32)   # a sphere off the centre
    R.save_predictions(str(inp / "chair_pc.pkl"), cloud, num_points=np.array([400, 500]))
    R.save_predictions(str(inp / "table_pc.pkl"), cloud[1:] * np.float32(0.9), num_points=np.array([400]))   # shares chair's call
    R.save_predictions(str(inp / "lamp_pc.pkl"), cloud[:1, :300])                                            # a length of its own
    grid = O.ball((9, 8, 7))
    np.save(str(inp / "ball.npy"), grid[None, ..., None])
    args = ["--inp_dir=%s" % inp, "--out_dir=%s" % out, "--vox_size=16", "--sigma_rel=1.5", "--iso_level=0.1"]
    assert mod.main(args) == {"written": ["ball", "chair", "lamp", "table"], "skipped": []}

    def read(path):
        v = [[float(x) for x in l.split()[1:]] for l in open(path) if l.startswith("v ")]
        f = [[int(x) for x in l.split()[1:]] for l in open(path) if l.startswith("f ")]
        return np.array(v).reshape(-1, 3), np.array(f).reshape(-1, 3)

    want = O.extract(grid, 0.1)
    v, f = read(str(out / "ball.obj"))
    assert np.array_equal(v, O.unit_cube(want[0], grid.shape)) and np.array_equal(f - 1, want[1])     # a grid: the unit cube

    class Cfg:
        vox_size = 16

    for name, pts in (("chair", cloud[0, :400]), ("table", cloud[1, :400] * np.float32(0.9)), ("lamp", cloud[0, :300])):
        # one model at a time here, batched in the tool: the same grid, swapped back to (x, y, z), in the cloud's frame
        vox = R.pointcloud2voxels(Cfg(), dev(pts[None]), 1.5 / 16)[0, ..., 0].transpose(0, 1).contiguous()
        ref = O.extract(vox.cpu().numpy(), 0.1)
        v, f = read(str(out / (name + ".obj")))
        assert len(v) > 100 and np.array_equal(v, 2.0 * O.unit_cube(ref[0], (16, 16, 16))) and np.array_equal(f - 1, ref[1]), name
        # the mesh overlays its cloud: the vertices of a shell around the sphere average to the sphere's centre, within
        # half a cell (a cell is 2 / 15) -- at half scale, or with x and y exchanged, they would be 0.13 or more away
        scale = 0.9 if name == "table" else 1.0
        assert np.abs(v.mean(axis=0) - scale * shift).max() < 1.0 / 15, (name, v.mean(axis=0))
        assert O.signed_volume(v, f - 1) > 0                                                          # still wound outward
    assert mod.main(args) == {"written": [], "skipped": ["ball", "chair", "lamp", "table"]}


# 7 the launch record -------------------------------------------------------------------------------------------------
def test_the_sweep_launches_every_kernel_of_the_object(sweep):
    """The instantiations in the launch record over the sweep are the kernels dpc_surface.o compiles
    (tests/test_surface_host.py compares the object's symbols with the same set)."""
    launched = {i for i in sweep[1] if i.startswith("k_surface")}
    assert launched == KERNELS, sorted(launched ^ KERNELS)
