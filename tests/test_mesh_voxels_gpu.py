"""The mesh voxeliser on the GPU (csrc/dpc_mesh_voxels.hip) against the numpy definition of its rules
(tests/mesh_voxels_oracle.py).  Everything is compared exactly: every output is bits or a count.

The sweep of `sweep` runs once per module.  Grids: 2^3, 5^3, 8 x 9 x 9 and 12 x 16 x 16 (sides differ, W % 32 != 0), 32^3
(the largest of the first size class), 33^3 (rows straddle words; the second class), 64^3 (its largest) and 128^3 (four
slabs; an icosphere of 320 faces).  Per grid a batch of four fp32 meshes (a sphere, a box, an open hemisphere, scattered
triangles that poke out of the cube), the same batch widened to fp64, and a sphere whose vertices are genuinely fp64; all
three fills.  One more batch at 33^3 mixes the edge cases (mesh_voxels_oracle.mixed_batch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dpc.render as R
import mesh_voxels_oracle as O
import voxels_oracle as VO
from dpc.render import _native
from test_abi_and_host import device_object_output
from test_mesh_voxels_host import MESHES, POINT_RULE

pytestmark = pytest.mark.gpu

GRIDS = [(2, -1), (5, -1), (9, 8), (16, 12), (32, -1), (33, -1), (64, -1), (128, -1)]   # (vox_size, vox_size_z)
EXPECTED = {"k_mv_surface<%d, %d, %d>" % (f, w, t) for f in (0, 1) for w, t in ((1024, 256), (8192, 512), (16384, 512))} | \
           {"k_mv_parity<%d, %d>" % (f, t) for f in (0, 1) for t in (256, 1024)} | {"k_mv_carve<256>", "k_mv_carve<1024>"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def grid_id(g):
    return "%dx%d" % (g[0], g[0] if g[1] == -1 else g[1])


def batch_of(g):
    """The fp32 meshes of a grid, and the fp64 sphere."""
    if g[0] == 128:
        return [O.icosphere(2, 0.41, (0.02, 0.01, -0.03), np.float32)], []
    return ([MESHES["ico2"]()[0], MESHES["box"]()[0], MESHES["hemi2"]()[0], O.soup(100, 7 + g[0], 0.2)],
            [O.icosphere(1, 0.43, (0.01, -0.02, 0.03), np.float64)])


def reference(meshes, shape):
    """{fill: (grids [M,D,H,W], info [M,2])} and the OR of the status bits, the surface of a mesh computed once."""
    out = {f: ([], []) for f in O.FILLS}
    status = 0
    for V, F in meshes:
        s, st, outside = O.surface(V, F, shape)
        par, opened = O.parity(V, F, shape)
        status |= st
        for f, grid, n_open in (("none", s, 0), ("carve", O.carve(s), 0), ("parity", s | par, opened)):
            out[f][0].append(grid)
            out[f][1].append([outside, n_open])
    return {f: (np.stack(g), np.array(i, dtype=np.int32)) for f, (g, i) in out.items()}, status


def run(meshes, g, fill, as_f64=False):
    m = [(dev(V.astype(np.float64) if as_f64 else V), F) for V, F in meshes]
    grids, info = R.voxelise_meshes(m, g[0], g[1], fill=fill, return_info=True)
    shape = O.shape_of(*g)
    assert grids.dtype == torch.bool and grids.is_cuda and tuple(grids.shape) == (len(meshes),) + shape
    assert info.dtype == torch.int32 and tuple(info.shape) == (len(meshes), 2)
    return grids.cpu().numpy(), info.cpu().numpy()


@pytest.fixture(scope="module")
def sweep():
    """({grid: {(batch, fill): (grids, info)}}, the references, the instantiations launched)."""
    got, want, launched = {}, {}, set()
    R.check_status()
    for g in GRIDS:
        f32, f64 = batch_of(g)
        shape = O.shape_of(*g)
        want[g] = {"f32": reference(f32, shape)[0], "native": reference(f64, shape)[0] if f64 else None}
        got[g] = {}

        def job():
            for fill in O.FILLS:
                got[g]["f32", fill] = run(f32, g, fill)
                got[g]["f64", fill] = run(f32, g, fill, as_f64=True)
                if f64:
                    got[g]["native", fill] = run(f64, g, fill)

        launched |= _native.launched_instantiations(job, torch.device("cuda"))
    assert R.check_status() == 0
    return got, want, launched


# 1 parity with the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", O.FILLS)
@pytest.mark.parametrize("g", GRIDS, ids=grid_id)
def test_voxelise_meshes_equals_the_oracle(sweep, g, fill):
    got, want, _ = sweep
    grids, info = got[g]["f32", fill]
    ref_grids, ref_info = want[g]["f32"][fill]
    assert ref_grids.any()
    for k in range(len(grids)):
        assert (grids[k] == ref_grids[k]).all(), (g, fill, k, int((grids[k] != ref_grids[k]).sum()))
    assert info.tolist() == ref_info.tolist()
    wide, wide_info = got[g]["f64", fill]
    assert wide.tobytes() == grids.tobytes() and wide_info.tolist() == info.tolist()      # fp32 vertices widen exactly
    if want[g]["native"] is not None:
        grids, info = got[g]["native", fill]
        assert (grids == want[g]["native"][fill][0]).all() and info.tolist() == want[g]["native"][fill][1].tolist()


def test_the_sweep_launches_every_compiled_instantiation(sweep):
    launched = {i for i in sweep[2] if i.startswith("k_mv_")}
    assert launched == EXPECTED, sorted(launched ^ EXPECTED)
    built = set()
    for line in device_object_output("dpc_mesh_voxels.o", ["llvm-readelf", "-sW"]).splitlines():
        f = line.split()
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)(\w+)$", f[7]) if len(f) >= 8 and f[3] == "FUNC" else None
        if m:
            n = int(m.group(1))
            name, rest = m.group(2)[:n], m.group(2)[n:]
            targs = re.match(r"I((?:Li-?\d+E)+)E", rest)
            built.add(name + ("<%s>" % ", ".join(re.findall(r"Li(-?\d+)E", targs.group(1))) if targs else ""))
    built = {b for b in built if b.startswith("k_mv_")}
    assert launched == built, sorted(launched ^ built)


@pytest.fixture(scope="module")
def mixed():
    """The edge-case batch at 33^3, fp32: its reference, and what the GPU returned per fill with the status bits."""
    g = (33, -1)
    meshes = O.mixed_batch(np.float32)
    want, status = reference(meshes, O.shape_of(*g))
    got = {}
    R.check_status()
    for fill in O.FILLS:
        got[fill] = run(meshes, g, fill) + (R.check_status(),)
    return g, meshes, want, status, got


@pytest.mark.parametrize("fill", O.FILLS)
def test_the_mixed_batch(mixed, fill):
    """No faces; one face; zero-area and repeated-vertex faces; a face spanning the grid among 2000 tiny ones; faces partly
    and wholly outside the cube; a NaN and an infinite vertex, whose faces are skipped and reported."""
    g, meshes, want, status, got = mixed
    grids, info, bits = got[fill]
    assert status == O.STATUS_NONFINITE and bits == _native.DPC_STATUS_NONFINITE
    for k in range(len(meshes)):
        assert (grids[k] == want[fill][0][k]).all(), (fill, k, int((grids[k] != want[fill][0][k]).sum()))
    assert info.tolist() == want[fill][1].tolist()
    assert not grids[0].any() and not grids[6].any() and grids[1].any() and grids[5].any()
    assert info[3, 0] > 0 and info[4, 0] == 3 and (fill != "parity" or info[1, 1] > 0)


# 2 order, neighbours, repeats ------------------------------------------------------------------------------------
def test_face_order_batch_neighbours_and_repeats_do_not_matter(mixed):
    g, meshes, want, _, got = mixed
    rng = np.random.default_rng(3)
    shuffled = [(V, F[rng.permutation(len(F))]) for V, F in meshes]
    for fill in O.FILLS:
        grids, info, _ = got[fill]
        again = run(shuffled, g, fill)
        assert again[0].tobytes() == grids.tobytes() and again[1].tolist() == info.tolist(), fill
        twice = run(meshes, g, fill)
        assert twice[0].tobytes() == grids.tobytes() and twice[1].tolist() == info.tolist(), fill
        for k in (3, 5, 1):                                                # alone, and between other neighbours
            alone = run([meshes[k]], g, fill)
            assert alone[0][0].tobytes() == grids[k].tobytes() and alone[1][0].tolist() == info[k].tolist(), (fill, k)
        back = run(meshes[::-1], g, fill)
        assert back[0][::-1].tobytes() == grids.tobytes() and back[1][::-1].tolist() == info.tolist(), fill
    R.check_status()


def test_a_face_index_outside_its_mesh_is_skipped_on_the_device():
    """The Python layer refuses such a mesh; dpc_voxelise_meshes itself skips the face, reports it, and the index never
    becomes an address: the grid is the oracle's, which skips it too."""
    shape = (12, 16, 16)
    V, F = O.icosphere(1, 0.4, dtype=np.float32)
    F = F.copy()
    F[5, 1], F[17, 0], F[40, 2] = len(V), -1, 2 ** 31 - 1
    want, status = reference([(V, F)], shape)
    assert status == O.STATUS_BAD_INDEX
    desc = np.array([[0, len(V), 0, len(F)]], dtype=np.int32)
    words = (shape[0] * shape[1] * shape[2] + 31) // 32
    V_d, F_d, desc_d = dev(V), dev(F), dev(desc)
    for fill in O.FILLS:
        bits = torch.full((1, words), -1, dtype=torch.int32, device="cuda")
        scratch, info = torch.empty_like(bits), torch.full((1, 2), -1, dtype=torch.int32, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = _native.lib().dpc_voxelise_meshes(_native.ptr(V_d), len(V), 0, _native.ptr(F_d), len(F), _native.ptr(desc_d),
                                               desc.ctypes.data_as(ctypes.c_void_p), 1, shape[0], shape[1], shape[2],
                                               R.meshvoxels.FILLS[fill], _native.ptr(bits), _native.ptr(scratch), _native.ptr(info),
                                               _native.ptr(st), _native.stream_ptr(torch.device("cuda")))
        assert rc == 0
        assert int(st.item()) == _native.DPC_STATUS_BAD_INDEX
        assert bits.cpu().numpy().view(np.uint32).reshape(-1).tolist() == O.pack_bits(want[fill][0][0]).tolist(), fill
        assert info.cpu().numpy().tolist() == want[fill][1].tolist()


# 3 carve_voxels, the point rule, the split ---------------------------------------------------------------------------
@pytest.mark.parametrize("g", [(5, -1), (16, 12), (33, -1), (64, -1), (128, 80), (65, 128)], ids=grid_id)
def test_carve_voxels_of_voxelised_clouds_equals_the_oracle(g):
    """(128, 80): 80 x 128 x 128, six slabs; (65, 128): 128 x 65 x 65, three words a row, H * W odd: slabs with a halo plane."""
    shape = O.shape_of(*g)
    clouds = [O.face_points(*MESHES[name]()[0], 6, 5).astype(np.float32) for name in ("ico2", "hemi2", "soup")]
    clouds += [np.zeros((0, 3), dtype=np.float32), VO.cloud(3000, 9, np.float32, shape)]
    shells = R.voxelise([dev(c) for c in clouds], g[0], g[1])
    want = np.stack([VO.voxelise(c, shape)[0] for c in clouds])
    assert (shells.cpu().numpy() == want).all()
    got = R.carve_voxels(shells)
    assert got.dtype == torch.bool and got.is_cuda and tuple(got.shape) == tuple(shells.shape)
    assert (got.cpu().numpy() == O.carve(want)).all()
    assert (R.carve_voxels(want.astype(np.uint8)).cpu().numpy() == O.carve(want)).all()     # a host uint8 array
    assert (R.carve_voxels(got) == got).all()                                               # idempotent
    R.check_status()


@pytest.mark.parametrize("name,shape,seed", POINT_RULE, ids=[p[0] for p in POINT_RULE])
def test_points_on_the_faces_fall_inside_the_surface(name, shape, seed):
    """voxelise of points sampled on the faces sets no node that the fill="none" surface of the mesh leaves clear; the
    oracle alone has zero misses for these meshes and seeds (tests/test_mesh_voxels_host.py)."""
    (V, F), _ = MESHES[name]()
    pts = O.face_points(V, F, 8, seed)
    cloud = R.voxelise([dev(pts)], shape[1], shape[0])[0]
    surface = R.voxelise_meshes([(V, F)], shape[1], shape[0], fill="none")[0]
    assert bool(cloud.any()) and int((cloud & ~surface).sum()) == 0
    R.check_status()


def test_solid_iou_of_split_against_the_counts_composed_by_hand():
    G, views = 16, 2
    shape = (G, G, G)
    names = ("ico2", "box", "hemi2")
    meshes = [MESHES[n]()[0] for n in names]
    rng = np.random.default_rng(11)
    preds = []
    for V, F in meshes:
        pts = O.face_points(V, F, 2, 13)
        pts = np.stack([pts[rng.integers(0, len(pts), 300)] + rng.normal(0, 0.02, (300, 3)) for _ in range(views)]).astype(np.float32)
        pts[0, :3] = [[0.7, 0, 0], [0, -0.6, 0], [0.5, 0.5, 0.51]]                          # dropped
        preds.append((pts, np.array([300, 250])))
    for fill, carve_predictions in (("carve", True), ("parity", True), ("none", False)):
        out = R.solid_iou_of_split(preds, meshes, vox_size=G, fill=fill, carve_predictions=carve_predictions, models_per_call=2)
        assert set(out) == {"stats", "iou", "dropped", "info"}
        for m, (V, F) in enumerate(meshes):
            gt, info, _ = O.voxelise_mesh(V, F, shape, fill)
            assert out["info"][m].tolist() == info.tolist()
            for v in range(views):
                cloud = preds[m][0][v, :preds[m][1][v]]
                p, dropped = VO.voxelise(cloud, shape)
                s = VO.stats(O.carve(p) if carve_predictions else p, gt)
                assert out["stats"][m, v].tolist() == s.tolist(), (fill, m, v)
                assert out["dropped"][m, v] == dropped and out["iou"][m, v] == VO.iou(s)
        assert out["dropped"][0, 0] == 3
    R.check_status()


@pytest.mark.parametrize("carve_predictions", [True, False])
def test_solid_iou_of_split_does_not_depend_on_models_per_call(carve_predictions):
    """Three models (the last group is short at 2 per call), two views of 24 points, one view truncated to 16, a rotation,
    a tetrahedron per model."""
    rng = np.random.default_rng(21)
    preds = [((rng.random((2, 24, 3)) * 0.6 - 0.3).astype(np.float32), np.array([24, 16]) if m == 1 else None) for m in range(3)]
    corners = np.array([[-0.4, -0.4, -0.4], [0.4, -0.3, -0.35], [-0.3, 0.4, -0.3], [-0.35, -0.3, 0.4]])
    meshes = [((corners * (1.0 - 0.1 * m)).astype(np.float32), np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])) for m in range(3)]
    q = np.array([[0.9, 0.1, -0.3, 0.2]])
    got = [R.solid_iou_of_split(preds, meshes, reference_rotation=q, vox_size=8, carve_predictions=carve_predictions,
                                models_per_call=step) for step in (1, 2, 256)]
    assert set(got[0]) == {"stats", "iou", "dropped", "info"} and got[0]["stats"].shape == (3, 2, 5) and got[0]["stats"][..., 1].any()
    for key, a in got[0].items():
        assert a.dtype == got[1][key].dtype == got[2][key].dtype and a.tobytes() == got[1][key].tobytes() == got[2][key].tobytes(), key
    R.check_status()
