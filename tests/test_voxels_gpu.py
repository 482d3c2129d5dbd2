"""Voxel-grid evaluation on the GPU (csrc/dpc_voxels.hip) against the numpy restatement of its conventions
(tests/voxels_oracle.py).  Everything is compared exactly: bit-OR and popcount do not depend on order and voxel2pc's
coordinates are fixed by np.linspace, so every output has one right answer.

The sweep of `sweep` runs once per module.  Grids: 1^3, 2^3, 3^3 (27 bits: a partial word), 31^3, 32^3 (the largest of the
launcher's first size class), 33^3 (the first of the second), 64^3 (its largest), 65^3 (the first of the slab class, one
slab), 81^3 (the first with two slabs), 128^3 (four slabs, the limit) and 8 x 16 x 16 through vox_size_z.  Clouds of 0, 1,
63, 64, 65, 1025 and 8000 points, as fp32 and as their fp64 copies, with points exactly on the cube's faces, exactly
half-way between nodes and just outside the cube (voxels_oracle.cloud)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dpc.render as R
import voxels_oracle as O
from dpc.render import _native
from test_abi_and_host import device_object_output

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(1, -1), (2, -1), (3, -1), (31, -1), (32, -1), (33, -1), (64, -1), (16, 8), (65, -1), (81, -1), (128, -1)]   # (vox_size, vox_size_z)
SIZES = [0, 1, 63, 64, 65, 1025, 8000]
EXPECTED = {"k_voxelise<%d, %d, %d>" % (f, w, t) for f in (0, 1) for w, t in ((1024, 256), (8192, 512), (16384, 1024))} | \
           {"k_voxel_threshold<%d>" % d for d in (0, 1, 2)} | {"k_voxel_unpack", "k_voxel_stats", "k_voxel_count", "k_voxel2pc"}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def grid_id(g):
    return "%dx%d" % (g[0], g[0] if g[1] == -1 else g[1])


def special_grids(G, dtype, seed):
    """[6,G,G,G]: all zero, all one, one voxel at each corner, one voxel alone, and two random grids."""
    v = np.zeros((6, G, G, G), dtype=dtype)
    v[1] = 1
    for c in np.ndindex(2, 2, 2):
        v[2][tuple(np.array(c) * (G - 1))] = 1
    v[3, G - 1, 0, G // 2] = 1
    v[4:] = O.float_grids(2, (G, G, G), seed, dtype)
    return v


@pytest.fixture(scope="module")
def sweep():
    """({grid: (clouds32, grids and dropped for fp32, for fp64)}, the grid-grid and voxel2pc results, the instantiations
    launched)."""
    out, launched = {"vox": {}, "stats": {}, "pc": {}}, set()
    R.check_status()
    for g in GRIDS:
        shape = O.shape_of(*g)
        c32 = [O.cloud(n, 17 * n + g[0], np.float32, shape) for n in SIZES]
        got = {}

        def run():
            for name, clouds in (("f32", c32), ("f64", [c.astype(np.float64) for c in c32])):
                grids, dropped = R.voxelise([dev(c) for c in clouds], g[0], g[1], return_dropped=True)
                assert grids.dtype == torch.bool and grids.is_cuda and tuple(grids.shape) == (len(SIZES),) + shape
                assert dropped.dtype == torch.int32 and tuple(dropped.shape) == (len(SIZES),)
                got[name] = (grids.cpu().numpy(), dropped.cpu().numpy())

        launched |= _native.launched_instantiations(run, torch.device("cuda"))
        out["vox"][g] = (c32, got["f32"], got["f64"])
    for dtype in (np.float32, np.float64):
        for thr in (0.3, 0.5):
            preds = O.float_grids(5, (7, 9, 11), 5 + int(thr * 10), dtype)
            gts = O.float_grids(3, (7, 9, 11), 50, np.float32) > 0.6
            gt_of = [0, 1, 2, 1, 1]
            got = {}

            def run():
                got["s"] = R.voxel_stats(dev(preds), dev(gts), gt_of=gt_of, threshold=thr)

            launched |= _native.launched_instantiations(run, torch.device("cuda"))
            out["stats"][np.dtype(dtype).name, thr] = (preds, gts, gt_of, got["s"])
    for G in (2, 3, 33, 64):
        v = special_grids(G, np.float32 if G != 33 else np.float64, G)
        got = {}

        def run():
            got["p"] = R.voxels2pc_batched(dev(v), 0.5)

        launched |= _native.launched_instantiations(run, torch.device("cuda"))
        out["pc"][G] = (v, got["p"])
    assert R.check_status() == 0
    return out, launched


# 1 voxelise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", GRIDS, ids=grid_id)
def test_voxelise_equals_the_oracle_for_fp32_and_fp64(sweep, g):
    c32, f32, f64 = sweep[0]["vox"][g]
    shape = O.shape_of(*g)
    assert f32[0].tobytes() == f64[0].tobytes() and f32[1].tolist() == f64[1].tolist()   # an fp32 cloud and its fp64 copy
    for k, c in enumerate(c32):
        ref, dropped = O.voxelise(c, shape)
        assert (f32[0][k] == ref).all(), (g, SIZES[k], int((f32[0][k] != ref).sum()))
        assert f32[1][k] == dropped, (g, SIZES[k])
    assert f32[1][-1] > 0 and f32[0][-1].any() and not f32[0][0].any()     # the sweep does drop points; no points, no voxels


def test_the_sweep_launches_every_compiled_instantiation(sweep):
    """The instantiations in the launch record over the sweep == the launcher's class table == the kernel symbols of
    dpc_voxels.o: a size class added without a grid in GRIDS that reaches it fails here."""
    launched = {i for i in sweep[1] if i.startswith("k_vox")}
    assert launched == EXPECTED, sorted(launched ^ EXPECTED)
    built = set()
    for line in device_object_output("dpc_voxels.o", ["llvm-readelf", "-sW"]).splitlines():
        f = line.split()
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)(\w+)$", f[7]) if len(f) >= 8 and f[3] == "FUNC" else None
        if m:
            n = int(m.group(1))
            name, rest = m.group(2)[:n], m.group(2)[n:]
            targs = re.match(r"I((?:Li-?\d+E)+)E", rest)
            built.add(name + ("<%s>" % ", ".join(re.findall(r"Li(-?\d+)E", targs.group(1))) if targs else ""))
    built = {b for b in built if b.startswith("k_vox")}
    assert launched == built, sorted(launched ^ built)


def raw_voxelise(pts, rows, shape, status=None, fill=-1, host_rows=None):
    """dpc_voxelise itself on a packed device buffer and a table of (start, count) rows: (uint32 words [C, words], dropped)."""
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))
    host = desc if host_rows is None else np.ascontiguousarray(np.asarray(host_rows, dtype=np.int32).reshape(-1, 2))
    words = (shape[0] * shape[1] * shape[2] + 31) // 32
    bits = torch.full((len(desc), words), fill, dtype=torch.int32, device="cuda")
    dropped = torch.full((len(desc),), -7, dtype=torch.int32, device="cuda")
    rc = _native.lib().dpc_voxelise(_native.ptr(pts), int(pts.shape[0]), int(pts.dtype == torch.float64), _native.ptr(dev(desc)),
                                    host.ctypes.data_as(ctypes.c_void_p), len(desc), shape[0], shape[1], shape[2], _native.ptr(bits),
                                    _native.ptr(dropped), _native.ptr(status), _native.stream_ptr(pts.device))
    assert rc == 0
    return bits.cpu().numpy().view(np.uint32), dropped.cpu().numpy()


@pytest.mark.parametrize("shape", [(3, 3, 3), (33, 33, 33), (8, 16, 16), (5, 7, 9), (81, 81, 81)], ids=str)
def test_bit_layout_padding_bits_and_shared_rows(shape):
    """The words themselves, written over a buffer of all ones: voxel f is bit f & 31 of word f >> 5, the padding bits of the
    last word are zero, and clouds may share or be sub-ranges of the same rows."""
    P = O.cloud(3000, 9, np.float32, shape)
    rows = [(0, 3000), (0, 0), (100, 1), (500, 2000), (0, 3000)]
    bits, dropped = raw_voxelise(dev(P), rows, shape)
    for k, (start, count) in enumerate(rows):
        ref, d = O.voxelise(P[start:start + count], shape)
        assert bits[k].tobytes() == O.pack_bits(ref).tobytes(), (shape, k)
        assert dropped[k] == d
    V = shape[0] * shape[1] * shape[2]
    if V % 32:
        assert (bits[:, -1] >> np.uint32(V % 32) == 0).all()


def test_one_call_or_one_cloud_at_a_time():
    for g in ((33, -1), (16, 8), (81, -1)):
        shape = O.shape_of(*g)
        clouds = [dev(O.cloud(n, n + 3, np.float32 if n % 2 else np.float64, shape)) for n in (0, 65, 1025, 4000)]
        grids, dropped = R.voxelise(clouds, g[0], g[1], return_dropped=True)
        rev = R.voxelise(clouds[::-1], g[0], g[1])
        for k, c in enumerate(clouds):
            one, d = R.voxelise([c], g[0], g[1], return_dropped=True)
            assert torch.equal(one[0], grids[k]) and d[0] == dropped[k] and torch.equal(rev[len(clouds) - 1 - k], grids[k])
    both = R.voxelise(torch.stack([clouds[2][:900].float(), clouds[3][:900].float()]), 16)   # a [B,n,3] tensor
    assert tuple(both.shape) == (2, 16, 16, 16) and torch.equal(both[1], R.voxelise([clouds[3][:900]], 16)[0])
    assert R.check_status() == 0


def test_nonfinite_points_are_dropped_and_flagged():
    shape = (16, 16, 16)
    a = O.cloud(700, 1, np.float32, shape)
    nan, inf = a.copy(), a.astype(np.float64)
    nan[13, 1] = np.nan
    inf[650, 2] = -np.inf
    inf[651, 0] = np.inf
    R.check_status()   # clean slate
    grids, dropped = R.voxelise([dev(a), dev(nan), dev(inf), dev(a)], 16, return_dropped=True)
    assert R.check_status() == _native.DPC_STATUS_NONFINITE and R.check_status() == 0
    for k, c in enumerate((a, nan, inf, a)):
        ref, d = O.voxelise(c, shape)
        assert (grids[k].cpu().numpy() == ref).all() and int(dropped[k]) == d
    assert int(dropped[1]) >= int(dropped[0]) and int(dropped[2]) >= int(dropped[0])
    R.voxelise([dev(a)], 16)
    assert R.check_status() == 0   # finite points outside the cube are dropped without a flag


def test_device_tables_that_differ_from_the_host_tables_are_not_run():
    """The guards of the header: a device row outside its array sets DPC_STATUS_BAD_INDEX, is not read and leaves its
    outputs as they were; the other rows are unaffected."""
    shape = (9, 9, 9)
    P = O.cloud(600, 8, np.float32, shape)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    bits, dropped = raw_voxelise(dev(P), [(0, 700), (0, 300), (-1, 5)], shape, status, fill=-1, host_rows=[(0, 600), (0, 300), (0, 5)])
    assert status.item() == _native.DPC_STATUS_BAD_INDEX
    assert (bits[0] == 0xFFFFFFFF).all() and (bits[2] == 0xFFFFFFFF).all() and dropped.tolist()[::2] == [-7, -7]
    assert bits[1].tobytes() == O.pack_bits(O.voxelise(P[:300], shape)[0]).tobytes()
    # dpc_voxel_stats: pair 1 names a grid that is not there
    a = dev(np.stack([O.pack_bits(O.voxelise(P[:300], shape)[0]), O.pack_bits(O.voxelise(P[300:], shape)[0])]).view(np.int32))
    host = np.array([(0, 1), (1, 0), (1, 1)], dtype=np.int32)
    bad = host.copy()
    bad[1] = (2, 0)
    stats = torch.full((3, 5), -7, dtype=torch.int64, device="cuda")
    status.zero_()
    rc = _native.lib().dpc_voxel_stats(_native.ptr(a), 2, _native.ptr(a), 2, 9, 9, 9, _native.ptr(dev(bad)),
                                       host.ctypes.data_as(ctypes.c_void_p), 3, _native.ptr(stats), _native.ptr(status),
                                       _native.stream_ptr(a.device))
    assert rc == 0 and status.item() == _native.DPC_STATUS_BAD_INDEX
    s = stats.cpu().numpy()
    g0, g1 = O.voxelise(P[:300], shape)[0], O.voxelise(P[300:], shape)[0]
    assert s[0].tolist() == O.stats(g0, g1).tolist() and (s[1] == -7).all() and s[2].tolist() == O.stats(g1, g1).tolist()
    # dpc_voxel2pc: a table whose count is not the grid's writes nothing beyond its range and is flagged
    n = int(g0.sum())
    xyz = torch.full((n + 4, 3), -7.0, dtype=torch.float64, device="cuda")
    desc = np.array([(0, n - 2)], dtype=np.int32)
    status.zero_()
    rc = _native.lib().dpc_voxel2pc(_native.ptr(a), 1, 9, _native.ptr(dev(desc)), desc.ctypes.data_as(ctypes.c_void_p), n + 4,
                                    _native.ptr(xyz), _native.ptr(status), _native.stream_ptr(a.device))
    assert rc == 0 and status.item() == _native.DPC_STATUS_BAD_INDEX
    ref = O.voxel2pc(g0.astype(np.float32), 0.5)[0]
    got = xyz.cpu().numpy()
    assert got[:n - 2].tobytes() == ref[:n - 2].tobytes() and (got[n - 2:] == -7.0).all()


# 2 voxel_stats / voxel_iou -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thr", [0.3, 0.5])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_grid_grid_stats_with_voxels_exactly_on_the_threshold(sweep, dtype, thr):
    preds, gts, gt_of, got = sweep[0]["stats"][dtype, thr]
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (5, 5)
    t = preds.dtype.type(thr)
    assert ((preds == t).sum(axis=(1, 2, 3)) >= 1).all() and np.isnan(preds).any()     # the inputs do sit on the threshold
    want = np.stack([O.stats(O.threshold(preds[i], thr, True), gts[k]) for i, k in enumerate(gt_of)])
    assert got.cpu().numpy().tolist() == want.tolist()


def test_cloud_and_grid_sources_shared_ground_truth_and_the_trivial_pairs():
    g = (16, 8)
    shape = O.shape_of(*g)
    clouds = [O.cloud(n, 70 + n, np.float32 if n % 2 else np.float64, shape) for n in (300, 301, 0, 1500)]
    gt_clouds = [O.cloud(2000, 5, np.float64, shape), np.zeros((0, 3), dtype=np.float32)]
    vox = [O.voxelise(c, shape)[0] for c in clouds]
    gt_vox = [O.voxelise(c, shape)[0] for c in gt_clouds]
    gt_of = [0, 0, 1, 1]
    want = np.stack([O.stats(vox[i], gt_vox[k]) for i, k in enumerate(gt_of)])
    # cloud - cloud, views sharing a ground truth; pair 2 is empty against empty
    got = R.voxel_stats([dev(c) for c in clouds], [dev(c) for c in gt_clouds], gt_of=gt_of, vox_size=16, vox_size_z=8)
    assert got.cpu().numpy().tolist() == want.tolist() and want[2].tolist() == [0, 0, 0, 0, 0]
    iou = R.voxel_iou([dev(c) for c in clouds], [dev(c) for c in gt_clouds], gt_of=gt_of, vox_size=16, vox_size_z=8)
    assert iou.dtype == torch.float64 and iou.cpu().numpy().tobytes() == O.iou(want).tobytes()
    assert np.isnan(iou[2].item()) and iou[3].item() == 0.0
    # grid - cloud: float predictions against ground-truth clouds, the shape taken from the grid
    fl = O.float_grids(4, shape, 3, np.float32)
    got = R.voxel_stats(dev(fl), [dev(c) for c in gt_clouds], gt_of=gt_of, threshold=0.3)
    assert got.cpu().numpy().tolist() == [O.stats(O.threshold(fl[i], 0.3, True), gt_vox[k]).tolist() for i, k in enumerate(gt_of)]
    # cloud - grid: bool and uint8 ground-truth grids, numpy clouds
    gt_grid = np.stack(gt_vox)
    for gg in (dev(gt_grid), dev(gt_grid.astype(np.uint8) * 3)):
        assert R.voxel_stats(clouds, gg, gt_of=gt_of).cpu().numpy().tolist() == want.tolist()
    # identical inputs: IoU 1, no difference
    same = R.voxel_stats([dev(clouds[3])], [dev(clouds[3])], vox_size=16, vox_size_z=8).cpu().numpy()[0]
    n = int(vox[3].sum())
    assert same.tolist() == [0, n, n, 0, 0] and n > 0
    assert R.voxel_iou(dev(fl[:1].astype(np.float64)), dev(O.threshold(fl[:1].astype(np.float64), 0.5, True))).item() == 1.0
    assert tuple(R.voxel_stats([], [], vox_size=4).shape) == (0, 5)
    assert R.check_status() == 0


def test_stats_of_the_largest_grid():
    """128^3: 65536 words per grid, 256 per thread of the pair's workgroup."""
    rng = np.random.default_rng(2)
    a = rng.random((2, 128, 128, 128), dtype=np.float32)
    g = rng.random((1, 128, 128, 128)) < 0.3
    got = R.voxel_stats(dev(a), dev(g), gt_of=[0, 0], threshold=0.5).cpu().numpy()
    assert got.tolist() == [O.stats(a[i] >= np.float32(0.5), g[0]).tolist() for i in range(2)]


# 3 voxel2pc ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [2, 3, 33, 64])
def test_voxels2pc_batched_equals_the_oracle_byte_for_byte(sweep, G):
    v, got = sweep[0]["pc"][G]
    assert len(got) == len(v)
    for b in range(len(v)):
        ref, occ = O.voxel2pc(v[b], 0.5)
        assert got[b].dtype == torch.float64 and got[b].is_cuda and tuple(got[b].shape) == ref.shape, (G, b)
        assert got[b].cpu().numpy().tobytes() == ref.tobytes(), (G, b)
    assert len(got[0]) == 0 and len(got[1]) == G ** 3 and len(got[2]) == 8 and len(got[3]) == 1
    # ascending flat index: recover (i, j, k) from (x[j], x[i], x[k]) and compare with the occupied voxels in order
    x = O.axis_coordinates(G)
    p = got[5].cpu().numpy()
    j, i, k = (np.searchsorted(x, p[:, c]) for c in range(3))
    flat = (i * G + j) * G + k
    assert (np.diff(flat) > 0).all() and flat.tolist() == np.flatnonzero(O.threshold(v[5], 0.5, False).reshape(-1)).tolist()


@pytest.mark.parametrize("G", [2, 5, 33])
def test_round_trip_through_voxelise_is_the_transposed_mask(G):
    v = O.float_grids(3, (G, G, G), 60 + G, np.float32)
    clouds = R.voxels2pc_batched(dev(v), 0.3)
    grids, dropped = R.voxelise(clouds, G, return_dropped=True)
    assert dropped.cpu().tolist() == [0, 0, 0]
    assert (grids.cpu().numpy() == O.threshold(v, 0.3, False).transpose(0, 2, 1, 3)).all()


def test_reference_functions_on_the_fixture_inputs_equal_the_fixture():
    """evaluate_voxel_prediction and voxel2pc on the inputs the fixture's seeds regenerate == what the reference returned."""
    f = np.load(os.path.join(ROOT, "tests", "golden", "f25_voxels.npz"))
    for key, G, thr, dtype, seed in O.golden_cases():
        voxels, preds, gt = O.golden_inputs(G, seed, dtype)
        assert f[key + "/inputs"].tolist() == [O.digest(voxels), O.digest(preds), O.digest(gt)], key
        xyz, occ = R.voxel2pc(voxels, thr)
        assert isinstance(xyz, np.ndarray) and xyz.dtype == np.float64 and occ.dtype == bool and occ.shape == (G ** 3,)
        assert O.digest(xyz) == str(f[key + "/xyz_digest"]) and np.packbits(occ).tobytes() == f[key + "/occupancies"].tobytes(), key
        sums = R.evaluate_voxel_prediction(preds, gt, thr)
        assert isinstance(sums, np.ndarray) and sums.dtype == np.int64 and sums.tolist() == f[key + "/sums"].tolist(), key
    # tensors in, device tensors out
    xyz_t, occ_t = R.voxel2pc(dev(voxels), thr)
    assert xyz_t.is_cuda and occ_t.dtype == torch.bool and xyz_t.cpu().numpy().tobytes() == xyz.tobytes()
    assert torch.equal(occ_t.cpu(), torch.from_numpy(occ))
    assert R.evaluate_voxel_prediction(dev(preds), dev(gt), thr).tolist() == sums.tolist()
    assert R.check_status() == 0


# 4 iou_of_split ------------------------------------------------------------------------------------------------------
def test_iou_of_split_against_per_pair_oracle_calls():
    """3 models x 2 views, one model with truncated views, a reference rotation: stats, iou and dropped equal the oracle on
    the rotated, truncated views; models_per_call 1 and 256 agree bit for bit."""
    from dpc.render._split import _host_unit_quaternion, _rotate

    rng = np.random.default_rng(12)
    M, V, N, G = 3, 2, 300, 16
    preds = [((rng.random((V, N, 3)) * 0.9 - 0.45).astype(np.float32), np.array([250, 0]) if m == 1 else None) for m in range(M)]
    gts = [rng.random((310 + m, 3)) - 0.5 for m in range(M)]
    q = np.array([[0.9, 0.1, -0.3, 0.2]])
    R.check_status()
    got = R.iou_of_split(preds, gts, reference_rotation=q, vox_size=G, models_per_call=256)
    one = R.iou_of_split(preds, gts, reference_rotation=q, vox_size=G, models_per_call=1)
    assert got["stats"].shape == (M, V, 5) and got["stats"].dtype == np.int64 and got["iou"].shape == (M, V)
    assert got["iou"].dtype == np.float64 and got["dropped"].shape == (M, V) and got["dropped"].dtype == np.int64
    for k in ("stats", "iou", "dropped"):
        assert got[k].tobytes() == one[k].tobytes(), k
    qn = _host_unit_quaternion(q)
    for m in range(M):
        rot = _rotate(torch.from_numpy(preds[m][0]), qn, torch.device("cuda")).cpu().numpy()
        gt_vox = O.voxelise(gts[m], (G, G, G))[0]
        for i in range(V):
            n = N if preds[m][1] is None else int(preds[m][1][i])
            vox, dropped = O.voxelise(rot[i][:n], (G, G, G))
            want = O.stats(vox, gt_vox)
            assert got["stats"][m, i].tolist() == want.tolist() and got["dropped"][m, i] == dropped, (m, i)
            assert got["iou"][m, i].tobytes() == O.iou(want).tobytes()
    assert got["dropped"].sum() > 0 and got["iou"][1, 1] == 0.0 and (got["iou"][0] > 0).all()
    plain = R.iou_of_split(preds, gts, vox_size=G, vox_size_z=8)
    assert plain["stats"][0, 0].tolist() == O.stats(O.voxelise(preds[0][0][0], (8, G, G))[0], O.voxelise(gts[0], (8, G, G))[0]).tolist()
    assert R.check_status() == 0


# 5 render_voxels -----------------------------------------------------------------------------------------------------
def test_render_voxels_is_voxel2pc_then_render_point_clouds():
    v = O.float_grids(1, (9, 9, 9), 4, np.float32)[0]
    img = R.render_voxels(v.reshape(1, 9, 9, 9, 1), 0.5, image_size=32, supersample=1, point_size=0.01)
    xyz, _ = R.voxel2pc(dev(v), 0.5)
    want = R.render_point_clouds([xyz], image_size=32, supersample=1, point_size=0.01)[0]
    assert tuple(img.shape) == (32, 32, 3) and img.dtype == torch.uint8 and torch.equal(img, want)
    assert len(torch.unique(img.reshape(-1, 3), dim=0)) > 1   # something was drawn


def test_render_predictions_tool_in_voxels_mode(tmp_path):
    """tools/render_predictions.py --voxels: <model>_vox.npz ("arr_0", the first view, squeezed) -> <model>.png, equal to
    render_voxels with the same camera; a second run skips what is there."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("render_predictions", os.path.join(ROOT, "tools", "render_predictions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    inp, out = tmp_path / "pred", tmp_path / "render"
    inp.mkdir()
    v = O.float_grids(2, (9, 9, 9), 8, np.float32).reshape(2, 9, 9, 9, 1)      # two views; the first is drawn
    np.savez(str(inp / "chair_vox.npz"), v)
    args = ["--inp_dir=%s" % inp, "--out_dir=%s" % out, "--voxels", "--vis_threshold=0.3", "--render_image_size=32", "--supersample=1"]
    assert mod.main(args) == {"written": ["chair"], "skipped": []}
    want = R.render_voxels(v[0], 0.3, azimuth=140.0, elevation=15.0, dist=2.0, image_size=32, supersample=1, lens_mm=35.0,
                           point_size=0.01)
    assert np.array_equal(R.read_png_any(str(out / "chair.png")), want.cpu().numpy())
    assert mod.main(args) == {"written": [], "skipped": ["chair"]}
