"""dpc_mesh_winding and dpc_mesh_winding_voxels on the GPU: the winding sums against the 50-digit sums of the fixture
f32_winding.npz, the chunked path, reproducibility, the guards, the inside test, the signed distance and the solid fill.

Tolerance.  Away from the surface an fp64 term is right to about 1e-16 against the quantum 2^-40 ~ 9e-13, so a device
term's quantised value differs from the exactly evaluated term's by at most one quantum:
|sum_device - sum_mpmath| <= the usable faces of the row (winding_oracle.bound), and nothing is added to it.  The
conditioning fails only next to edges, so every compared query keeps 1e-3 of the mesh's extent from the surface
(tests/test_winding_host.py checks the fixture's; the meshes made here are checked here, with point_mesh_distance).  The
guard cases (a point on a vertex, in a face's plane) and every reproducibility check compare bit for bit.

Measured on an MI355X (the tests print them): see DESIGN.md section 4, "Generalized winding numbers"."""
import ctypes

import numpy as np
import pytest
import torch

import point_mesh_oracle as PM
import winding_oracle as WO
import dpc.render as R
from dpc.render import _native

pytestmark = pytest.mark.gpu

BLOCK, TILE, CHUNK = _native.DPC_PM_BLOCK, _native.DPC_PM_FACE_TILE, _native.DPC_PM_FACE_TILE * _native.DPC_PM_CHUNK_TILES
ONE = 1 << WO.FRAC_BITS
Q = 2.0 ** -WO.FRAC_BITS


@pytest.fixture(scope="module")
def f32(golden):
    return golden("f32_winding.npz")


def case(f32, name):
    return f32[name + "_P"], f32[name + "_V"], f32[name + "_F"]


def sums_of(P, V, F):
    w, s = R.winding_numbers([P], [(V, F)], return_sums=True)
    assert w[0].is_cuda and w[0].dtype == torch.float64 and s[0].dtype == torch.int64 and w[0].shape == s[0].shape == (len(P),)
    assert torch.equal(w[0], s[0].double() * Q)                         # winding is sums * 2^-40 exactly
    return s[0].cpu().numpy()


@pytest.fixture(scope="module")
def results(f32):
    """Every case once, one row each: {name: int64 sums as numpy}."""
    R.check_status()
    out = {str(name): sums_of(*case(f32, name)) for name in f32["cases"]}
    assert R.check_status() == 0
    return out


def extent(V):
    v = np.asarray(V).astype(np.float64)
    return float((v.max(axis=0) - v.min(axis=0)).max())


@pytest.fixture(scope="module")
def ball():
    """extract_surfaces of a Gaussian ball on a 24^3 grid, in index units: (V fp64, F int32) as numpy, the field and the
    iso level.  More than two chunks of faces, so a call of a few points splits its face range."""
    G, c, r, sigma = 24, np.array([11.6, 11.4, 11.7]), 9.2, 5.0
    n = np.stack(np.meshgrid(*[np.arange(G, dtype=np.float64)] * 3, indexing="ij"), axis=-1)
    field = np.exp(-((n - c) ** 2).sum(-1) / (2 * sigma * sigma))
    iso = float(np.exp(-r * r / (2 * sigma * sigma)))
    (V, F), = R.extract_surfaces(torch.from_numpy(field).cuda()[None], iso)
    V, F = V.cpu().numpy(), F.cpu().numpy().astype(np.int32)
    assert len(F) >= 2 * CHUNK + 1, len(F)
    return V, F, field, iso, n.reshape(-1, 3), c


def test_values_against_the_exact_sums(f32, results):
    """Every clear case within one quantum per usable face of the mpmath sums; closed meshes give w = 1 or 0 wound outward
    and -1 or 0 wound inward; the soup in all four dtype instantiations, which the launch record shows ran."""
    worst = {}
    for name in f32["clear"]:
        got, want, bound = results[str(name)], f32[name + "_sums"], int(f32[name + "_bound"])
        worst[str(name)] = int(np.abs(got - want).max())
        print("winding %-9s |device - mpmath| max %d quanta (bound %d)" % (name, worst[str(name)], bound))
    for name in f32["clear"]:
        assert worst[str(name)] <= int(f32[name + "_bound"]), (name, worst)
    for name, sign in (("cube", 1), ("tetra", 1), ("cube_in", -1), ("tetra_in", -1)):
        s, n = results[name], int(f32[name + "_bound"])
        inside = np.abs(f32[name.replace("_in", "") + "_sums"] - ONE) <= n
        assert 5 <= inside.sum() <= len(s) - 5
        assert (np.abs(s[inside] - sign * ONE) <= n).all() and (np.abs(s[~inside]) <= n).all(), name
    P, V, F = case(f32, "soup32")
    combos = [(P.astype(pd), V.astype(vd)) for pd in (np.float32, np.float64) for vd in (np.float32, np.float64)]
    for Pd, Vd in combos:                                                # fp32 widens exactly: the same sums, bit for bit
        assert np.array_equal(sums_of(Pd, Vd, F), results["soup32"]), (Pd.dtype, Vd.dtype)
    ran = _native.launched_instantiations(lambda: [R.winding_numbers([Pd], [(Vd, F)]) for Pd, Vd in combos], torch.device("cuda"))
    assert {"k_wn_sum<%d, %d>" % (p, v) for p in (0, 1) for v in (0, 1)} | {"k_wn_finish<0>", "k_wn_finish<1>"} <= ran, ran


def test_chunked_path_and_the_extractor_is_closed_and_outward(ball):
    """5 points against more than two chunks of faces (the face range is split over workgroups), against mpmath; every
    node of the ball's grid that keeps the clearance: inside nodes give w = 1, outside nodes w = 0 within the bound, so
    extract_surfaces' mesh is closed and wound outward; 300 points (two point blocks) against 3 faces."""
    V, F, field, iso, nodes, c = ball
    mesh, n = (V, F), len(F)
    P = np.array([c, c + (3, 1, 2), (1.0, 1.0, 1.0), (20.0, 20.0, 3.0), c + (0, 0, 10.5)])
    d, = R.point_mesh_distance([P], [mesh])
    assert float(d.min()) >= WO.CLEARANCE * extent(V)
    tab = np.ascontiguousarray([[0, 5, 0, len(V), 0, n]], dtype=np.int32)
    assert _native.lib().dpc_mesh_winding_workspace_bytes(tab.ctypes.data_as(ctypes.c_void_p), 1) >= 3 * 5 * 8    # three chunks
    got, (want, status) = sums_of(P, V, F), WO.mesh_sums_mp(P, V, F)
    print("winding chunked: %d faces, |device - mpmath| %s quanta" % (n, np.abs(got - want).tolist()))
    assert status == 0 and WO.bound(V, F) == n and (np.abs(got - want) <= n).all()
    assert (np.abs(got - np.array([ONE, ONE, 0, 0, 0])) <= n).all()

    d, = R.point_mesh_distance([nodes], [mesh])
    clear = (d >= WO.CLEARANCE * extent(V)).cpu().numpy()
    inside = (field > iso).reshape(-1)
    assert clear.sum() >= 0.9 * len(nodes) and 1000 < inside[clear].sum() < len(nodes) - 1000
    got = sums_of(nodes, V, F)
    err = np.abs(got - np.where(inside, ONE, 0))[clear]
    print("winding ball: %d of %d nodes clear, |sum - {2^40, 0}| max %d quanta (bound %d)" % (clear.sum(), len(nodes), err.max(), n))
    assert (err <= n).all()

    rng = np.random.default_rng(11)
    V3 = rng.uniform(-0.5, 0.5, size=(3 * 3, 3)).astype(np.float32)
    F3 = np.arange(9, dtype=np.int32).reshape(3, 3)
    pts = []
    while len(pts) < 300:                                                # by the geometry alone, before anything is run
        p = rng.uniform(-0.6, 0.6, size=(1, 3)).astype(np.float32)
        if np.sqrt(PM.mesh_d2(p, V3, F3)[0][0]) >= 2 * WO.CLEARANCE * extent(V3):
            pts.append(p[0])
    P3 = np.asarray(pts)
    got, (want, _) = sums_of(P3, V3, F3), WO.mesh_sums_mp(P3, V3, F3)
    print("winding 300 x 3: |device - mpmath| max %d quanta" % np.abs(got - want).max())
    assert len(P3) > BLOCK and (np.abs(got - want) <= 3).all()


def test_sums_do_not_depend_on_order_batching_or_chunking(f32, results, ball):
    P, V, F = case(f32, "soup64")
    base = torch.from_numpy(results["soup64"]).cuda()
    sums = lambda clouds, meshes, mesh_of=None: R.winding_numbers(clouds, meshes, mesh_of, return_sums=True)[1]
    perm = np.random.default_rng(3).permutation(len(P))
    assert torch.equal(sums([P[perm]], [(V, F)])[0], base[torch.from_numpy(perm).cuda()])                   # reordered
    assert torch.equal(torch.cat(sums([P[:7], P[7:30], P[30:]], [(V, F)], [0, 0, 0])), base)                 # split into rows
    Pc, Vc, Fc = case(f32, "cube")
    Pt, Vt, Ft = case(f32, "tetra_in")
    got = sums([Pc, P, Pt, P[:0]], [(Vc, Fc), (V, F), (Vt, Ft)], [0, 1, 2, 1])                               # batched with others
    assert torch.equal(got[1], base) and len(got[3]) == 0
    assert np.array_equal(got[0].cpu().numpy(), results["cube"]) and np.array_equal(got[2].cpu().numpy(), results["tetra_in"])
    shared, copies = sums([P, P[::-1].copy()], [(V, F)], [0, 0]), sums([P, P[::-1].copy()], [(V, F), (V.copy(), F.copy())])
    assert torch.equal(shared[0], base) and torch.equal(shared[1], base.flip(0))                             # one mesh copy
    assert torch.equal(copies[0], base) and torch.equal(copies[1], base.flip(0))
    # one point, chunked (alone: three chunks of faces) and unchunked (one of 2048 one-point rows: the point blocks fill
    # the device, every row walks all faces in one work item)
    Vb, Fb, _, _, nodes, c = ball
    rows = 8 * 256
    pts = nodes[np.random.default_rng(4).choice(len(nodes), rows, replace=False)].copy()
    pts[0] = c + (3, 1, 2)
    tab = lambda k: np.ascontiguousarray([[i, 1, 0, len(Vb), 0, len(Fb)] for i in range(k)], dtype=np.int32)
    ws = lambda t: _native.lib().dpc_mesh_winding_workspace_bytes(t.ctypes.data_as(ctypes.c_void_p), len(t))
    assert ws(tab(1)) >= 3 * 8 + 3 * 2 * 4 and ws(tab(rows)) <= rows * 8 + 3 * (rows + 1) * 4 + 5 * 16     # 3 slots a point; 1
    alone = sums([pts[:1]], [(Vb, Fb)])[0]
    many = sums([p[None] for p in pts], [(Vb, Fb)], [0] * rows)
    assert torch.equal(many[0], alone) and abs(int(alone[0]) - ONE) <= len(Fb)
    every = sums([pts], [(Vb, Fb)])[0]                                                                       # and as one row
    assert torch.equal(torch.cat(many), every)


def raw(P, V, F, rows, dev_rows=None, want=(True, True)):
    """dpc_mesh_winding itself (the Python functions refuse what the guards are for): (sums, w, status) as numpy, the
    outputs pre-filled with a sentinel."""
    dev = torch.device("cuda")
    pts, verts = torch.from_numpy(np.ascontiguousarray(P)).to(dev), torch.from_numpy(np.ascontiguousarray(V)).to(dev)
    faces = torch.from_numpy(np.ascontiguousarray(F, dtype=np.int32)).to(dev)
    host = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 6)
    desc = torch.from_numpy(host if dev_rows is None else np.ascontiguousarray(dev_rows, dtype=np.int32).reshape(-1, 6)).to(dev)
    n = int(host[:, 1].sum())
    sums = torch.full((n,), -77, dtype=torch.int64, device=dev) if want[0] else None
    w = torch.full((n,), -77.0, dtype=torch.float64, device=dev) if want[1] else None
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(16, _native.lib().dpc_mesh_winding_workspace_bytes(host.ctypes.data_as(ctypes.c_void_p), len(host))),),
                     dtype=torch.uint8, device=dev)
    _native.call(dev, "dpc_mesh_winding", _native.ptr(pts), len(P), int(pts.dtype == torch.float64), _native.ptr(verts), len(V),
                 int(verts.dtype == torch.float64), _native.ptr(faces), len(F), _native.ptr(desc), host.ctypes.data, len(host),
                 _native.ptr(sums), _native.ptr(w), _native.ptr(ws), _native.ptr(status))
    torch.cuda.synchronize()
    return (None if sums is None else sums.cpu().numpy()), (None if w is None else w.cpu().numpy()), int(status.item())


def test_guards(f32, results):
    P, V, F = case(f32, "cube")
    row = [[0, len(P), 0, len(V), 0, len(F)]]
    s, w, status = raw(P, V, F, row)
    assert status == 0 and np.array_equal(s, results["cube"]) and np.array_equal(w, s * Q)
    s, w, _ = raw(P, V, F, row, want=(False, True))
    assert s is None and np.array_equal(w, results["cube"] * Q)
    s, w, _ = raw(P, V, F, row, want=(True, False))
    assert w is None and np.array_equal(s, results["cube"])
    # a NaN vertex, an infinite one and one of 2^64: their faces are skipped; the rest is summed as ever
    for bad in (np.nan, np.inf, 2.0 ** 64):
        Vn = V.copy()
        Vn[7, 1] = bad
        want, wstatus = WO.mesh_sums_mp(P, Vn, F)
        s, _, status = raw(P, Vn, F, row)
        assert status == wstatus == _native.DPC_STATUS_NONFINITE and 0 < WO.bound(Vn, F) < len(F)
        assert (np.abs(s - want) <= WO.bound(Vn, F)).all(), bad
    # a face index outside the row's vertices: skipped, never an address
    Fb = F.copy()
    Fb[3, 1], Fb[5, 0], Fb[8, 2] = len(V), -1, 2 ** 30
    want, wstatus = WO.mesh_sums_mp(P, V, Fb)
    s, _, status = raw(P, V, Fb, row)
    assert status == wstatus == _native.DPC_STATUS_BAD_INDEX and WO.bound(V, Fb) == len(F) - 3
    assert (np.abs(s - want) <= len(F) - 3).all()
    # points that are not finite: sum 0, w = NaN, the status bit; the others as ever
    Pn = P.copy()
    Pn[2, 0], Pn[9, 2], Pn[17, 1] = np.nan, -np.inf, 2.0 ** 64
    s, w, status = raw(Pn, V, F, row)
    hit = np.zeros(len(P), dtype=bool)
    hit[[2, 9, 17]] = True
    assert status == _native.DPC_STATUS_NONFINITE and (s[hit] == 0).all() and np.isnan(w[hit]).all()
    assert np.array_equal(s[~hit], results["cube"][~hit]) and np.array_equal(w[~hit], s[~hit] * Q)
    # a device-table row outside its arrays: the status bit, and nothing of that row is read or written
    two = [[0, 20, 0, len(V), 0, len(F)], [20, 20, 0, len(V), 0, len(F)]]
    for broken in ([20, 20, 0, len(V) + 1, 0, len(F)], [20, 20, 0, len(V), 1, len(F)], [20, 2 ** 30, 0, len(V), 0, len(F)], [-1, 20, 0, len(V), 0, len(F)]):
        s, w, status = raw(P, V, F, two, dev_rows=[two[0], broken])
        assert status == _native.DPC_STATUS_BAD_INDEX, broken
        assert np.array_equal(s[:20], results["cube"][:20]) and (s[20:] == -77).all() and (w[20:] == -77.0).all(), broken
    # exactly on a vertex, exactly in a face's plane: the rule's zero terms, the same bits as the oracle
    for name in f32["exact"]:
        assert np.array_equal(results[str(name)], f32[name + "_sums"]), name
        assert np.array_equal(results[str(name)], WO.mesh_sums(*case(f32, name))[0]), name
    R.check_status()


def test_points_inside_and_signed_distance(f32, results):
    for name in f32["clear"]:
        P, V, F = case(f32, name)
        for thr in (0.5, 0.25, -0.5):
            got, = R.points_inside_meshes([P], [(V, F)], threshold=thr)
            assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), f32[name + "_sums"] > WO.threshold_q(thr)), (name, thr)
        # the clearance keeps the sums far from the threshold: far more than the bound
        assert np.abs(f32[name + "_sums"] - WO.threshold_q(0.5)).min() > 1000 * int(f32[name + "_bound"]), name
    P, V, F = case(f32, "cube")
    inside = torch.from_numpy(np.abs(f32["cube_sums"] - ONE) <= 12).cuda()
    for squared in (False, True):
        mag, = R.point_mesh_distance([P], [(V, F)], squared=squared)
        got, = R.signed_point_mesh_distance([P], [(V, F)], squared=squared)
        assert got.dtype == torch.float64 and torch.equal(got.abs(), mag) and (mag > 0).all()             # the magnitude, bit for bit
        assert torch.equal(got < 0, inside) and 5 <= int(inside.sum()) <= len(P) - 5
    # several clouds in one call, a shared mesh, the inward cube: nothing is inside it at 0.5, what was outside at -0.5
    Pt, Vt, Ft = case(f32, "tetra")
    three = [(V, F), (Vt, Ft), (V, F[:, ::-1].copy())]
    got = R.signed_point_mesh_distance([P, Pt, P], three, [0, 1, 2])
    mags = R.point_mesh_distance([P, Pt, P], three, [0, 1, 2])
    assert all(torch.equal(g.abs(), m) for g, m in zip(got, mags)) and torch.equal(got[0] < 0, inside) and not (got[2] < 0).any()
    assert torch.equal(got[1] < 0, torch.from_numpy(np.abs(f32["tetra_sums"] - ONE) <= 4).cuda())
    flipped, = R.signed_point_mesh_distance([P], [(V, F[:, ::-1].copy())], threshold=-0.5)                     # -1 inside, 0 outside
    assert torch.equal(flipped < 0, ~inside)
    # +inf (no usable face) passes through, whatever the threshold says
    Vn = np.full_like(V, np.nan)
    R.check_status()
    got, = R.signed_point_mesh_distance([P[:3]], [(Vn, F)], threshold=-0.5)
    assert torch.isinf(got).all() and (got > 0).all() and R.check_status() == _native.DPC_STATUS_NONFINITE
    assert [len(x) for x in R.points_inside_meshes([P[:0], P[:2]], [(V, F)], [0, 0])] == [0, 2]
    assert R.winding_numbers([], []) == [] and R.signed_point_mesh_distance([P[:0]], [(V, F)])[0].shape == (0,)


def test_winding_voxels(ball):
    cases = WO.voxel_cases()
    (Vc, Fc), (Vo, Fo) = cases["cube"], cases["open_box"]
    empty = (Vc, Fc[:0])
    R.check_status()
    for vox, vz in ((8, -1), (8, 16)):
        shape = (vox if vz == -1 else vz, vox, vox)
        for thr in (0.5, 0.25):
            got = R.winding_voxels([(Vc, Fc), (Vo, Fo), empty, (Vc.astype(np.float64), Fc)], vox, vox_size_z=vz, threshold=thr, surface=False)
            assert got.dtype == torch.bool and tuple(got.shape) == (4,) + shape and got.is_cuda
            g = got.cpu().numpy()
            assert np.array_equal(g[0], WO.winding_grid(Vc, Fc, shape, thr)), (shape, thr)
            assert np.array_equal(g[1], WO.winding_grid(Vo, Fo, shape, thr)), (shape, thr)
            assert not g[2].any() and np.array_equal(g[3], g[0]) and g[0].any() and g[1].any()
        assert not np.array_equal(WO.winding_grid(Vo, Fo, shape, 0.25), WO.winding_grid(Vo, Fo, shape, 0.5))
        solid = R.winding_voxels([(Vc, Fc), (Vo, Fo), empty], vox, vox_size_z=vz)                            # surface=True
        shell = R.voxelise_meshes([(Vc, Fc), (Vo, Fo), empty], vox, vox_size_z=vz, fill="none")
        inner = R.winding_voxels([(Vc, Fc), (Vo, Fo), empty], vox, vox_size_z=vz, surface=False)
        assert torch.equal(solid, shell | inner) and bool((solid & ~shell).any()) and not solid[2].any()
        parity = R.voxelise_meshes([(Vc, Fc)], vox, vox_size_z=vz, fill="parity")
        assert torch.equal(solid[:1], parity)                                                                # exact for a closed mesh
        assert not R.winding_voxels([empty], vox, vox_size_z=vz, threshold=-1.0).any()
        stats = R.voxel_stats(parity.float(), solid[:1])                                                     # a ground truth as it is
        assert int(stats[0, 0]) == 0 and int(stats[0, 1]) == int(stats[0, 2]) == int(solid[0].sum()) and float(R.voxel_iou(parity.float(), solid[:1])[0]) == 1.0
    assert R.winding_voxels([], 8).shape == (0, 8, 8, 8)
    assert R.check_status() == 0
    # a mesh of more than two chunks of faces on a grid of two node blocks: the face range is split (k_wn_vox's chunks)
    V, F, _, _, _, _ = ball
    Vu = V / 23.0 - 0.5
    shape = (8, 8, 8)
    tab = np.ascontiguousarray([[0, len(Vu), 0, len(F)]], dtype=np.int32)
    assert _native.lib().dpc_mesh_winding_voxels_workspace_bytes(tab.ctypes.data_as(ctypes.c_void_p), 1, 8, 8, 8) >= 3 * 512 * 8
    sums, _ = WO.voxel_sums(Vu, F, shape)
    assert np.abs(sums - WO.threshold_q(0.5)).min() > 10 ** 6 * len(F)        # no node is near the threshold: the grid is beyond doubt
    got = R.winding_voxels([(Vu, F)], 8, surface=False)[0].cpu().numpy()
    assert np.array_equal(got, (sums > WO.threshold_q(0.5)).reshape(shape)) and 20 < got.sum() < 400
