"""dpc_ray_mesh_intersect on the GPU against tests/raycast_oracle.py.

The kernels are built with -ffp-contract=off and perform the oracle's IEEE operations one by one, so every comparison
with the oracle here is bit equality on t, face, weights, hits and normal (NaNs included) -- on the fixture's rays, which
all keep the clearance under which the oracle's decisions are the exact ones (tests/test_raycast_host.py), and on any
other ray.  Two checks are not bit equality, both stated where they are made: the parity of hits against
points_inside_meshes, and the distance of a hit point from its mesh, bounded by 8 * 2^-52 * (|O| + t |D|).

Measured on an MI355X (the tests print them): see DESIGN.md section 4, "Ray-mesh intersection"."""
import ctypes

import numpy as np
import pytest
import torch

import dpc.render as R
import point_mesh_oracle as PM
import raycast_oracle as RO
import winding_oracle as WO
from dpc.render import _native

pytestmark = pytest.mark.gpu

BLOCK, TILE = _native.DPC_PM_BLOCK, _native.DPC_PM_FACE_TILE
CHUNK = TILE * _native.DPC_PM_CHUNK_TILES
FIELDS = ("t", "face", "weights", "hits", "normal")
INF = float("inf")


@pytest.fixture(scope="module")
def f33(golden):
    return golden("f33_raycast.npz")


def case(f33, name):
    return f33[name + "_O"], f33[name + "_D"], f33[name + "_V"], f33[name + "_F"], tuple(f33[name + "_range"])


def host(rec):
    return {k: getattr(rec, k).cpu().numpy() for k in rec._fields}


def same(got, want, what):
    """A record (or a dict of numpy arrays) against a dict of the oracle's arrays: dtype, shape and every bit."""
    got = host(got) if hasattr(got, "_fields") else got
    for k in FIELDS:
        if k in got:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
            assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])


def cast(O, D, V, rd, vd):
    return O.astype(rd), D.astype(rd), V.astype(vd)


def soup(rng, n_faces, n_verts=60):
    V = rng.uniform(-0.5, 0.5, size=(n_verts, 3))
    return V, rng.integers(0, n_verts, size=(n_faces, 3)).astype(np.int32)


def rays(rng, n, dtype=np.float64):
    O = rng.uniform(-1.0, 1.0, size=(n, 3))
    return O.astype(dtype), ((rng.uniform(-0.5, 0.5, size=(n, 3)) - O) * rng.uniform(0.5, 2.0, size=(n, 1))).astype(dtype)


def ws_bytes(rows):
    tab = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 6)
    return _native.lib().dpc_ray_mesh_workspace_bytes(tab.ctypes.data_as(ctypes.c_void_p), len(tab))


def ws_size(pairs, slots):
    r16 = lambda n: (n + 15) // 16 * 16
    return 3 * r16(4 * (pairs + 1)) + r16(8 * slots) + 2 * r16(4 * slots) + 16


def test_fixture_cases_in_all_four_instantiations(f33):
    """Every case as stored against the stored outputs, and cast to each of the four (ray, vertex) dtype pairs against
    the oracle on the cast inputs; the launch record shows the four instantiations ran."""
    R.check_status()
    for name in list(f33["generic"]) + list(f33["dyadic"]):
        O, D, V, F, rng = case(f33, name)
        rec, = R.ray_mesh_intersect([O], [D], [(V, F)], t_min=rng[0], t_max=rng[1], normals=True)
        assert all(x.is_cuda for x in rec) and rec.face.dtype == rec.hits.dtype == torch.int32 and rec.t.dtype == torch.float64
        same(rec, {k: f33["%s_%s" % (name, k)] for k in FIELDS}, name)
        for rd in (np.float32, np.float64):
            for vd in (np.float32, np.float64):
                Oc, Dc, Vc = cast(O, D, V, rd, vd)
                got, = R.ray_mesh_intersect([Oc], [Dc], [(Vc, F)], t_min=rng[0], t_max=rng[1], normals=True)
                same(got, RO.ray_mesh(Oc, Dc, Vc, F, *rng), (name, rd, vd))
        plain, = R.ray_mesh_intersect([O], [D], [(V, F)], t_min=rng[0], t_max=rng[1])
        assert len(plain) == 4 and torch.equal(plain.face, rec.face) and torch.equal(plain.hits, rec.hits)
    assert R.check_status() == 0
    O, D, V, F, rng = case(f33, "cube64")
    ran = _native.launched_instantiations(
        lambda: [R.ray_mesh_intersect([o], [d], [(v, F)]) for o, d, v in (cast(O, D, V, rd, vd) for rd in (np.float32, np.float64)
                                                                          for vd in (np.float32, np.float64))], torch.device("cuda"))
    assert {"k_rc_%s<%d, %d>" % (k, r, v) for k in ("hit", "finish") for r in (0, 1) for v in (0, 1)} <= ran, ran


def test_edges_of_the_decomposition():
    """Ray counts around a block of rays against 130 faces (two tiles), and face counts around a tile and a chunk against
    five rays, which force the chunked path: the workspace size shows how many chunks were planned."""
    rng = np.random.default_rng(33)
    V, F = soup(rng, 130)
    for n in (1, 255, 256, 257):
        O, D = rays(rng, n)
        got, = R.ray_mesh_intersect([O], [D], [(V, F)], normals=True)
        same(got, RO.ray_mesh(O, D, V, F), n)
    assert BLOCK == 256 and TILE == 128 and CHUNK == 1024
    O, D = rays(rng, 5)
    for n in (1, 127, 128, 129, 1023, 1024, 1025, 2 * 1024 + 1):
        V, F = soup(rng, n, 200)
        chunks = (n + CHUNK - 1) // CHUNK
        assert ws_bytes([[0, 5, 0, len(V), 0, n]]) == ws_size(1, 5 * chunks) and (chunks > 1) == (n > 1024), n
        got, = R.ray_mesh_intersect([O], [D], [(V, F)], normals=True)
        want = RO.ray_mesh(O, D, V, F)
        same(got, want, n)
        assert n < 1023 or want["hits"].max() > 20                       # the rays do cross the soup
    assert R.check_status() == 0


def test_ties_go_to_the_lower_index(f33):
    """A face listed twice, once in the first chunk and once in the third, in front of a soup: the lower index is the one
    reported whichever chunk holds it, and both count.  On the dyadic fan the rays through shared vertices and edges
    give the oracle's hits and face."""
    rng = np.random.default_rng(34)
    V, F = soup(rng, 2 * CHUNK + 1, 200)
    V = np.concatenate([V, [[-0.4, -0.4, -2.0], [0.4, -0.4, -2.0], [0.0, 0.4, -2.0]]])
    front = [200, 201, 202]
    O = np.array([[0.0, 0.0, -5.0], [0.1, -0.1, -4.0], [-0.1, -0.2, -6.0], [0.05, 0.1, -3.0]])
    D = np.array([[0.01, 0.02, 1.0], [0.0, 0.0, 0.5], [0.02, 0.01, 2.0], [-0.01, 0.0, 0.25]])
    assert ws_bytes([[0, 4, 0, len(V), 0, len(F)]]) == ws_size(1, 4 * 3)
    for a, b in ((5, 2 * CHUNK - 3), (2 * CHUNK - 3, 5), (CHUNK - 1, CHUNK), (CHUNK + 7, CHUNK + 8)):
        Fd = F.copy()
        Fd[a], Fd[b] = front, front
        got, = R.ray_mesh_intersect([O], [D], [(V, Fd)], normals=True)
        want = RO.ray_mesh(O, D, V, Fd)
        same(got, want, (a, b))
        assert (want["face"] == min(a, b)).all() and (want["hits"] >= 2).all(), (a, b)
        back, = R.ray_mesh_intersect([O], [D], [(V, Fd)], cull_backfaces=True)
        same(back, RO.ray_mesh(O, D, V, Fd, cull_backfaces=True), (a, b, "cull"))
    for name in f33["dyadic"]:
        O, D, V, F, rng_ = case(f33, name)
        got, = R.ray_mesh_intersect([O], [D], [(V, F)], t_min=rng_[0], t_max=rng_[1])
        g = host(got)
        assert np.array_equal(g["hits"], f33[name + "_hits"]) and np.array_equal(g["face"], f33[name + "_face"]), name
        assert g["hits"].max() == 8 and (g["hits"] == 2).sum() >= 8                  # the shared vertex, the shared edges


def test_range_ends_are_inclusive_and_backfaces_are_culled():
    V, F = RO.cube()
    O, D = np.array([[0.25, 0.5, -2.0]]), np.array([[0.0, 0.0, 0.5]])           # hits at t = 4 and t = 6 exactly
    for lo, hi, n, first in ((4.0, 6.0, 2, 4.0), (4.0, 5.0, 1, 4.0), (5.0, 6.0, 1, 6.0), (6.0, 6.0, 1, 6.0), (4.0, 4.0, 1, 4.0),
                             (np.nextafter(4.0, 5.0), np.nextafter(6.0, 5.0), 0, INF), (-INF, INF, 2, 4.0)):
        got, = R.ray_mesh_intersect([O], [D], [(V, F)], t_min=lo, t_max=hi, normals=True)
        same(got, RO.ray_mesh(O, D, V, F, lo, hi), (lo, hi))
        assert got.hits.tolist() == [n] and got.t.tolist() == [first], (lo, hi)
    # rays from outside towards the cube: with culling the near side stays and the far one goes
    rng = np.random.default_rng(35)
    O = rng.uniform(-1.0, 2.0, size=(64, 3))
    O[:, 0] = np.where(rng.random(64) < 0.5, -1.5, 2.5)
    D = rng.uniform(0.2, 0.8, size=(64, 3)) - O
    full, = R.ray_mesh_intersect([O], [D], [(V, F)])
    cull, = R.ray_mesh_intersect([O], [D], [(V, F)], cull_backfaces=True, normals=True)
    same(cull, RO.ray_mesh(O, D, V, F, cull_backfaces=True), "cull")
    assert (full.hits == 2).all() and (cull.hits == 1).all() and torch.equal(cull.t, full.t) and torch.equal(cull.face, full.face)
    assert bool(((cull.normal * torch.from_numpy(D).cuda()).sum(dim=1) < 0).all())


def test_order_batching_and_chunking_do_not_change_a_bit(f33):
    rng = np.random.default_rng(36)
    V, F = soup(rng, 130)
    O, D = rays(rng, 2048)
    alone, = R.ray_mesh_intersect([O], [D], [(V, F)], normals=True)
    same(alone, RO.ray_mesh(O, D, V, F), "2048 rays")
    rows = R.ray_mesh_intersect([o[None] for o in O], [d[None] for d in D], [(V, F)], mesh_of=[0] * len(O), normals=True)
    assert len(rows) == 2048
    for k in FIELDS:                                                    # one-ray rows: a block of rays each
        assert torch.equal(torch.cat([getattr(r, k) for r in rows]).view(torch.uint8), getattr(alone, k).view(torch.uint8)), k
    # a ragged batch over shared meshes, mixed dtypes and an empty bundle; permuted rows, meshes and mesh_of
    names = ["soup64", "cube32", "open64", "soup32", "cube64"]
    geo = [case(f33, n) for n in names]
    meshes = [(geo[0][2], geo[0][3]), (geo[4][2], geo[4][3]), (geo[2][2], geo[2][3])]          # soup64, cube64, open64
    Os = [geo[0][0], geo[1][0], geo[2][0], np.zeros((0, 3)), geo[3][0], geo[4][0]]
    Ds = [geo[0][1], geo[1][1], geo[2][1], np.zeros((0, 3)), geo[3][1], geo[4][1]]
    mesh_of = [0, 1, 2, 1, 0, 1]
    base = R.ray_mesh_intersect(Os, Ds, meshes, mesh_of, normals=True)
    assert [len(b.t) for b in base] == [len(o) for o in Os] and base[3].weights.shape == (0, 3)
    for i, k in enumerate(mesh_of):
        one, = R.ray_mesh_intersect([Os[i]], [Ds[i]], [meshes[k]], normals=True)
        same(one, host(base[i]), i)
        same(base[i], RO.ray_mesh(Os[i], Ds[i], *meshes[k]), i)
    same(base[0], {k: f33["soup64_" + k] for k in FIELDS}, "soup64 in a batch")
    perm = [4, 2, 0, 5, 3, 1]
    other = R.ray_mesh_intersect([Os[i] for i in perm], [Ds[i] for i in perm], meshes[::-1], [2 - mesh_of[i] for i in perm], normals=True)
    for j, i in enumerate(perm):
        same(other[j], host(base[i]), ("permuted", i))
    # the faces listed in reverse: the same t and hits, and face maps through the reversal
    O, D, V, F, _ = case(f33, "soup64")
    rev, = R.ray_mesh_intersect([O], [D], [(V, F[::-1].copy())])
    fwd = host(base[0])
    assert np.array_equal(rev.t.cpu().numpy(), fwd["t"]) and np.array_equal(rev.hits.cpu().numpy(), fwd["hits"])
    assert np.array_equal(rev.face.cpu().numpy(), np.where(fwd["face"] >= 0, len(F) - 1 - fwd["face"], -1))
    assert R.check_status() == 0


def raw(O, D, V, F, rows, dev_rows=None, want=(True, True), t_range=(0.0, INF), cull=0):
    """dpc_ray_mesh_intersect itself (the Python functions refuse what some guards are for): a dict of numpy arrays, the
    outputs pre-filled with a sentinel, and the status word."""
    dev = torch.device("cuda")
    org, dirs, verts = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (O, D, V))
    faces = torch.from_numpy(np.ascontiguousarray(F, dtype=np.int32)).to(dev)
    tab = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 6)
    desc = torch.from_numpy(tab if dev_rows is None else np.ascontiguousarray(dev_rows, dtype=np.int32).reshape(-1, 6)).to(dev)
    n = int(tab[:, 1].sum())
    t = torch.full((n,), -77.0, dtype=torch.float64, device=dev)
    face = torch.full((n,), -77, dtype=torch.int32, device=dev)
    weights = torch.full((n, 3), -77.0, dtype=torch.float64, device=dev)
    hits = torch.full((n,), -77, dtype=torch.int32, device=dev) if want[0] else None
    normal = torch.full((n, 3), -77.0, dtype=torch.float64, device=dev) if want[1] else None
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(16, ws_bytes(tab)),), dtype=torch.uint8, device=dev)
    _native.call(dev, "dpc_ray_mesh_intersect", _native.ptr(org), _native.ptr(dirs), len(O), int(org.dtype == torch.float64),
                 _native.ptr(verts), len(V), int(verts.dtype == torch.float64), _native.ptr(faces), len(F), _native.ptr(desc),
                 tab.ctypes.data, len(tab), t_range[0], t_range[1], cull, _native.ptr(t), _native.ptr(face), _native.ptr(weights),
                 _native.ptr(hits), _native.ptr(normal), _native.ptr(ws), _native.ptr(status))
    torch.cuda.synchronize()
    out = dict(t=t, face=face, weights=weights, hits=hits, normal=normal)
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}, int(status.item())


def test_guards(f33):
    O, D, V, F, _ = case(f33, "cube64")
    n = len(O)
    row = [[0, n, 0, len(V), 0, len(F)]]
    base = {k: f33["cube64_" + k] for k in FIELDS}
    got, status = raw(O, D, V, F, row)
    same(got, base, "raw")
    assert status == 0
    got, status = raw(O, D, V, F, row, want=(False, False))
    assert sorted(got) == ["face", "t", "weights"] and status == 0
    same(got, base, "without hits and normal")
    # a NaN vertex, an infinite one and one of 2^64: their faces are skipped, the others answer as ever
    for bad in (np.nan, np.inf, 2.0 ** 64):
        Vn = V.copy()
        Vn[7, 1] = bad
        want = RO.ray_mesh(O, D, Vn, F)
        got, status = raw(O, D, Vn, F, row)
        same(got, want, bad)
        assert status == want["status"] == _native.DPC_STATUS_NONFINITE and 0 < (want["hits"] < base["hits"]).sum() < n
    # a face index outside the row's vertices: skipped, never an address
    Fb = F.copy()
    Fb[3, 1], Fb[5, 0], Fb[8, 2] = len(V), -1, 2 ** 30
    want = RO.ray_mesh(O, D, V, Fb)
    got, status = raw(O, D, V, Fb, row)
    same(got, want, "bad index")
    assert status == want["status"] == _native.DPC_STATUS_BAD_INDEX and (want["hits"] > 0).any()
    # rays that are not finite: t = NaN, face = -1, hits = 0, NaN weights, zero normal; the others as ever
    On, Dn = O.copy(), D.copy()
    On[2, 0], Dn[9, 2], On[17, 1], Dn[20, 0] = np.nan, -np.inf, 2.0 ** 64, np.nan
    want = RO.ray_mesh(On, Dn, V, F)
    got, status = raw(On, Dn, V, F, row)
    same(got, want, "rays that are not finite")
    bad = np.zeros(n, dtype=bool)
    bad[[2, 9, 17, 20]] = True
    assert status == _native.DPC_STATUS_NONFINITE and np.isnan(got["t"][bad]).all() and (got["face"][bad] == -1).all()
    assert (got["hits"][bad] == 0).all() and np.isnan(got["weights"][bad]).all() and (got["normal"][bad] == 0).all()
    assert np.array_equal(got["t"][~bad], base["t"][~bad])
    rec, = R.ray_mesh_intersect([On], [Dn], [(V, F)], normals=True)               # the Python function passes them through
    same(rec, want, "rays that are not finite, from Python")
    assert R.check_status() == _native.DPC_STATUS_NONFINITE
    # a device-table row outside its arrays: the status bit, and nothing of that row is read or written
    h = n // 2
    two = [[0, h, 0, len(V), 0, len(F)], [h, n - h, 0, len(V), 0, len(F)]]
    for broken in ([h, n - h, 0, len(V) + 1, 0, len(F)], [h, n - h, 0, len(V), 1, len(F)], [h, 2 ** 30, 0, len(V), 0, len(F)],
                   [-1, n - h, 0, len(V), 0, len(F)]):
        got, status = raw(O, D, V, F, two, dev_rows=[two[0], broken])
        assert status == _native.DPC_STATUS_BAD_INDEX, broken
        for k in FIELDS:
            assert np.array_equal(got[k][:h], base[k][:h]) and (got[k][h:] == -77).all(), (broken, k)
    # a row with rays and no faces: all miss, and a ray that is not finite is still reported
    for Fz, nf in ((F[:0], 0), (F, 0)):
        got, status = raw(O, D, V, Fz, [[0, n, 0, len(V), 0, nf]])
        assert status == 0 and (got["t"] == INF).all() and (got["face"] == -1).all() and (got["hits"] == 0).all()
        assert np.isnan(got["weights"]).all() and (got["normal"] == 0).all()
    got, status = raw(On, Dn, V, F, [[0, n, 0, len(V), 0, 0]])
    assert status == _native.DPC_STATUS_NONFINITE and np.isnan(got["t"][bad]).all() and (got["t"][~bad] == INF).all()
    rec, miss = R.ray_mesh_intersect([O, O[:3]], [D, D[:3]], [(V, F), (V, F[:0])], normals=True)
    same(rec, base, "beside a mesh without faces")
    assert (miss.t == INF).all() and (miss.face == -1).all() and (miss.hits == 0).all() and bool(torch.isnan(miss.weights).all())
    # empty bundles, and nothing at all
    e, = R.ray_mesh_intersect([O[:0]], [D[:0]], [(V, F)], normals=True)
    assert e.t.shape == (0,) and e.weights.shape == (0, 3) and e.normal.shape == (0, 3) and e.hits.dtype == torch.int32
    assert R.ray_mesh_intersect([], [], []) == [] and R.visible_points([], [], [0.0, 0.0, 1.0], 1e-6) == []
    assert R.check_status() == 0


def extent(V):
    return float((V.max(axis=0) - V.min(axis=0)).max())


def edge_clear(O, D, V, F, margin=2.0 ** -20):
    """[n] bool, by the geometry alone (host arithmetic, nothing the device computed): for every face the line of the ray
    is not parallel to, each of u, v and 1 - u - v keeps the margin from 0 -- the ray passes no edge and no vertex."""
    v = V.astype(np.float64)
    ok = np.ones(len(O), dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        for k in range(0, len(F), 512):
            f = F[k:k + 512]
            det, a, b, _ = RO._terms(O[:, None, :], D[:, None, :], v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None])
            u, w = a / det, b / det
            near = np.minimum(np.minimum(np.abs(u), np.abs(w)), np.abs(1.0 - u - w)) < margin
            ok &= ~((det != 0) & near).any(axis=1)
    return ok


@pytest.fixture(scope="module")
def ball():
    """test_winding_gpu's mesh: extract_surfaces of a Gaussian ball on a 24^3 grid, closed and wound outward."""
    G, c, r, sigma = 24, np.array([11.6, 11.4, 11.7]), 9.2, 5.0
    n = np.stack(np.meshgrid(*[np.arange(G, dtype=np.float64)] * 3, indexing="ij"), axis=-1)
    field = np.exp(-((n - c) ** 2).sum(-1) / (2 * sigma * sigma))
    (V, F), = R.extract_surfaces(torch.from_numpy(field).cuda()[None], float(np.exp(-r * r / (2 * sigma * sigma))))
    return V.cpu().numpy(), F.cpu().numpy().astype(np.int32)


def test_agreement_with_the_point_queries(ball):
    """On the cube and on the ball: for query points that keep the winding tests' clearance from the surface and a
    direction that keeps clear of every edge, hits is odd exactly where points_inside_meshes says inside; and every hit
    point O + t D lies within 8 * 2^-52 * (|O| + t |D|) of its mesh by point_mesh_distance -- a rounding bound: the hit
    point is formed by one multiplication and one addition per axis from a t right to a few ulps."""
    rng = np.random.default_rng(37)
    direction = np.array([0.5317, 0.3081, 0.7883])
    for name, (V, F) in (("cube", RO.cube()), ("ball", ball)):
        lo, e = V.min(axis=0), extent(V)
        pts = []
        while len(pts) < 200:                                            # by the geometry alone, before anything is run
            p = lo + rng.uniform(-0.15, 1.15, size=(64, 3)) * e
            d = np.broadcast_to(direction * e, p.shape)
            keep = (np.sqrt(PM.mesh_d2(p, V, F)[0]) >= WO.CLEARANCE * e) & edge_clear(p, d, V, F)
            pts.extend(p[keep])
        O = np.asarray(pts[:200])
        D = np.broadcast_to(direction * e, O.shape).copy()
        rec, = R.ray_mesh_intersect([O], [D], [(V, F)])
        inside, = R.points_inside_meshes([O], [(V, F)])
        odd = (rec.hits % 2 == 1)
        assert torch.equal(odd, inside) and 20 <= int(inside.sum()) <= 180, name
        hit = (rec.face >= 0).cpu().numpy()
        P, = R.rays_hit_points([O], [D], [rec])
        assert P.dtype == torch.float64 and bool(torch.isnan(P[torch.from_numpy(~hit).cuda()]).all())
        assert P.cpu().numpy().tobytes() == RO.hit_points(O, D, rec.t.cpu().numpy()).tobytes()
        dist, = R.point_mesh_distance([P[torch.from_numpy(hit).cuda()]], [(V, F)])
        t = rec.t.cpu().numpy()[hit]
        bound = 8 * 2.0 ** -52 * (np.linalg.norm(O[hit], axis=1) + t * np.linalg.norm(D[hit], axis=1))
        ratio = float((dist.cpu().numpy() / bound).max())
        print("%s: %d of 200 rays hit, %d origins inside; hit point to mesh distance at most %.3f of the bound" % (name, hit.sum(), int(inside.sum()), ratio))
        assert hit.sum() >= 50 and ratio <= 1.0, (name, ratio)
    assert R.check_status() == 0


def test_visible_points_on_the_cube():
    """From a viewpoint off the corner (1, 1, 1) the samples on the three sides turned to it are visible and those on the
    other three are not; in the box without its lid the floor is seen through the opening, and under the lid it is not."""
    V, F = RO.cube()
    g = np.array([0.15, 0.35, 0.6, 0.8])
    a, b = (x.reshape(-1) for x in np.meshgrid(g, g[::-1] + 0.03))
    side = lambda axis, at: np.insert(np.stack([a, b], axis=1), axis, at, axis=1)
    clouds = [side(ax, at) for at in (1.0, 0.0) for ax in (0, 1, 2)]                # three turned to the viewpoint, three away
    view = [3.0, 2.5, 3.5]
    vis = R.visible_points(clouds, [(V, F)], view, 1e-9, mesh_of=[0] * 6)
    assert [v.dtype for v in vis] == [torch.bool] * 6 and [int(v.sum()) for v in vis] == [16, 16, 16, 0, 0, 0]
    f32 = R.visible_points([c.astype(np.float32) for c in clouds], [(V, F)], [view] * 6, 1e-6, mesh_of=[0] * 6)
    assert [int(v.sum()) for v in f32] == [16, 16, 16, 0, 0, 0]
    # the definition: no hit of the ray C -> P with t in [0, 1 - eps]
    C = np.broadcast_to(np.asarray(view), clouds[0].shape)
    for i in (0, 4):
        want = RO.ray_mesh(C, clouds[i] - C, V, F, 0.0, 1.0 - 1e-9)["hits"] == 0
        assert np.array_equal(vis[i].cpu().numpy(), want), i
    assert bool(R.visible_points([np.asarray([view, [0.5, 0.5, 0.5]])], [(V, F)], view, 1e-6)[0][0])   # P == C is visible
    floor = side(2, 0.0)[(np.abs(side(2, 0.0)[:, :2] - 0.5) < 0.2).all(axis=1)]
    above = [0.5, 0.45, 4.0]
    assert len(floor) >= 4
    closed, opened = R.visible_points([floor, floor], [(V, F), RO.cube(lid=False)], above, 1e-9)
    assert not bool(closed.any()) and bool(opened.all())
    nan = floor.copy()
    nan[0, 1] = np.nan
    seen, = R.visible_points([nan], [RO.cube(lid=False)], above, 1e-9)
    assert not bool(seen[0]) and bool(seen[1:].all()) and R.check_status() == _native.DPC_STATUS_NONFINITE
