"""dpc_point_mesh_closest on the GPU: the nearest face, the closest point, its weights, the face normal, the surface loss
and the mesh-based normal consistency, against the exact values of the fixture f31_closest.npz.

Tolerances.  A closest point may differ from the fixture's Q (the exact Q, rounded once to fp64) by 8 * ratio units of
2^-52 S (S the largest absolute coordinate of the row, closest_oracle.unit_len) and no more: ratio is the worst error of
the numpy oracle against that same stored Q, recorded by tests/golden/make_golden_closest.py -- max_ratio_q over the
well-shaped cases, sliver's own sliver_ratio_q on the sliver; likewise max_ratio_wv for sum w V rebuilt in exact
arithmetic from the returned weights (well-shaped cases only).  The factor 8 allows the kernel another formulation and
fused multiply-adds, the convention of test_point_mesh_gpu.py.  Nothing is added to it and nothing is derived from the
kernel's own output.  d2 is compared with point_mesh_distance bit for bit.  Normals: 4 ulp (of 1) per component against
closest_oracle.face_normals, the same plain fp64 formula; unit length to 4 ulp.

Measured on an MI355X (the tests print them): see DESIGN.md section 4, "Closest points on meshes"."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import closest_oracle as C
import dpc.render as R
from dpc.render import _native

pytestmark = pytest.mark.gpu

BLOCK, TILE = _native.DPC_PM_BLOCK, _native.DPC_PM_FACE_TILE
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def f31(golden):
    return golden("f31_closest.npz")


@pytest.fixture(scope="module")
def f28(golden):
    return golden("f28_point_mesh.npz")


def geometry(f28, f31, name):
    src = f31 if name + "_P" in f31 else f28
    return src[name + "_P"], src[name + "_V"], src[name + "_F"]


@pytest.fixture(scope="module")
def results(f28, f31):
    """Every case once, one row each, with normals: {name: (record as numpy, status word)}; and the distances of
    point_mesh_distance for the same rows."""
    out = {}
    for name in f31["cases"]:
        P, V, F = geometry(f28, f31, name)
        R.check_status()
        rec, = R.closest_points_on_meshes([P], [(V, F)], normals=True)
        assert all(t.is_cuda for t in rec) and rec.face.dtype == torch.int32 and all(t.dtype == torch.float64 for t in (rec.d2, rec.point, rec.weights, rec.normal))
        status = R.check_status()
        d2, = R.point_mesh_distance([P], [(V, F)], squared=True)
        R.check_status()
        out[str(name)] = (type(rec)(*(t.cpu().numpy() for t in rec)), status, d2.cpu().numpy())
    return out


def dtypes(P, V):
    for pd in (np.float32, np.float64):
        for vd in (np.float32, np.float64):
            yield P.astype(pd), V.astype(vd)


def test_d2_is_point_mesh_distance_bit_for_bit(f28, f31, results):
    """d2 equals point_mesh_distance(..., squared=True) bit for bit: every case, and every case again in all four dtype
    instantiations (inputs cast to fp32 / fp64), which the launch record shows were the kernels that ran."""
    for name in f31["cases"]:
        rec, _, d2 = results[str(name)]
        assert rec.d2.tobytes() == d2.tobytes(), name
        P, V, F = geometry(f28, f31, name)
        for Pd, Vd in dtypes(P, V):
            with np.errstate(invalid="ignore", over="ignore"):
                ok = np.isfinite(Pd).all()
            if not ok:
                continue
            got, = R.closest_points_on_meshes([Pd], [(Vd, F)])
            want, = R.point_mesh_distance([Pd], [(Vd, F)], squared=True)
            assert torch.equal(got.d2, want), (name, Pd.dtype, Vd.dtype)
            assert len(got) == 4
    R.check_status()
    P, V, F = geometry(f28, f31, "regions")
    ran = _native.launched_instantiations(lambda: [R.closest_points_on_meshes([Pd], [(Vd, F)]) for Pd, Vd in dtypes(P, V)],
                                          torch.device("cuda"))
    assert {"k_pc_%s<%d, %d>" % (k, p, v) for k in ("arg", "finish") for p in (0, 1) for v in (0, 1)} <= ran, ran


def test_face_is_an_exact_near_minimiser(f31, results):
    """The returned face is one of the exact near-minimisers; the exact argmin where it is beyond doubt (unique, split);
    the lowest index where one triangle is listed three times (duplicates)."""
    for name in f31["cases"]:
        rec, _, _ = results[str(name)]
        near = f31[name + "_near"]
        fin = np.isfinite(f31[name + "_d2"])
        assert (rec.face[~fin] == -1).all(), name
        assert all(rec.face[i] >= 0 and rec.face[i] in near[i] for i in np.nonzero(fin)[0]), (name, rec.face, near)
    assert (results["unique"][0].face == f31["unique_argmin"][:, 0]).all()
    assert (results["duplicates"][0].face == int(f31["dup_j"])).all()
    assert results["split"][0].face.tolist() == f31["split_argmin"][:, 0].tolist()


def test_closest_point_and_weights(f28, f31, results):
    """Q against the fixture's Q; weights >= 0 and summing to 1 within 2^-51; sum w V, evaluated exactly from the returned
    weights, against Q (well-shaped cases; on the sliver only Q, the signs and the sum)."""
    worst = {}
    for name in f31["cases"]:
        rec, _, _ = results[str(name)]
        P, V, F = geometry(f28, f31, name)
        unit, v64 = C.unit_len(P, V), np.asarray(V).astype(np.float64)
        fin = np.isfinite(f31[name + "_d2"])
        assert np.isnan(rec.point[~fin]).all() and np.isnan(rec.weights[~fin]).all(), name
        sliver = name == "sliver"
        allow_q = 8.0 * float(f31["sliver_ratio_q" if sliver else "max_ratio_q"])
        allow_wv = 8.0 * float(f31["max_ratio_wv"])
        eq = ewv = esum = 0.0
        for i in np.nonzero(fin)[0]:
            exact = [Fraction(float(x)) for x in f31[name + "_q"][i]]
            eq = max(eq, C.point_error(rec.point[i], exact) / unit)
            assert (rec.weights[i] >= 0).all(), (name, i, rec.weights[i])
            esum = max(esum, float(abs(sum(Fraction(float(x)) for x in rec.weights[i]) - 1)))
            if (rec.weights[i] == 1.0).any():                                    # a vertex: Q is the vertex itself
                assert (rec.point[i] == v64[F[rec.face[i]][int(np.argmax(rec.weights[i]))]]).all(), (name, i)
            if not sliver:
                ewv = max(ewv, C.point_error(C.combine_exact(rec.weights[i], v64[F[rec.face[i]]]), exact) / unit)
        print("%-20s Q %.3f units (allowed %.3f), sum w V %.3f units (allowed %.3f), |sum w - 1| %.3g"
              % (name, eq, allow_q, ewv, allow_wv, esum))
        worst[str(name)] = (eq, ewv)
        assert eq <= allow_q, (name, eq, allow_q)
        assert ewv <= allow_wv, (name, ewv, allow_wv)
        assert esum <= 2.0 ** -51, (name, esum)
    at_vertex = (results["regions"][0].weights == 1.0).any(axis=1)
    assert at_vertex.sum() == 6                                                  # three vertex regions, from both sides
    print("worst Q error: well-shaped %.3f units, sliver %.3f; worst sum w V error %.3f units"
          % (max(v[0] for k, v in worst.items() if k != "sliver"), worst["sliver"][0], max(v[1] for v in worst.values())))


def test_normals(f28, f31, results):
    """Unit length to 4 ulp; equal within 4 ulp to the normalised cross product of F[face] in the caller's order; zeros on
    zero-area winners and where there is no face; face_normals_at returns the same normals."""
    worst = 0.0
    for name in f31["cases"]:
        rec, _, _ = results[str(name)]
        P, V, F = geometry(f28, f31, name)
        want = C.face_normals(V, F)
        fin = rec.face >= 0
        assert (rec.normal[~fin] == 0).all(), name
        n, w = rec.normal[fin], want[rec.face[fin]]
        flat = (w == 0).all(axis=1)
        assert (n[flat] == 0).all(), name                                        # zero-area winners
        length = np.sqrt((n[~flat] ** 2).sum(axis=1))
        assert (np.abs(length - 1.0) <= 4 * ULP).all(), (name, length)
        err = float(np.abs(n - w).max()) / ULP if len(n) else 0.0
        worst = max(worst, err)
        assert err <= 4.0, (name, err)
        plain, = R.closest_points_on_meshes([P], [(V, F)])
        assert len(plain) == 4 and np.array_equal(plain.face.cpu().numpy(), rec.face)
    print("worst normal error %.3f ulp" % worst)
    assert (results["degenerate_only"][0].normal == 0).all() and (results["degenerate_nearest"][0].normal[:2] == 0).all()
    got, = R.face_normals_at([f28["ico_P"]], [(f28["ico_V"], f28["ico_F"])])
    assert np.array_equal(got.cpu().numpy(), results["ico"][0].normal)


def test_no_usable_face(f28, f31, results):
    """A mesh without a usable face: +inf, -1, NaN, NaN, zeros and the status bit; a NaN point is refused by name."""
    rec, status, _ = results["nan_only"]
    assert (rec.d2 == np.inf).all() and (rec.face == -1).all() and np.isnan(rec.point).all() and np.isnan(rec.weights).all()
    assert (rec.normal == 0).all() and status == _native.DPC_STATUS_NONFINITE
    assert results["nan_among"][1] == _native.DPC_STATUS_NONFINITE and results["regions"][1] == 0
    P, V, F = geometry(f28, f31, "regions")
    bad = P.copy()
    bad[3, 1] = np.nan
    R.check_status()                                                          # clears what earlier calls have set
    with pytest.raises(ValueError, match=r"clouds\[1\] holds a NaN or inf coordinate"):
        R.closest_points_on_meshes([P, bad], [(V, F)], mesh_of=[0, 0])
    assert R.closest_points_on_meshes([], []) == [] and R.check_status() == 0


def same(a, b):
    """Two records, bit for bit (NaNs included)."""
    return len(a) == len(b) and all(x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


def ragged(f28):
    """test_point_mesh_gpu's ragged batch: five rows over two meshes, one row without points, mixed dtypes."""
    tri, soup = (f28["regions_V"], f28["regions_F"]), (f28["tile_p1_V"], f28["tile_p1_F"])
    clouds = [f28["regions_P"], f28["regions_p32_P"], f28["tile_p1_P"], np.zeros((0, 3)), f28["cross_P"]]
    return clouds, [tri, soup], [0, 0, 1, 1, 0]


def test_order_and_batching_do_not_change_a_bit(f28, f31, results):
    """A ragged batch in one call against row-by-row calls; the rows permuted; and the split row (3 points, several
    chunks of faces) and the duplicates row alone and beside rows whose points fill the device, where they are not split."""
    clouds, meshes, mesh_of = ragged(f28)
    assert clouds[1].dtype == np.float32 and meshes[0][0].dtype == np.float64 and meshes[1][0].dtype == np.float32
    base = R.closest_points_on_meshes(clouds, meshes, mesh_of, normals=True)
    assert [len(b.d2) for b in base] == [len(c) for c in clouds] and base[3].point.shape == (0, 3)
    for i, k in enumerate(mesh_of):
        # alone, a row computes in its own dtypes: fp32 widens exactly, so the bits are the same
        alone, = R.closest_points_on_meshes([clouds[i]], [meshes[k]], normals=True)
        assert same(alone, base[i]), i
    for i, name in ((0, "regions"), (1, "regions_p32"), (2, "tile_p1"), (4, "cross")):
        assert all(np.array_equal(a.cpu().numpy(), b, equal_nan=True) for a, b in zip(base[i], results[name][0])), name
    perm = [4, 2, 0, 3, 1]
    other = R.closest_points_on_meshes([clouds[i] for i in perm], meshes[::-1], [1 - mesh_of[i] for i in perm], normals=True)
    for j, i in enumerate(perm):
        assert same(other[j], base[i]), i
    rng = np.random.default_rng(3)
    filler = (rng.random((8 * 256 * BLOCK, 3)) - 0.5).astype(np.float32)   # point blocks enough for one chunk per row
    tri = meshes[0]
    for name in ("split", "duplicates"):
        P, V, F = geometry(f28, f31, name)
        alone, = R.closest_points_on_meshes([P], [(V, F)], normals=True)
        both = R.closest_points_on_meshes([filler, P], [tri, (V, F)], normals=True)
        assert same(both[1], alone), name
        assert all(np.array_equal(a.cpu().numpy(), b, equal_nan=True) for a, b in zip(alone, results[name][0])), name
    assert same(both[0], R.closest_points_on_meshes([filler], [tri], normals=True)[0])
    assert torch.equal(both[0].d2, R.point_mesh_distance([filler], [tri], squared=True)[0])


def test_point_surface_loss(f28, f31, results):
    """The loss is np.mean of the distance's d2; backward gives 2 (P - Q) / n * g within Q's tolerance propagated, in the
    cloud's dtype; a shared mesh, an empty cloud and an array in one call; grouping changes no bit."""
    names = ["regions", "blocks", "mm", "ico", "unique"]
    geo = [geometry(f28, f31, n) for n in names]
    clouds = [torch.tensor(g[0], device="cuda", requires_grad=True) for g in geo]
    assert clouds[1].dtype == torch.float32 and clouds[0].dtype == torch.float64
    meshes = [(g[1], g[2]) for g in geo]
    loss = R.point_surface_loss(clouds, meshes)
    assert loss.shape == (5,) and loss.dtype == torch.float64 and loss.is_cuda
    for i, n in enumerate(names):                                   # the mean of check 1's d2, as np.mean takes it
        assert float(loss[i].detach()) == float(np.mean(results[n][2])), n
    g = torch.tensor([1.0, -2.0, 0.5, 3.0, 1.0], dtype=torch.float64, device="cuda")
    (loss * g).sum().backward()
    for i, n in enumerate(names):
        P, V, _ = geo[i]
        grad = clouds[i].grad
        assert grad.dtype == clouds[i].dtype and grad.shape == clouds[i].shape, n
        p64, q = np.asarray(P).astype(np.float64), f31[n + "_q"]
        scale = 2.0 * abs(float(g[i])) / len(P)
        want = (p64 - q) * (2.0 * float(g[i]) / len(P))
        # Q may be off by test_closest_point_and_weights' tolerance; the fp64 subtraction and product add an ulp of the
        # result each; an fp32 gradient is rounded once more to fp32
        tol = scale * 8.0 * float(f31["max_ratio_q"]) * C.unit_len(P, V) + 2 * ULP * np.abs(want)
        if grad.dtype == torch.float32:
            tol = tol + 2.0 ** -24 * np.abs(want)
        err = np.abs(grad.double().cpu().numpy() - want)
        print("%-10s worst gradient error / tolerance %.3f" % (n, float((err / np.maximum(tol, 1e-300)).max())))
        assert (err <= tol).all(), (n, float((err / np.maximum(tol, 1e-300)).max()))
    # a mesh shared by two clouds, an empty cloud (NaN) and an array (no gradient) in one call; grouping changes no bit
    a = clouds[0].detach().clone().requires_grad_(True)
    b = clouds[0].detach()[:5].clone().requires_grad_(True)
    shared = R.point_surface_loss([a, b, np.zeros((0, 3)), geo[1][0]], [meshes[0], meshes[1]], mesh_of=[0, 0, 0, 1])
    assert torch.equal(shared[0], loss[0].detach()) and torch.equal(shared[3], loss[1].detach()) and bool(torch.isnan(shared[2]))
    (shared[:2] * g[:2]).sum().backward()
    b2 = b.detach().clone().requires_grad_(True)
    alone = R.point_surface_loss([b2], [meshes[0]])
    assert torch.equal(alone[0].detach(), shared[1].detach())
    (alone * g[1:2]).sum().backward()
    assert torch.equal(a.grad, clouds[0].grad) and torch.equal(b.grad, b2.grad) and bool((b.grad != 0).any())
    assert not R.point_surface_loss([geo[0][0]], [meshes[0]]).requires_grad
    assert R.point_surface_loss([], []).shape == (0,)


def test_normal_consistency_with_gt_meshes(f28):
    """gt_meshes= is gt_normals=face_normals_at(gts, meshes) bit for bit and differs from the PCA default, which is
    unchanged; GT samples predicted exactly with their faces' normals score 1, 1, 1 within 4 ulp; the split likewise."""
    import mesh_voxels_oracle as MV

    V, F = f28["ico_V"], f28["ico_F"]
    rng = np.random.default_rng(8)
    gts = [MV.face_points(V, F, 2, 5)[6 * len(F):][:400], MV.face_points(V, F, 1, 6)[6 * len(F):]]   # interior samples
    preds = [gts[0][::2] * 1.01, (gts[1] + 0.004 * rng.normal(size=gts[1].shape)).astype(np.float32), gts[0][:50]]
    gt_of, meshes = [0, 1, 0], [(V, F), (V, F)]
    normals = R.face_normals_at(gts, meshes)
    got = R.normal_consistency(preds, gts, gt_of, gt_meshes=meshes)
    want = R.normal_consistency(preds, gts, gt_of, gt_normals=normals)
    assert got.shape == (3, 3) and torch.equal(got, want)
    pca = R.normal_consistency(preds, gts, gt_of)
    assert not torch.equal(pca, got) and torch.equal(pca, R.normal_consistency(preds, gts, gt_of, gt_meshes=None))
    # interior samples of the faces (no sample on an edge or vertex, where two faces are equally near), predicted exactly,
    # with their faces' normals: every |n . n'| is 1 up to the rounding of a unit normal's squared length
    inner = MV.face_points(V, F, 3, 9)[6 * len(F):]
    rec, = R.closest_points_on_meshes([inner], [(V, F)], normals=True)
    assert (rec.face.cpu().numpy() == np.repeat(np.arange(len(F)), 3)).all()
    one = R.normal_consistency([inner], [inner], pred_normals=[rec.normal], gt_meshes=[(V, F)])
    print("normal consistency of the GT samples with their face normals: 1 - value =", (1.0 - one).cpu().tolist())
    assert one.shape == (1, 3) and bool(((one - 1.0).abs() <= 4 * ULP).all())
    # the split: grouping does not change a bit, and the meshes replace the PCA estimate there too
    pts = np.stack([inner[:300], inner[300:600]]).astype(np.float32)
    predictions, gtc = [(pts, None), (pts[:, ::-1].copy(), np.array([300, 120]))], [inner, gts[0]]
    all_ = R.normal_consistency_of_split(predictions, gtc, gt_meshes=meshes)
    one_ = R.normal_consistency_of_split(predictions, gtc, gt_meshes=meshes, models_per_call=1)
    assert all_.shape == (2, 2, 3) and all_.tobytes() == one_.tobytes()
    by_hand = R.normal_consistency_of_split(predictions, gtc, gt_normals=R.face_normals_at(gtc, meshes))
    assert all_.tobytes() == by_hand.tobytes()
    assert all_.tobytes() != R.normal_consistency_of_split(predictions, gtc).tobytes()
