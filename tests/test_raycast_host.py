"""Host-side checks of the ray-mesh intersection (no GPU): the numpy oracle (tests/raycast_oracle.py) against the fixture
f33_raycast.npz and against the same rule in exact rational arithmetic, the clearance of every stored ray re-derived from
the stored inputs, closed forms, every refusal of the Python functions before a device is looked for, the entry point's dry
run, the workspace size and the LDS budget."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import mesh_voxels_oracle as MV
import raycast_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("t", "face", "weights", "hits", "normal")


@pytest.fixture(scope="module")
def f33(golden):
    return golden("f33_raycast.npz")


def case(f33, name):
    return f33[name + "_O"], f33[name + "_D"], f33[name + "_V"], f33[name + "_F"], tuple(f33[name + "_range"])


class _DeviceLookedFor(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    """Valid arguments get as far as looking for a device, and no further, whatever this machine has."""
    from dpc.render import _batch

    def device(*a, **k):
        raise _DeviceLookedFor()

    monkeypatch.setattr(_batch, "device", device)


def test_fixture_holds_the_cases_in_both_dtypes(f33):
    assert sorted(f33["generic"]) == sorted(k + s for k in ("soup", "cube", "open", "dups") for s in ("32", "64"))
    assert sorted(f33["dyadic"]) == ["fan32", "fan64"]
    for name in list(f33["generic"]) + list(f33["dyadic"]):
        O, D, V, F, _ = case(f33, name)
        want = np.float32 if name.endswith("32") else np.float64
        assert O.dtype == D.dtype == V.dtype == want and F.dtype == np.int32 and O.shape == D.shape, name
    assert 90 <= len(f33["soup64_F"]) <= 110 and len(f33["cube64_F"]) == 12 and len(f33["open64_F"]) == 10
    F = f33["dups64_F"]
    assert all((F[30 + k] == F[j]).all() for k, j in enumerate((1, 3, 11))) and {1, 3, 11} <= set(f33["dups64_face"].tolist())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "f33_raycast.npz")) <= 64 * 1024


def test_oracle_reproduces_the_fixture_bit_for_bit(f33):
    for name in list(f33["generic"]) + list(f33["dyadic"]):
        O, D, V, F, rng = case(f33, name)
        res = RO.ray_mesh(O, D, V, F, *rng)
        assert res["status"] == 0, name
        for k in FIELDS:
            assert res[k].dtype == f33["%s_%s" % (name, k)].dtype and res[k].tobytes() == f33["%s_%s" % (name, k)].tobytes(), (name, k)


def test_every_stored_generic_ray_keeps_the_clearance(f33):
    """The clearance conditions, re-derived in exact arithmetic from the stored inputs, hold for every ray: none is left
    out of any comparison."""
    for name in f33["generic"]:
        O, D, V, F, rng = case(f33, name)
        ok = RO.clearance(O, D, V, F, *rng)
        assert ok.shape == (len(O),) and ok.all(), (name, np.nonzero(~ok)[0])
    O, D, V, F, rng = case(f33, "fan64")
    assert not RO.clearance(O, D, V, F, *rng).all()                      # the dyadic rays sit on the boundaries on purpose


def test_oracle_against_exact_arithmetic(f33):
    """face and hits equal the exact ones on every stored ray (the dyadic ones too: their products are exact).  t and the
    weights are within 2^-24 of the exact values, relative to the value or, for a weight, to the clearance 2^-20 where the
    value is smaller (dyadic: to 1).  The bound is reasoned, not measured: a triple product of the rule carries some 2^3
    roundings of 2^-52 relative to the product of its vectors' lengths, the clearance keeps |det| above 2^-20 of that
    product, and 2^5 is left for the shape of the stored faces: 2^(3 - 52 + 20 + 5)."""
    worst = 0.0
    for name in list(f33["generic"]) + list(f33["dyadic"]):
        O, D, V, F, rng = case(f33, name)
        exact = RO.ray_mesh_exact(O, D, V, F, *rng)
        assert [e["face"] for e in exact] == f33[name + "_face"].tolist(), name
        assert [e["hits"] for e in exact] == f33[name + "_hits"].tolist(), name
        for i, e in enumerate(exact):
            t, w = f33[name + "_t"][i], f33[name + "_weights"][i]
            if e["face"] < 0:
                assert t == np.inf and np.isnan(w).all() and (f33[name + "_normal"][i] == 0).all(), (name, i)
                continue
            for got, want in ((t, e["t"]), (w[1], e["u"]), (w[2], e["v"]), (w[0], 1 - e["u"] - e["v"])):
                err = abs(Fraction(float(got)) - want)
                scale = max(abs(want), Fraction(1, 2 ** 20)) if name in f33["generic"] else max(abs(want), 1)
                worst = max(worst, float(err / scale))
    print("worst relative error of t, u, v, 1 - u - v against exact arithmetic: %.3g" % worst)
    assert worst <= 2.0 ** -24


def test_closed_forms():
    V, F = RO.cube()
    # an axis ray through the cube, off the faces' diagonals: two hits, t the slab distances, the near face first
    res = RO.ray_mesh([[0.25, 0.5, -2.0]], [[0.0, 0.0, 0.5]], V, F)
    assert res["hits"].tolist() == [2] and res["t"].tolist() == [4.0] and res["face"].tolist() in ([8], [9])
    assert res["weights"].sum() == 1.0 and (res["weights"] >= 0).all() and res["normal"].tolist() == [[0.0, 0.0, -1.0]]
    far = RO.ray_mesh([[0.25, 0.5, -2.0]], [[0.0, 0.0, 0.5]], V, F, t_min=4.5)
    assert far["hits"].tolist() == [1] and far["t"].tolist() == [6.0] and far["normal"].tolist() == [[0.0, 0.0, 1.0]]
    w = res["weights"][0]
    assert ((w[:, None] * V[F[res["face"][0]]]).sum(axis=0) == [0.25, 0.5, 0.0]).all()
    # through the centre of a side the ray lies on the diagonal both of its triangles share: both report it (not watertight)
    assert RO.ray_mesh([[0.5, 0.5, -2.0]], [[0.0, 0.0, 1.0]], V, F)["hits"].tolist() == [4]
    # culling keeps the near side, seen from its front, and loses the far one
    cull = RO.ray_mesh([[0.25, 0.5, -2.0]], [[0.0, 0.0, 0.5]], V, F, cull_backfaces=True)
    assert cull["hits"].tolist() == [1] and cull["t"].tolist() == [4.0]
    # a ray in a face's plane misses that face; a zero D misses everything; both ends of the range are inclusive
    flat = RO.ray_mesh([[-1.0, 0.25, 0.0], [0.25, 0.25, 0.5]], [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]], V, F[8:10])
    assert flat["hits"].tolist() == [0, 0] and (flat["t"] == np.inf).all() and (flat["face"] == -1).all()
    assert np.isnan(flat["weights"]).all() and (flat["normal"] == 0).all() and flat["status"] == 0
    for lo, hi, n in ((4.0, 6.0, 2), (4.0, 5.0, 1), (5.0, 6.0, 1), (np.nextafter(4.0, 5.0), np.nextafter(6.0, 5.0), 0)):
        assert RO.ray_mesh([[0.25, 0.5, -2.0]], [[0.0, 0.0, 0.5]], V, F, lo, hi)["hits"].tolist() == [n], (lo, hi)
    # guards: a NaN vertex and an index out of range skip their faces; a ray that is not finite answers NaN, -1, 0
    Vn = V.copy()
    Vn[0, 0] = np.nan
    res = RO.ray_mesh([[0.75, 0.25, -2.0]], [[0.0, 0.0, 1.0]], Vn, F)
    assert res["status"] == RO.STATUS_NONFINITE and res["hits"].tolist() == [1] and res["t"].tolist() == [3.0]
    Fb = F.copy()
    Fb[8, 1] = 8
    res = RO.ray_mesh([[0.25, 0.5, -2.0], [0.75, 0.25, -2.0]], [[0.0, 0.0, 1.0]] * 2, V, Fb)
    assert res["status"] == RO.STATUS_BAD_INDEX and res["hits"].tolist() == [1, 2]
    res = RO.ray_mesh([[np.nan, 0.5, -2.0], [0.25, 0.5, -2.0]], [[0.0, 0.0, 1.0], [0.0, np.inf, 1.0]], V, F)
    assert res["status"] == RO.STATUS_NONFINITE and np.isnan(res["t"]).all() and (res["face"] == -1).all() and (res["hits"] == 0).all()
    assert np.isnan(res["weights"]).all() and (res["normal"] == 0).all()
    assert np.isnan(RO.hit_points([[0, 0, 0]] * 2, [[1, 0, 0]] * 2, [np.inf, np.nan])).all()
    assert RO.hit_points([[1, 2, 3]], [[0.5, 0, -1]], [2.0]).tolist() == [[2.0, 2.0, 1.0]]
    e = RO.ray_mesh_exact([[0.25, 0.5, -2.0]], [[0.0, 0.0, 0.5]], V, F)[0]
    assert (e["hits"], e["t"], e["u"] + e["v"] <= 1) == (2, 4, True)


def test_header_symbols_and_exports():
    from dpc.render import _native
    import dpc.render as R

    header = open(os.path.join(ROOT, "include", "dpc_render.h")).read()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ("dpc_ray_mesh_intersect", "dpc_ray_mesh_workspace_bytes"):
        assert name in _native.SYMBOLS and hasattr(lib, name), name
    assert re.search(r"\bint dpc_ray_mesh_intersect\(", header) and re.search(r"\bsize_t dpc_ray_mesh_workspace_bytes\(", header)
    assert "not watertight" in header
    for name in ("ray_mesh_intersect", "rays_hit_points", "visible_points"):
        assert name in R.__all__ and callable(getattr(R, name)), name
    src = open(os.path.join(ROOT, "pytorch-unsup-pc_amd", "csrc", "dpc_raycast.hip")).read()
    assert '#include "dpc_point_mesh.h"' in src and "pm_walk<" in src and "pm_fetch<" in src and not re.search(r"atomic[A-Z]", src)
    # the LDS budget: a tile of faces of nine doubles padded to five double2, the winding's footprint, in the default limit
    lds = int(re.search(r"#define DPC_RAY_LDS_BYTES (\d+)", header).group(1))
    assert lds == _native.DPC_RAY_LDS_BYTES == _native.DPC_PM_FACE_TILE * 5 * 16 == 10240 and lds <= 64 * 1024


def _tab(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 6))


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from dpc.render import _native

    L, SHAPE, NUL, N = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL, None
    inf = float("inf")

    def run(rows, n_rays=10, n_verts=5, n_faces=3, pairs=None, t_min=0.0, t_max=inf):
        t = _tab(rows)
        tp = t.ctypes.data_as(ctypes.c_void_p) if len(t) else N
        return L.dpc_ray_mesh_intersect(N, N, n_rays, 0, N, n_verts, 0, N, n_faces, N, tp, len(t) if pairs is None else pairs, t_min, t_max,
                                        0, N, N, N, N, N, N, N, N)

    good = (0, 10, 0, 5, 0, 3)
    assert run([good]) == NUL and run([good, (0, 0, 0, 5, 0, 3), (2, 3, 0, 5, 1, 2)]) == NUL
    assert run([(0, 10, 0, 5, 0, 0)]) == NUL and run([(0, 10, 0, 0, 3, 0)]) == NUL          # rays and no faces: every ray misses
    assert run([]) == 0 and run([(0, 0, 0, 5, 0, 3)]) == 0 and run([(0, 0, 0, 0, 0, 0)]) == 0
    assert L.dpc_ray_mesh_intersect(N, N, 10, 0, N, 5, 0, N, 3, N, N, 1, 0.0, inf, 0, N, N, N, N, N, N, N, N) == NUL
    assert run([good], n_rays=-1) == SHAPE and run([good], n_verts=-1) == SHAPE and run([good], n_faces=-1) == SHAPE
    assert run([], pairs=-1) == SHAPE
    for row in ((0, 11, 0, 5, 0, 3), (1, 10, 0, 5, 0, 3), (-1, 5, 0, 5, 0, 3), (0, -1, 0, 5, 0, 3), (0, 10, 0, 6, 0, 3), (0, 10, 1, 5, 0, 3),
                (0, 10, -1, 5, 0, 3), (0, 10, 0, -1, 0, 3), (0, 10, 0, 5, 0, 4), (0, 10, 0, 5, 1, 3), (0, 10, 0, 5, -1, 3),
                (0, 10, 0, 5, 0, -1), (0, 10, 0, 5, 4, 0)):
        assert run([row]) == SHAPE, row
    nan = float("nan")
    for lo, hi in ((nan, 1.0), (0.0, nan), (nan, nan), (1.0, 0.5), (inf, 1.0), (0.0, -inf)):
        assert run([good], t_min=lo, t_max=hi) == SHAPE, (lo, hi)
    for lo, hi in ((0.0, 0.0), (-inf, inf), (-2.0, -1.0), (inf, inf)):
        assert run([good], t_min=lo, t_max=hi) == NUL, (lo, hi)
    big = 2 ** 31 - 1
    assert run([(0, big, 0, 5, 0, 3)], n_rays=big) == NUL                                    # the most one call takes
    oversized = [(0, big, 0, 5, 0, 3), (0, 1, 0, 5, 0, 3)]
    # 2^31 output rays, which are 2^31 slots as well: rays enough to fill the device are never cut into chunks, and rays
    # that are cut (fewer than 2^19) have at most 2^11 chunks, so the rays are the only way to that many slots
    assert run(oversized, n_rays=big) == SHAPE
    CH = _native.DPC_PM_FACE_TILE * _native.DPC_PM_CHUNK_TILES
    ws = lambda rows: L.dpc_ray_mesh_workspace_bytes(_tab(rows).ctypes.data_as(ctypes.c_void_p), len(rows))
    assert ws(oversized) == 0 and ws([(0, -1, 0, 5, 0, 3)]) == 0
    assert L.dpc_ray_mesh_workspace_bytes(N, 1) == 0 and L.dpc_ray_mesh_workspace_bytes(_tab([good]).ctypes.data_as(ctypes.c_void_p), 0) == 0
    r16 = lambda n: (n + 15) // 16 * 16
    size = lambda pairs, n_slots: 3 * r16(4 * (pairs + 1)) + r16(8 * n_slots) + 2 * r16(4 * n_slots) + 16
    assert ws([good]) == size(1, 10)                                                         # one chunk: a slot per ray
    assert ws([(0, 10, 0, 5, 0, 0)]) == size(1, 0)                                           # no faces: no chunk, no slot
    assert ws([(0, 3, 0, 5, 0, 4 * CH + 1), good]) == size(2, 5 * 3 + 10)                    # 3 rays in 5 chunks of faces


def test_refusals_come_before_a_device_is_needed(no_device):
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    good, pts, dirs = (V, F), np.zeros((4, 3), dtype=np.float32), np.ones((4, 3), dtype=np.float32)
    fn = R.ray_mesh_intersect
    with pytest.raises(_DeviceLookedFor):
        fn([pts, pts[:0]], [dirs, dirs[:0]], [good], mesh_of=[0, 0], normals=True, cull_backfaces=True)
    with pytest.raises(_DeviceLookedFor):
        fn([pts], [dirs], [(V, F[:0])])                                      # rays and no faces: allowed here
    with pytest.raises(_DeviceLookedFor):
        fn([pts], [dirs], [good], t_min=-1.0, t_max=float("inf"))
    with pytest.raises(ValueError, match=r"ray_mesh_intersect: origins\[1\] must be \[n,3\]"):
        fn([pts, pts[:, :2]], [dirs, dirs], [good, good])
    with pytest.raises(ValueError, match=r"ray_mesh_intersect: directions\[0\] must be \[n,3\]"):
        fn([pts], [dirs[:, :2]], [good])
    with pytest.raises(ValueError, match="2 origins and 1 directions"):
        fn([pts, pts], [dirs], [good, good])
    with pytest.raises(ValueError, match=r"origins\[0\] is \(4, 3\) torch.float32 but directions\[0\] is \(3, 3\) torch.float32"):
        fn([pts], [dirs[:3]], [good])
    with pytest.raises(ValueError, match=r"origins\[0\] is \(4, 3\) torch.float32 but directions\[0\] is \(4, 3\) torch.float64"):
        fn([pts], [dirs.astype(np.float64)], [good])
    with pytest.raises(ValueError, match=r"mesh 0: F must be \[f,3\]"):
        fn([pts], [dirs], [(V, F[:, :2])])
    with pytest.raises(R.MeshError, match=r"mesh 0: F holds a vertex index outside \[0, 12\)"):
        fn([pts], [dirs], [(V, F + 1)])
    with pytest.raises(ValueError, match="2 origins and 1 meshes need mesh_of"):
        fn([pts, pts], [dirs, dirs], [good])
    with pytest.raises(ValueError, match="mesh_of must map each of the 2 origins to one of 1 meshes"):
        fn([pts, pts], [dirs, dirs], [good], mesh_of=[0, 1])
    for lo, hi in ((float("nan"), 1.0), (0.0, float("nan")), (2.0, 1.0), ("a", 1.0), (None, 1.0)):
        with pytest.raises(ValueError, match="t_min and t_max must be numbers with t_min <= t_max"):
            fn([pts], [dirs], [good], t_min=lo, t_max=hi)

    vis = R.visible_points
    with pytest.raises(_DeviceLookedFor):
        vis([pts, pts], [good], [0.0, 0.0, 3.0], 1e-6, mesh_of=[0, 0])
    with pytest.raises(_DeviceLookedFor):
        vis([pts, pts], [good], [[0.0, 0.0, 3.0], torch.tensor([1.0, 2.0, 3.0])], 0.0, mesh_of=[0, 0])
    with pytest.raises(TypeError):
        vis([pts], [good], [0.0, 0.0, 3.0])                                  # eps has no default
    for eps in (-1e-9, 1.0, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match=r"visible_points: eps must be a number in \[0, 1\)"):
            vis([pts], [good], [0.0, 0.0, 3.0], eps)
    for view in ([0.0, 0.0], [[0.0, 0.0, 3.0]] * 3, [0.0, float("nan"), 1.0], 3.0, [[0.0, 0.0, 3.0], [1.0, 2.0]]):
        with pytest.raises(ValueError, match="viewpoints must be one finite"):
            vis([pts, pts], [good], view, 1e-6, mesh_of=[0, 0])
    with pytest.raises(ValueError, match=r"visible_points: clouds\[0\] must be \[n,3\]"):
        vis([pts[:, :2]], [good], [0.0, 0.0, 3.0], 1e-6)
    with pytest.raises(R.MeshError, match="visible_points: mesh 0: F holds a vertex index outside"):
        vis([pts], [(V, F + 1)], [0.0, 0.0, 3.0], 1e-6)

    hp = R.rays_hit_points
    rec = R.raycast.RayHits(torch.zeros(4, dtype=torch.float64), None, None, None)
    assert hp([], [], []) == []
    got, = hp([pts], [dirs], [rec])                                          # needs no device of its own: it follows hits[i].t
    assert got.dtype == torch.float64 and got.tolist() == [[0.0, 0.0, 0.0]] * 4
    with pytest.raises(ValueError, match="1 origins, 1 directions and 0 records"):
        hp([pts], [dirs], [])
    with pytest.raises(ValueError, match=r"rays_hit_points: directions\[0\] must be \[n,3\]"):
        hp([pts], [dirs[:, :1]], [rec])
    for o, d, h in ((pts[:3], dirs, rec), (pts, dirs[:3], rec), (pts[:3], dirs[:3], rec), (pts, dirs, R.raycast.RayHits(np.zeros(4), None, None, None))):
        with pytest.raises(ValueError, match="do not describe the same rays"):
            hp([o], [d], [h])


def test_a_device_is_needed_after_the_checks():
    import dpc.render as R

    V, F = MV.icosphere(0, dtype=np.float32)
    pts = np.zeros((4, 3), dtype=np.float32)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="MI355X only"):
            R.ray_mesh_intersect([pts], [pts], [(V, F)])
        with pytest.raises(RuntimeError, match="MI355X only"):
            R.visible_points([pts], [(V, F)], [0.0, 0.0, 3.0], 1e-6)
