"""Host side of the mesh densification (dpc/render/densify.py, tests/densify_oracle.py), against F17: the reference's
own densify_single.densify_model run on CPU (tests/golden/make_golden_densify.py).  No GPU needed."""
import os

import numpy as np
import pytest

import densify_oracle as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F17 = np.load(os.path.join(ROOT, "tests", "golden", "f17_densify.npz"))
NAMES = [str(n) for n in F17["names"]]


def write_obj(tmp_path, text, name="model.obj"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_reference_by_bytes(name):
    pts = D.oracle_densify(F17[name + "/V"], F17[name + "/E"], F17[name + "/F"], int(F17[name + "/n"]))
    assert pts.dtype == np.float64 and pts.tobytes() == F17[name + "/points"].tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_load_obj_mesh_equals_the_reference_parse(tmp_path, name):
    from dpc.render import load_obj_mesh

    V, E, F = load_obj_mesh(write_obj(tmp_path, str(F17[name + "/text"])))
    assert V.tobytes() == F17[name + "/V"].tobytes()
    assert np.array_equal(E, F17[name + "/E"]) and np.array_equal(F, F17[name + "/F"])


def test_messy_and_one_triangle_cases_are_what_they_claim():
    assert len(F17["messy/F"]) == 5 and len(F17["messy/V"]) == 12   # duplicate, degenerate, two rank-2 faces dropped
    assert len(F17["one_tri/F"]) == 0 and len(F17["one_tri/E"]) == 3   # the removeWeirdDuplicate quirk
    E = F17["messy/E"]
    faces_on_12 = sum(1 for f in F17["messy/F"] if 0 in f and 1 in f)
    assert faces_on_12 == 3 and [0, 1] in E.tolist()


def test_batched_matrix_rank_equals_the_per_face_call():
    rng = np.random.default_rng(3)
    M = rng.standard_normal((4000, 3, 3))
    M[::7, 2] = M[::7, 0] + M[::7, 1]            # rank 2
    M[::11, 1] = M[::11, 0]                       # two equal rows
    M[::13, :, 2] = 0.0                           # a plane through the origin
    M[::17] *= 1e-300
    batched = np.linalg.matrix_rank(M)
    assert np.array_equal(batched, [np.linalg.matrix_rank(m) for m in M])


def test_length_formula_equals_numpy_norm():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((20000, 3)) * rng.uniform(1e-3, 10.0, (20000, 1))
    got = np.array([D.edge_length(v, np.zeros(3)) for v in x])
    ref = np.array([np.linalg.norm(v) for v in x])
    assert got.tobytes() == ref.tobytes()


def test_exact_fma_matches_fractions():
    from fractions import Fraction

    rng = np.random.default_rng(9)
    for d, c in zip(rng.standard_normal(3000) * 10.0 ** rng.integers(-8, 8, 3000), np.abs(rng.standard_normal(3000))):
        assert D._sq_fma(float(d), float(c)) == float(Fraction(float(d)) ** 2 + Fraction(float(c)))


def _check_monotone(V, E, F, n):
    _, pops, children = D.oracle_densify(V, E, F, n, record=True)
    assert all(a >= b for a, b in zip(pops, pops[1:])), "a pop was longer than the one before it"
    worst = max((c / p for kids in children for c, p in kids), default=0.0)
    assert worst < 0.87, worst
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_pops_never_lengthen_and_children_are_short(name):
    _check_monotone(F17[name + "/V"], F17[name + "/E"], F17[name + "/F"], int(F17[name + "/n"]))


@pytest.mark.parametrize("seed", range(3))
def test_pops_never_lengthen_on_random_meshes(tmp_path, seed):
    from dpc.render import load_obj_mesh

    rng = np.random.default_rng(seed)
    V = rng.uniform(-1, 1, (40, 3))
    F = np.array([rng.choice(40, 3, replace=False) for _ in range(60)])
    text = "".join("v %r %r %r\n" % tuple(float(x) for x in v) for v in V) + "".join("f %d %d %d\n" % tuple(f + 1) for f in F)
    _check_monotone(*load_obj_mesh(write_obj(tmp_path, text)), 3000)


def test_load_obj_mesh_refusals(tmp_path):
    from dpc.render import load_obj_mesh

    base = "v 0.1 0.2 0.3\nv 1.0 0.1 0.2\nv 0.2 1.1 0.3\n"
    with pytest.raises(ValueError, match="<= 0"):
        load_obj_mesh(write_obj(tmp_path, base + "f -1 -2 -3\n"))
    with pytest.raises(IndexError):
        load_obj_mesh(write_obj(tmp_path, base + "f 1 2 4\n"))
    with pytest.raises(ValueError, match="no face"):
        load_obj_mesh(write_obj(tmp_path, base + "v 0 0 0\nf 1 2 4\n"))  # rank 2: nothing left
    with pytest.raises(ValueError):
        load_obj_mesh(write_obj(tmp_path, "v 0.1 x 0.3\n"))               # float("x"), as the reference
    with pytest.raises(ValueError):
        load_obj_mesh(write_obj(tmp_path, base + "f 1 2 a\n"))            # int("a"), as the reference


def test_densify_refusals_before_any_device():
    from dpc.render import densify_meshes

    V = np.array([[0.1, 0.2, 0.3], [1.0, 0.1, 0.2], [0.2, 1.1, 0.3]])
    E = np.array([[0, 1], [0, 2], [1, 2]])
    F = np.array([[0, 1, 2]])
    with pytest.raises(ValueError, match=">= 0"):
        densify_meshes([(V, E, F)], -1)
    with pytest.raises(ValueError, match="no edges"):
        densify_meshes([(V, np.zeros((0, 2), np.int64), np.zeros((0, 3), np.int64))], 10)
    with pytest.raises(ValueError, match="NaN or inf"):
        densify_meshes([(np.where(np.eye(3, dtype=bool), np.inf, V), E, F)], 10)
    with pytest.raises(ValueError, match="outside"):
        densify_meshes([(V, np.array([[0, 1], [0, 3], [1, 2]]), F)], 10)
    with pytest.raises(ValueError, match="not in E"):
        densify_meshes([(V, E[:2], F)], 10)


def test_abi_refuses_bad_descriptors_without_a_device():
    import ctypes

    from dpc.render import _native

    L = _native.lib()
    desc = np.array([[0, 3, 0, 3, 0, 1, 10]], dtype=np.int32)
    call = lambda d, nv=3, ne=3, nf=1, most=2: L.dpc_densify(None, nv, None, ne, None, None, nf, None,
                                                             d.ctypes.data_as(ctypes.c_void_p), len(d), most, 1, 1,
                                                             None, None, None, None, None)
    assert call(desc) == _native.DPC_ERR_NULL                     # valid: only the device pointers are missing
    assert call(desc, nv=2) == _native.DPC_ERR_SHAPE              # a range beyond its array
    neg = desc.copy(); neg[0, 6] = -1
    assert call(neg) == _native.DPC_ERR_SHAPE                     # a negative budget
    none = np.array([[0, 3, 0, 0, 0, 0, 10]], dtype=np.int32)
    assert call(none) == _native.DPC_ERR_SHAPE                    # splits but no edges
    big = desc.copy(); big[0, 6] = 400_000_000
    assert call(big) == _native.DPC_ERR_SHAPE                     # edge ids beyond int32
    assert call(desc, most=-1) == _native.DPC_ERR_SHAPE
    assert L.dpc_densify_workspace_bytes(1, 3, 1, 10, 2) > 0 and L.dpc_densify_workspace_bytes(0, 3, 1, 10, 2) == 0


def test_face_edges_join_the_other_two_vertices():
    from dpc.render import densify as RD

    for name in ("sphere_box", "icosphere", "messy"):
        V, E32, F32, fe, most = RD._mesh((F17[name + "/V"], F17[name + "/E"], F17[name + "/F"]), 0)
        for j, (x, y) in enumerate(((1, 2), (0, 2), (0, 1))):
            got = np.sort(E32[fe[:, j]], axis=1)
            assert np.array_equal(got, np.sort(F32[:, [x, y]], axis=1)), (name, j)
        assert most == np.bincount(fe.ravel()).max()


def test_jobs_are_cut_at_the_workspace_limit_and_the_model_count():
    from dpc.render import _native
    from dpc.render import densify as RD

    L = _native.lib()
    small = (None, np.zeros((100, 2)), np.zeros((60, 3)), None, 2)
    wide = (None, np.zeros((100, 2)), np.zeros((60, 3)), None, 40)   # one strongly non-manifold model
    one = L.dpc_densify_workspace_bytes(1, 100, 60, 1000, 2)
    groups = list(RD._groups([small] * 6, 1000, 4, 1 << 40))
    assert groups == [(0, 4), (4, 6)]
    groups = list(RD._groups([small] * 6, 1000, 100, 3 * one + 1))
    assert groups == [(0, 3), (3, 6)]
    # the wide model's degree would inflate its neighbours' bound: it goes alone, and so does a model over the limit
    groups = list(RD._groups([small, small, wide, small, small], 1000, 100, 3 * one + 1))
    assert groups == [(0, 2), (2, 3), (3, 5)]
    assert list(RD._groups([wide], 1000, 100, 1)) == [(0, 1)]


def test_split_names_or_records_models_that_fail_to_load():
    from dpc.render import densify_split

    def load(name):
        if name == "gone":
            raise OSError("no such file")
        raise ValueError("no face of rank 3")

    with pytest.raises(ValueError, match="'flat'"):
        densify_split(["flat"], load, 100)
    errors = {}
    assert densify_split(["flat", "gone"], load, 100, errors=errors) == {}
    assert set(errors) == {"flat", "gone"} and "rank 3" in errors["flat"]


def test_densify_gt_refuses_zero_points(tmp_path, monkeypatch):
    import importlib.util

    spec = importlib.util.spec_from_file_location("densify_gt", os.path.join(ROOT, "tools", "densify_gt.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with pytest.raises(SystemExit):
        tool.main(["--shapenet_path", str(tmp_path), "--synth_set", "x", "--output_dir", str(tmp_path), "--num_points", "0"])
