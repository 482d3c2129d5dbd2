"""Mesh densification on the GPU (csrc/dpc_densify.hip): every output point against F17 (the reference's own
densify_model) and against the heap oracle of tests/densify_oracle.py at the full 100 000 splits, by bytes; budgets
that end inside a group of tied edges; independence from batching; reproducibility; refusals; and the GT pipeline
densify_gt.py -> downsample_gt.py -> eval_chamfer on a fake ShapeNet tree."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import scipy.io
import torch

import densify_oracle as D
import dpc.render as R
from dpc.render import _native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F17 = np.load(os.path.join(ROOT, "tests", "golden", "f17_densify.npz"))
NAMES = [str(n) for n in F17["names"]]


def f17_mesh(name):
    return F17[name + "/V"], F17[name + "/E"], F17[name + "/F"]


def mesh_of(tmp_path, text, name="m"):
    p = tmp_path / ("%s.obj" % name)
    p.write_text(text)
    return R.load_obj_mesh(str(p))


def same(got, want, what):
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError("%s: %d rows differ, first %d: %r vs %r" % (what, len(bad), bad[0], got[bad[0]], want[bad[0]]))


@pytest.mark.parametrize("name", NAMES)
def test_f17_case_alone_equals_the_reference(name):
    got, = R.densify_meshes([f17_mesh(name)], int(F17[name + "/n"]))
    same(got, F17[name + "/points"], name)


def test_f17_batched_equals_the_reference():
    n = min(int(F17[name + "/n"]) for name in NAMES)  # a smaller densifyN gives a prefix of the reference's midpoints
    outs = R.densify_meshes([f17_mesh(name) for name in NAMES], n)
    for name, got in zip(NAMES, outs):
        want = F17[name + "/points"]
        same(got, want[:len(F17[name + "/V"]) + n], name)


def test_full_budget_equals_the_oracle_on_20k_face_meshes(tmp_path):
    meshes = [mesh_of(tmp_path, D.sphere_box_obj(60, 160, box_div=12), "sb"),
              mesh_of(tmp_path, D.icosphere_obj(5), "ico")]
    assert all(19000 < len(m[2]) < 22000 for m in meshes), [len(m[2]) for m in meshes]
    outs = R.densify_meshes(meshes, 100000)
    for k, (m, got) in enumerate(zip(meshes, outs)):
        same(got, D.oracle_densify(*m, 100000), "mesh %d" % k)


@pytest.mark.parametrize("n", [1, 37, 100, 157, 320, 555])
def test_budget_ending_inside_a_group_of_tied_edges(tmp_path, n):
    # 10 x 10 unit squares: 100 diagonals tie at sqrt(2), then 220 sides and 200 half-diagonals ... tie at 1 and below
    mesh = mesh_of(tmp_path, D.grid_obj(10, 10))
    got, = R.densify_meshes([mesh], n)
    same(got, D.oracle_densify(*mesh, n), "grid, %d splits" % n)


def _ragged(tmp_path):
    return [mesh_of(tmp_path, D.sphere_box_obj(6, 8), "a"), f17_mesh("messy"), mesh_of(tmp_path, D.grid_obj(3, 7), "g"),
            f17_mesh("one_tri"), mesh_of(tmp_path, D.icosphere_obj(2), "i"), mesh_of(tmp_path, D.sphere_box_obj(20, 30, box_div=3), "b")]


def test_ragged_batch_does_not_depend_on_batching(tmp_path):
    meshes = _ragged(tmp_path)
    n = 4000
    together = R.densify_meshes(meshes, n)
    for k, m in enumerate(meshes):
        alone, = R.densify_meshes([m], n)
        same(together[k], alone, "mesh %d" % k)
        same(alone, D.oracle_densify(*m, n), "mesh %d vs the oracle" % k)
    names = ["m%d" % k for k in range(len(meshes))]
    for per_call in (1, 4):
        split = R.densify_split(names, lambda s: meshes[int(s[1:])], n, models_per_call=per_call)
        for k, s in enumerate(names):
            same(split[s], together[k], "densify_split %d per call, %s" % (per_call, s))
    for rounds in (1, 3):  # rounds between two reads of the counter
        again = R.densify_meshes(meshes, n, rounds_per_sync=rounds)
        for k in range(len(meshes)):
            same(again[k], together[k], "%d rounds per sync, mesh %d" % (rounds, k))


def test_runs_repeat_bit_for_bit(tmp_path):
    meshes = _ragged(tmp_path)
    a = R.densify_meshes(meshes, 20000)
    b = R.densify_meshes(meshes, 20000)
    for k in range(len(meshes)):
        same(a[k], b[k], "mesh %d" % k)


def test_zero_budget_returns_the_vertices():
    got = R.densify_meshes([f17_mesh("sphere_box"), f17_mesh("messy")], 0)
    same(got[0], F17["sphere_box/V"], "sphere_box")
    same(got[1], F17["messy/V"], "messy")


def test_refusals():
    V, E, F = f17_mesh("icosphere")
    with pytest.raises(ValueError, match="no edges"):
        R.densify_meshes([(V, np.zeros((0, 2), np.int64), F[:0])], 10)
    Vn = V.copy()
    Vn[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or inf"):
        R.densify_meshes([(Vn, E, F)], 10)
    Eb = E.copy()
    Eb[0, 1] = len(V)
    with pytest.raises(ValueError, match="outside"):
        R.densify_meshes([(V, Eb, F)], 10)
    with pytest.raises(ValueError, match=">= 0"):
        R.densify_meshes([(V, E, F)], -5)


def test_device_checks_of_an_inconsistent_mesh():
    """The library's own checks: a face whose edge does not join its other two vertices, or an edge with more faces than
    max_face_count, sets DPC_STATUS_BAD_INDEX and leaves that model undensified; a huge coordinate whose length
    overflows sets DPC_STATUS_NONFINITE."""
    dev = torch.device("cuda", torch.cuda.current_device())

    def run(mesh, fe_x=None, most_x=None, scale=1.0, n=50):
        V, E32, F32, fe, most = R.densify._mesh(mesh, 0)
        fe = fe if fe_x is None else fe_x
        most = most if most_x is None else most_x
        Vx = V * scale
        desc = np.array([[0, len(Vx), 0, len(E32), 0, len(F32), n]], dtype=np.int32)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        v, e, f, x, d = t(Vx), t(E32), t(F32), t(fe), t(desc)
        out = torch.zeros((len(Vx) + n, 3), dtype=torch.float64, device=dev)
        info = torch.zeros(2, dtype=torch.int32, device=dev)
        L = _native.lib()
        ws = torch.empty(L.dpc_densify_workspace_bytes(1, len(E32), len(F32), n, most), dtype=torch.uint8, device=dev)
        rc = L.dpc_densify(_native.ptr(v), len(Vx), _native.ptr(e), len(E32), _native.ptr(f), _native.ptr(x), len(F32),
                           _native.ptr(d), desc.ctypes.data_as(ctypes.c_void_p), 1, most, 1, 4, _native.ptr(out),
                           _native.ptr(info[:1]), _native.ptr(info[1:]), _native.ptr(ws), _native.stream_ptr(dev))
        _native.check(rc, "dpc_densify")
        return [int(i) for i in info.cpu()], out.cpu().numpy()

    ico, messy = f17_mesh("icosphere"), f17_mesh("messy")
    (status, left), _ = run(ico)
    assert status == 0 and left == 0
    fe = R.densify._mesh(ico, 0)[3].copy()
    fe[5, 0], fe[5, 1] = fe[5, 1], fe[5, 0]
    (status, left), out = run(ico, fe_x=fe)
    assert status == _native.DPC_STATUS_BAD_INDEX and left == 0
    assert not out[len(ico[0]):].any()  # nothing was densified
    assert R.densify._mesh(messy, 0)[4] == 3
    (status, left), _ = run(messy, most_x=2)  # edge 1-2 has three faces
    assert status == _native.DPC_STATUS_BAD_INDEX
    (status, left), _ = run(ico, scale=1e308)  # finite vertices, lengths beyond the largest double
    assert status == _native.DPC_STATUS_NONFINITE


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gt_pipeline_from_obj_files_to_eval_chamfer(tmp_path, monkeypatch):
    names = ["sphere_box", "icosphere", "messy"]
    n = 1500
    shapenet = tmp_path / "shapenet"
    for name in names:
        (shapenet / "03001627" / name).mkdir(parents=True)
        (shapenet / "03001627" / name / "model.obj").write_text(str(F17[name + "/text"]))
    (tmp_path / "splits").mkdir()
    (tmp_path / "splits" / "03001627_test.txt").write_text("\n".join(names) + "\n")
    monkeypatch.chdir(tmp_path)
    densify = _tool("densify_gt")
    argv = ["--shapenet_path", str(shapenet), "--synth_set", "03001627", "--subset", "test", "--output_dir",
            str(tmp_path / "dense"), "--num_points", str(n), "--models_per_call", "2"]
    assert densify.main(argv) == {"written": names, "skipped": [], "failed": {}}
    dense_dir = tmp_path / "dense" / "03001627"
    for name in names:
        got = scipy.io.loadmat(str(dense_dir / ("%s.mat" % name)))["points"]
        same(got, F17[name + "/points"][:len(F17[name + "/V"]) + n], name)
    assert densify.main(argv) == {"written": [], "skipped": names, "failed": {}}

    down = _tool("downsample_gt")
    assert down.main(["--inp_dir", str(tmp_path / "dense"), "--out_dir", str(tmp_path / "down"), "--synth_set",
                      "03001627"])["written"] == sorted(names)
    down_dir = tmp_path / "down" / "03001627"
    rng = np.random.default_rng(4)
    preds = tmp_path / "preds"
    preds.mkdir()
    for name in names:
        R.save_predictions(str(preds / ("%s_pc.pkl" % name)), rng.random((2, 500, 3)).astype(np.float32) - 0.5)
    res = R.eval_chamfer(str(preds), names, lambda s: scipy.io.loadmat(str(down_dir / ("%s.mat" % s)))["points"])
    ref_dense = {s: F17[s + "/points"][:len(F17[s + "/V"]) + n] for s in names}
    ref = R.eval_chamfer(str(preds), names, lambda s: R.voxel_down_sample(ref_dense[s], 0.01).cpu().numpy())
    assert res["model_names"] == names
    assert res["chamfer"].tobytes() == ref["chamfer"].tobytes() and np.isfinite(res["final"]).all()


def test_a_failing_model_is_named_and_does_not_stop_the_others():
    ico, messy = f17_mesh("icosphere"), f17_mesh("messy")
    huge = (ico[0] * 1e308, ico[1], ico[2])  # finite vertices; the device finds lengths beyond the largest double
    meshes = {"a": ico, "bad": huge, "b": messy}
    n = 500
    with pytest.raises(R.MeshError, match="'bad'.*not finite"):
        R.densify_split(list(meshes), meshes.get, n)
    errors, saved = {}, {}
    out = R.densify_split(list(meshes), meshes.get, n, save=saved.__setitem__, errors=errors, keep=False)
    assert out == {} and list(errors) == ["bad"] and sorted(saved) == ["a", "b"]
    for name in ("a", "b"):
        same(saved[name], D.oracle_densify(*meshes[name], n), name)
    with pytest.raises(R.MeshError, match="mesh 1"):
        R.densify_meshes([ico, huge], n)


def test_models_of_different_face_degrees_split_into_jobs(tmp_path):
    meshes = _ragged(tmp_path)
    n = 3000
    together = R.densify_meshes(meshes, n)
    tight = R.densify_meshes(meshes, n, workspace_limit=1)  # every model its own job
    for k in range(len(meshes)):
        same(tight[k], together[k], "mesh %d" % k)


def test_gt_tool_reports_a_bad_model_and_writes_the_rest(tmp_path, monkeypatch):
    shapenet = tmp_path / "shapenet" / "c"
    texts = {"good": str(F17["icosphere/text"]), "relative": "v 0 0 1\nv 1 0 1\nv 0 1 1\nf -1 -2 -3\n",
             "flat": "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n", "messy": str(F17["messy/text"])}
    for name, text in texts.items():
        (shapenet / name).mkdir(parents=True)
        (shapenet / name / "model.obj").write_text(text)
    (tmp_path / "splits").mkdir()
    (tmp_path / "splits" / "c_val.txt").write_text("\n".join(texts) + "\n")
    monkeypatch.chdir(tmp_path)
    res = _tool("densify_gt").main(["--shapenet_path", str(tmp_path / "shapenet"), "--synth_set", "c", "--output_dir",
                                    str(tmp_path / "dense"), "--num_points", "300"])
    assert res["written"] == ["good", "messy"] and sorted(res["failed"]) == ["flat", "relative"]
    for name, case in (("good", "icosphere"), ("messy", "messy")):
        got = scipy.io.loadmat(str(tmp_path / "dense" / "c" / ("%s.mat" % name)))["points"]
        same(got, F17[case + "/points"][:len(F17[case + "/V"]) + 300], name)
