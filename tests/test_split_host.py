"""dpc/render/_split.py on the host: the checks every *_of_split function shares, the groups, the views of a group against
a loop written out by hand, the walk over a split by model name, and the isolation of a model after a MeshError."""
import numpy as np
import pytest
import torch

import dpc.render as R
from dpc.render import _split
from dpc.render._split import Split, _host_unit_quaternion, _rotate, batches, isolate

CPU = torch.device("cpu")
Q = np.array([[0.9, 0.1, -0.3, 0.2]])


def pred(V=2, N=5, nums=None, seed=0, dtype=np.float32):
    return (np.random.default_rng(seed).random((V, N, 3)).astype(dtype) - 0.5, nums)


def gt(n=4, seed=1):
    return np.random.default_rng(seed).random((n, 3)) - 0.5


def test_shared_refusals_carry_the_messages_of_the_seven():
    p, g = pred(), gt()
    with pytest.raises(ValueError, match=r"^chamfer_of_split: 1 predictions and 2 GT clouds$"):
        Split("chamfer_of_split", [p], [g, g], None, 256)
    with pytest.raises(ValueError, match=r"^solid_iou_of_split: 2 predictions and 1 meshes$"):
        Split("solid_iou_of_split", [p, p], [g], None, 256, noun="meshes", gt_label=None)
    with pytest.raises(ValueError, match=r"^emd_of_split: models_per_call must be >= 1$"):
        Split("emd_of_split", [p], [g], None, 0)
    with pytest.raises(ValueError, match=r"^predictions\[1\] must be \(points, num_points\) or load_predictions' "
                                         r"\(points, camera_pose, num_points\)$"):
        Split("iou_of_split", [p, p[0]], [g, g], None, 256)
    with pytest.raises(ValueError, match=r"^predictions\[0\] points must be \[V,N,3\], got \(2, 5\)$"):
        Split("iou_of_split", [(np.zeros((2, 5)), None)], [g], None, 256)
    with pytest.raises(ValueError, match=r"^predictions\[0\] num_points must be 2 integers in \[0, 5\], got array\(\[3, 6\]\)$"):
        Split("iou_of_split", [pred(nums=np.array([3, 6]))], [g], None, 256)
    with pytest.raises(ValueError, match=r"^predictions\[0\] num_points must be 2 integers in \[0, 5\]"):
        Split("iou_of_split", [pred(nums=np.array([3.0, 4.0]))], [g], None, 256)
    with pytest.raises(ValueError, match=r"^fscore_of_split: every model needs the same number of views, got \[2, 3\]$"):
        Split("fscore_of_split", [pred(V=3), pred(V=2)], [g, g], None, 256)
    with pytest.raises(ValueError, match=r"^gt_clouds\[1\] must be \[n,3\], got \(4, 2\)$"):
        Split("chamfer_of_split", [p, p], [g, g[:, :2]], None, 256)
    with pytest.raises(ValueError, match=r"^fscore_of_split: gt_clouds\[0\] must be \[n,3\], got \(4, 2\)$"):
        Split("fscore_of_split", [p], [g[:, :2]], None, 256, gt_label="fscore_of_split: gt_clouds[%d]")
    with pytest.raises(ValueError, match=r"^reference_rotation must be a \[1,4\] quaternion, got \(4,\)$"):
        Split("chamfer_of_split", [p], [g], Q[0], 256)


def test_an_empty_gt_cloud_is_refused_only_when_asked_and_only_under_a_non_empty_view():
    p, none = pred(), np.zeros((0, 3))
    with pytest.raises(ValueError, match=r"^chamfer_of_split: GT cloud 1 is empty$"):
        Split("chamfer_of_split", [p, p], [gt(), none], None, 256, refuse_empty_gt=True)
    s = Split("iou_of_split", [p, p], [gt(), none], None, 256)
    assert len(s.gts[1]) == 0 and s.M == 2
    s = Split("chamfer_of_split", [pred(nums=np.array([0, 0]))], [none], None, 256, refuse_empty_gt=True)   # nothing to match
    assert s.counts == [[0, 0]]


@pytest.mark.parametrize("M", [0, 1, 3])
@pytest.mark.parametrize("step", [1, 2, 256])
def test_groups_cover_the_models_in_order(M, step):
    s = Split("chamfer_of_split", [pred()] * M, [gt()] * M, None, step)
    assert (s.M, s.V) == (M, 2 if M else 0) and s.empty == (M == 0)
    assert [list(g) for g in s.groups] == [list(range(a, min(M, a + step))) for a in range(0, M, step)]
    assert all(1 <= len(g) <= step for g in s.groups) and [m for g in s.groups for m in g] == list(range(M))


def test_no_targets_and_no_views():
    s = Split("solid_iou_of_split", [pred(V=0)] * 2, ["mesh", "mesh"], None, 1, noun="meshes", gt_label=None)
    assert s.gts == [] and s.V == 0 and s.M == 2 and s.empty and s.counts == [[], []] and len(s.groups) == 2
    assert s.tensors()[1] == [] and [t.shape for t in s.tensors()[0]] == [(0, 5, 3)] * 2


def test_views_of_a_group_equal_a_loop_written_out_by_hand():
    """Three models of two views, a float64 rotation; model 1 truncates its views to 3 and 0 points."""
    preds = [pred(seed=3), pred(nums=np.array([3, 0]), seed=4), pred(nums=torch.tensor([5, 2]), seed=5)]
    s = Split("chamfer_of_split", preds, [gt()] * 3, Q, 2)
    qn = _host_unit_quaternion(Q)
    assert s.qn.dtype == torch.float64 and torch.equal(s.qn, qn) and s.counts == [[5, 5], [3, 0], [5, 2]]
    for group in s.groups:
        views_list, gt_of = s.views(group, CPU)
        assert gt_of == [j for j in range(len(group)) for _ in range(2)] and len(views_list) == 2 * len(group)
        k = 0
        for m in group:
            rot = _rotate(torch.from_numpy(preds[m][0]), qn, CPU)
            for i in range(2):
                want = rot[i, :s.counts[m][i]]
                got = views_list[k]
                assert got.dtype == torch.float64 and got.shape == want.shape and torch.equal(got, want), (m, i)
                assert not got.requires_grad
                k += 1
    per_model = s.model(1, CPU)
    assert [tuple(v.shape) for v in per_model] == [(3, 3), (0, 3)]


def test_without_a_rotation_the_views_are_the_input_itself():
    pts = torch.from_numpy(pred(seed=6)[0]).requires_grad_(True)
    s = Split("chamfer_of_split", [(pts, np.array([4, 5]))], [gt()], None, 256)
    (views_list, gt_of), = [s.views(g, CPU) for g in s.groups]
    assert gt_of == [0, 0] and [v.dtype for v in views_list] == [torch.float32] * 2 and not any(v.requires_grad for v in views_list)
    assert views_list[0].shape == (4, 3) and views_list[0].data_ptr() == pts.data_ptr()             # a view, not a copy
    assert views_list[1].shape == (5, 3) and views_list[1].data_ptr() == pts[1].data_ptr()
    assert all(torch.equal(v, pts.detach()[i, :n]) for i, (v, n) in enumerate(zip(views_list, (4, 5))))
    assert s.model(0, CPU, on_device=True)[0].data_ptr() == pts.data_ptr()                            # already there


def test_store_writes_a_group_back_reshaped():
    s = Split("chamfer_of_split", [pred()] * 3, [gt()] * 3, None, 2)
    out = np.zeros((3, 2, 4), dtype=np.float64)
    for group in s.groups:
        res = torch.arange(len(group) * 2 * 4, dtype=torch.float64).reshape(len(group) * 2, 4) + 100 * group[0]
        host = s.store(out, group, res)
        assert host.shape == (len(group), 2, 4) and np.array_equal(out[group[0]:group[-1] + 1], host)
    assert np.array_equal(out[:2].reshape(-1), np.arange(16.0)) and np.array_equal(out[2].reshape(-1), np.arange(8.0) + 200)
    flat = np.zeros((3, 2), dtype=np.int64)
    s.store(flat, s.groups[1], torch.tensor([7, 8]))
    assert flat.tolist() == [[0, 0], [0, 0], [7, 8]]


def test_batches_skip_flush_and_number_the_pending_items():
    seen = []

    def load(name, i):
        seen.append((name, i))
        return None if name.startswith("skip") else name.upper()

    names = ["a", "skip1", "b", "c", "skip2", "d", "e"]
    got = list(batches(names, load, 2))
    assert got == [[("a", "A"), ("b", "B")], [("c", "C"), ("d", "D")], [("e", "E")]]
    assert seen == [("a", 0), ("skip1", 1), ("b", 1), ("c", 0), ("skip2", 1), ("d", 1), ("e", 0)]
    assert list(batches([], load, 2)) == [] and list(batches(["skip"], load, 2)) == []
    assert [len(b) for b in batches(names, load, 256)] == [5]


def test_batches_name_record_or_pass_on_what_the_loader_raises():
    def load(name, i):
        if name == "bad":
            raise IndexError("a face line with 2 indices")
        if name == "worse":
            raise KeyError("worse")
        return name

    with pytest.raises(IndexError, match=r"^model 'bad': a face line with 2 indices$") as info:
        list(batches(["a", "bad", "b"], load, 2, None, (ValueError, IndexError)))
    assert isinstance(info.value.__cause__, IndexError)
    errors = {}
    assert list(batches(["a", "bad", "b", "c"], load, 2, errors, (ValueError, IndexError))) == [[("a", "a"), ("b", "b")], [("c", "c")]]
    assert errors == {"bad": "a face line with 2 indices"}
    for errors in (None, {}):
        with pytest.raises(KeyError) as info:                               # outside the tuple: untouched
            list(batches(["a", "worse"], load, 2, errors, (ValueError, IndexError)))
        assert info.value.args == ("worse",) and not errors
    with pytest.raises(IndexError, match=r"^a face line with 2 indices$"):  # the default catches nothing
        list(batches(["bad"], load, 2, {}))


@pytest.mark.parametrize("k", [0, 2, 3])
def test_isolate_runs_the_models_of_a_refused_batch_alone(k):
    items, names = [10, 11, 12, 13], ["m0", "m1", "m2", "m3"]
    calls = []

    def run(batch):
        calls.append(list(batch))
        if items[k] in batch:
            raise R.MeshError("mesh %d is bad" % batch.index(items[k]))
        return [2 * x for x in batch]

    errors = {}
    got = isolate(run, items, names, errors)
    assert got == [None if i == k else 2 * x for i, x in enumerate(items)]
    assert errors == {names[k]: "mesh 0 is bad"} and calls == [items] + [[x] for x in items]
    with pytest.raises(R.MeshError, match=r"^model 'm%d': mesh 0 is bad$" % k) as info:
        isolate(run, items, names, None)
    assert isinstance(info.value.__cause__, R.MeshError)
    calls.clear()
    assert isolate(run, [1, 2], ["x", "y"], None) == [2, 4] and calls == [[1, 2]]      # a batch that passes runs once

    def other(batch):
        raise ValueError("not a mesh error")

    with pytest.raises(ValueError, match=r"^not a mesh error$"):
        isolate(other, items, names, {})


def test_the_helpers_have_one_home():
    for name in ("_host_unit_quaternion", "_rotate", "_prediction"):
        assert hasattr(_split, name) and not hasattr(R.chamfer, name)
