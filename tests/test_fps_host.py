"""Host-side checks of farthest-point sampling (no GPU): the numpy oracle (tests/fps_oracle.py) against closed forms and an
independent brute force, the argument refusals of dpc_fps / farthest_point_sample / emd_of_split(sampling=...) before any
launch, and the unchanged random subsampling rule."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fps_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def line(n=17):
    return np.stack([np.arange(n, dtype=np.float64), np.zeros(n), np.zeros(n)], axis=1)


def test_oracle_closed_forms():
    """17 points at x = 0..16: from 0 the farthest is 16, then the midpoints by bisection; every tie in the answer (8 is
    alone, but 4 | 12, 2 | 6 | 10 | 14 and the odd points tie) is decided by the lowest index."""
    idx, rad = O.fps(line(), 17, 0)
    assert idx.tolist() == [0, 16, 8, 4, 12, 2, 6, 10, 14, 1, 3, 5, 7, 9, 11, 13, 15]
    assert rad[0] == np.inf and rad[1:].tolist() == [256.0, 64.0, 16.0, 16.0] + [4.0] * 4 + [1.0] * 8
    idx5, rad5 = O.fps(line(), 17, 5)
    assert idx5[:3].tolist() == [5, 16, 0] and rad5[1:3].tolist() == [121.0, 25.0]
    assert sorted(idx5.tolist()) == list(range(17))
    same = np.tile(np.array([[0.25, -0.5, 3.0]]), (9, 1))
    idx, rad = O.fps(same, 9, 4)
    assert idx.tolist() == [4, 0, 1, 2, 3, 5, 6, 7, 8] and rad[0] == np.inf and (rad[1:] == 0).all()
    assert O.fps(same, 1, 8)[0].tolist() == [8]
    assert idx.dtype == np.int32 and rad.dtype == np.float64


def test_oracle_against_brute_force():
    """20 random clouds with n <= 12, some on a lattice (exact ties), some fp32: indices, radius2 and distinctness equal an
    independent O(n^2 m) evaluation of the greedy rule."""
    rng = np.random.default_rng(0)
    for case in range(20):
        n = int(rng.integers(1, 13))
        m = int(rng.integers(1, n + 1))
        first = int(rng.integers(0, n))
        P = O.clouds("lattice" if case % 3 == 0 else "random", n, 100 + case, np.float32 if case % 2 else np.float64)
        idx, rad = O.fps(P, m, first)
        bidx, brad = O.brute_force(P, m, first)
        assert idx.tolist() == bidx.tolist(), case
        assert rad.tobytes() == brad.tobytes(), case
        assert len(set(idx.tolist())) == m and idx[0] == first
        assert (np.diff(rad[1:]) <= 0).all()


def _dry(rows, n_pts):
    from dpc.render import _native

    t = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 5))
    return _native.lib().dpc_fps(None, n_pts, 0, None, t.ctypes.data_as(ctypes.c_void_p), len(t), None, None, None, None)


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """dpc_fps with the real host table and NULL device pointers: DPC_ERR_SHAPE for what the header lists, DPC_ERR_NULL
    (nothing launched) for a valid table.  Rows are (start, count, first, out_start, samples)."""
    from dpc.render import _native

    N, SHAPE, NUL = _native.DPC_FPS_MAX_POINTS, _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL
    assert _dry([(0, 5, 0, 0, 5), (5, N, N - 1, 5, 1024)], 5 + N) == NUL
    assert _dry([(0, 5, 4, 0, 1), (0, 5, 0, 1, 5), (2, 3, 1, 9, 2)], 5) == NUL    # shared input rows, a gap in the output
    assert _dry([], 0) == 0                                          # no clouds: nothing to do
    assert _native.lib().dpc_fps(None, 5, 0, None, None, 1, None, None, None, None) == NUL
    assert _dry([(0, 5, 0, 0, 5)], -1) == SHAPE                      # negative sizes
    assert _native.lib().dpc_fps(None, 5, 0, None, None, -1, None, None, None, None) == SHAPE
    assert _dry([(-1, 5, 0, 0, 5)], 5) == SHAPE
    assert _dry([(0, 5, 0, -1, 5)], 5) == SHAPE
    assert _dry([(0, 5, 0, 0, 5)], 4) == SHAPE and _dry([(1, 5, 0, 0, 5)], 5) == SHAPE   # a range outside its buffer
    assert _dry([(0, 5, 0, 0, 0)], 5) == SHAPE and _dry([(0, 5, 0, 0, 6)], 5) == SHAPE   # samples outside [1, count]
    assert _dry([(0, 5, -1, 0, 5)], 5) == SHAPE and _dry([(0, 5, 5, 0, 5)], 5) == SHAPE  # first outside [0, count)
    assert _dry([(0, 0, 0, 0, 0)], 0) == SHAPE                       # count = 0
    assert _dry([(0, N + 1, 0, 0, 8)], N + 1) == SHAPE               # beyond the limit
    assert _dry([(0, 5, 0, 0, 5), (0, 5, 0, 4, 5)], 5) == SHAPE      # overlapping output ranges
    assert _dry([(0, 5, 0, 5, 5), (0, 5, 0, 0, 5)], 5) == SHAPE      # descending output ranges
    assert _dry([(0, 5, 0, 2 ** 31 - 3, 5)], 5) == SHAPE             # the output range ends beyond int32


def test_limit_matches_the_header():
    from dpc.render import _native, sampling

    header = open(os.path.join(ROOT, "include", "dpc_render.h")).read()
    assert "#define DPC_FPS_MAX_POINTS %d" % _native.DPC_FPS_MAX_POINTS in header
    assert sampling.MAX_POINTS == _native.DPC_FPS_MAX_POINTS >= 12647
    assert "dpc_fps" in _native.SYMBOLS


def test_built_instantiations_are_the_class_table():
    """The k_fps symbols of dpc_fps.o are the eight instantiations the GPU sweep (tests/test_fps_gpu.py) must launch."""
    import re

    from test_abi_and_host import device_object_output

    names = re.findall(r"_ZN12_GLOBAL__N_15k_fpsILi(\d+)ELi(\d+)ELi(\d+)EEEv", device_object_output("dpc_fps.o", ["llvm-readelf", "-sW"]))
    assert {(int(f), int(t), int(p)) for f, t, p in names} == {(f, t, p) for f in (0, 1)
                                                                 for t, p in ((256, 4), (1024, 4), (1024, 8), (1024, 16))}


def test_farthest_point_sample_names_the_offending_cloud():
    """Every refusal comes before a device is looked for (this machine may have none), as ValueError naming the cloud."""
    import dpc.render as R

    ok = np.zeros((4, 3), dtype=np.float32)
    with pytest.raises(ValueError, match=r"clouds\[1\] must be \[n,3\]"):
        R.farthest_point_sample([ok, np.zeros((4, 2), dtype=np.float32)], 2)
    with pytest.raises(ValueError, match=r"must be \[B,n,3\]"):
        R.farthest_point_sample(torch.zeros(4, 3), 2)
    with pytest.raises(ValueError, match=r"clouds\[1\] is empty"):
        R.farthest_point_sample([ok, ok[:0]], 1)
    big = np.zeros((R.sampling.MAX_POINTS + 1, 3), dtype=np.float32)
    with pytest.raises(ValueError, match=r"clouds\[1\] has %d points, the limit is DPC_FPS_MAX_POINTS" % len(big)):
        R.farthest_point_sample([ok, big], 2)
    for m in (0, 5, -1):
        with pytest.raises(ValueError, match=r"clouds\[0\] has 4 points, num_samples = %d is outside \[1, 4\]" % m):
            R.farthest_point_sample([ok], m)
    with pytest.raises(ValueError, match=r"clouds\[1\] has 4 points, num_samples = 5"):
        R.farthest_point_sample([ok, ok], [4, 5])
    for f in (-1, 4):
        with pytest.raises(ValueError, match=r"clouds\[1\] has 4 points, first = %d is outside \[0, 4\)" % f):
            R.farthest_point_sample([ok, ok], 2, first=[0, f])
    with pytest.raises(ValueError, match="num_samples has .* entries for 2 clouds"):
        R.farthest_point_sample([ok, ok], [2, 2, 2])
    with pytest.raises(ValueError, match="num_samples must be an integer"):
        R.farthest_point_sample([ok], 1.5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        R.farthest_point_sample(torch.zeros(2, 4, 3), 2)


def test_emd_of_split_sampling_argument():
    """An unknown value, and the refusals of sampling="fps", come before a device is looked for and name the model."""
    import dpc.render as R

    pts = np.zeros((2, 200, 3), dtype=np.float32)
    gt = np.zeros((300, 3), dtype=np.float32)
    with pytest.raises(ValueError, match='sampling must be "random" or "fps", got \'furthest\''):
        R.emd_of_split([(pts, None)], [gt], num_points=128, sampling="furthest")
    with pytest.raises(ValueError, match="view 1 of model 0 has 100 points, fewer than num_points = 128"):
        R.emd_of_split([(pts, np.array([200, 100]))], [gt], num_points=128, sampling="fps")
    with pytest.raises(ValueError, match="GT cloud of model 1 has 100 points"):
        R.emd_of_split([(pts, None)] * 2, [gt, gt[:100]], num_points=128, sampling="fps")
    big = np.zeros((R.sampling.MAX_POINTS + 1, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="GT cloud of model 1 has %d points, sampling=\"fps\" takes at most" % len(big)):
        R.emd_of_split([(pts, None)] * 2, [gt, big], num_points=128, sampling="fps")
    with pytest.raises(ValueError, match="view 0 of model 0 has %d points, sampling=\"fps\"" % len(big)):
        R.emd_of_split([(big[None], None)], [gt], num_points=128, sampling="fps")
    # the default is the random draw: the same refusal as before, from subsample_indices
    with pytest.raises(ValueError, match="view 1 of model 0 has 100 points"):
        R.emd_of_split([(pts, np.array([200, 100]))], [gt], num_points=128)


def test_random_subsampling_is_unchanged():
    """sampling="random" is the default and takes subsample_indices as it was: the draws of one default_rng(seed), per
    model the GT cloud's, then its views' in order."""
    import inspect

    import dpc.render as R

    assert inspect.signature(R.emd_of_split).parameters["sampling"].default == "random"
    counts = [(300, [200, 150]), (128, [128, 400])]
    got = R.emd.subsample_indices(counts, 128, 7)
    rng = np.random.default_rng(7)
    for (gn, views), (gi, vi) in zip(counts, got):
        assert (gi == rng.choice(gn, 128, replace=False)).all()
        for vn, idx in zip(views, vi):
            assert (idx == rng.choice(vn, 128, replace=False)).all()
