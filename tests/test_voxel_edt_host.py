"""Host-side checks of the voxel distance transforms (no GPU): the numpy oracle (tests/voxel_edt_oracle.py) against its
fixture (f34_voxel_edt.npz), its brute-force and separable versions against each other, against scipy where that is
importable and against closed forms; the header, the binding and the built kernels; every refusal of the dpc_voxel_edt*
entry points before any launch and its order; every ValueError of the Python layer; the exported names."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import voxel_edt_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "f34_voxel_edt.npz")
ENTRY_POINTS = ("dpc_voxel_edt", "dpc_voxel_shell", "dpc_voxel_edt_stats")
SHAPES = [(1, 1, 1), (3, 5, 7), (5, 33, 31), (2, 1, 40), (9, 16, 40)]
# the instantiations tests/test_voxel_edt_gpu.py must launch
INSTANTIATIONS = {"k_edt_plane<32, 256>", "k_edt_plane<64, 256>", "k_edt_plane<128, 512>", "k_edt_depth<32>", "k_edt_depth<64>",
                  "k_edt_depth<128>", "k_voxel_shell", "k_voxel_edt_stats"}


def test_oracle_equals_its_fixture():
    f = np.load(GOLDEN)
    cases = list(O.golden_cases())
    assert len(cases) == len(O.GOLDEN_SHAPES) * len(O.CONTENTS) == 42
    assert f["taus"].tolist() == list(O.GOLDEN_TAUS) and f["thresholds_sq"].tolist() == [0, 1, 2, 4, 9]
    thr = O.thresholds_sq(O.GOLDEN_TAUS)
    assert thr.tolist() == f["thresholds_sq"].tolist()
    for key, shape, kind, g in cases:
        assert O.pack_bits(g).tobytes() == f[key + "/bits"].tobytes(), key
        fields = [O.edt_separable(g, of_clear) for of_clear in (False, True)]
        assert [O.digest(x) for x in fields] == f[key + "/sq_digests"].tolist(), key
        if g.size <= 128:
            assert np.array_equal(np.stack(fields), f[key + "/sq"]) and f[key + "/sq"].dtype == np.int32, key
        assert O.pack_bits(O.shell(g)).tobytes() == f[key + "/shell"].tobytes(), key
        stats = np.stack([O.surface_stats(g, O.golden_partner(shape), thr, surface) for surface in (True, False)])
        assert stats.dtype == np.int64 and np.array_equal(stats, f[key + "/stats"]), key
        assert O.fscore(stats).tobytes() == f[key + "/fscore"].tobytes(), key


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_brute_force_equals_the_separable_passes(shape):
    for kind in O.CONTENTS:
        g = O.grid(shape, kind, 7)
        for of_clear in (False, True):
            a, b = O.edt_brute(g, of_clear), O.edt_separable(g, of_clear)
            assert a.dtype == b.dtype == np.int32 and np.array_equal(a, b), (shape, kind, of_clear)


def test_oracle_equals_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    for shape in SHAPES:
        for fill in (0.02, 0.3):
            g = rng.random(shape) < fill
            if not g.any():
                g[0, 0, 0] = True
            want = np.rint(ndimage.distance_transform_edt(~g) ** 2).astype(np.int32)
            assert np.array_equal(O.edt_brute(g), want) and np.array_equal(O.edt_separable(g), want), (shape, fill)
    g = rng.random((64, 64, 64)) < 0.05
    assert np.array_equal(O.edt_separable(g), np.rint(ndimage.distance_transform_edt(~g) ** 2).astype(np.int32))


def test_oracle_closed_forms():
    # one seed: the squared distance to it
    shape, seed = (5, 6, 7), (4, 0, 3)
    g = np.zeros(shape, dtype=bool)
    g[seed] = True
    d, h, w = np.ogrid[:5, :6, :7]
    want = (d - 4) ** 2 + h ** 2 + (w - 3) ** 2
    assert np.array_equal(O.edt_brute(g), want) and np.array_equal(O.edt_separable(g), want)
    # a full grid is 0 everywhere, an empty grid NONE everywhere, and the other seed mode swaps them
    full, empty = np.ones(shape, dtype=bool), np.zeros(shape, dtype=bool)
    for edt in (O.edt_brute, O.edt_separable):
        assert (edt(full) == 0).all() and (edt(empty) == O.NONE).all()
        assert (edt(full, True) == O.NONE).all() and (edt(empty, True) == 0).all()
    assert O.NONE == np.iinfo(np.int32).max
    # the far corner of the largest grid
    g = np.zeros((128, 128, 128), dtype=bool)
    g[127, 127, 127] = True
    f = O.edt_separable(g)
    assert f[0, 0, 0] == 48387 == 3 * 127 ** 2 and f[127, 127, 127] == 0 and f[127, 127, 0] == 127 ** 2
    # the shell: a solid block loses its interior, a slab one voxel thick and the grid's border voxels stay
    block = np.zeros((6, 6, 6), dtype=bool)
    block[1:5, 1:5, 1:5] = True
    s = O.shell(block)
    assert s.sum() == 4 ** 3 - 2 ** 3 and not s[2:4, 2:4, 2:4].any()
    inner = np.zeros(shape, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True
    assert np.array_equal(O.shell(full), ~inner)                       # a neighbour outside the grid counts as clear
    slab = np.zeros(shape, dtype=bool)
    slab[2] = True
    assert np.array_equal(O.shell(slab), slab)
    # thresholds: floor(tau^2) in fp64
    assert O.thresholds_sq([0, 0.5, 1, 1.5, np.sqrt(2), 2, 1e6]).tolist() == [0, 0, 1, 2, 2, 4, O.NONE - 1]
    # stats and the F-score conventions
    a = np.zeros((1, 1, 8), dtype=bool)
    a[0, 0, [0, 1]] = True
    b = np.zeros((1, 1, 8), dtype=bool)
    b[0, 0, [1, 4]] = True
    s = O.surface_stats(a, b, O.thresholds_sq([0, 1, 3]), surface=False)
    assert s.tolist() == [[2, 2, 1, 1, 2, 2], [2, 2, 9, 1, 1, 2]]
    assert O.fscore(s).tolist() == [[0.5, 0.5, 0.5], [1.0, 0.5, 2 / 3], [1.0, 1.0, 1.0]]
    none = np.zeros((1, 1, 8), dtype=bool)
    s = O.surface_stats(none, b, O.thresholds_sq([1]), surface=False)
    assert s.tolist() == [[0, 0, 0, 0], [2, 0, 0, 0]]                   # nothing to measure; nothing reached
    p, r, f = O.fscore(s)[0]
    assert np.isnan(p) and r == 0.0 and np.isnan(f)                     # an empty prediction: precision NaN, and so F
    p, r, f = O.fscore(O.surface_stats(b, none, O.thresholds_sq([1]), surface=False))[0]
    assert p == 0.0 and np.isnan(r) and np.isnan(f)
    assert O.fscore(np.array([[2, 2, 5, 0], [3, 3, 9, 0]]))[0].tolist() == [0.0, 0.0, 0.0]   # P + R = 0: F is 0
    # the signed field: no value in (-1, 1)
    neg, mag = O.signed_sq(block)
    assert np.array_equal(neg, block) and (mag >= 1).all() and mag[2, 2, 2] == 4 and mag[0, 0, 0] == 3


def test_header_binding_and_limits():
    from dpc.render import _native, voxeldist

    header = open(os.path.join(ROOT, "include", "dpc_render.h")).read()
    assert "#define DPC_VOXEL_EDT_NONE %d" % _native.DPC_VOXEL_EDT_NONE in header and _native.DPC_VOXEL_EDT_NONE == O.NONE
    assert "#define DPC_VOXEL_EDT_MAX_THRESHOLDS %d" % _native.DPC_VOXEL_EDT_MAX_THRESHOLDS in header
    assert _native.DPC_VOXEL_EDT_MAX_THRESHOLDS == O.MAX_THRESHOLDS == voxeldist.MAX_THRESHOLDS == 8 and voxeldist.NONE == O.NONE
    assert int(re.search(r"#define DPC_ABI_VERSION (\d+)", header).group(1)) == 15 == _native.lib().dpc_abi_version()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _native.SYMBOLS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, header), name


def test_public_names():
    import dpc.render as R

    for name in ("voxel_distance_transform", "voxel_signed_distance", "voxel_shell", "voxel_surface_stats", "voxel_fscore",
                 "voxel_fscore_of_split"):
        assert name in R.__all__ and callable(getattr(R, name)), name


def test_built_kernels_are_the_class_table_and_use_no_scratch():
    """The kernels of dpc_voxel_edt.o are the instantiations the GPU sweep must launch, and none of them spills."""
    from test_abi_and_host import device_object_output

    built = set()
    for line in device_object_output("dpc_voxel_edt.o", ["llvm-readelf", "-sW"]).splitlines():
        f = line.split()
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)(\w+)$", f[7]) if len(f) >= 8 and f[3] == "FUNC" else None
        if m:
            n = int(m.group(1))
            name, rest = m.group(2)[:n], m.group(2)[n:]
            targs = re.match(r"I((?:Li-?\d+E)+)E", rest)
            built.add(name + ("<%s>" % ", ".join(re.findall(r"Li(-?\d+)E", targs.group(1))) if targs else ""))
    assert built == INSTANTIATIONS, sorted(built ^ INSTANTIATIONS)
    notes = device_object_output("dpc_voxel_edt.o", ["llvm-readelf", "--notes"])
    scratch = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", notes)]
    assert len(scratch) == len(INSTANTIATIONS) and not any(scratch), scratch


def _tab(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))


def _p(t):
    return t.ctypes.data_as(ctypes.c_void_p)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every entry point with NULL device pointers: DPC_ERR_SHAPE for what the header lists, DPC_ERR_NULL (nothing
    launched) for valid arguments, DPC_OK for zero items; a shape error wins over a NULL pointer."""
    from dpc.render import _native

    L, SHAPE, NUL, S = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL, _native.DPC_VOXEL_MAX_SIDE
    N = None
    word = np.zeros(4, dtype=np.uint32)
    thr = lambda v: _p(np.ascontiguousarray(np.asarray(v, dtype=np.int32)))
    stats = lambda rows, n_fields, n_grids, t=(1,), D=4, H=4, W=4, pairs=None, K=None: L.dpc_voxel_edt_stats(
        N, n_fields, N, n_grids, D, H, W, N, _p(_tab(rows)) if len(rows) else N, len(rows) if pairs is None else pairs,
        thr(t) if len(t) else N, len(t) if K is None else K, N, N, N)

    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (S + 1, 4, 4), (4, S + 1, 4), (4, 4, S + 1), (-1, 4, 4)):
        for of_clear in (0, 1):
            assert L.dpc_voxel_edt(N, 2, bad[0], bad[1], bad[2], of_clear, N, N) == SHAPE, bad
        assert L.dpc_voxel_shell(N, 2, bad[0], bad[1], bad[2], N, N) == SHAPE, bad
        assert stats([(0, 0)], 1, 1, D=bad[0], H=bad[1], W=bad[2]) == SHAPE, bad
        assert L.dpc_voxel_edt(N, 0, bad[0], bad[1], bad[2], 0, N, N) == SHAPE      # also with nothing to do

    for sides in ((4, 4, 4), (1, 1, 1), (S, S, S), (1, S, 1)):
        assert L.dpc_voxel_edt(N, 2, *sides, 0, N, N) == NUL and L.dpc_voxel_edt(N, 2, *sides, 1, N, N) == NUL
        assert L.dpc_voxel_edt(_p(word), 2, *sides, 0, N, N) == NUL and L.dpc_voxel_edt(N, 2, *sides, 0, _p(word), N) == NUL
        assert L.dpc_voxel_shell(N, 2, *sides, N, N) == NUL and L.dpc_voxel_shell(_p(word), 2, *sides, N, N) == NUL
        assert L.dpc_voxel_edt(N, 0, *sides, 0, N, N) == 0 and L.dpc_voxel_shell(N, 0, *sides, N, N) == 0
    assert L.dpc_voxel_edt(N, -1, 4, 4, 4, 0, N, N) == SHAPE and L.dpc_voxel_shell(N, -1, 4, 4, 4, N, N) == SHAPE
    # in place: refused before anything is launched (both pointers are host memory here: nothing may touch them)
    assert L.dpc_voxel_shell(_p(word), 1, 1, 1, 4, _p(word), N) == SHAPE
    assert L.dpc_voxel_shell(_p(word), 0, 1, 1, 4, _p(word), N) == 0

    assert stats([(0, 0), (0, 1), (2, 1)], 3, 2) == NUL                              # pairs share a field and a grid
    assert stats([(0, 0)], 1, 1, t=()) == NUL and stats([(0, 0)], 1, 1, t=(0,) * 8) == NUL      # K = 0 and K = 8
    assert stats([(0, 0)], 1, 1, t=(0, O.NONE - 1)) == NUL
    assert stats([], 0, 0) == 0 and stats([], 3, 2, t=()) == 0
    assert stats([], 3, 2, pairs=-1) == SHAPE and stats([(0, 0)], -1, 2) == SHAPE and stats([(0, 0)], 3, -1) == SHAPE
    assert stats([(0, 0)], 1, 1, t=(0,) * 9) == SHAPE and stats([(0, 0)], 1, 1, K=-1) == SHAPE   # K out of range
    assert stats([(0, 0)], 1, 1, t=(1, -1)) == SHAPE and stats([(0, 0)], 1, 1, t=(O.NONE,)) == SHAPE
    assert stats([], 0, 0, t=(-1,)) == SHAPE                                        # checked with nothing to do, too
    assert stats([(3, 0)], 3, 2) == SHAPE and stats([(0, 2)], 3, 2) == SHAPE and stats([(-1, 0)], 3, 2) == SHAPE
    assert stats([(0, -1)], 3, 2) == SHAPE
    # host tables that have entries but are NULL: DPC_ERR_NULL, behind the sizes
    assert L.dpc_voxel_edt_stats(N, 3, N, 2, 4, 4, 4, N, N, 1, thr((1,)), 1, N, N, N) == NUL
    assert L.dpc_voxel_edt_stats(N, 3, N, 2, 4, 4, 4, N, _p(_tab([(0, 0)])), 1, N, 1, N, N, N) == NUL
    assert L.dpc_voxel_edt_stats(N, 3, N, 2, 4, 4, 4, N, N, 1, N, 9, N, N, N) == SHAPE


def test_python_refusals_come_before_any_launch():
    """Every refusal is a ValueError raised before a device is looked for (this machine may have none)."""
    import dpc.render as R

    cloud = np.zeros((4, 3), dtype=np.float32)
    f = lambda *s: np.zeros(s, dtype=np.float32)
    b = lambda *s: np.zeros(s, dtype=bool)
    big = R.voxels.MAX_SIDE + 1
    for fn in (R.voxel_distance_transform, R.voxel_signed_distance, R.voxel_shell):
        with pytest.raises(ValueError, match=r"grids must be \[B,D,H,W\]"):
            fn(f(4, 4, 4))
        with pytest.raises(ValueError, match=r"grids must be \[B,D,H,W\]"):
            fn([f(4, 4, 4)])
        with pytest.raises(ValueError, match="grids must be a float32 / float64 / bool / uint8 grid, got torch.int64"):
            fn(np.zeros((1, 4, 4, 4), dtype=np.int64))
        with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
            fn(b(1, 2, big, 2))
        with pytest.raises(ValueError, match="an empty side"):
            fn(f(1, 2, 0, 2))
        with pytest.raises(ValueError, match="threshold must be a number"):
            fn(f(1, 4, 4, 4), threshold="half")
        with pytest.raises(ValueError, match="threshold must not be NaN"):
            fn(f(1, 4, 4, 4), threshold=float("nan"))
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn(torch.zeros(1, 4, 4, 4))
    with pytest.raises(ValueError, match="to must be \"occupied\" or \"empty\""):
        R.voxel_distance_transform(f(1, 4, 4, 4), to="full")
    for fn in (R.voxel_surface_stats, R.voxel_fscore):
        for bad in ((), (1, -0.5), (1, float("inf")), (float("nan"),), (1,) * 9, None, 1.0, ("a",)):
            with pytest.raises(ValueError, match="thresholds must be a non-empty sequence of at most 8 non-negative finite"):
                fn(f(2, 4, 4, 4), b(2, 4, 4, 4), bad)
        with pytest.raises(ValueError, match=r"preds are grids of \(4, 4, 4\) and gts grids of \(4, 4, 5\)"):
            fn(f(2, 4, 4, 4), b(2, 4, 4, 5), [1])
        with pytest.raises(ValueError, match="clouds on both sides need vox_size"):
            fn([cloud], [cloud], [1])
        with pytest.raises(ValueError, match="2 predictions and 1 ground truths need gt_of"):
            fn(f(2, 4, 4, 4), b(1, 4, 4, 4), [1])
        with pytest.raises(ValueError, match="gt_of must map each of the 2 predictions to one of 1 ground truths"):
            fn(f(2, 4, 4, 4), b(1, 4, 4, 4), [1], gt_of=[0, 1])
        with pytest.raises(ValueError, match="preds must be a float32 / float64 grid, got torch.bool"):
            fn(b(2, 4, 4, 4), b(2, 4, 4, 4), [1])
        with pytest.raises(ValueError, match="gts must be a bool / uint8 grid, got torch.float32"):
            fn(f(2, 4, 4, 4), f(2, 4, 4, 4), [1])
        with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
            fn([cloud], [cloud], [1], vox_size=big)
        with pytest.raises(ValueError, match="threshold must not be NaN"):
            fn(f(2, 4, 4, 4), b(2, 4, 4, 4), [1], threshold=float("nan"))
        with pytest.raises(RuntimeError, match="MI355X only"):
            fn(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4, dtype=torch.bool), [1])
    pts = np.zeros((2, 50, 3), dtype=np.float32)
    split = R.voxel_fscore_of_split
    with pytest.raises(ValueError, match="thresholds must be a non-empty sequence"):
        split([(pts, None)], [cloud], [])
    with pytest.raises(ValueError, match="1 predictions and 2 GT clouds"):
        split([(pts, None)], [cloud, cloud], [1])
    with pytest.raises(ValueError, match="models_per_call must be >= 1"):
        split([(pts, None)], [cloud], [1], models_per_call=0)
    with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
        split([(pts, None)], [cloud], [1], vox_size=big)
    with pytest.raises(ValueError, match="vox_size must be an integer"):
        split([(pts, None)], [cloud], [1], vox_size=8.5)
    with pytest.raises(ValueError, match="same number of views"):
        split([(pts, None), (pts[:1], None)], [cloud, cloud], [1])
    with pytest.raises(ValueError, match=r"num_points must be 2 integers in \[0, 50\]"):
        split([(pts, np.array([10, 51]))], [cloud], [1])
    with pytest.raises(ValueError, match=r"reference_rotation must be a \[1,4\] quaternion"):
        split([(pts, None)], [cloud], [1], reference_rotation=np.zeros(4))
    with pytest.raises(ValueError, match=r"gt_clouds\[0\] must be \[n,3\]"):
        split([(pts, None)], [np.zeros((4, 2))], [1])
    empty = split([], [], [1, 2])
    assert empty["stats"].shape == (0, 0, 2, 5) and empty["fscore"].shape == (0, 0, 2, 3) and empty["dropped"].shape == (0, 0)
