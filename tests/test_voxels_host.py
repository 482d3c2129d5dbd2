"""Host-side checks of the voxel-grid evaluation (no GPU): the numpy oracle (tests/voxels_oracle.py) against what the
reference's util/voxel.py returned (fixture f25_voxels.npz, byte for byte) and against closed forms, the transpose relation
of voxel2pc, every refusal of the Python layer and of the dpc_voxel* entry points before any launch, and the exported
symbols."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import voxels_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "f25_voxels.npz")
ENTRY_POINTS = ("dpc_voxelise", "dpc_voxel_threshold", "dpc_voxel_unpack", "dpc_voxel_stats", "dpc_voxel_count", "dpc_voxel2pc")


def test_oracle_equals_the_reference_fixture_byte_for_byte():
    f = np.load(GOLDEN)
    cases = list(O.golden_cases())
    assert len(cases) == 16 and {c[1] for c in cases} == {2, 3, 5, 33}
    for key, G, thr, dtype, seed in cases:
        voxels, preds, gt = O.golden_inputs(G, seed, dtype)
        assert int(f[key + "/seed"]) == seed
        assert f[key + "/inputs"].tolist() == [O.digest(voxels), O.digest(preds), O.digest(gt)], key
        xyz, occ = O.voxel2pc(voxels, thr)
        assert xyz.dtype == np.float64 and list(xyz.shape) == f[key + "/xyz_shape"].tolist(), key
        assert O.digest(xyz) == str(f[key + "/xyz_digest"]), key
        if G <= 5:
            assert xyz.tobytes() == f[key + "/xyz"].tobytes(), key
        assert occ.dtype == bool and np.packbits(occ).tobytes() == f[key + "/occupancies"].tobytes(), key
        assert O.evaluate_voxel_prediction(preds, gt, thr).tolist() == f[key + "/sums"].tolist(), key


def test_oracle_closed_forms():
    # the nearest node: the cube's corners, the centre, points half-way between nodes (they go up), the outlier filter
    g, dropped = O.voxelise(np.array([[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [0.51, 0, 0], [np.nan, 0, 0]]), (3, 3, 3))
    assert dropped == 2 and sorted(map(tuple, np.argwhere(g))) == [(0, 0, 0), (1, 1, 1), (2, 2, 2)]
    valid, idx = O.nodes(np.array([[-0.25, 0.25, 0.0]]), (3, 5, 2))       # t = (0.5, 3.0, 0.5): floor(t + 0.5) = (1, 3, 1)
    assert valid.all() and idx.tolist() == [[1, 3, 1]]
    assert O.voxelise(np.zeros((4, 3)), (1, 1, 1))[0].all()               # one node: everything inside lands on it
    f32 = O.cloud(500, 3, np.float32, (9, 9, 9))
    assert (O.voxelise(f32, (9, 9, 9))[0] == O.voxelise(f32.astype(np.float64), (9, 9, 9))[0]).all()
    # bits: 27 voxels are one word with five padding bits; voxel f is bit f & 31 of word f >> 5
    assert O.pack_bits(np.ones((3, 3, 3), bool)).tolist() == [(1 << 27) - 1]
    m = np.zeros((2, 4, 8), bool)
    m[1, 0, 1] = m[0, 0, 0] = True
    assert O.pack_bits(m).tolist() == [1, 2]
    # thresholds in the grid's dtype: float32(0.3) > 0.3, so a float32 voxel at float32(0.3) is occupied for >= and not for >,
    # where a comparison in fp64 would call it occupied
    v = np.array([np.float32(0.3), np.nextafter(np.float32(0.3), np.float32(1)), np.nan], dtype=np.float32)
    assert O.threshold(v, 0.3, True).tolist() == [True, True, False] and O.threshold(v, 0.3, False).tolist() == [False, True, False]
    assert (v.astype(np.float64) > 0.3).tolist() == [True, True, False] and float(np.float32(0.3)) > 0.3   # fp64 would differ
    p, q = np.array([1, 1, 0, 0], bool), np.array([1, 0, 1, 0], bool)
    assert O.stats(p, q).tolist() == [2, 1, 3, 1, 1] and O.iou(O.stats(p, q)) == 1 / 3
    assert np.isnan(O.iou(O.stats(~p & p, ~q & q)))
    assert O.axis_coordinates(5).tobytes() == np.linspace(-0.5, 0.5, 5).tobytes()
    for G in (2, 3, 33, 64, 128):
        assert O.axis_coordinates(G).tobytes() == np.linspace(-0.5, 0.5, G).tobytes(), G


@pytest.mark.parametrize("G", [2, 3, 5, 33])
def test_voxelising_the_points_of_voxel2pc_gives_the_transposed_mask(G):
    v = O.float_grids(1, (G, G, G), 40 + G, np.float32)[0]
    for thr in (0.3, 0.5):
        xyz, occ = O.voxel2pc(v, thr)
        grid, dropped = O.voxelise(xyz, (G, G, G))
        assert dropped == 0 and len(xyz) == occ.sum()
        assert (grid == occ.reshape(G, G, G).transpose(1, 0, 2)).all()
        assert (occ.reshape(G, G, G) == O.threshold(v, thr, False)).all()


def _tab(rows):
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))


def _p(t):
    return t.ctypes.data_as(ctypes.c_void_p)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every dpc_voxel* entry point with NULL device pointers: DPC_ERR_SHAPE for what the header lists, DPC_ERR_NULL
    (nothing launched) for valid arguments, DPC_OK for zero items."""
    from dpc.render import _native

    L, SHAPE, NUL, S = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL, _native.DPC_VOXEL_MAX_SIDE
    N = None
    vox = lambda rows, n_pts, D=4, H=4, W=4, clouds=None: L.dpc_voxelise(
        N, n_pts, 0, N, _p(_tab(rows)) if len(rows) else N, len(rows) if clouds is None else clouds, D, H, W, N, N, N, N)
    assert vox([(0, 5), (5, 0), (2, 3)], 5) == NUL                    # an empty cloud and shared rows are fine
    assert vox([(0, 5)], 5, S, S, S) == NUL and vox([(0, 5)], 5, 1, 1, 1) == NUL
    assert vox([], 0) == 0
    assert L.dpc_voxelise(N, 5, 0, N, N, 1, 4, 4, 4, N, N, N, N) == NUL
    assert vox([(0, 5)], -1) == SHAPE and vox([], 0, clouds=-1) == SHAPE
    assert vox([(0, 5)], 4) == SHAPE and vox([(1, 5)], 5) == SHAPE and vox([(-1, 5)], 5) == SHAPE and vox([(0, -1)], 5) == SHAPE
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (S + 1, 4, 4), (4, S + 1, 4), (4, 4, S + 1), (-1, 4, 4)):
        assert vox([(0, 5)], 5, *bad) == SHAPE, bad
        assert L.dpc_voxel_threshold(N, 0, 2, bad[0], bad[1], bad[2], 0.5, 1, N, N) == SHAPE
        assert L.dpc_voxel_unpack(N, 2, bad[0], bad[1], bad[2], N, N) == SHAPE
        assert L.dpc_voxel_count(N, 2, bad[0], bad[1], bad[2], N, N) == SHAPE
        assert L.dpc_voxel_stats(N, 1, N, 1, bad[0], bad[1], bad[2], N, _p(_tab([(0, 0)])), 1, N, N, N) == SHAPE

    for dtype in (0, 1, 2):
        assert L.dpc_voxel_threshold(N, dtype, 2, 4, 4, 4, 0.5, 0, N, N) == NUL
    assert L.dpc_voxel_threshold(N, 3, 2, 4, 4, 4, 0.5, 0, N, N) == SHAPE and L.dpc_voxel_threshold(N, -1, 2, 4, 4, 4, 0.5, 0, N, N) == SHAPE
    assert L.dpc_voxel_threshold(N, 0, 0, 4, 4, 4, 0.5, 0, N, N) == 0 and L.dpc_voxel_threshold(N, 0, -1, 4, 4, 4, 0.5, 0, N, N) == SHAPE

    assert L.dpc_voxel_unpack(N, 2, 4, 4, 4, N, N) == NUL and L.dpc_voxel_unpack(N, 0, 4, 4, 4, N, N) == 0
    assert L.dpc_voxel_unpack(N, -1, 4, 4, 4, N, N) == SHAPE
    assert L.dpc_voxel_count(N, 2, 4, 4, 4, N, N) == NUL and L.dpc_voxel_count(N, 0, 4, 4, 4, N, N) == 0
    assert L.dpc_voxel_count(N, -1, 4, 4, 4, N, N) == SHAPE

    st = lambda rows, n_pred, n_gt, pairs=None: L.dpc_voxel_stats(
        N, n_pred, N, n_gt, 4, 4, 4, N, _p(_tab(rows)) if len(rows) else N, len(rows) if pairs is None else pairs, N, N, N)
    assert st([(0, 0), (1, 0), (2, 1)], 3, 2) == NUL                  # views share a ground truth
    assert st([], 0, 0) == 0 and st([], 3, 2, pairs=-1) == SHAPE
    assert L.dpc_voxel_stats(N, 3, N, 2, 4, 4, 4, N, N, 1, N, N, N) == NUL
    assert st([(3, 0)], 3, 2) == SHAPE and st([(0, 2)], 3, 2) == SHAPE and st([(-1, 0)], 3, 2) == SHAPE and st([(0, -1)], 3, 2) == SHAPE
    assert st([(0, 0)], -1, 2) == SHAPE and st([(0, 0)], 3, -1) == SHAPE

    pc = lambda rows, G, n_out, B=None: L.dpc_voxel2pc(N, len(rows) if B is None else B, G, N, _p(_tab(rows)) if len(rows) else N,
                                                       n_out, N, N, N)
    assert pc([(0, 5), (5, 0), (7, 8)], 2, 15) == NUL                 # a gap in the output, an empty grid, a full one
    assert pc([], 4, 0) == 0 and pc([], 4, 0, B=-1) == SHAPE
    assert L.dpc_voxel2pc(N, 1, 4, N, N, 5, N, N, N) == NUL
    assert pc([(0, 5)], 1, 5) == SHAPE and pc([(0, 5)], 0, 5) == SHAPE and pc([(0, 5)], S + 1, 5) == SHAPE   # G = 1, beyond the limit
    assert pc([(0, 9)], 2, 9) == SHAPE                                # more points than the grid has voxels
    assert pc([(0, 5)], 4, 4) == SHAPE and pc([(0, 5)], 4, -1) == SHAPE and pc([(-1, 5)], 4, 9) == SHAPE and pc([(0, -1)], 4, 9) == SHAPE
    assert pc([(0, 5), (4, 5)], 4, 20) == SHAPE and pc([(5, 5), (0, 5)], 4, 20) == SHAPE     # overlapping, descending


def test_header_symbols_and_limit():
    from dpc.render import _native, voxels

    header = open(os.path.join(ROOT, "include", "dpc_render.h")).read()
    assert "#define DPC_VOXEL_MAX_SIDE %d" % _native.DPC_VOXEL_MAX_SIDE in header and _native.DPC_VOXEL_MAX_SIDE >= 128
    assert voxels.MAX_SIDE == _native.DPC_VOXEL_MAX_SIDE
    assert int(re.search(r"#define DPC_ABI_VERSION (\d+)", header).group(1)) == 15 == _native.lib().dpc_abi_version()
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in ENTRY_POINTS:
        assert name in _native.SYMBOLS and hasattr(lib, name) and re.search(r"\bint %s\(" % name, header), name


def test_public_names():
    import dpc.render as R

    for name in ("voxelise", "voxel_stats", "voxel_iou", "evaluate_voxel_prediction", "voxel2pc", "voxels2pc_batched", "iou_of_split",
                 "render_voxels"):
        assert name in R.__all__ and callable(getattr(R, name)), name


def test_built_instantiations_are_the_class_table():
    """The kernels of dpc_voxels.o are the instantiations the GPU sweep (tests/test_voxels_gpu.py) must launch."""
    from test_abi_and_host import device_object_output

    out = device_object_output("dpc_voxels.o", ["llvm-readelf", "-sW"])
    vox = re.findall(r"_ZN12_GLOBAL__N_110k_voxeliseILi(\d+)ELi(\d+)ELi(\d+)EEEv", out)
    assert {tuple(map(int, v)) for v in vox} == {(f, w, t) for f in (0, 1) for w, t in ((1024, 256), (8192, 512), (16384, 1024))}
    assert {int(d) for d in re.findall(r"_ZN12_GLOBAL__N_117k_voxel_thresholdILi(\d+)EEEv", out)} == {0, 1, 2}
    for name in ("14k_voxel_unpack", "13k_voxel_stats", "13k_voxel_count", "10k_voxel2pc"):
        assert "_ZN12_GLOBAL__N_1" + name + "E" in out, name


def test_python_refusals_come_before_any_launch():
    """Every refusal is a ValueError raised before a device is looked for (this machine may have none)."""
    import dpc.render as R

    cloud = np.zeros((4, 3), dtype=np.float32)
    f = lambda *s: np.zeros(s, dtype=np.float32)
    b = lambda *s: np.zeros(s, dtype=bool)
    big = R.voxels.MAX_SIDE + 1
    # voxelise
    with pytest.raises(ValueError, match=r"clouds\[1\] must be \[n,3\]"):
        R.voxelise([cloud, np.zeros((4, 2), dtype=np.float32)], 8)
    with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
        R.voxelise([cloud], big)
    with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
        R.voxelise([cloud], 8, vox_size_z=big)
    with pytest.raises(ValueError, match="an empty side"):
        R.voxelise([cloud], 0)
    with pytest.raises(ValueError, match="vox_size must be an integer"):
        R.voxelise([cloud], 8.5)
    # voxel_stats / voxel_iou
    for fn in (R.voxel_stats, R.voxel_iou):
        with pytest.raises(ValueError, match=r"preds are grids of \(4, 4, 4\) and gts grids of \(4, 4, 5\)"):
            fn(f(2, 4, 4, 4), b(2, 4, 4, 5))
        with pytest.raises(ValueError, match=r"ask for grids of \(8, 8, 8\), the grids given are \(4, 4, 4\)"):
            fn(f(2, 4, 4, 4), [cloud, cloud], vox_size=8)
        with pytest.raises(ValueError, match="clouds on both sides need vox_size"):
            fn([cloud], [cloud])
        with pytest.raises(ValueError, match="2 predictions and 1 ground truths need gt_of"):
            fn(f(2, 4, 4, 4), b(1, 4, 4, 4))
        for bad in ([0], [0, 1], [0, -1], [0, 0.5], [0, 0, 0]):
            with pytest.raises(ValueError, match="gt_of must map each of the 2 predictions to one of 1 ground truths"):
                fn(f(2, 4, 4, 4), b(1, 4, 4, 4), gt_of=bad)
        with pytest.raises(ValueError, match="preds must be a float32 / float64 grid, got torch.int64"):
            fn(np.zeros((2, 4, 4, 4), dtype=np.int64), b(2, 4, 4, 4))
        with pytest.raises(ValueError, match="preds must be a float32 / float64 grid, got torch.bool"):
            fn(b(2, 4, 4, 4), b(2, 4, 4, 4))
        with pytest.raises(ValueError, match="gts must be a bool / uint8 grid, got torch.float32"):
            fn(f(2, 4, 4, 4), f(2, 4, 4, 4))
        with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
            fn([cloud], [cloud], vox_size=big)
        with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
            fn(torch.zeros(1, 2, 2, big), [cloud])
        with pytest.raises(ValueError, match=r"preds must be a list of \[n,3\] clouds"):
            fn(f(4, 4), [cloud], vox_size=4)
    # voxel2pc, voxels2pc_batched, render_voxels
    for fn in (R.voxel2pc, R.render_voxels):
        with pytest.raises(ValueError, match="must squeeze to a cubic"):
            fn(f(1, 4, 4, 5), 0.5)
        with pytest.raises(ValueError, match="must squeeze to a cubic"):
            fn(f(4, 4), 0.5)
        with pytest.raises(ValueError, match="must squeeze to a cubic"):
            fn(f(1, 1, 1), 0.5)                                    # G = 1 squeezes to nothing, as in the reference
        with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
            fn(np.zeros((big, big, big), dtype=bool), 0.5)
    with pytest.raises(ValueError, match="G = 1"):
        R.voxels2pc_batched(f(2, 1, 1, 1), 0.5)
    with pytest.raises(ValueError, match="must squeeze to a cubic"):
        R.voxels2pc_batched(f(2, 4, 4, 5), 0.5)
    with pytest.raises(ValueError, match=r"voxels must be \[B,G,G,G\]"):
        R.voxels2pc_batched(f(4, 4, 4), 0.5)
    with pytest.raises(ValueError, match="must be float32, float64, integer or bool"):
        R.voxel2pc(np.zeros((4, 4, 4), dtype=np.float16), 0.5)
    # evaluate_voxel_prediction
    with pytest.raises(ValueError, match=r"must both be \[B,2,D,H,W\]"):
        R.evaluate_voxel_prediction(f(2, 2, 4, 4, 4), f(2, 2, 4, 4, 5), 0.5)
    with pytest.raises(ValueError, match=r"must both be \[B,2,D,H,W\]"):
        R.evaluate_voxel_prediction(f(2, 1, 4, 4, 4), f(2, 1, 4, 4, 4), 0.5)
    with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
        R.evaluate_voxel_prediction(torch.zeros(1, 2, 2, 2, big), torch.zeros(1, 2, 2, 2, big), 0.5)
    # iou_of_split
    pts = np.zeros((2, 50, 3), dtype=np.float32)
    with pytest.raises(ValueError, match="1 predictions and 2 GT clouds"):
        R.iou_of_split([(pts, None)], [cloud, cloud])
    with pytest.raises(ValueError, match="models_per_call must be >= 1"):
        R.iou_of_split([(pts, None)], [cloud], models_per_call=0)
    with pytest.raises(ValueError, match="a side above DPC_VOXEL_MAX_SIDE"):
        R.iou_of_split([(pts, None)], [cloud], vox_size=big)
    with pytest.raises(ValueError, match="same number of views"):
        R.iou_of_split([(pts, None), (pts[:1], None)], [cloud, cloud])
    with pytest.raises(ValueError, match=r"num_points must be 2 integers in \[0, 50\]"):
        R.iou_of_split([(pts, np.array([10, 51]))], [cloud])
    with pytest.raises(ValueError, match=r"reference_rotation must be a \[1,4\] quaternion"):
        R.iou_of_split([(pts, None)], [cloud], reference_rotation=np.zeros(4))
    with pytest.raises(ValueError, match=r"gt_clouds\[0\] must be \[n,3\]"):
        R.iou_of_split([(pts, None)], [np.zeros((4, 2))])
    # a CPU tensor is refused like everywhere in the package, after the argument checks
    with pytest.raises(RuntimeError, match="MI355X only"):
        R.voxel_stats(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 4, dtype=torch.bool))


def test_render_predictions_tool_takes_voxels_arguments():
    import importlib.util

    spec = importlib.util.spec_from_file_location("render_predictions", os.path.join(ROOT, "tools", "render_predictions.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    cfg = mod.parse_arguments(["--inp_dir=a", "--out_dir=b"])
    assert cfg.voxels is False and cfg.vis_threshold == 0.5
    cfg = mod.parse_arguments(["--inp_dir=a", "--out_dir=b", "--voxels", "--vis_threshold=0.3"])
    assert cfg.voxels is True and cfg.vis_threshold == 0.3
