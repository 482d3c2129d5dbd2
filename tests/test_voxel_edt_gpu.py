"""Voxel distance transforms on the GPU (csrc/dpc_voxel_edt.hip) against the numpy restatement of their rules
(tests/voxel_edt_oracle.py).  Everything is compared exactly: squared index distances, counts and int64 sums have one right
answer; the F-score's ratios are the same IEEE divisions on both sides.

The sweep of `sweep` runs once per module.  Shapes, the smallest at which each thing can break: the degenerate and
single-axis grids, (3,5,7) and (5,33,31) (rows straddle words, the total is no multiple of 32), (9,16,40), 32^3 / 33^3 and
64^3 / 65^3 (the last of a size class and the first of the next, for the plane pass and the depth pass), and 128^3 in a
test of its own.  Contents (voxel_edt_oracle.grid): empty, full, a voxel at each corner, one voxel alone, random at 5 % and
50 %, voxels only in the last d-plane; each with both seed modes.  The oracle is the brute-force definition for seed lists
of at most 4096 voxels and the separable numpy passes beyond (tests/test_voxel_edt_host.py shows the two equal)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import dpc.render as R
import voxel_edt_oracle as O
import voxels_oracle as VO
from dpc.render import _native
from test_voxel_edt_host import INSTANTIATIONS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 1), (1, 1, 128), (1, 128, 1), (128, 1, 1), (3, 5, 7), (5, 33, 31), (9, 16, 40),
          (32, 32, 32), (33, 33, 33), (64, 64, 64), (65, 65, 65)]
MODES = (("occupied", False), ("empty", True))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def shape_id(s):
    return "%dx%dx%d" % tuple(s)


def edt(g, of_clear=False):
    """The oracle: the definition itself while the seed list is short, the separable passes beyond."""
    return O.edt_brute(g, of_clear) if int(O.seeds_of(g, of_clear).sum()) <= 4096 else O.edt_separable(g, of_clear)


def grids_of(shape, seed=3):
    return np.stack([O.grid(shape, kind, seed) for kind in O.CONTENTS])


@pytest.fixture(scope="module")
def sweep():
    """({shape: {"occupied" | "empty": fields [7,D,H,W], "shell": [7,D,H,W]}}, the instantiations launched)."""
    out, launched = {}, set()
    R.check_status()
    for shape in SHAPES:
        g = dev(grids_of(shape))
        got = {}

        def run():
            for to, _ in MODES:
                sq = R.voxel_distance_transform(g, to=to)
                assert sq.dtype == torch.int32 and sq.is_cuda and tuple(sq.shape) == (len(O.CONTENTS),) + shape
                got[to] = sq.cpu().numpy()
            sh = R.voxel_shell(g)
            assert sh.dtype == torch.bool and sh.is_cuda and tuple(sh.shape) == tuple(g.shape)
            got["shell"] = sh.cpu().numpy()

        launched |= _native.launched_instantiations(run, torch.device("cuda"))
        out[shape] = got

    def stats():
        p = dev(VO.float_grids(2, (3, 5, 7), 1, np.float32))
        R.voxel_surface_stats(p, p >= 0.5, [1.0])

    launched |= _native.launched_instantiations(stats, torch.device("cuda"))
    assert R.check_status() == 0
    return out, launched


# 1 dpc_voxel_edt -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_fields_equal_the_oracle_in_both_seed_modes(sweep, shape):
    grids = grids_of(shape)
    for to, of_clear in MODES:
        for k, kind in enumerate(O.CONTENTS):
            want = edt(grids[k], of_clear)
            got = sweep[0][shape][to][k]
            assert np.array_equal(got, want), (shape, kind, to, int((got != want).sum()))
    assert (sweep[0][shape]["occupied"][0] == O.NONE).all() and (sweep[0][shape]["empty"][1] == O.NONE).all()   # no seed at all
    assert (sweep[0][shape]["occupied"][1] == 0).all() and (sweep[0][shape]["empty"][0] == 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_shells_equal_the_oracle(sweep, shape):
    grids = grids_of(shape)
    for k, kind in enumerate(O.CONTENTS):
        assert np.array_equal(sweep[0][shape]["shell"][k], O.shell(grids[k])), (shape, kind)


def test_the_sweep_launches_every_compiled_instantiation(sweep):
    """The instantiations in the launch record over the sweep == the launcher's class table, which
    tests/test_voxel_edt_host.py holds equal to the kernel symbols of dpc_voxel_edt.o: a size class added without a shape
    in SHAPES (or the 128^3 test) that reaches it fails here or there."""
    launched = {i for i in sweep[1] if i.startswith(("k_edt", "k_voxel_shell", "k_voxel_edt"))}
    big = {"k_edt_plane<128, 512>", "k_edt_depth<128>"}
    assert launched == INSTANTIATIONS, sorted(launched ^ INSTANTIATIONS)
    assert big <= launched          # (1,1,128), (1,128,1) and (128,1,1) reach the largest classes without a large grid


CASES_128 = ("far_corner", "sparse64", "dense5")


@pytest.mark.parametrize("case", CASES_128)
def test_the_largest_grid(case):
    """128^3: one seed in the far corner (3 * 127^2 = 48387 at the origin), 64 scattered seeds against brute force, and a
    dense grid against the separable oracle; the other seed mode of each is dense too."""
    shape = (128, 128, 128)
    if case == "far_corner":
        g = np.zeros(shape, dtype=bool)
        g[127, 127, 127] = True
    elif case == "sparse64":
        g = O.sparse_grid(shape, 64, 5)
    else:
        g = O.grid(shape, "rand5", 9)
    gd = dev(g[None])
    got = R.voxel_distance_transform(gd).cpu().numpy()[0]
    assert np.array_equal(got, edt(g))
    if case == "far_corner":
        assert got[0, 0, 0] == 48387 and got[127, 127, 127] == 0 and got.max() == 48387
    if case != "dense5":     # its complement is the same kind of case as dense5 itself
        assert np.array_equal(R.voxel_distance_transform(gd, to="empty").cpu().numpy()[0], O.edt_separable(g, True))


def raw_edt(bits, shape, of_clear, fill=-7):
    """dpc_voxel_edt itself on uint32 words [B, words]: int32 [B,D,H,W], written over `fill`."""
    b = dev(np.ascontiguousarray(bits).view(np.int32))
    sq = torch.full((len(bits),) + tuple(shape), fill, dtype=torch.int32, device="cuda")
    rc = _native.lib().dpc_voxel_edt(_native.ptr(b), len(bits), shape[0], shape[1], shape[2], of_clear, _native.ptr(sq),
                                     _native.stream_ptr(b.device))
    assert rc == 0
    return sq.cpu().numpy()


def raw_shell(bits, shape, fill=-1):
    b = dev(np.ascontiguousarray(bits).view(np.int32))
    out = torch.full(tuple(bits.shape), fill, dtype=torch.int32, device="cuda")
    rc = _native.lib().dpc_voxel_shell(_native.ptr(b), len(bits), shape[0], shape[1], shape[2], _native.ptr(out),
                                       _native.stream_ptr(b.device))
    assert rc == 0
    return out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (5, 33, 31), (33, 33, 33)], ids=shape_id)
def test_garbage_in_the_padding_bits_is_never_a_seed_and_never_written(shape):
    """The entry points on words whose padding bits are all ones: the fields of both modes are those of the clean words
    (an empty grid stays without a seed, a full grid has no clear voxel), and dpc_voxel_shell writes zero padding over a
    buffer of ones."""
    V = shape[0] * shape[1] * shape[2]
    assert V % 32
    grids = grids_of(shape, 4)
    clean = np.stack([O.pack_bits(g) for g in grids])
    dirty = clean.copy()
    dirty[:, -1] |= np.uint32((0xFFFFFFFF << (V % 32)) & 0xFFFFFFFF)
    for of_clear in (0, 1):
        got = raw_edt(dirty, shape, of_clear)
        for k, kind in enumerate(O.CONTENTS):
            assert np.array_equal(got[k], edt(grids[k], bool(of_clear))), (shape, kind, of_clear)
        assert np.array_equal(got, raw_edt(clean, shape, of_clear))
    assert (raw_edt(dirty, shape, 0)[0] == O.NONE).all() and (raw_edt(clean, shape, 1)[1] == O.NONE).all()
    for words in (clean, dirty):
        sh = raw_shell(words, shape)
        assert (sh[:, -1] >> np.uint32(V % 32) == 0).all()
        for k in range(len(grids)):
            assert sh[k].tobytes() == O.pack_bits(O.shell(grids[k])).tobytes(), (shape, k)


def test_one_call_or_one_grid_at_a_time():
    for shape in ((5, 33, 31), (33, 33, 33), (2, 65, 3)):
        g = dev(grids_of(shape, 6))
        for to, _ in MODES:
            both = R.voxel_distance_transform(g, to=to)
            rev = R.voxel_distance_transform(g.flip(0), to=to)
            for k in range(len(g)):
                assert torch.equal(R.voxel_distance_transform(g[k:k + 1], to=to)[0], both[k]) and torch.equal(rev[len(g) - 1 - k], both[k])
        shells = R.voxel_shell(g)
        for k in range(len(g)):
            assert torch.equal(R.voxel_shell(g[k:k + 1])[0], shells[k])
    assert R.check_status() == 0


def test_float_grids_are_thresholded_like_voxel_stats_and_roots_are_taken_in_fp64():
    shape = (9, 16, 40)
    for dtype in (np.float32, np.float64):
        v = VO.float_grids(3, shape, 21, dtype, occupancy=0.05)
        for thr in (0.3, 0.5):
            occ = VO.threshold(v, thr, True)                     # inclusive, in the grid's dtype; a NaN voxel is empty
            got = R.voxel_distance_transform(dev(v), threshold=thr).cpu().numpy()
            assert np.array_equal(got, np.stack([edt(o) for o in occ])), (dtype, thr)
    assert np.array_equal(R.voxel_distance_transform(dev(occ.astype(np.uint8) * 3)).cpu().numpy(), got)
    root = R.voxel_distance_transform(dev(occ), squared=False)
    assert root.dtype == torch.float64 and np.array_equal(np.rint(root.cpu().numpy() ** 2).astype(np.int32), got)
    none = R.voxel_distance_transform(dev(np.zeros((1,) + shape, dtype=bool)), squared=False)
    assert bool(torch.isinf(none).all()) and bool((none > 0).all())
    assert tuple(R.voxel_distance_transform(dev(np.zeros((0,) + shape, dtype=bool))).shape) == (0,) + shape


def test_fields_of_the_fixture_grids():
    f = np.load(os.path.join(ROOT, "tests", "golden", "f34_voxel_edt.npz"))
    for shape in O.GOLDEN_SHAPES:
        cases = [c for c in O.golden_cases() if c[1] == shape]
        bits = np.stack([f[c[0] + "/bits"] for c in cases])
        fields = [raw_edt(bits, shape, of_clear) for of_clear in (0, 1)]
        shells = raw_shell(bits, shape)
        for k, (key, _, _, g) in enumerate(cases):
            assert [O.digest(fields[0][k]), O.digest(fields[1][k])] == f[key + "/sq_digests"].tolist(), key
            assert shells[k].tobytes() == f[key + "/shell"].tobytes(), key


# 2 dpc_voxel_edt_stats ---------------------------------------------------------------------------------------------------
def raw_stats(sq, bits, shape, rows, thr, status=None, host_rows=None, fill=-7):
    """dpc_voxel_edt_stats itself: int64 [P, 3+K] written over `fill`."""
    desc = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))
    host = desc if host_rows is None else np.ascontiguousarray(np.asarray(host_rows, dtype=np.int32).reshape(-1, 2))
    thr = np.ascontiguousarray(np.asarray(thr, dtype=np.int32))
    out = torch.full((len(desc), 3 + len(thr)), fill, dtype=torch.int64, device="cuda")
    rc = _native.lib().dpc_voxel_edt_stats(_native.ptr(sq), int(sq.shape[0]), _native.ptr(bits), int(bits.shape[0]), shape[0],
                                           shape[1], shape[2], _native.ptr(dev(desc)), host.ctypes.data_as(ctypes.c_void_p),
                                           len(desc), thr.ctypes.data_as(ctypes.c_void_p) if len(thr) else None, len(thr),
                                           _native.ptr(out), _native.ptr(status), _native.stream_ptr(sq.device))
    assert rc == 0
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", [(5, 33, 31), (33, 33, 33)], ids=shape_id)      # 160 words: one round a wave; 1124: five
def test_stats_of_pairs_that_share_fields_for_every_threshold_count_and_a_bad_device_row(shape):
    grids = [O.grid(shape, "rand5", 1), O.grid(shape, "rand50", 2), np.zeros(shape, dtype=bool)]
    words = np.stack([O.pack_bits(g) for g in grids])
    words[:, -1] |= np.uint32((0xFFFFFFFF << (shape[0] * shape[1] * shape[2] % 32)) & 0xFFFFFFFF)      # padding bits are not voxels
    fields = raw_edt(words, shape, 0)
    assert (fields[2] == O.NONE).all()
    sq, bits = dev(fields), dev(words.view(np.int32))
    rows = [(0, 1), (0, 0), (1, 0), (2, 1), (0, 2), (0, 1)]          # field 0 serves four pairs; field 2 has no seed; grid 2 is empty
    top = int(fields[0].max())
    for thr in ([], [0], [0, 1, 2, 4, 9, top, top + 1, O.NONE - 1]):   # K = 0, 1 and 8; 0, and beyond the grid's largest value
        got = raw_stats(sq, bits, shape, rows, thr)
        want = np.stack([O.edt_stats(fields[a], grids[b], thr) for a, b in rows])
        assert got.dtype == np.int64 and np.array_equal(got, want), thr
    assert want[3].tolist() == [int(grids[1].sum())] + [0] * 10 and want[4].tolist() == [0] * 11 and want[1][2] == 0
    assert want[0][3 + 4] < want[0][0] and want[0][3 + 5] == want[0][3 + 6] == want[0][3 + 7] == want[0][0] == want[0][1]
    # a device row that names a field that is not there: flagged, its output row untouched, the others unaffected
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    bad = list(rows)
    bad[1], bad[4] = (3, 0), (0, -1)
    got = raw_stats(sq, bits, shape, bad, [0, 4], status, host_rows=rows)
    assert status.item() == _native.DPC_STATUS_BAD_INDEX
    want = np.stack([O.edt_stats(fields[a], grids[b], [0, 4]) for a, b in rows])
    assert (got[1] == -7).all() and (got[4] == -7).all() and np.array_equal(got[[0, 2, 3, 5]], want[[0, 2, 3, 5]])


# 3 the Python layer ----------------------------------------------------------------------------------------------------
def test_surface_stats_and_fscore_equal_the_oracle_with_empty_sides():
    shape = (9, 16, 40)
    taus = [0, 0.5, 1, 1.5, 2, 3, 5, 100]
    thr = O.thresholds_sq(taus)
    preds = VO.float_grids(5, shape, 31, np.float32, occupancy=0.1)
    preds[3] = 0.0                                                    # an empty prediction
    gts = np.stack([O.ball(shape, (4, 8, 20), 4), O.grid(shape, "rand5", 8), np.zeros(shape, dtype=bool)])
    gt_of = [0, 1, 1, 0, 2]                                           # views share a ground truth; pair 4 has an empty one
    occ = VO.threshold(preds, 0.5, True)
    for surface in (True, False):
        got = R.voxel_surface_stats(dev(preds), dev(gts), taus, gt_of=gt_of, surface=surface)
        assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == (5, 2, 11)
        want = np.stack([O.surface_stats(occ[i], gts[k], thr, surface, edt=edt) for i, k in enumerate(gt_of)])
        assert np.array_equal(got.cpu().numpy(), want), surface
        fs = R.voxel_fscore(dev(preds), dev(gts), taus, gt_of=gt_of, surface=surface)
        assert fs.dtype == torch.float64 and tuple(fs.shape) == (5, 8, 3)
        assert np.array_equal(fs.cpu().numpy(), O.fscore(want), equal_nan=True), surface
    fs = fs.cpu().numpy()
    assert np.isnan(fs[3, :, 0]).all() and (fs[3, :, 1] == 0).all() and np.isnan(fs[3, :, 2]).all()    # nothing predicted
    assert (fs[4, :, 0] == 0).all() and np.isnan(fs[4, :, 1]).all()                                    # nothing to find
    assert (fs[0, -1] == 1).all() and 0 < fs[0, 2, 2] < 1
    # clouds on the prediction side, voxelised like voxelise; another threshold for float predictions
    clouds = [VO.cloud(n, 40 + n, np.float32, shape) for n in (300, 0, 1200)]
    got = R.voxel_surface_stats([dev(c) for c in clouds], dev(gts), [1, 2], gt_of=[0, 0, 1])
    want = np.stack([O.surface_stats(VO.voxelise(c, shape)[0], gts[k], O.thresholds_sq([1, 2]), edt=edt) for c, k in zip(clouds, [0, 0, 1])])
    assert np.array_equal(got.cpu().numpy(), want)
    got = R.voxel_surface_stats(dev(preds[:2]), dev(gts[:2]), [1], threshold=0.3)
    want = np.stack([O.surface_stats(VO.threshold(preds[i], 0.3, True), gts[i], O.thresholds_sq([1]), edt=edt) for i in range(2)])
    assert np.array_equal(got.cpu().numpy(), want)
    assert tuple(R.voxel_fscore([], [], [1], vox_size=4).shape) == (0, 1, 3)
    assert R.check_status() == 0


def test_fscore_of_a_grid_with_itself_and_of_a_shell_shifted_by_one_voxel():
    shape = (24, 24, 24)
    a, b = O.ball(shape, (12, 12, 12), 7), O.ball(shape, (12, 12, 13), 7)
    same = R.voxel_fscore(dev(a[None].astype(np.float32)), dev(a[None]), [0, 0.5, 1]).cpu().numpy()
    assert (same == 1.0).all()
    # every shell voxel has its shifted copy at distance exactly 1: some coincide with other shell voxels, not all
    fs = R.voxel_fscore(dev(a[None].astype(np.float64)), dev(b[None]), [0.5, 1]).cpu().numpy()[0]
    assert (0 < fs[0]).all() and (fs[0] < 1).all() and fs[1].tolist() == [1.0, 1.0, 1.0]
    stats = R.voxel_surface_stats(dev(a[None].astype(np.float32)), dev(b[None]), [1]).cpu().numpy()[0]
    n = int(O.shell(a).sum())
    assert stats[:, 0].tolist() == [n, n] and stats[:, 1].tolist() == [n, n] and stats[:, 3].tolist() == [n, n]
    assert (stats[:, 2] < n).all() and (stats[:, 2] > 0).all()        # sum of squares: 0 or 1 per voxel


def test_signed_distance_sign_and_squared_magnitude():
    """The sign and rint(sd^2) against the integer fields, so nothing rests on how a square root rounds."""
    shape = (9, 16, 40)
    grids = grids_of(shape, 12)
    sd = R.voxel_signed_distance(dev(grids))
    assert sd.dtype == torch.float64 and sd.is_cuda and tuple(sd.shape) == grids.shape
    sd = sd.cpu().numpy()
    for k, kind in enumerate(O.CONTENTS):
        neg, mag = O.signed_sq(grids[k], edt=edt)
        assert np.array_equal(np.signbit(sd[k]), neg), kind
        finite = mag != O.NONE
        assert np.array_equal(np.isinf(sd[k]), ~finite), kind
        assert np.array_equal(np.rint(sd[k][finite] ** 2).astype(np.int64), mag[finite]), kind
    assert (sd[0] == np.inf).all() and (sd[1] == -np.inf).all() and not ((sd > -1) & (sd < 1)).any()
    f32 = VO.float_grids(2, shape, 3, np.float32, occupancy=0.3)
    got = R.voxel_signed_distance(dev(f32), threshold=0.3).cpu().numpy()
    assert np.array_equal(np.signbit(got), VO.threshold(f32, 0.3, True))


def test_fscore_of_split_does_not_depend_on_the_grouping():
    """3 models x 2 views on a 16^3 grid, one model with truncated views: models_per_call 1 and 256 agree bit for bit and
    equal the oracle on the voxelised views."""
    M, V, N, G = 3, 2, 300, 16
    preds, gts = O.clouds_of_split(M, V, N, 14)
    taus = [0.5, 1, 2]
    R.check_status()
    got = R.voxel_fscore_of_split(preds, gts, taus, vox_size=G, models_per_call=256)
    one = R.voxel_fscore_of_split(preds, gts, taus, vox_size=G, models_per_call=1)
    assert got["stats"].shape == (M, V, 2, 6) and got["stats"].dtype == np.int64 and got["fscore"].shape == (M, V, 3, 3)
    assert got["fscore"].dtype == np.float64 and got["dropped"].shape == (M, V) and got["dropped"].dtype == np.int64
    for k in ("stats", "fscore", "dropped"):
        assert got[k].tobytes() == one[k].tobytes(), k
    thr = O.thresholds_sq(taus)
    for m in range(M):
        gt_vox = VO.voxelise(gts[m], (G, G, G))[0]
        for i in range(V):
            n = N if preds[m][1] is None else int(preds[m][1][i])
            vox, dropped = VO.voxelise(preds[m][0][i][:n], (G, G, G))
            want = O.surface_stats(vox, gt_vox, thr, edt=edt)
            assert np.array_equal(got["stats"][m, i], want) and got["dropped"][m, i] == dropped, (m, i)
            assert np.array_equal(got["fscore"][m, i], O.fscore(want), equal_nan=True), (m, i)
    assert np.isnan(got["fscore"][1, 1, :, 0]).all() and (got["fscore"][0, :, -1, 2] > 0.5).all()
    solid = R.voxel_fscore_of_split(preds, gts, taus, vox_size=G, vox_size_z=8, surface=False)
    want = O.surface_stats(VO.voxelise(preds[0][0][0], (8, G, G))[0], VO.voxelise(gts[0], (8, G, G))[0], thr, False, edt=edt)
    assert np.array_equal(solid["stats"][0, 0], want)
    assert R.check_status() == 0
