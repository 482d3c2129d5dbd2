"""Clamp-mask words of k_splat_xl (csrc/dpc_slab_xl.hip): bit x of word (b, z, y) <=> raw[b, z, y, x] <= 1.

A wave of the kernel holds 16 grid rows of one plane and writes their 16 words in one store.  Waves in which no voxel
exceeds 1 take a wave-uniform short cut (all sixteen words are all-ones); the others write each row's ballot into its lane.
The inputs here give both kinds next to each other: stacks of 40 points on one voxel (raw far above 1 there and in the
voxel's neighbours) among 200 scattered points (raw far below 1), with stacks in the last row of a wave's 16-row segment
(y = 31, spilling into y = 32 of the neighbouring wave) and in the grid's last row and column (y = 63, x = 63).
D = 62 leaves the last slab of four planes with two: waves without a plane write nothing.

The reference is `raw <= 1` with raw from the stage-level splat (pointcloud2voxels3d_fast's dpc_splat_fwd) on the very
points the fused forward located (its tr_pc output).  dpc_project_fwd without a `raw` output on a 64 x 64 plane at tap radius
3 launches k_splat_xl (launch_splat, csrc/dpc_slab_fwd.hip); asked for `raw` it launches k_splat_hw, whose mask words are
compared as well.  No value of raw lies near 1 (asserted), so the comparison does not hang on a last bit."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G, NSTACK, NSCATTER = 64, 40, 200


@pytest.fixture(scope="module")
def R():
    import dpc.render as R

    return R


@pytest.fixture(scope="module")
def O():
    from oracle import dpc_oracle as O

    return O


def _points(cfg, D, stacks, nscatter, seed):
    """[NSTACK * len(stacks) + nscatter, 3] points (identity pose) whose grid coordinates are the stacks' (z, y, x) and
    uniformly scattered ones: the camera of the forward inverted in float64."""
    rng = np.random.RandomState(seed)
    g = np.concatenate([np.repeat(np.asarray(stacks, dtype=np.float64), NSTACK, axis=0),
                        rng.uniform(1.0, [D - 2, G - 2, G - 2], size=(nscatter, 3))])
    Z, Y, X = g[:, 0] / (D - 1) - 0.5, g[:, 1] / (G - 1) - 0.5, g[:, 2] / (G - 1) - 0.5
    f, d = float(getattr(cfg, "focal_length", 1.875)), float(getattr(cfg, "camera_distance", 2.0))
    return np.stack([Z, Y * (Z + d) / f, X * (Z + d) / f], axis=1)


@pytest.mark.parametrize("D", [64, 62])
def test_mask_words_equal_raw_le_one(R, O, D):
    from dpc.render import _native as N, _geometry
    from dpc.render._ops import _new_cells

    cfg = O.Cfg(vox_size=G, pc_gauss_kernel_size=21)
    geom = _geometry(cfg, R.smoothing_kernel(cfg, 0.64))
    # cloud 0: one stack near voxel (5, 17, 40); cloud 1: one in the last row of a wave's segment, one in the last row and column
    clouds = [_points(cfg, D, [(5.1, 17.25, 40.25)], NSCATTER + NSTACK, 1),
              _points(cfg, D, [(D - 2 + 0.1, 31.25, 10.25), (D - 2 + 0.1, 62.75, 62.75)], NSCATTER, 2)]
    pc = torch.tensor(np.stack(clouds), dtype=torch.float32, device="cuda")
    B, Np = pc.shape[0], pc.shape[1]
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]] * B, device="cuda")
    s = torch.ones(B, 1, device="cuda")
    P = geom.params(B, Np)
    P.D = D
    L = N.lib()
    assert L.dpc_taps_bucket(geom.kern_ptrs()[0], P.taps_xy) == 3 and L.dpc_mask_words_per_plane(ctypes.byref(P)) == G
    kxy, kz = geom.kern_ptrs()
    f = lambda *sh: torch.empty(sh, dtype=torch.float32, device="cuda")

    def forward(want_raw):
        tr, wh, proj, trans = f(B, Np, 3), f(B, D, G, G), f(B, G, G), f(B, G, G)
        raw = f(B, D, G, G) if want_raw else None
        mask = torch.full((B, D, G), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        rc = L.dpc_project_fwd(ctypes.byref(P), N.ptr(pc), N.ptr(q), None, None, N.ptr(s), kxy, kz, N.ptr(tr), N.ptr(_new_cells(P, pc.device)),
                               None if raw is None else N.ptr(raw), N.ptr(wh), None, N.ptr(mask), N.ptr(proj), N.ptr(trans),
                               N.stream_ptr(pc.device))
        assert rc == 0
        torch.cuda.synchronize()
        return tr, mask.cpu().numpy().view(np.uint64)

    tr, words_xl = forward(False)    # k_splat_xl
    _, words_hw = forward(True)      # k_splat_hw
    raw = f(B, D, G, G)
    rc = L.dpc_splat_fwd(ctypes.byref(P), N.ptr(tr), 0, N.ptr(_new_cells(P, pc.device)), N.ptr(raw), N.stream_ptr(pc.device))
    assert rc == 0
    torch.cuda.synchronize()
    raw = raw.cpu().numpy()
    assert not ((raw > 0.9) & (raw < 1.1)).any(), "a voxel near the threshold: the comparison would hang on its last bit"
    passes = raw <= 1.0
    want = np.packbits(passes.reshape(B, D, G, G), axis=-1, bitorder="little").view(np.uint64).reshape(B, D, G)
    # the inputs do what the docstring says: a few waves (plane, 16 rows) with a cleared bit, most without
    waves = passes.reshape(B, D, G // 16, 16 * G).all(axis=-1)
    assert 3 <= (~waves).sum() <= 16 and waves.sum() > 0.9 * waves.size, ((~waves).sum(), waves.size)
    assert not passes[0, 5, 17, 40] and not passes[1, D - 2, 31, 10] and not passes[1, D - 2, 32, 10] and not passes[1, D - 1, 63, 63]
    for name, words in (("k_splat_xl", words_xl), ("k_splat_hw", words_hw)):
        bad = np.argwhere(words != want)
        assert bad.size == 0, "%s: %d mask words differ from raw <= 1, first (b, z, y) = %s: %016x != %016x" % (
            name, len(bad), bad[0], words[tuple(bad[0])], want[tuple(bad[0])])
