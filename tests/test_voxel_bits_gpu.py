"""GPU checks of what the voxel kernels share, against closed forms: the dynamic-LDS limit of the mesh-voxel kernels
(csrc/dpc_launch.h, set_lds) over grid sizes that grow and shrink within one process, and the masked word
(csrc/dpc_voxel_bits.h, voxel_word) of a grid whose voxel count is no multiple of 32."""
import ctypes

import numpy as np
import pytest
import torch

import dpc.render as R
import mesh_voxels_oracle as MO
import voxel_edt_oracle as EO
import voxels_oracle as VO
from dpc.render import _native

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def solid_box(G):
    """(the nodes G/4 .. G - G/4 of a G^3 grid on every axis, the same without its interior: a shell one node thick)."""
    a, b = G // 4, G - G // 4
    solid = np.zeros((G, G, G), dtype=bool)
    solid[a:b + 1, a:b + 1, a:b + 1] = True
    shell = solid.copy()
    shell[a + 1:b, a + 1:b, a + 1:b] = False
    return solid, shell


@pytest.mark.parametrize("sides", [(8, 128, 8), (40, 128, 40)], ids=str)
def test_the_lds_limit_follows_a_size_that_grows_and_shrinks(sides):
    """carve_voxels of a hollow box shell is the solid box, and voxelise_meshes(fill="parity") of the 12-face cube through
    the same node centres is the solid box too ((b - a + 1)^3 nodes, the count of
    test_mesh_voxels_host.test_the_cube_through_node_centres), at a small grid, the largest, and the small one again.
    (8, 128, 8) goes from the 256-thread kernels with under 1 KiB of LDS to the 1024-thread ones with 64 KiB and back;
    (40, 128, 40) stays in the 1024-thread kernels, whose limit is first set to 26 KiB, raised, and then left alone."""
    carved, filled = [], []
    for G in sides:
        solid, shell = solid_box(G)
        got = R.carve_voxels(dev(shell[None]))[0].cpu().numpy()
        assert np.array_equal(got, solid), G
        carved.append(got)
    for G in sides:
        a, b = G // 4, G - G // 4
        grids, info = R.voxelise_meshes([MO.node_box((a,) * 3, (b,) * 3, (G,) * 3)], G, fill="parity", return_info=True)
        got = grids[0].cpu().numpy()
        assert got.sum() == (b - a + 1) ** 3 and np.array_equal(got, solid_box(G)[0]), G
        assert info.cpu().numpy().tolist() == [[0, 0]]
        filled.append(got)
    for runs in (carved, filled):
        assert np.array_equal(runs[0], runs[2]) and runs[1].sum() == 65 ** 3
    assert R.check_status() == 0


def test_padding_bits_of_a_5x3x7_grid_are_not_voxels():
    """105 voxels: four words, the last with 23 padding bits, all set.  dpc_voxel_count, dpc_voxel_stats of the grids against
    themselves and each other, and dpc_voxel_edt_stats (what voxel_surface_stats is made of) give the counts of the clean
    words; the fields are brute force on the host, so nothing but the masked word is under test."""
    shape, L = (5, 3, 7), _native.lib()
    V = 105
    grids = [EO.grid(shape, kind, 3) for kind in ("empty", "full", "rand50", "last_plane", "single")]
    assert grids[1].reshape(-1)[96:].all() and grids[3].reshape(-1)[96:].any()     # voxels in the last word, next to the padding
    clean = np.stack([VO.pack_bits(g) for g in grids])
    dirty = clean.copy()
    dirty[:, -1] |= np.uint32((0xFFFFFFFF << (V % 32)) & 0xFFFFFFFF)
    assert clean.shape == (5, 4) and (dirty[:, -1] != clean[:, -1]).all()
    pairs = np.ascontiguousarray(np.array([(i, j) for i in range(5) for j in range(5)], dtype=np.int32))
    thr = np.array([1, 4], dtype=np.int32)
    fields = np.stack([EO.edt_brute(g) for g in grids])
    stream = _native.stream_ptr(torch.device("cuda"))
    for words in (clean, dirty):
        bits, pairs_d = dev(words.view(np.int32)), dev(pairs)
        counts = torch.full((5,), -7, dtype=torch.int32, device="cuda")
        assert L.dpc_voxel_count(_native.ptr(bits), 5, *shape, _native.ptr(counts), stream) == 0
        assert counts.cpu().numpy().tolist() == [int(g.sum()) for g in grids]
        stats = torch.full((25, 5), -7, dtype=torch.int64, device="cuda")
        assert L.dpc_voxel_stats(_native.ptr(bits), 5, _native.ptr(bits), 5, *shape, _native.ptr(pairs_d),
                                 pairs.ctypes.data_as(ctypes.c_void_p), 25, _native.ptr(stats), None, stream) == 0
        stats = stats.cpu().numpy()
        for (i, j), row in zip(pairs, stats):
            assert row.tolist() == VO.stats(grids[i], grids[j]).tolist(), (i, j)
            if i == j:
                n = int(grids[i].sum())
                assert row.tolist() == [0, n, n, 0, 0]
        out = torch.full((25, 5), -7, dtype=torch.int64, device="cuda")
        assert L.dpc_voxel_edt_stats(_native.ptr(dev(fields)), 5, _native.ptr(bits), 5, *shape, _native.ptr(pairs_d),
                                     pairs.ctypes.data_as(ctypes.c_void_p), 25, thr.ctypes.data_as(ctypes.c_void_p), 2,
                                     _native.ptr(out), None, stream) == 0
        for (i, j), row in zip(pairs, out.cpu().numpy()):
            assert row.tolist() == EO.edt_stats(fields[i], grids[j], thr).tolist(), (i, j)
