"""Host-side checks of what the voxel entry points share (csrc/dpc_voxel_bits.h, check_pairs of csrc/dpc_batch.h; no GPU):
the side check of every entry point that takes (D, H, W), with NULL pointers so that nothing can be launched, and the
pair-table check of the two entry points that take one."""
import ctypes

import numpy as np
import pytest

N = None

# name -> (the smallest side it accepts, the call with `items` clouds / grids / pairs / meshes and NULL everywhere)
ENTRIES = {
    "dpc_voxelise": (1, lambda L, D, H, W, items: L.dpc_voxelise(N, 0, 0, N, N, items, D, H, W, N, N, N, N)),
    "dpc_voxel_threshold": (1, lambda L, D, H, W, items: L.dpc_voxel_threshold(N, 0, items, D, H, W, 0.5, 1, N, N)),
    "dpc_voxel_unpack": (1, lambda L, D, H, W, items: L.dpc_voxel_unpack(N, items, D, H, W, N, N)),
    "dpc_voxel_stats": (1, lambda L, D, H, W, items: L.dpc_voxel_stats(N, 1, N, 1, D, H, W, N, N, items, N, N, N)),
    "dpc_voxel_count": (1, lambda L, D, H, W, items: L.dpc_voxel_count(N, items, D, H, W, N, N)),
    "dpc_voxelise_meshes": (2, lambda L, D, H, W, items: L.dpc_voxelise_meshes(N, 0, 0, N, 0, N, N, items, D, H, W, 0, N, N, N, N, N)),
    "dpc_voxel_carve": (1, lambda L, D, H, W, items: L.dpc_voxel_carve(N, items, D, H, W, N, N)),
    "dpc_voxel_edt": (1, lambda L, D, H, W, items: L.dpc_voxel_edt(N, items, D, H, W, 0, N, N)),
    "dpc_voxel_shell": (1, lambda L, D, H, W, items: L.dpc_voxel_shell(N, items, D, H, W, N, N)),
    "dpc_voxel_edt_stats": (1, lambda L, D, H, W, items: L.dpc_voxel_edt_stats(N, 1, N, 1, D, H, W, N, N, items, N, 0, N, N, N)),
    "dpc_mesh_winding_voxels": (2, lambda L, D, H, W, items: L.dpc_mesh_winding_voxels(N, 0, 0, N, 0, N, N, items, D, H, W, 0, N, N, N, N)),
}


def test_the_table_lists_every_entry_point_with_three_sides():
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dpc_render.h")).read()
    declared = set(re.findall(r"^int (dpc_\w+)\([^;]*?int D, int H, int W[^;]*;", header, flags=re.M))
    assert declared == set(ENTRIES), sorted(declared ^ set(ENTRIES))


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_side_checks_before_any_launch(name):
    """A side of 0, -1 or DPC_VOXEL_MAX_SIDE + 1 on any axis is DPC_ERR_SHAPE; a side of 1 is refused by the entry points
    that divide by side - 1 and by no other (they get as far as DPC_ERR_NULL: one item, no table); the largest grid with
    no item is DPC_OK."""
    from dpc.render import _native

    L, SHAPE, NUL, S = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL, _native.DPC_VOXEL_MAX_SIDE
    min_side, call = ENTRIES[name]
    assert call(L, 4, 4, 4, 1) == NUL and call(L, S, S, S, 1) == NUL and call(L, 2, 2, 2, 1) == NUL
    for axis in range(3):
        for bad in (0, -1, S + 1):
            sides = [4, 4, 4]
            sides[axis] = bad
            assert call(L, *sides, 1) == SHAPE, sides
            assert call(L, *sides, 0) == SHAPE, sides
        sides = [4, 4, 4]
        sides[axis] = 1
        assert call(L, *sides, 1) == (SHAPE if min_side == 2 else NUL), sides
    assert call(L, 1, 1, 1, 1) == (SHAPE if min_side == 2 else NUL)
    assert call(L, S, S, S, 0) == 0


def test_voxel2pc_keeps_its_own_lower_bound():
    from dpc.render import _native

    L, SHAPE, S = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_VOXEL_MAX_SIDE
    for G in (0, -1, 1, S + 1):
        assert L.dpc_voxel2pc(N, 0, G, N, N, 0, N, N, N) == SHAPE, G
    assert L.dpc_voxel2pc(N, 0, 2, N, N, 0, N, N, N) == 0 and L.dpc_voxel2pc(N, 0, S, N, N, 0, N, N, N) == 0


def test_both_pair_tables_refuse_the_same_rows():
    """dpc_voxel_stats and dpc_voxel_edt_stats on a table whose second row is bad: an index equal to the count and a
    negative one, on either side."""
    from dpc.render import _native

    L, SHAPE, NUL = _native.lib(), _native.DPC_ERR_SHAPE, _native.DPC_ERR_NULL

    def both(rows, n_a, n_b):
        t = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1, 2))
        p = t.ctypes.data_as(ctypes.c_void_p)
        return (L.dpc_voxel_stats(N, n_a, N, n_b, 4, 4, 4, N, p, len(t), N, N, N),
                L.dpc_voxel_edt_stats(N, n_a, N, n_b, 4, 4, 4, N, p, len(t), N, 0, N, N, N))

    assert both([(0, 0), (2, 1), (1, 1)], 3, 2) == (NUL, NUL)            # every row inside: as far as the NULL pointers
    for bad in ((3, 0), (0, 2), (-1, 0), (0, -1)):
        assert both([(0, 0), bad], 3, 2) == (SHAPE, SHAPE), bad
        assert both([(2, 1), (0, 0), bad], 3, 2) == (SHAPE, SHAPE), bad
    assert both([(0, 0), (0, 0)], 0, 1) == (SHAPE, SHAPE) and both([(0, 0), (0, 0)], 1, 0) == (SHAPE, SHAPE)
