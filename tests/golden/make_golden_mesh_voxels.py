"""Writes tests/golden/f26_mesh_voxels.npz: what the numpy oracle of the mesh voxeliser (tests/mesh_voxels_oracle.py, the
definition of its rules: there is no counterpart program in the reference) returns for the seeded meshes of
mesh_voxels_oracle.golden_cases, so that a change of the oracle's operation order shows.  Per case: checksums of the
vertices and faces that the case regenerates (not the mesh), and for every fill the grid packed to bits (voxel f is bit
f & 31 of word f >> 5), the two counts and the status bits.  Run from the repository root:

    python tests/golden/make_golden_mesh_voxels.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mesh_voxels_oracle as O  # noqa: E402
from voxels_oracle import digest  # noqa: E402


def main():
    out = {}
    for key, shape, V, F in O.golden_cases():
        out[key + "/inputs"] = np.array([digest(V), digest(F)])
        for fill in O.FILLS:
            grid, info, status = O.voxelise_mesh(V, F, shape, fill)
            out["%s/%s/bits" % (key, fill)] = O.pack_bits(grid)
            out["%s/%s/info" % (key, fill)] = info
            out["%s/%s/status" % (key, fill)] = np.int32(status)
            print(key, shape, fill, int(grid.sum()), info.tolist(), status)
    path = os.path.join(HERE, "f26_mesh_voxels.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
