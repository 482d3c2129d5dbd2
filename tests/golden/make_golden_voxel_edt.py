"""Writes tests/golden/f34_voxel_edt.npz: what the numpy oracle of the voxel distance transform (tests/voxel_edt_oracle.py,
the definition of its rules: there is no counterpart program in the reference) returns for the seeded grids of
voxel_edt_oracle.golden_cases, so that a change of the oracle shows.  Per case: the grid packed to bits (voxel f is bit
f & 31 of word f >> 5), checksums of the two fields (seeds = the set voxels, then seeds = the clear voxels) by brute force,
the fields themselves for the grids of at most 128 voxels, the shell packed to bits, and the surface stats [2,2,3+K] and the
F-score [2,K,3] against the shape's partner grid: first with shells, then with all voxels.  Run from the repository root:

    python tests/golden/make_golden_voxel_edt.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import voxel_edt_oracle as O  # noqa: E402


def main():
    out = {"taus": np.asarray(O.GOLDEN_TAUS, dtype=np.float64), "thresholds_sq": O.thresholds_sq(O.GOLDEN_TAUS)}
    thr = out["thresholds_sq"]
    for key, shape, kind, g in O.golden_cases():
        out[key + "/bits"] = O.pack_bits(g)
        fields = [O.edt_brute(g, of_clear) for of_clear in (False, True)]
        out[key + "/sq_digests"] = np.array([O.digest(f) for f in fields])
        if g.size <= 128:
            out[key + "/sq"] = np.stack(fields)
        out[key + "/shell"] = O.pack_bits(O.shell(g))
        partner = O.golden_partner(shape)
        stats = np.stack([O.surface_stats(g, partner, thr, surface, edt=O.edt_brute) for surface in (True, False)])
        out[key + "/stats"] = stats
        out[key + "/fscore"] = O.fscore(stats)
        print(key, int(g.sum()), stats[0].tolist())
    path = os.path.join(HERE, "f34_voxel_edt.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
