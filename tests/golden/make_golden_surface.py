#!/usr/bin/env python3
"""Generate tests/golden/f29_surface.npz from the numpy oracle (tests/surface_oracle.py): the 256 x 16 triangulation table
and the meshes of three tiny grids.  There is no reference program for this rule (the reference calls skimage), so the
fixture pins the oracle itself: a later change to the oracle, the generator or the committed header shows up as a diff.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_surface.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import surface_oracle as O  # noqa: E402


def grids():
    """(name, grid, level): a ball, a bordered noise grid with a node exactly at the level, a slab with a side of 1."""
    noise = O.noise((4, 5, 6), 29)
    noise[1, 2, 3] = 0.5
    line = np.array([0.0, 1.0, 0.25, 0.75, 0.0, 1.0, 1.0], dtype=np.float64).reshape(1, 1, 7)
    return (("ball", O.ball((5, 5, 5), np.float32), 0.5), ("noise", noise, 0.5), ("line", line, 0.3))


def main():
    out = {"table": O.table()}
    for name, grid, iso in grids():
        verts, faces, nonfinite = O.extract(grid, iso)
        assert not nonfinite
        out[name + "/grid"], out[name + "/iso"] = grid, np.float64(iso)
        out[name + "/verts"], out[name + "/faces"] = verts, faces
    path = os.path.join(HERE, "f29_surface.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
