#!/usr/bin/env python3
"""Generate tests/golden/f17_densify.npz by running the REFERENCE's own densification (densify/densify_single.py with
densify/utils.py) on CPU.

F17: four .obj texts are laid out as <dir>/<category>/<model>/model.obj and densify_single.densify_model is run on each,
with its module constant densifyN set to the case's split count.  Stored per case: the text, the split count, the
reference's parsed inputs (utils.parseObj, then utils.removeWeirdDuplicate: V, E, F) and the "points" array it saved.
  * sphere_box: a UV sphere and an axis-aligned box, 2 500 splits (many exactly tied edge lengths);
  * icosphere:  a level-1 icosphere, 2 000 splits (near-equilateral: two or three band edges in one face per round);
  * messy:      tests/densify_oracle.MESSY_OBJ (quad, a/b/c forms, vn/vt, a non-manifold edge, a duplicated, a degenerate
                and two rank-2 faces, an unused vertex), 1 500 splits;
  * one_tri:    a file whose faces are all one triangle (the reference keeps no face, only the edges), 300 splits.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_densify.py
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import scipy.io  # noqa: E402

from make_golden import REF  # noqa: E402  (the reference's location)

sys.path.insert(0, os.path.join(REF, "dpc", "densify"))
import densify_single  # noqa: E402
import utils as ref_utils  # noqa: E402

import densify_oracle as D  # noqa: E402

CASES = [
    ("sphere_box", D.sphere_box_obj(), 2500),
    ("icosphere", D.icosphere_obj(1), 2000),
    ("messy", D.MESSY_OBJ, 1500),
    ("one_tri", D.ONE_TRIANGLE_OBJ, 300),
]


def main():
    out = {"names": np.array([c[0] for c in CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        shapenet, dense = os.path.join(tmp, "shapenet"), os.path.join(tmp, "dense", "cat")
        os.makedirs(dense)
        for name, text, n in CASES:
            os.makedirs(os.path.join(shapenet, "cat", name))
            path = os.path.join(shapenet, "cat", name, "model.obj")
            with open(path, "w") as fh:
                fh.write(text)
            V, E, F = ref_utils.parseObj(path)
            F = ref_utils.removeWeirdDuplicate(F)
            densify_single.densifyN = n
            densify_single.densify_model(name, dense, shapenet, "cat")
            pts = scipy.io.loadmat(os.path.join(dense, name + ".mat"))["points"]
            out[name + "/text"] = np.array(text)
            out[name + "/n"] = np.array(n)
            out[name + "/V"] = np.asarray(V, dtype=np.float64)
            out[name + "/E"] = np.asarray(E, dtype=np.int64).reshape(-1, 2)
            out[name + "/F"] = np.asarray(F, dtype=np.int64).reshape(-1, 3)
            out[name + "/points"] = np.asarray(pts, dtype=np.float64)
            print(name, "V", len(V), "E", len(E), "F", len(F), "points", pts.shape)
    np.savez_compressed(os.path.join(HERE, "f17_densify.npz"), **out)


if __name__ == "__main__":
    main()
