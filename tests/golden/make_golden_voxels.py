"""Writes tests/golden/f25_voxels.npz: what the reference's util/voxel.py (it needs only numpy) returns for voxel2pc and
evaluate_voxel_prediction on the seeded grids of voxels_oracle.golden_cases (G in {2, 3, 5, 33}, thresholds 0.3 and 0.5,
float32 and float64).  Per case: the seed, checksums of the inputs that seed regenerates (not the inputs), the shape and a
checksum of voxel2pc's xyz (xyz itself up to G = 5), its occupancies packed to bits, and the five sums of
evaluate_voxel_prediction.  Run from the repository root, DPC_REFERENCE naming the reference checkout:

    python tests/golden/make_golden_voxels.py
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import voxels_oracle as O  # noqa: E402

REF = os.environ.get("DPC_REFERENCE", "/root/reference")


def reference_module():
    spec = importlib.util.spec_from_file_location("reference_util_voxel", os.path.join(REF, "dpc", "util", "voxel.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = reference_module()
    out = {}
    for key, G, thr, dtype, seed in O.golden_cases():
        voxels, preds, gt = O.golden_inputs(G, seed, dtype)
        xyz, occ = ref.voxel2pc(voxels.copy(), thr)
        sums = ref.evaluate_voxel_prediction(preds.copy(), gt.copy(), thr)
        out[key + "/seed"] = np.int64(seed)
        out[key + "/inputs"] = np.array([O.digest(voxels), O.digest(preds), O.digest(gt)])
        out[key + "/xyz_shape"] = np.array(xyz.shape, dtype=np.int64)
        out[key + "/xyz_digest"] = np.array(O.digest(xyz))
        if G <= 5:
            out[key + "/xyz"] = xyz
        out[key + "/occupancies"] = np.packbits(occ)
        out[key + "/sums"] = np.asarray(sums, dtype=np.int64)
        print(key, seed, xyz.shape, sums.tolist())
    path = os.path.join(HERE, "f25_voxels.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
