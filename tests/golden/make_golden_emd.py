"""Writes tests/golden/f24_emd.npz: for every case of emd_oracle.FIXTURE_CASES its seed, a checksum of the clouds that
seed regenerates (not the clouds), scipy's optimal total cost of the fp64 cost matrix, and that matrix's largest entry.
The GPU tests read the optima from here and need no scipy.  Run from the repository root:

    python tests/golden/make_golden_emd.py
"""
import os
import sys

import numpy as np
from scipy.optimize import linear_sum_assignment

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import emd_oracle as O  # noqa: E402


def main():
    out = {}
    for seed, (kind, n, dt, squared) in enumerate(O.FIXTURE_CASES):
        P, G = O.clouds(kind, n, seed, np.dtype(dt))
        C = O.cost_matrix(P, G, squared)
        r, c = linear_sum_assignment(C)
        key = O.case_key(kind, n, dt, squared)
        out[key + "/seed"] = np.int64(seed)
        out[key + "/checksum"] = np.array(O.checksum(P, G))
        out[key + "/optimum"] = np.float64(C[r, c].sum())
        out[key + "/max_cost"] = np.float64(C.max())
        print(key, seed, out[key + "/optimum"])
    path = os.path.join(HERE, "f24_emd.npz")
    np.savez(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
