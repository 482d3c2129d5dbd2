"""The closed-form gradient of the batched Chamfer distance (include/dpc_render.h, dpc_nearest_batched_bwd) in numpy
float64, summed exactly.  A helper for tests/test_chamfer_loss_host.py and tests/test_chamfer_loss_gpu.py; not collected.

For source point i of pair p with s its coordinates, t = target idx[i], d = |t - s|, n_p = src_count and the weight
w = gdist[i] + gmean[p] / n_p:
    distance mode   the target receives c = w (t - s) / d and the source -c; d == 0: both receive exactly zero;
    squared mode    the target receives c = 2 w (t - s) and the source -c.
The gradient of a packed point is the math.fsum of everything it receives, in any role, in any pair."""
import math

import numpy as np


def nearest_brute(points, pairs):
    """(min_dist, idx) of every pair, packed in pair order: numpy float64, first minimum of the distances."""
    pts = np.asarray(points, dtype=np.float64)
    dist, idx = [], []
    for s0, ns, t0, nt in np.asarray(pairs, dtype=np.int64):
        d = pts[t0:t0 + nt][None, :, :] - pts[s0:s0 + ns][:, None, :]
        dd = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        j = np.argmin(dd, axis=1) if ns else np.zeros((0,), np.int64)
        idx.append(j)
        dist.append(dd[np.arange(ns), j])
    return np.concatenate(dist), np.concatenate(idx).astype(np.int64)


def chamfer_grad(points, pairs, idx, gmean=None, gdist=None, squared=False):
    """points [n,3], pairs [P,4], idx [sum src_count] (relative to tgt_start), gmean [P] | None, gdist [sum src_count] |
    None.  Returns (grad [n,3] float64, abs_sum [n,3] = sum of |contribution| per component, count [n] = contributions)."""
    pts = np.asarray(points, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 4)
    n = len(pts)
    terms = [[[], [], []] for _ in range(n)]
    count = np.zeros(n, dtype=np.int64)
    o = 0
    for p, (s0, ns, t0, nt) in enumerate(pairs):
        for i in range(ns):
            w = (0.0 if gdist is None else float(gdist[o + i])) + (0.0 if gmean is None else float(gmean[p]) / float(ns))
            a, b = s0 + i, t0 + int(idx[o + i])
            diff = pts[b] - pts[a]
            if squared:
                c = 2.0 * w * diff
            else:
                d = math.sqrt(float(diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]))
                c = w * diff / d if d > 0.0 else np.zeros(3)
            for k in range(3):
                terms[a][k].append(-float(c[k]))
                terms[b][k].append(float(c[k]))
            count[a] += 1
            count[b] += 1
        o += ns
    grad = np.array([[math.fsum(t[k]) for k in range(3)] for t in terms], dtype=np.float64).reshape(n, 3)
    abs_sum = np.array([[math.fsum(abs(v) for v in t[k]) for k in range(3)] for t in terms], dtype=np.float64).reshape(n, 3)
    return grad, abs_sum, count
