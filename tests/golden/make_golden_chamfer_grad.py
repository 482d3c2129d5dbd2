#!/usr/bin/env python3
"""Generate tests/golden/f19_chamfer_grad.npz by differentiating the REFERENCE's own point_cloud_distance on CPU.

F19, the gradient of the Chamfer distance: util.point_cloud_distance.point_cloud_distance is the reference's own, imported
(nothing of it is restated here); torch autograd differentiates it in float64.  Three pairs share one target cloud of 300
points: sources of 257, 64 and 5 points.  The inputs are seeded and continuous: no coincident points (the reference's
gradient is NaN there) and no ties, which the generator asserts, so the reference alone is finite and unambiguous.

The loss is  sum_p a[p] * mean(minDist_p) + sum_i b[i] * minDist[i]  for recorded random a [3] and b [326] (packed in pair
order).  Stored: the clouds, idx and minDist per pair (packed), a, b, and the reference's gradients with respect to each
source cloud and to the shared target.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_chamfer_grad.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import REF, save  # noqa: E402,F401  (reference import path and numpy shims)

from util.point_cloud_distance import point_cloud_distance  # noqa: E402

SIZES = (257, 64, 5)
NT = 300


def main():
    rng = np.random.default_rng(19)
    tgt = torch.from_numpy(rng.random((NT, 3)) - 0.5).requires_grad_(True)
    srcs = [torch.from_numpy(rng.random((n, 3)) - 0.5).requires_grad_(True) for n in SIZES]
    a = rng.standard_normal(len(SIZES))
    b = rng.standard_normal(sum(SIZES))
    loss, dists, idxs, o = 0.0, [], [], 0
    for p, src in enumerate(srcs):
        _, min_dist, idx = point_cloud_distance(src, tgt)
        loss = loss + a[p] * min_dist.mean() + (torch.from_numpy(b[o:o + len(src)]) * min_dist).sum()
        o += len(src)
        dists.append(min_dist.detach().numpy())
        idxs.append(idx.numpy())
        # no coincident points and no ties: the two smallest distances of every source point are apart, the smallest > 0
        d = (tgt.detach()[None] - src.detach()[:, None]).norm(dim=2).sort(dim=1).values
        assert float(d[:, 0].min()) > 1e-4 and float((d[:, 1] - d[:, 0]).min()) > 1e-9
    loss.backward()
    grads = [s.grad.numpy() for s in srcs] + [tgt.grad.numpy()]
    assert all(np.isfinite(g).all() for g in grads)
    save("f19_chamfer_grad.npz", tgt=tgt.detach(), src0=srcs[0].detach(), src1=srcs[1].detach(), src2=srcs[2].detach(),
         a=a, b=b, idx=np.concatenate(idxs), min_dist=np.concatenate(dists), grad_src0=grads[0], grad_src1=grads[1],
         grad_src2=grads[2], grad_tgt=grads[3])


if __name__ == "__main__":
    main()
