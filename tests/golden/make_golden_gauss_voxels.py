#!/usr/bin/env python3
"""Generate tests/golden/f23_gauss_voxels.npz: the exact Gaussian renderer of cfg.pc_fast == false.

pointcloud_project (dpc/util/point_cloud.py:219-226) exists in the reference's TF-1 original only, so its voxel stage is
the fp64 restatement of tests/gauss_voxels_oracle.py (the literal broadcast form of :17-57, numpy for the values, the same
lines in torch for the gradients; the two are compared here), between the REFERENCE's own torch functions where they run:
    util.point_cloud_to.pc_perspective_transform      :220
    util.drc.drc_projection                           :224

One case: B = 2, N = 300, vox_size 16, sigma_rel 1.5, the default normalisation (pc_normalise_gauss_analytical).  Stored: the
inputs, the transformed points, raw (the sums before the clip), voxels and proj in the layouts pointcloud_project returns,
and d(points), d(quaternion) of  sum(voxels * dvox) + sum(proj * dproj)  for seeded dvox, dproj.  For the other two
normalisation modes the transformed points' raw grids are stored too (values only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gauss_voxels.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import leaf, make_cfg, quiet, save, synth_inputs  # noqa: E402  (reference import path and numpy shims)

import util.point_cloud_to as ref_pc  # noqa: E402
from util.drc import drc_projection  # noqa: E402

import gauss_voxels_oracle as GO  # noqa: E402

B, N, G, SIGMA_REL, SEED = 2, 300, 16, 1.5, 2323


def main():
    cfg = make_cfg(vox_size=G, vox_size_z=-1)
    assert cfg.pc_normalise_gauss_analytical and not cfg.pc_normalise_gauss       # default_config.yaml:51-52
    sigma = SIGMA_REL / G                                                          # vis_projections_pc.py:84-85
    pc, q, _, _, _, _ = synth_inputs(B, N, G, SEED)
    rng = np.random.default_rng(SEED)
    dvox = rng.standard_normal((B, G, G, G, 1))
    dproj = rng.standard_normal((B, G, G, 1))
    lp, lq = leaf(pc.double()), leaf(q.double())
    with quiet():
        tr_pc = ref_pc.pc_perspective_transform(cfg, lp, lq, None, None)           # :220
    raw, voxels = GO.literal_torch(tr_pc, G, sigma, GO.normalise_mode(cfg))        # :221
    voxels = voxels.permute(0, 2, 1, 3, 4)                                         # :222
    raw = raw.permute(0, 2, 1, 3, 4)
    proj, _ = drc_projection(voxels, cfg)                                          # :224
    proj = torch.flip(proj, [1])                                                   # :225
    ((voxels * torch.from_numpy(dvox)).sum() + (proj * torch.from_numpy(dproj)).sum()).backward()
    out = dict(pc=pc, q=q, sigma=sigma, tr_pc=tr_pc, raw=raw, voxels=voxels, proj=proj, dvox=dvox, dproj=dproj,
               dpc=lp.grad, dq=lq.grad)
    tr = tr_pc.detach().numpy()
    for mode, tag in ((GO.NONE, "none"), (GO.ANALYTICAL, "analytical"), (GO.PER_POINT, "per_point")):
        raw_np, _ = GO.pointcloud2voxels_literal(tr, G, sigma, mode)              # numpy, [B,G,G,G,1] in :55's layout
        raw_t, _ = GO.literal_torch(tr_pc.detach(), G, sigma, mode)
        assert np.abs(raw_np - raw_t.numpy()).max() <= 1e-13 * max(1.0, raw_np.max())
        out["raw_" + tag] = raw_np
    assert np.array_equal(out["raw_analytical"].transpose(0, 2, 1, 3, 4), raw.detach().numpy()) or \
        np.abs(out["raw_analytical"].transpose(0, 2, 1, 3, 4) - raw.detach().numpy()).max() <= 1e-13
    lo, near1 = GO.clip_margin(raw.detach().numpy())
    assert lo >= 0.0 and near1 > 1e-6, (lo, near1)
    assert (raw > 1).any() and (raw < 1).any(), "the case should clip somewhere and pass somewhere"
    save("f23_gauss_voxels.npz", **out)


if __name__ == "__main__":
    main()
