#!/usr/bin/env python3
"""Generate tests/golden/f18_mesh_views.npz by running the REFERENCE's own camera and projection code on CPU (fp64).

F18, what pins the mesh renderer's views (dpc.render.meshviews, csrc/dpc_mesh_raster.hip) to the reference's camera:
  * a small mesh without mirror or rotation symmetry (four boxes: 48 faces, one material each) and 3 camera positions;
  * 2 000 points on its surface;
  * per view util/camera.py quaternion_from_campos(cam_pos) and util/point_cloud_to.py pc_perspective_transform of those
    points with that quaternion (camera_distance 2.0, focal_length 1.875, float64): its output (d - camera_distance, v, u).
Data only: no code of the reference is stored.  make_golden.py's numpy shims are applied by importing it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mesh_views.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_golden import AttrDict, quiet, ref_pc, save  # noqa: E402  (reference import path and numpy shims)
import util.camera as ref_cam  # noqa: E402
import mesh_render_oracle as O  # noqa: E402

BOXES = [((-0.24, -0.04, -0.20), (0.20, 0.03, 0.24)),    # a seat
         ((-0.24, 0.03, -0.20), (-0.17, 0.34, 0.24)),    # a back on one side
         ((0.08, -0.32, 0.11), (0.18, -0.04, 0.22)),     # one leg
         ((-0.04, 0.03, 0.10), (0.10, 0.13, 0.24))]      # a block on the seat, off centre: all inside every view
KD = [[0.8, 0.2, 0.2], [0.2, 0.7, 0.3], [0.2, 0.3, 0.9], [0.9, 0.8, 0.1]]
CAM_POS = [[1.2, -0.9, 0.7], [-0.6, 1.7, 0.45], [-1.5, -0.8, -0.35]]


def main():
    V, F, mat = O.box_mesh(BOXES)
    points = O.sample_surface(V, F, 2000, 1800)
    cfg = AttrDict(camera_distance=2.0, focal_length=1.875, pose_quaternion=True)
    quats, trs = [], []
    for pos in CAM_POS:
        q = np.asarray(ref_cam.quaternion_from_campos(np.array(pos, dtype=np.float64)), dtype=np.float64)
        with quiet():
            tr = ref_pc.pc_perspective_transform(cfg, torch.from_numpy(points)[None].clone(), torch.from_numpy(q)[None])
        assert tr.dtype == torch.float64
        assert float(tr[0, :, 1:].abs().max()) < 0.47, "the mesh must stay inside the image"
        quats.append(q)
        trs.append(tr[0].numpy())
    save("f18_mesh_views.npz", V=V, F=F.astype(np.int32), material=mat.astype(np.int32), Kd=np.array(KD), cam_pos=np.array(CAM_POS),
         points=points, q=np.stack(quats), transformed=np.stack(trs), camera_distance=2.0, focal_length=1.875)


if __name__ == "__main__":
    main()
