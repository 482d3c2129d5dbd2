#!/usr/bin/env python3
"""Generate tests/golden/f14_pooled_loss.npz by running the REFERENCE's own loss code on CPU (fp64).

F14: ModelPointCloud.add_proj_loss and add_student_loss (dpc/models/model_pc_to.py:339-385, 410-489) on a fake `self`
(the way make_golden.py does F8), with masks larger than the silhouettes -- the reference pools them with
nn.AvgPool2d(gt_size // pred_size) -- and cfg.variable_num_views, which weights every sample's residual and student term
by inputs["valid_samples"].  K = 4 pose candidates, a student, and two pooling factors: [S,1,32,32] binary masks and
[S,1,48,48] U(0,1) masks, both onto 16 x 16 silhouettes.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pooled.py

Recorded per factor f (keys suffixed _f2, _f3): masks, pred, weights, poses, student, the projection loss, min_loss
(the winners), d loss / d pred, the student loss and d student loss / d student.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

from make_golden import REF, make_cfg, save  # noqa: E402  (sets up the reference's import path and numpy shims)


def f14_pooled_loss():
    from models import model_pc_to as m

    K, S, G = 4, 6, 16
    cfg = make_cfg(pose_predict_num_candidates=K, variable_num_views=True, pose_predictor_student=True,
                   pose_student_align_loss=False, pose_predictor_student_loss_weight=1.0)

    class Fake:   # what add_proj_loss needs of its model: the config and the two loss methods
        proj_loss_pose_candidates = m.ModelPointCloud.proj_loss_pose_candidates
        add_student_loss = m.ModelPointCloud.add_student_loss

        def cfg(self):
            return cfg

    g = torch.Generator().manual_seed(1400)
    weights = torch.tensor([1.0, 0.0, 0.5, 1.0, 0.5, 0.0], dtype=torch.float64)
    out = {}
    for f, binary in ((2, True), (3, False)):
        masks = torch.rand(S, 1, f * G, f * G, generator=g, dtype=torch.float64)
        if binary:
            masks = (masks > 0.5).double()
        pred = torch.rand(S * K, G, G, 1, generator=g, dtype=torch.float64).requires_grad_(True)
        poses = torch.randn(S * K, 4, generator=g, dtype=torch.float64)
        student = torch.randn(S, 4, generator=g, dtype=torch.float64).requires_grad_(True)
        inputs = {"masks": masks.clone(), "valid_samples": weights.clone()}
        outputs = {"projs": pred, "poses": poses, "pose_student": student}
        total, min_loss = m.ModelPointCloud.add_proj_loss(Fake(), inputs, outputs, 1.0, None, False)
        stud = m.ModelPointCloud.add_student_loss(Fake(), inputs, outputs, min_loss, None, False)
        total.backward()
        sfx = "_f%d" % f
        out.update({"masks" + sfx: masks, "pred" + sfx: pred, "poses" + sfx: poses, "student" + sfx: student,
                    "loss" + sfx: (total - stud).detach(), "min_loss" + sfx: min_loss, "dpred" + sfx: pred.grad,
                    "student_loss" + sfx: stud.detach(), "dstudent" + sfx: student.grad})
    save("f14_pooled_loss.npz", weights=weights, K=K, **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    f14_pooled_loss()
    assert not os.path.exists(os.path.join(REF, "dpc/util/__pycache__")), "left bytecode in the reference"
