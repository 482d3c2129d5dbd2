#!/usr/bin/env python3
"""Generate tests/golden/f15_alignment.npz by running the REFERENCE's own alignment and pose-evaluation code on CPU (fp64).

F15, the host side of the unsupervised evaluation:
  * util/camera.py quaternion_from_campos (with util/euler.py) on 40 camera positions;
  * util/quaternion.py as_rotation_matrix and from_rotation_matrix on random quaternions, plus rotations within 1e-9 of
    180 degrees, where from_rotation_matrix's w = sqrt(1 + tr) / 2 turns NaN;
  * run/compute_alignment.py compute_alignment(): the per-model view selection, the model selection and Markley's average,
    on the reference's own experiments/chair_unsupervised/reference_rotations.mat_old (50 models x 5 views).  Its
    compute_alignment_candidates (the open3d ICP loop) is replaced by a copy of that file into place;
  * run/eval_camera_pose_to.py run_eval(): per-view angle errors, accuracy and median for synthetic predicted cameras and
    that rotation.
The import chain's unavailable modules (open3d, cv2, the config parser, the dataset) are stubbed in sys.modules;
make_golden.py's numpy shims are applied by importing it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_alignment.py
"""
import os
import pickle
import shutil
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import scipy.io  # noqa: E402
import torch  # noqa: E402

from make_golden import REF, AttrDict, quiet, save  # noqa: E402  (reference import path and numpy shims)

ROT_FILE = os.path.join(REF, "experiments/chair_unsupervised/reference_rotations.mat_old")


def _stub(name, **attrs):
    mod = types.ModuleType(name)
    mod.__dict__.update(attrs)
    sys.modules[name] = mod
    return mod


class _Dataset:
    """What compute_alignment / run_eval read of run.ShapeRecords: len, file_names and sample["cam_pos"]."""
    cam_pos = None

    def __init__(self, folder, cfg, split):
        self.file_names = ["m%02d" % k for k in range(cfg.num_dataset_samples)]

    def __len__(self):
        return len(self.file_names)

    def __getitem__(self, k):
        return {"cam_pos": _Dataset.cam_pos[k]}


def _import_reference(cfg):
    _stub("startup")
    _stub("open3d")
    _stub("cv2")
    _stub("util.app_config", config=cfg)
    _stub("util.simple_dataset", Dataset3D=None)
    _stub("run.ShapeRecords", ShapeRecords=_Dataset)
    sys.path.insert(0, os.path.join(REF, "dpc", "run"))
    import run.compute_alignment as ca
    import run.eval_camera_pose_to as ep
    import util.camera as cam
    import util.quaternion as q

    return ca, ep, cam, q


def main():
    g = np.random.default_rng(1500)
    work = tempfile.mkdtemp()
    try:
        cfg = AttrDict(checkpoint_dir=work, inp_dir=work, num_dataset_samples=50, num_views=5, save_predictions_dir="pred",
                       eval_split="val", models_list="", pose_accuracy_threshold=30, gpu="")
        ca, ep, cam, q = _import_reference(cfg)
        out = {}

        # quaternion_from_campos: 40 positions at random directions and distances, a few on the y / z axes' sides
        cam_pos = g.normal(size=(40, 3)) * g.uniform(0.5, 3.0, size=(40, 1))
        cam_pos[:4, :2] *= [[1, -1], [-1, 1], [-1, -1], [1, 1]] * np.sign(cam_pos[:4, :2])
        out["campos"] = cam_pos
        out["campos_quat"] = np.stack([cam.quaternion_from_campos(c) for c in cam_pos])

        # as_rotation_matrix / from_rotation_matrix on random quaternions and near-180-degree rotations
        quats = g.normal(size=(64, 4))
        axes = g.normal(size=(16, 3))
        axes /= np.linalg.norm(axes, axis=1, keepdims=True)
        half = np.pi / 2 - g.uniform(0, 1e-9, size=(16, 1))   # half-angles within 1e-9 of 90 degrees: rotations near 180
        quats = np.concatenate([quats, np.concatenate([np.cos(half), np.sin(half) * axes], axis=1)])
        out["quats"] = quats
        out["rotmats"] = q.as_rotation_matrix(torch.from_numpy(quats.copy())).reshape(-1, 3, 3)
        out["rotmats_quat"] = np.stack([q.from_rotation_matrix(m[None].copy()).numpy() for m in out["rotmats"]])

        # compute_alignment's selection and average on the reference's stored candidates
        ca.compute_alignment_candidates = lambda cfg_, dataset, path: shutil.copy(ROT_FILE, path)
        with quiet():
            ca.compute_alignment()
        stored = scipy.io.loadmat(ROT_FILE)
        out["cand_rotations"], out["cand_rmse"] = stored["rotations"], stored["rmse"]
        ref_rot = scipy.io.loadmat(os.path.join(work, "final_reference_rotation.mat"))["rotation"]
        out["reference_rotation"] = ref_rot

        # run_eval on synthetic cameras: predictions = GT camera * reference rotation, perturbed up to ~60 degrees
        M, V = 12, 5
        _Dataset.cam_pos = g.normal(size=(M, V, 3)) * 2.0
        os.makedirs(os.path.join(work, "pred"), exist_ok=True)
        pred = np.zeros((M, V, 4))
        for m in range(M):
            for v in range(V):
                qg = cam.quaternion_from_campos(_Dataset.cam_pos[m, v])
                ax = g.normal(size=3)
                ang = g.uniform(0, np.pi / 3)
                qp = q.quaternion_multiply_np(np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax / np.linalg.norm(ax)]),
                                              q.quaternion_multiply_np(qg, ref_rot.reshape(4)))
                pred[m, v] = qp * g.uniform(0.5, 2.0) * (1 if g.uniform() < 0.7 else -1)   # unnormalised, either sign
            with open(os.path.join(work, "pred", "m%02d_pc.pkl" % m), "wb") as f:
                pickle.dump({"camera_pose": pred[m].copy()}, f)
        cfg.num_dataset_samples = M
        ep.app_config, ep.ShapeRecords = cfg, lambda folder, cfg_, split: _Dataset(folder, cfg_, split)
        with quiet():
            ep.run_eval()
        res = scipy.io.loadmat(os.path.join(work, "pose_error_pred_val.mat"))
        out.update(pose_pred=pred, pose_cam_pos=_Dataset.cam_pos, pose_angle_error=res["angle_error"],
                   pose_accuracy=res["accuracy"].reshape(()), pose_median=res["median_error"].reshape(()))
        save("f15_alignment.npz", **out)
    finally:
        shutil.rmtree(work)


if __name__ == "__main__":
    main()
    assert not os.path.exists(os.path.join(REF, "dpc/util/__pycache__")), "left bytecode in the reference"
