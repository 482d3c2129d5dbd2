"""The Python drop-in next to a second `util` package (reference imports: dpc/models/model_pc_to.py:15-24,
path set-up dpc/run/startup.py:4-6).  Runs in a child interpreter so that the `util` of this process is untouched."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pytorch-unsup-pc_amd")


def _run(code, *paths):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    proc = subprocess.run([sys.executable, "-c", textwrap.dedent(code)] + list(paths), capture_output=True, text=True, env=env)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    return proc.stdout


def test_overlay_next_to_a_second_util_package(tmp_path):
    """A stand-in for the reference's dpc/ directory: a regular package `util` with modules this build replaces
    (point_cloud_to, quaternion) and modules it does not (app_config, camera)."""
    ref = tmp_path / "dpc"
    (ref / "util").mkdir(parents=True)
    (ref / "util" / "__init__.py").write_text("")
    (ref / "util" / "app_config.py").write_text("config = 'the reference config module'\n")
    (ref / "util" / "camera.py").write_text("from util.quaternion import quaternion_multiply, as_rotation_matrix\nWHO = 'ref camera'\n")
    (ref / "util" / "point_cloud_to.py").write_text("WHO = 'ref'\ndef pointcloud_project_fast(*a, **k):\n    raise AssertionError('shadowed')\n"
                                                    "def select_3d(data, indices):\n    return 'ref select_3d'\n")
    (ref / "util" / "quaternion.py").write_text("def quaternion_multiply(a, b):\n    raise AssertionError('shadowed')\n"
                                                 "def as_rotation_matrix(q):\n    return 'ref as_rotation_matrix'\n")
    (ref / "util" / "gauss_kernel.py").write_text("def gauss_smoothen_image(cfg, img, sigma_rel):\n    return 'ref gauss_smoothen_image'\n")
    out = _run("""
        import sys
        sys.path.insert(0, sys.argv[1])      # the line a maintainer adds to dpc/run/startup.py
        sys.path.append(sys.argv[2])         # startup.py's own line
        from util.app_config import config
        from util.point_cloud_to import pc_point_dropout, pointcloud_project_fast
        from util.gauss_kernel import smoothing_kernel
        from util.quaternion import quaternion_multiply as q_mul, quaternion_normalise as q_norm, \\
            quaternion_rotate as q_rotate, quaternion_conjugate as q_conj
        import util.camera, util.point_cloud_to, util.gauss_kernel, util.drc, util.point_cloud_distance
        import dpc.render as R
        assert config == 'the reference config module'
        assert pointcloud_project_fast is R.pointcloud_project_fast and pc_point_dropout is R.pc_point_dropout
        assert smoothing_kernel is R.smoothing_kernel and q_mul is R.quaternion_multiply and q_rotate is R.quaternion_rotate
        assert q_norm is R.quaternion_normalise and q_conj is R.quaternion_conjugate
        assert util.drc.drc_projection is R.drc_projection and util.point_cloud_distance.point_cloud_distance is R.point_cloud_distance
        # modules this build does not replace come from the second package, and THEIR imports resolve through the overlay
        assert util.camera.WHO == 'ref camera' and util.camera.quaternion_multiply is R.quaternion_multiply
        # names the replaced modules do not define fall through to the module they overlay
        assert util.camera.as_rotation_matrix(None) == 'ref as_rotation_matrix'
        assert util.point_cloud_to.select_3d(0, 0) == 'ref select_3d'
        assert util.gauss_kernel.gauss_smoothen_image(0, 0, 0) == 'ref gauss_smoothen_image'
        try:
            util.point_cloud_to.no_such_name
        except AttributeError as e:
            assert 'no_such_name' in str(e)
        else:
            raise AssertionError('missing attribute did not raise')
        print('ok')
        """, PKG, str(ref))
    assert out.strip().endswith("ok")


def _reference_layout():
    with open(os.path.join(ROOT, "tests", "golden", "f13_caller_layout.json")) as fh:
        return json.load(fh)


def _stand_in_reference(tmp_path, layout):
    """A dpc/ directory laid out like the reference's (fixture f13): every module of its util package, each a stub that
    says where it lives, and a models/model_pc_to.py that binds the names the reference's caller binds from the replaced
    util modules (model_pc_to.py:15-24, recorded alias by alias) and calls the renderer as that caller's forward does."""
    ref = tmp_path / "dpc"
    (ref / "util").mkdir(parents=True)
    (ref / "util" / "__init__.py").write_text("")
    for name in layout["util_modules"]:
        (ref / "util" / (name + ".py")).write_text("WHERE = 'reference util.%s'\n" % name)
    (ref / "models").mkdir()
    (ref / "models" / "__init__.py").write_text("")
    lines = ["from %s import %s as %s" % (mod, name, alias) for alias, (mod, name) in sorted(layout["caller_bindings"].items())]
    lines += ["",
              "def compute_projection(cfg, point_cloud, transform, predicted_translation, scaling_factor, focal_length, sigma_rel):",
              "    kernel = smoothing_kernel(cfg, sigma_rel)",
              "    return pointcloud_project_fast(cfg, point_cloud, transform, predicted_translation, None, kernel,",
              "                                   scaling_factor=scaling_factor, focal_length=focal_length)", ""]
    (ref / "models" / "model_pc_to.py").write_text("\n".join(lines))
    return ref


def test_overlay_next_to_the_reference_itself(tmp_path):
    """With a directory laid out like the reference's dpc/ on the path (its util modules as recorded in fixture f13): its
    caller's import lines (model_pc_to.py:15-24) bind to this build, its other util modules are found where they were."""
    layout = _reference_layout()
    ref = _stand_in_reference(tmp_path, layout)
    replaced = ("point_cloud_to", "drc", "gauss_kernel", "quaternion", "point_cloud_distance")
    assert set(replaced) <= set(layout["util_modules"])
    out = _run("""
        import sys, importlib.util, json
        sys.path.insert(0, sys.argv[1])
        sys.path.append(sys.argv[2])
        replaced, others = json.loads(sys.argv[3]), json.loads(sys.argv[4])
        from util.point_cloud_to import pc_point_dropout, pointcloud_project_fast
        from util.gauss_kernel import smoothing_kernel
        from util.quaternion import quaternion_multiply as q_mul, quaternion_normalise as q_norm, \\
            quaternion_rotate as q_rotate, quaternion_conjugate as q_conj
        import dpc.render as R
        assert pointcloud_project_fast is R.pointcloud_project_fast and smoothing_kernel is R.smoothing_kernel
        for name in others:
            spec = importlib.util.find_spec('util.' + name)
            assert spec is not None and spec.origin.startswith(sys.argv[2] + '/util/'), (name, spec)
        for name in replaced:
            assert importlib.util.find_spec('util.' + name).origin.startswith(sys.argv[1]), name
        import util.fs                      # a module of the reference's util package: really importable
        assert util.fs.__file__.startswith(sys.argv[2] + '/util/') and util.fs.WHERE == 'reference util.fs'
        print('ok')
        """, PKG, str(ref), json.dumps(replaced), json.dumps([m for m in layout["util_modules"] if m not in replaced]))
    assert out.strip().endswith("ok")


def test_the_references_own_caller_through_the_overlay(tmp_path):
    """north_star: "so dpc/run/train_eval_to.py can import it as a drop-in".  A caller module binding exactly the names the
    reference's caller (dpc/models/model_pc_to.py, import block :15-24) binds, recorded in fixture f13, is imported with the
    overlay in front of a directory laid out like the reference's dpc/: the names it binds ARE this build's functions, this
    build's networks have the parameter count of the reference's ModelPointCloud for the experiment's config, and the
    renderer call of the reference's forward (compute_projection, :239-282; config and argument shapes as recorded) binds --
    on a GPU-less host that call ends in dpc.render's loud "MI355X only" error, raised after the config, the kernel list and
    the tensors were accepted (there is no CPU path to fall into)."""
    layout = _reference_layout()
    ref = _stand_in_reference(tmp_path, layout)
    out = _run("""
        import sys, json
        sys.path.insert(0, sys.argv[1])            # the line a maintainer adds to dpc/run/startup.py
        sys.path.append(sys.argv[2])               # startup.py's own line (dpc/run/startup.py:4-6)
        layout = json.loads(open(sys.argv[3]).read())
        import torch
        from models import model_pc_to
        import dpc.render as R
        from dpc.harness import chair_unsupervised
        from dpc.harness.nets import StepNets
        assert model_pc_to.pointcloud_project_fast is R.pointcloud_project_fast
        assert model_pc_to.smoothing_kernel is R.smoothing_kernel and model_pc_to.pc_point_dropout is R.pc_point_dropout
        assert model_pc_to.q_mul is R.quaternion_multiply and model_pc_to.q_norm is R.quaternion_normalise
        assert model_pc_to.q_rotate is R.quaternion_rotate and model_pc_to.q_conj is R.quaternion_conjugate
        for alias, (mod, name) in layout['caller_bindings'].items():
            assert getattr(model_pc_to, alias) is getattr(R, name), alias
        assert model_pc_to.__file__.startswith(sys.argv[2] + '/models/')

        full = StepNets(chair_unsupervised())
        assert sum(p.numel() for p in full.parameters()) == layout['parameters'] == 61042134      # SURVEY 8(c)
        del full

        class Cfg(dict):
            __getattr__ = dict.__getitem__
            __setattr__ = dict.__setitem__
        cfg = Cfg(layout['tiny_cfg'])
        call = layout['renderer_call']
        assert call['all_rgb'] is None and [k[-3:] for k in call['kernel']] == [[1, 1, cfg.pc_gauss_kernel_size],
                                                                                 [1, cfg.pc_gauss_kernel_size, 1],
                                                                                 [cfg.pc_gauss_kernel_size, 1, 1]]
        g = torch.Generator().manual_seed(3)
        make = lambda shape: None if shape is None else torch.rand(*shape, generator=g)
        pc, q = make(call['point_cloud']) - 0.5, make(call['transform'])
        t, s, f = make(call['predicted_translation']), make(call['scaling_factor']), make(call['focal_length'])
        seen = {}
        real = R._native.require_device
        def spy(*tensors):
            seen['tensors'] = [None if x is None else tuple(x.shape) for x in tensors]
            return real(*tensors)
        R._ops.N.require_device = spy
        try:
            model_pc_to.compute_projection(cfg, pc, q, t, s, f, cfg.pc_relative_sigma)
        except RuntimeError as e:
            assert 'MI355X' in str(e), e
        else:
            raise AssertionError('a CPU call went through: there must be no CPU path')
        # what arrived at the renderer: 2 objects x 2 views x 4 candidates = 16 clouds of 128 kept points, poses, scales
        assert seen['tensors'][:2] == [(16, 128, 3), (16, 4)] and seen['tensors'][4] == (16, 1), seen
        print('ok')
        """, PKG, str(ref), os.path.join(ROOT, "tests", "golden", "f13_caller_layout.json"))
    assert out.strip().endswith("ok")
