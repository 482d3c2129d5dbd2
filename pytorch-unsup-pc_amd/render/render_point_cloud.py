"""Drop-in for the reference's dpc/render/render_point_cloud.py: render_point_cloud(point_cloud, cfg) on the GPU."""
from dpc.render.visualise import render_point_cloud  # noqa: F401

from util._overlay import fall_through as _fall_through  # noqa: E402

__getattr__ = _fall_through(__name__, __file__, "render")   # everything else: the module of the same name it overlays
