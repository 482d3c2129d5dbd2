"""Drop-in for the reference's dpc/util/point_cloud_to.py (names as imported at dpc/models/model_pc_to.py:15)."""
from dpc.render import (pc_perspective_transform, pc_point_dropout, pointcloud2voxels3d_fast,  # noqa: F401
                        pointcloud_project, pointcloud_project_fast, smooth_voxels3d, smoothen_voxels3d)
# not in the reference's module: the fused depth map and depth loss of the projection's output dict (its torch port leaves
# add_proj_depth_loss half translated, dpc/util/losses_to.py)
from dpc.render import proj_depth_loss, project_depth  # noqa: F401
# the TF-1 original's exact renderer (dpc/util/point_cloud.py:17-57, 219-226), which the torch port calls without importing
# it (model_pc_to.py:270-273); `pointcloud_project` above stays the alias of the fast path it has always been here
from dpc.render import pointcloud2voxels, pointcloud_project_exact  # noqa: F401

from ._overlay import fall_through as _fall_through  # noqa: E402

__getattr__ = _fall_through(__name__, __file__)   # everything else: the module of the same name that this one overlays
