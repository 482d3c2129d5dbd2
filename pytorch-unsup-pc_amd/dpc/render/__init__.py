"""dpc.render -- MI355X-native differentiable point-cloud projection.

Drop-in for the projection path of NiteshBharadwaj/pytorch-unsup-pc: the functions below keep the
reference's names, argument order and defaults (reference file:line cited per function) and return tensors
of the same shapes.  They are also importable under the names the reference's caller really uses
(`util.point_cloud_to`, `util.drc`, `util.gauss_kernel`, `util.quaternion`) when this package's parent
directory is on sys.path -- the same arrangement as the reference's dpc/run/startup.py.

Differences from the reference, all deliberate (SURVEY.md section 8a "quirks"):
  * fp32 tensors on the device of the INPUTS (the reference promotes to fp64 and picks the device globally);
  * the Gaussian smoothing is applied (the reference's CUDA branch); `smooth=False` reproduces its CPU branch;
  * dead branches of the reference raise NotImplementedError naming the config key;
  * no `print` in the hot path; a point exactly on the +1/2 face contributes its in-range corners instead of
    raising IndexError.
"""
import os as _os

import numpy as np
import torch

from . import _native
from ._ops import (DepthLoss, DepthMap, DeviceSchedule, DeviceTaps, Drc, DrcLoss, DrcRgbLoss, GaussVoxels, Geometry, ProjectFused, ProjectLossFused, ProjectLossStep, RgbLoss, RgbMap, RgbSplat, RgbSplatFixed,
                   SilhouetteLoss, Smooth, Splat, Transform, status_word, taps_bucket)
from ._ops import _plane as _ops_plane
from ._ops import colour_sets as _ops_colour_sets
from ._ops import gt_smooth as _ops_gt_smooth
from .predictions import chamfer_of_predictions, load_predictions, save_predictions  # noqa: F401
from .alignment import (alignment_candidates, alignment_to_ground_truth, as_rotation_matrix, from_rotation_matrix,  # noqa: F401
                        icp_point_to_point, pose_errors, quat_w_avg_markley, quaternion_from_campos, reference_rotation)
from .chamfer import chamfer_batched, chamfer_loss, chamfer_of_split, eval_chamfer, nearest_batched  # noqa: F401
from .emd import emd_loss, emd_match, emd_of_split  # noqa: F401
from .sampling import farthest_point_sample  # noqa: F401
from .downsample import downsample_split, voxel_down_sample  # noqa: F401
from .voxels import (evaluate_voxel_prediction, iou_of_split, render_voxels, voxel2pc, voxel_iou, voxel_stats,  # noqa: F401
                     voxelise, voxels2pc_batched)
from .densify import MeshError, densify_meshes, densify_split, load_obj_mesh  # noqa: F401
from .meshvoxels import carve_voxels, solid_iou_of_split, voxelise_meshes  # noqa: F401
from .voxeldist import (voxel_distance_transform, voxel_fscore, voxel_fscore_of_split, voxel_shell, voxel_signed_distance,  # noqa: F401
                        voxel_surface_stats)
from .pointmesh import fscore, fscore_of_split, point_mesh_distance  # noqa: F401
from .normals import estimate_normals, knn_batched, normal_consistency, normal_consistency_of_split  # noqa: F401
from .closest import closest_points_on_meshes, face_normals_at, point_surface_loss  # noqa: F401
from .winding import points_inside_meshes, signed_point_mesh_distance, winding_numbers, winding_voxels  # noqa: F401
from .raycast import ray_mesh_intersect, rays_hit_points, visible_points  # noqa: F401
from .surface import augment_mesh, extract_surface, extract_surfaces, save_obj  # noqa: F401
from .visualise import (camera_frame, read_png_any, render_point_cloud, render_point_clouds, render_split, write_png,  # noqa: F401
                        write_png_gray16, write_png_rgba)
from .meshviews import (ShadedScene, camera_extrinsic, features_of_views, load_obj_scene, load_obj_scene_shaded,  # noqa: F401
                        render_mesh_views, render_training_views, sample_camera_positions, view_rotation, view_transform)

__all__ = [
    "pointcloud_project_fast", "pointcloud_project", "pc_perspective_transform", "pointcloud2voxels3d_fast",
    "pointcloud2voxels", "pointcloud_project_exact",
    "smoothen_voxels3d", "smooth_voxels3d", "smoothing_kernel", "gauss_kernel_1d", "separable_kernels",
    "drc_projection", "drc_event_probabilities", "drc_depth_projection", "drc_depth_grid", "pc_point_dropout",
    "quaternion_rotate", "quaternion_multiply", "quaternion_conjugate", "quaternion_normalise",
    "get_smooth_sigma", "get_dropout_prob", "ProjectionOutputs", "silhouette_loss", "pointcloud_project_loss",
    "point_cloud_distance", "compute_distance", "chamfer_distances", "graphed_project_loss", "prefer_direct_graph_launch", "point_dropout_indices", "save_predictions", "load_predictions", "chamfer_of_predictions",
    "DeviceSchedule", "check_status", "set_debug_checks", "taps_bucket", "project_loss_step", "project_depth", "proj_depth_loss",
    "project_rgb", "proj_rgb_loss", "replicate_rgb", "rgb_grids", "drc_loss", "drc_rgb_loss",
    "icp_point_to_point", "alignment_to_ground_truth", "alignment_candidates", "reference_rotation", "quat_w_avg_markley",
    "quaternion_from_campos", "as_rotation_matrix", "from_rotation_matrix", "pose_errors",
    "nearest_batched", "chamfer_batched", "chamfer_loss", "chamfer_of_split", "eval_chamfer", "voxel_down_sample", "downsample_split",
    "emd_loss", "emd_match", "emd_of_split", "farthest_point_sample",
    "voxelise", "voxel_stats", "voxel_iou", "evaluate_voxel_prediction", "voxel2pc", "voxels2pc_batched", "iou_of_split",
    "render_voxels", "voxelise_meshes", "carve_voxels", "solid_iou_of_split",
    "voxel_distance_transform", "voxel_signed_distance", "voxel_shell", "voxel_surface_stats", "voxel_fscore", "voxel_fscore_of_split",
    "point_mesh_distance", "fscore", "fscore_of_split",
    "knn_batched", "estimate_normals", "normal_consistency", "normal_consistency_of_split",
    "closest_points_on_meshes", "point_surface_loss", "face_normals_at",
    "winding_numbers", "points_inside_meshes", "signed_point_mesh_distance", "winding_voxels",
    "ray_mesh_intersect", "rays_hit_points", "visible_points",
    "extract_surfaces", "extract_surface", "augment_mesh", "save_obj",
    "load_obj_mesh", "densify_meshes", "densify_split", "MeshError",
    "camera_frame", "render_point_clouds", "render_point_cloud", "render_split", "write_png",
    "write_png_rgba", "write_png_gray16", "read_png_any",
    "load_obj_scene", "sample_camera_positions", "view_rotation", "view_transform", "render_mesh_views", "camera_extrinsic",
    "features_of_views", "render_training_views", "load_obj_scene_shaded", "ShadedScene",
    "smooth_gt", "gauss_smoothen_image", "DeviceTaps",
]


# ------------------------------------------------------------------------------------------------------
# config helpers (duck-typed cfg: any object with attribute access; fields of SURVEY.md section 5)
# ------------------------------------------------------------------------------------------------------
def _get(cfg, key, default):
    try:
        return getattr(cfg, key)
    except (AttributeError, KeyError):
        return default


def _grid(cfg):
    G = int(cfg.vox_size)
    vz = int(_get(cfg, "vox_size_z", -1))
    return (G if vz == -1 else vz), G, G


def _check_live_branches(cfg):
    if not _get(cfg, "pose_quaternion", True):
        raise NotImplementedError("pose_quaternion: false is a broken branch of the reference "
                                  "(dpc/util/point_cloud_to.py:153 UnboundLocalError)")
    if _get(cfg, "ptn_max_projection", False):
        raise NotImplementedError("ptn_max_projection: true returns a tuple in the reference (point_cloud_to.py:234)")
    if not _get(cfg, "drc_logsum", True) or not _get(cfg, "drc_tf_cumulative", True):
        raise NotImplementedError("drc_logsum: false / drc_tf_cumulative: false are dead branches of the reference "
                                  "(dpc/util/drc.py:45,84-92)")


_plain_geometries = {}   # Geometry objects of calls without a Gaussian, by their constants


def _geometry(cfg, kernel=None, schedule=None):
    """Per-call constants as a Geometry.  Geometry objects are immutable after construction and cache their own DpcParams
    blocks and buffer sizes per call shape, so they are reused: one per (kernel list, grid, camera constants) -- kept on the
    KernelList smoothing_kernel returned (a list of bare tensors, as a caller other than this package's smoothing_kernel
    may pass, is converted on every call as before)."""
    D, H, W = _grid(cfg)
    key = (D, H, W, _get(cfg, "camera_distance", 2.0), _get(cfg, "focal_length", 1.875), _get(cfg, "drc_logsum_clip_val", 1e-5),
           _get(cfg, "max_depth", 10.0), id(schedule))
    cache = (kernel.geometries if isinstance(kernel, KernelList) and kernel.untouched()
             else (_plain_geometries if kernel is None else None))
    if cache is not None:
        hit = cache.get(key)
        if hit is not None and hit.schedule is schedule:
            if kernel is not None and not _get(cfg, "pc_separable_gauss_filter", True):
                _kernel_taps(cfg, kernel)   # raises
            return hit
    kxy = kz = None
    if kernel is not None:
        kxy, kz = _kernel_taps(cfg, kernel)
    geom = Geometry(D, H, W, kxy, kz, key[3], key[4], key[5], key[6], schedule=schedule)
    if cache is not None:
        if len(cache) >= 16:
            cache.clear()
        cache[key] = geom
    return geom


# ------------------------------------------------------------------------------------------------------
# Bad point indices: an error, never a GPU fault         reference: fancy indexing raises IndexError
# ------------------------------------------------------------------------------------------------------
_debug_checks = _os.environ.get("DPC_RENDER_DEBUG", "0") not in ("", "0")


def set_debug_checks(on=True):
    """Debug mode (also DPC_RENDER_DEBUG=1): every call with a `point_index` checks its range on the HOST before anything
    is launched (one device-to-host synchronisation per call) and raises IndexError like the reference's fancy indexing
    (dpc/util/point_cloud_to.py:266-295).  Off, the default: the kernels drop an out-of-range entry (it never becomes an
    address) and flag it in the device status word, which check_status() turns into the same IndexError later."""
    global _debug_checks
    _debug_checks = bool(on)


def _validate_point_index(point_index, point_cloud):
    if point_index is None or not _debug_checks or point_index.numel() == 0:
        return
    lo, hi = int(point_index.min()), int(point_index.max())
    n = point_cloud.shape[1]
    if lo < 0 or hi >= n:
        raise IndexError("point_index holds %d (valid: 0 .. %d): index out of range for a point set of %d points"
                         % (lo if lo < 0 else hi, n - 1, n))


def check_status(device=None):
    """Read and clear the device status word (one synchronisation): raises IndexError when a `point_index` entry of any
    call since the last check was outside its point set -- the reference raises at the call itself; here the kernels dropped
    the point, flagged it and went on, and the error surfaces where the caller synchronises anyway (reading the loss, a
    checkpoint)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    word = status_word(dev)
    bits = int(word.item())
    if bits:
        word.zero_()
    if bits & _native.DPC_STATUS_BAD_INDEX:
        raise IndexError("dpc.render: a point_index entry was out of range for its point set (the point was dropped); "
                         "set DPC_RENDER_DEBUG=1 to find the call")
    return bits


def _kernel_taps(cfg, kernel):
    """Host tap arrays (x/y, z) from what smoothing_kernel returns: a list of three 5-D kernels
    [1,1,1,1,k], [1,1,1,k,1], [1,1,kz,1,1] applied in that order; a bare 1-D tensor is accepted too."""
    if not _get(cfg, "pc_separable_gauss_filter", True):
        raise NotImplementedError("pc_separable_gauss_filter: false leaves `kernel` unbound in the reference "
                                  "(dpc/util/gauss_kernel.py:52-55)")
    if isinstance(kernel, KernelList) and kernel.untouched():   # what smoothing_kernel returned: its host taps travel with it
        return kernel.taps
    host = lambda k: np.ascontiguousarray(k.detach().cpu().numpy() if isinstance(k, torch.Tensor) else k,
                                          dtype=np.float32).reshape(-1)
    if isinstance(kernel, (list, tuple)):
        if len(kernel) != 3:
            raise ValueError("kernel must be the list of 3 separable kernels returned by smoothing_kernel")
        kx, ky, kz = host(kernel[0]), host(kernel[1]), host(kernel[2])
        if kx.shape != ky.shape or not np.array_equal(kx, ky):
            raise NotImplementedError("different x and y kernels: smoothing_kernel never produces them")
        return kx, kz
    k = host(kernel)
    return k, k


# ------------------------------------------------------------------------------------------------------
# Gaussian kernels                                   reference: dpc/util/gauss_kernel.py
# ------------------------------------------------------------------------------------------------------
def gauss_kernel_1d(l, sig):
    """1-D Gaussian of side length l, fp32, normalised (dpc/util/gauss_kernel.py:5-11).  Host tensor: the
    weights travel to the GPU as kernel arguments, not as a device tensor."""
    x = torch.arange(float((-l) // 2) + 1.0, l // 2 + 1)
    k = torch.exp(-x ** 2 / (2.0 * sig ** 2))
    return k / k.sum()


class KernelList(list):
    """The list of three separable kernels smoothing_kernel returns -- a plain list to every caller (the reference passes it
    straight on to pointcloud_project_fast, dpc/models/model_pc_to.py:171-179, 262-265) that also carries what this package
    derives from it on every call: the host tap arrays (`taps`) and the per-grid Geometry objects built from them
    (`geometries`), so that a step pays for them once per kernel instead of once per call."""

    __slots__ = ("taps", "geometries", "_made_of")

    def __init__(self, items):
        super().__init__(items)
        kx, kz = (np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32).reshape(-1) for t in (items[0], items[2]))
        self.taps = (kx, kz)
        self.geometries = {}
        self._made_of = tuple(id(t) for t in items)

    def untouched(self):
        """Still the three tensors it was built from (a caller that replaced an element gets the slow, re-reading path)."""
        return len(self) == 3 and tuple(id(t) for t in self) == self._made_of


def separable_kernels(kernel):
    """[1,1,1,1,k], [1,1,1,k,1], [1,1,k,1,1] views of a 1-D kernel (dpc/util/gauss_kernel.py:27-32)."""
    n = kernel.shape[0]
    return KernelList([kernel.reshape((1, 1, 1, 1, n)), kernel.reshape((1, 1, 1, n, 1)), kernel.reshape((1, 1, n, 1, 1))])


_kernel_cache = {}     # (taps, sigma, z taps, z sigma) -> KernelList; a training loop asks for the same sigma_rel every step
                       # until the schedule moves it (model_pc_to.py:59-63), a benchmark loop for ever


def smoothing_kernel(cfg, sigma):
    """The three separable kernels for pc_gauss_kernel_size and sigma (in voxels)
    (dpc/util/gauss_kernel.py:35-55).  With vox_size_z != vox_size the z kernel has length
    floor(fsz*ratio)|1 and sigma*ratio -- what the reference intends; its own reshape at :49 raises.
    The result for a given (size, sigma) is memoised (the last few): the tensors are never modified by this package."""
    fsz = int(cfg.pc_gauss_kernel_size)
    vz = int(_get(cfg, "vox_size_z", -1))
    fz, ratio = fsz, 1.0
    if vz != -1:
        ratio = vz / int(cfg.vox_size)
        fz = int(np.floor(fsz * ratio))
        if fz % 2 == 0:
            fz += 1
    elif not _get(cfg, "pc_separable_gauss_filter", True):
        raise NotImplementedError("pc_separable_gauss_filter: false leaves `kernel` unbound in the reference "
                                  "(dpc/util/gauss_kernel.py:52-55)")
    key = (fsz, float(sigma), fz, float(ratio))
    hit = _kernel_cache.get(key)
    if hit is not None:
        return hit
    k = gauss_kernel_1d(fsz, sigma)
    if vz != -1:
        kz = k if (fz == fsz and ratio == 1.0) else gauss_kernel_1d(fz, sigma * ratio)
        out = KernelList([k.reshape((1, 1, 1, 1, fsz)), k.reshape((1, 1, 1, fsz, 1)), kz.reshape((1, 1, fz, 1, 1))])
    else:
        out = separable_kernels(k)
    if len(_kernel_cache) >= 8:
        _kernel_cache.pop(next(iter(_kernel_cache)))
    _kernel_cache[key] = out
    return out


# ------------------------------------------------------------------------------------------------------
# Quaternion helpers (host-side mirror; the fused kernels rotate in-register)   dpc/util/quaternion.py
# ------------------------------------------------------------------------------------------------------
def quaternion_multiply(a, b):
    """Hamilton product, (w,x,y,z) order (dpc/util/quaternion.py:69-86); 3-vectors get a leading 0."""
    pad = lambda v: torch.nn.functional.pad(v, (1, 0)) if v.shape[-1] == 3 else v
    a, b = pad(a), pad(b)
    if a.shape[-1] != 4 or b.shape[-1] != 4:
        raise ValueError("Can't create a quaternion: the last dimension must be 3 or 4.")
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx), dim=-1)


def quaternion_conjugate(q):
    """[w, -x, -y, -z] (dpc/util/quaternion.py:89-92)."""
    return torch.cat((q[..., :1], -q[..., 1:]), dim=-1)  # no host constant: usable while a HIP graph is being captured


def quaternion_normalise(q):
    """q / |q| (dpc/util/quaternion.py:100-107)."""
    return q / q.norm(p=2, dim=-1, keepdim=True)


def quaternion_rotate(pc, q, inverse=False):
    """Rotate [B,N,3] points by [B,4] quaternions, norm not detached (dpc/util/quaternion.py:110-132)."""
    qn = quaternion_normalise(q).unsqueeze(1)
    qc = quaternion_conjugate(qn)
    w = quaternion_multiply(quaternion_multiply(qc, pc), qn) if inverse else quaternion_multiply(quaternion_multiply(qn, pc), qc)
    return w[:, :, 1:4]


# ------------------------------------------------------------------------------------------------------
# Stage functions                                    reference: dpc/util/point_cloud_to.py, dpc/util/drc.py
# ------------------------------------------------------------------------------------------------------
def pc_perspective_transform(cfg, point_cloud, transform, predicted_translation=None, focal_length=None):
    """[B,N,3] xyz -> [B,N,3] (z, y, x) camera-space coordinates (dpc/util/point_cloud_to.py:118-178)."""
    _check_live_branches(cfg)
    return Transform.apply(point_cloud, transform, predicted_translation, focal_length, _geometry(cfg))


def pointcloud2voxels3d_fast(cfg, pc, rgb=None):
    """Trilinear splat of transformed points into [B,D,H,W] (dpc/util/point_cloud_to.py:10-87).
    Returns (voxels, None) like the reference."""
    if rgb is not None:
        raise NotImplementedError("rgb splatting is a dead branch of the reference (point_cloud_to.py:64 AttributeError)")
    return Splat.apply(pc, _geometry(cfg)), None


def smoothen_voxels3d(cfg, voxels, kernel):
    """Separable zero-padded Gaussian over [B,1,D,H,W] in W,H,D order (dpc/util/point_cloud_to.py:90-103)."""
    D, H, W = voxels.shape[-3:]
    kxy, kz = _kernel_taps(cfg, kernel)
    return Smooth.apply(voxels, Geometry(D, H, W, kxy, kz))


smooth_voxels3d = smoothen_voxels3d


def _drc_geometry(voxels, cfg):
    B, D, H, W = voxels.shape[:4]
    return Geometry(D, H, W, None, None, _get(cfg, "camera_distance", 2.0), _get(cfg, "focal_length", 1.875),
                    _get(cfg, "drc_logsum_clip_val", 1e-5), _get(cfg, "max_depth", 10.0))


def drc_event_probabilities(voxels, cfg):
    """Ray-termination probabilities [D+1,B,H,W,1] of a [B,D,H,W,1] occupancy grid (dpc/util/drc.py:109-111)."""
    _check_live_branches(cfg)
    _, probs, _ = Drc.apply(voxels.squeeze(-1), _drc_geometry(voxels, cfg))
    return probs.unsqueeze(-1)


def drc_projection(voxels, cfg):
    """(silhouette [B,H,W,1], probabilities [D+1,B,H,W,1]) (dpc/util/drc.py:114-129)."""
    _check_live_branches(cfg)
    proj, probs, _ = Drc.apply(voxels.squeeze(-1), _drc_geometry(voxels, cfg))
    return proj.unsqueeze(-1), probs.unsqueeze(-1)


def drc_depth_grid(cfg, z_size):
    """psi_k = k/D - 1/2 + camera_distance, last = max_depth (dpc/util/drc.py:145-149)."""
    i = torch.arange(0, z_size, 1, dtype=torch.float64)
    return torch.cat([i / z_size - 0.5 + cfg.camera_distance, torch.tensor([cfg.max_depth], dtype=torch.float64)])


def drc_depth_projection(p, cfg):
    """Expected depth sum_k p_k psi_k of probabilities [D+1,B,H,W,1] (dpc/util/drc.py:152-160)."""
    psi = drc_depth_grid(cfg, p.shape[0] - 1).to(device=p.device, dtype=p.dtype).reshape(-1, 1, 1, 1, 1)
    return (p * psi).sum(0)


# ------------------------------------------------------------------------------------------------------
# The projection                                     reference: dpc/util/point_cloud_to.py:191-263
# ------------------------------------------------------------------------------------------------------
class ProjectionOutputs(dict):
    """The reference's output dict.  `proj` (what the training loss consumes) comes from the fused kernels; the other
    entries are produced on first access, differentiably, so a step that never reads them never pays for them -- and a
    caller that reads them every step (ModelPointCloud.compute_projection does, dpc/models/model_pc_to.py:266-269) pays for
    what it reads only: `builder` is one callable for all lazy keys, or a dict key -> callable; a callable returns a dict
    and may fill several keys at once."""

    _LAZY = ("voxels", "tr_pc", "drc_probs", "proj_depth")

    def __init__(self, proj, builder, fused=None):
        super().__init__(proj=proj, voxels_rgb=None, proj_rgb=None)
        self._fused = fused   # (geom, grid_wh, s) of the fused path: what project_depth / proj_depth_loss start from
        self._builders = builder if isinstance(builder, dict) else {k: builder for k in self._LAZY}
        for k in self._LAZY:
            dict.__setitem__(self, k, None)
        self._pending = set(self._LAZY)

    def _materialise(self, key):
        if key in self._pending:
            for k, v in self._builders[key]().items():
                if k in self._pending:
                    dict.__setitem__(self, k, v)
                    self._pending.discard(k)
            self._pending.discard(key)

    def __getitem__(self, key):
        self._materialise(key)
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        self._materialise(key)
        return dict.get(self, key, default)

    def _materialise_all(self):
        for k in list(self._pending):
            self._materialise(k)

    def values(self):
        self._materialise_all()
        return dict.values(self)

    def items(self):
        self._materialise_all()
        return dict.items(self)


_OUTSIDE = 2.0   # a coordinate outside the unit cube [-1/2, 1/2]^3: such a point splats nothing (point_cloud_to.py:26-27)


def _mask_dead_slots(tr, schedule):
    """Under a DeviceSchedule with a live-point count, a cloud's row has `capacity` slots of which only the first *n_live hold
    points (k_locate turns the others into out-of-bounds records).  The stage-level path does the same without reading the
    count on the host (so it stays capturable): the transformed coordinates of the dead slots are replaced by a constant
    outside the unit cube -- no splat, no gradient -- which is also what `tr_pc` shows in those slots."""
    if schedule is None or schedule.n_live is None:
        return tr
    dead = (torch.arange(tr.shape[1], device=tr.device, dtype=torch.int32) >= schedule.n_live).view(1, -1, 1)
    return torch.where(dead, torch.full_like(tr, _OUTSIDE), tr)


def _outputs_from_grid(cfg, geom, grid_wh, pc, q, t, f, s, point_index):
    """Lazy entries of the output dict derived from what the fused forward left behind: `tr_pc` is one transform launch;
    `voxels`, `drc_probs`, `proj_depth` start from grid_wh (the grid after clamp and the W, H passes, a differentiable
    output of the fused node): D pass, occupancy scale + clamp, DRC probabilities and depth -- no second transform, splat
    or W/H smoothing (reference: point_cloud_to.py:95-97 third pass, :218-222, :228-247)."""
    def tr_pc():
        pts = pc
        if pts.shape[0] != q.shape[0]:
            pts = pts.repeat_interleave(q.shape[0] // pts.shape[0], dim=0)
        if point_index is not None:
            pts = pts.gather(1, point_index.long().unsqueeze(-1).expand(-1, -1, 3))
        return {"tr_pc": _mask_dead_slots(Transform.apply(pts, q, t, f, geom), geom.schedule)}

    cache = {}

    def voxels():
        if "vox" not in cache:
            vox = grid_wh
            if geom.kz is not None:
                vox = Smooth.apply(vox, Geometry(geom.D, geom.H, geom.W, None, geom.kz, schedule=geom.schedule))
            if s is not None:
                vox = torch.clamp(vox * s.reshape(-1, 1, 1, 1).to(vox.dtype), 0.0, 1.0)
            cache["vox"] = vox
        return cache["vox"]

    def vox_entry():
        return {"voxels": voxels().unsqueeze(-1)}

    def drc_entries():
        _, probs, _ = Drc.apply(voxels(), geom)
        probs = torch.flip(probs, [2]).unsqueeze(-1)
        return {"drc_probs": probs, "proj_depth": drc_depth_projection(probs, cfg)}

    return {"tr_pc": tr_pc, "voxels": vox_entry, "drc_probs": drc_entries, "proj_depth": drc_entries}


def _project_staged(cfg, geom, pc, q, t, f, s, smooth, point_index=None):
    """The same chain composed from the stage-level kernels (all differentiable)."""
    if pc.shape[0] != q.shape[0]:  # shared point sets: the stage kernels want one cloud per pose
        pc = pc.repeat_interleave(q.shape[0] // pc.shape[0], dim=0)
    if point_index is not None:    # every cloud's own subset, materialised
        pc = pc.gather(1, point_index.long().unsqueeze(-1).expand(-1, -1, 3))
    tr = _mask_dead_slots(Transform.apply(pc, q, t, f, geom), geom.schedule)
    raw = Splat.apply(tr, geom)
    vox = torch.clamp(raw, 0.0, 1.0)
    if smooth and geom.kxy is not None:
        vox = Smooth.apply(vox, geom)
    if s is not None:
        vox = torch.clamp(vox * s.reshape(-1, 1, 1, 1).to(vox.dtype), 0.0, 1.0)
    proj, probs, _ = Drc.apply(vox, geom)
    probs = torch.flip(probs, [2]).unsqueeze(-1)
    depth = drc_depth_projection(probs, cfg)
    return {"proj": torch.flip(proj, [1]).unsqueeze(-1), "voxels": vox.unsqueeze(-1), "tr_pc": tr,
            "drc_probs": probs, "proj_depth": depth}


def pointcloud_project_fast(cfg, point_cloud, transform, predicted_translation, all_rgb, kernel=None,
                            scaling_factor=None, focal_length=None, smooth=True, point_index=None, schedule=None):
    """Project [B,N,3] point clouds to [B,H,W,1] silhouettes (dpc/util/point_cloud_to.py:191-263).

    Same positional signature as the reference; returns a dict with the reference's keys
    (proj, voxels, tr_pc, voxels_rgb, proj_rgb, drc_probs, proj_depth).  `smooth=False` reproduces the
    reference's CPU branch, which skips the Gaussian (:210-212).

    Shared point sets: `point_cloud` may be [B/R,N,3] while `transform` (and the other per-cloud
    inputs) have B rows -- clouds b*R .. b*R+R-1 then use point set b, the layout tf_repeat_0 produces for the views and
    pose candidates of one object (dpc/models/model_pc_to.py:302-306), without materialising the B copies; the
    gradient comes back as [B/R,N,3], summed over the replicas inside the backward kernel.

    Per-cloud point subsets (point dropout without copies): `point_index` [B,n] integer tensor -- cloud b projects the points
    point_cloud[b // R][point_index[b]] only.  This is pc_point_dropout applied AFTER tf_repeat_0 as the reference does
    (model_pc_to.py:254-258: every replica drops its own points) with neither the replicated [B,N,3] tensor nor the
    gathered [B,n,3] one; the gradient has the shape of `point_cloud` (zeros at points no cloud kept).  Indices from
    dpc.render.point_dropout_indices (device RNG) or any other source; they may repeat.  An entry outside the point set is
    an IndexError: at once with set_debug_checks() / DPC_RENDER_DEBUG=1, otherwise from check_status() (the kernels drop the
    point and flag it; nothing out of range is ever read or written).

    `schedule` (a DeviceSchedule): the Gaussian's tap values and the number of live points are read from device memory at
    run time -- for a call captured in a HIP graph whose sigma / keep-count follow a schedule; `kernel` then only fixes the
    compiled tap windows (see DeviceSchedule)."""
    if all_rgb is not None:
        raise NotImplementedError("all_rgb: the rgb branch of the reference is dead (point_cloud_to.py:64 AttributeError); "
                                  "colour is a node of its own on the projection: dpc.render.project_rgb / proj_rgb_loss")
    _check_live_branches(cfg)
    _validate_point_index(point_index, point_cloud)
    geom = _geometry(cfg, kernel if smooth else None, schedule if smooth else None)
    staged = lambda: _project_staged(cfg, geom, point_cloud, transform, predicted_translation, focal_length,
                                     scaling_factor, smooth, point_index)
    try:
        proj, grid_wh = ProjectFused.apply(point_cloud, transform, predicted_translation, focal_length, scaling_factor, geom,
                                           point_index, torch.is_grad_enabled())
    except _native.DpcError as e:
        if e.code != _native.DPC_ERR_TAPS:
            raise
        # effective Gaussian radius > 15 voxels: beyond the fused kernels' register window; same math, staged
        out = staged()
        return ProjectionOutputs(out["proj"], lambda: out)
    return ProjectionOutputs(proj, _outputs_from_grid(cfg, geom, grid_wh, point_cloud, transform, predicted_translation,
                                                      focal_length, scaling_factor, point_index),
                             fused=(geom, grid_wh, scaling_factor))


pointcloud_project = pointcloud_project_fast


# ------------------------------------------------------------------------------------------------------
# The exact Gaussian occupancy (cfg.pc_fast == false)   reference: dpc/util/point_cloud.py:17-57, 219-226 (TF-1 original)
# ------------------------------------------------------------------------------------------------------
def _gauss_normalise(cfg):
    """point_cloud.py:43-51: pc_normalise_gauss wins, then pc_normalise_gauss_analytical (the default), then neither."""
    if _get(cfg, "pc_normalise_gauss", False):
        return _native.DPC_GAUSS_NORM_PER_POINT
    if _get(cfg, "pc_normalise_gauss_analytical", True):
        return _native.DPC_GAUSS_NORM_ANALYTICAL
    return _native.DPC_GAUSS_NORM_NONE


def _gauss_sigma(sigma):
    """sigma is a launch argument of this path: a number, or a one-element tensor on the host."""
    if isinstance(sigma, torch.Tensor):
        if sigma.is_cuda:
            raise ValueError("sigma must be a number or a host tensor: the exact renderer takes it as a launch argument")
        sigma = sigma.item()
    sigma = float(sigma)
    if not (sigma > 0.0) or sigma == float("inf"):
        raise ValueError("sigma must be positive and finite, got %r" % sigma)
    return sigma


def _gauss_grid(cfg):
    if int(_get(cfg, "vox_size_z", -1)) != -1:
        raise NotImplementedError("vox_size_z: pointcloud2voxels reads vox_size only (point_cloud.py:23-26), a grid with "
                                  "its own depth cannot broadcast in the reference")
    return int(cfg.vox_size)


def _gauss_voxels(cfg, tr, sigma):
    """[B,D,H,W] with axes following components 0, 1, 2 of tr: the kernels' layout."""
    if not torch.is_grad_enabled():
        # ctx.needs_input_grad follows requires_grad alone, also where no graph is recorded: detached, the node neither
        # allocates nor writes the sums before the clip, which only a backward reads
        tr = tr.detach()
    return GaussVoxels.apply(tr, _gauss_grid(cfg), _gauss_sigma(sigma), _gauss_normalise(cfg))


def pointcloud2voxels(cfg, input_pc, sigma):
    """Every point an isotropic Gaussian evaluated at every voxel centre of the grid linspace(-1, 1, vox_size)^3, summed
    over the points and clipped to [0,1] (dpc/util/point_cloud.py:17-57): [B,N,3] -> [B,G,G,G,1].

    The grid axes follow (input_pc[...,1], input_pc[...,0], input_pc[...,2]), the effect of tf.meshgrid's default 'xy'
    indexing; the kernels write axes following components 0, 1, 2, and this returns the transposed VIEW of that grid, not a
    copy.  cfg.pc_normalise_gauss / pc_normalise_gauss_analytical pick the normalisation like there.  No outlier filter:
    a point outside the cube adds its tail.  sigma: a number (absolute, the caller divides sigma_rel by vox_size)."""
    return _gauss_voxels(cfg, input_pc, sigma).transpose(1, 2).unsqueeze(-1)


def pointcloud_project_exact(cfg, point_cloud, transform, sigma):
    """pointcloud_project of the TF-1 original (dpc/util/point_cloud.py:219-226), the renderer of cfg.pc_fast == false:
    perspective transform, exact Gaussian occupancy, DRC silhouette.  Returns (proj [B,G,G,1], voxels [B,G,G,G,1]) like
    there.  Against pointcloud_project_fast: the grid spans [-1,1]^3, there is no outlier filter, no occupancy scale, no
    translation and no learned focal length (the reference passes none of them on this path), and sigma is a launch
    argument, so the call cannot follow a sigma schedule inside a captured graph."""
    _check_live_branches(cfg)
    G = _gauss_grid(cfg)
    geom = _geometry(cfg)
    tr_pc = Transform.apply(point_cloud, transform, None, None, geom)            # :220
    voxels = pointcloud2voxels(cfg, tr_pc, sigma)                                # :221
    voxels = voxels.permute(0, 2, 1, 3, 4)                                       # :222, the kernels' own layout again
    proj, _, _ = Drc.apply(voxels.squeeze(-1), Geometry(G, G, G, None, None, geom.camera_distance, geom.focal_length,
                                                        geom.clip_val, geom.max_depth))   # :224
    return torch.flip(proj, [1]).unsqueeze(-1), voxels                           # :225


def pointcloud_project_loss(cfg, point_cloud, transform, predicted_translation, all_rgb, kernel=None,
                            scaling_factor=None, focal_length=None, gt=None, num_candidates=1, smooth=True, point_index=None,
                            schedule=None, valid_samples=None):
    """pointcloud_project_fast followed by the model's projection loss, as ONE autograd node.

    What ModelPointCloud does in two steps -- compute_projection (dpc/models/model_pc_to.py:239-282) then
    add_proj_loss / proj_loss_pose_candidates (:339-385, 410-440) -- with the loss folded into the ray-march
    kernels: `gt` is the reference's inputs["masks"] as it is, [S,1,Hm,Wm] (or [S,Hm,Wm,1]) with Hm = f*H, Wm = f*W
    -- the kernels average-pool it f x f where they read a pixel, the bits of nn.AvgPool2d(f) (model_pc_to.py:346-354) --
    or [S,H,W,1] already pooled; `valid_samples` [S] | None is inputs["valid_samples"] (cfg.variable_num_views,
    :432-436).  `point_cloud` holds S*num_candidates clouds (candidate-minor, like tf_repeat_0).  Returns (loss, outputs,
    winner): the scalar loss sum_s w_s^2 min_k sum (gt-pred)^2 / S (w = valid_samples, 1 when None; the selection is
    unweighted), the usual output dict (`proj` from this pass, the rest lazy), and the
    winning candidate per sample.  Falls back to pointcloud_project_fast + silhouette_loss when the Gaussian is
    too long for the fused kernels.  `point_cloud` may hold shared point sets ([B/R,N,3]) and `point_index` per-cloud
    subsets of them (see pointcloud_project_fast).  Under cfg.pc_gauss_filter_gt `gt` must be the [S,H,W,1] masks
    smooth_gt prepared: full-size masks would be pooled without the smoothing and are refused."""
    if all_rgb is not None:
        raise NotImplementedError("all_rgb: the rgb branch of the reference is dead (point_cloud_to.py:64 AttributeError); "
                                  "colour is a node of its own on the projection: dpc.render.project_rgb / proj_rgb_loss")
    if gt is None:
        raise ValueError("gt (masks [S,1,Hm,Wm], or pooled [S,H,W,1]) is required")
    if gt.shape[0]:
        _refuse_full_size_masks(cfg, gt, _grid(cfg)[1] * _grid(cfg)[2], "pointcloud_project_loss")
    _check_live_branches(cfg)
    _validate_point_index(point_index, point_cloud)
    geom = _geometry(cfg, kernel if smooth else None, schedule if smooth else None)
    staged = lambda: _project_staged(cfg, geom, point_cloud, transform, predicted_translation, focal_length,
                                     scaling_factor, smooth, point_index)
    try:
        loss, proj, winner = ProjectLossFused.apply(point_cloud, transform, predicted_translation, focal_length,
                                                    scaling_factor, gt, geom, num_candidates, point_index,
                                                    torch.is_grad_enabled(), valid_samples)
    except _native.DpcError as e:
        if e.code != _native.DPC_ERR_TAPS:
            raise
        out = pointcloud_project_fast(cfg, point_cloud, transform, predicted_translation, None, kernel, scaling_factor,
                                      focal_length, smooth, point_index, schedule)
        loss, winner = silhouette_loss(out["proj"], gt, num_candidates, valid_samples)
        return loss, out, winner
    return loss, ProjectionOutputs(proj, staged), winner


def project_loss_step(cfg, kernel, num_clouds, num_points, device, schedule=None, num_candidates=1, point_replicas=1):
    """A ProjectLossStep plan for pointcloud_project_loss + backward at fixed shapes (`num_candidates` pose candidates per
    sample, `point_replicas` clouds per shared point set): static buffers, ONE native call per step that enqueues the four kernels -- instead of capturing the autograd path into a HIP
    graph (same kernels, same bits, 2-3 us per step faster than the replay on MI355X).  See dpc.render._ops.ProjectLossStep;
    reference call sequence: compute_projection + add_proj_loss + loss.backward() (dpc/models/model_pc_to.py:239-282, 339-385;
    dpc/run/train_to.py:122)."""
    _check_live_branches(cfg)
    return ProjectLossStep(_geometry(cfg, kernel, schedule), num_clouds, num_points, device, num_candidates, point_replicas)


def graphed_project_loss(cfg, kernel, point_cloud, transform, scaling_factor, gt, num_candidates=1):
    """pointcloud_project_loss for an eager training loop, captured into HIP graphs once.

    An eager call costs ~0.25-0.4 ms of Python, ctypes and allocator work for ~65 us of GPU time; this returns
    `step(point_cloud, transform, scaling_factor, gt) -> loss` built with torch.cuda.make_graphed_callables: forward and
    backward are each one graph launch, autograd works as usual (`loss.backward()`), results are the eager ones
    (bench: 379 -> 137 us per fwd+bwd at B=32, N=8000, 64^3).  The arguments are SAMPLE tensors fixing shapes, dtypes,
    device and requires_grad; what is frozen into the graphs: cfg, the Gaussian kernel (re-create the step when
    get_smooth_sigma has moved noticeably), num_candidates and the shapes.  Translation / focal-length inputs and the lazy
    output dict are not part of this shortcut -- use pointcloud_project_loss for those."""
    def step(pc, q, s, g):
        return pointcloud_project_loss(cfg, pc, q, None, None, kernel, scaling_factor=s, gt=g, num_candidates=num_candidates)[0]

    sample = tuple(t.detach().clone().requires_grad_(t.requires_grad) for t in (point_cloud, transform, scaling_factor, gt))
    return torch.cuda.make_graphed_callables(step, sample)


def pc_point_dropout(points, rgb, keep_prob):
    """Keep int(N*keep_prob) random points per cloud (dpc/util/point_cloud_to.py:269-295).  Same host RNG
    protocol as the reference (one np.random.choice(N, n, replace=False) per cloud, in batch order), so a
    seeded run selects the same points; the gather itself runs on the device."""
    B, Npts = points.shape[0], points.shape[1]
    n_out = int(Npts * keep_prob)
    idx = np.stack([np.random.choice(Npts, n_out, replace=False) for _ in range(B)]).astype(np.int64)
    idx_t = torch.from_numpy(idx).to(points.device)
    rows = torch.arange(B, device=points.device).unsqueeze(1)
    out_points = points[rows, idx_t]
    out_rgb = rgb[rows, idx_t] if rgb is not None else None
    return out_points, out_rgb


def prefer_direct_graph_launch():
    """Ask the ROCm runtime to replay HIP graphs as ordinary dispatches instead of pre-built AQL packets ("graph packet
    capture", the default of ROCm 7): on MI355X every kernel boundary inside a replayed graph is about 1 us shorter that way
    (the four-kernel fwd+bwd step: 61.2 -> 57.2 us).  The runtime reads the setting once, when HIP initialises, so this
    must run before the first CUDA call of the process (importing torch is fine); an explicit
    DEBUG_CLR_GRAPH_PACKET_CAPTURE in the environment wins.  Returns True when the setting is in force for this process."""
    if not torch.cuda.is_initialized():
        _os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
    # once HIP is up the runtime has read the variable: what the process started with stays
    return _os.environ.get("DEBUG_CLR_GRAPH_PACKET_CAPTURE") == "0"


def point_dropout_indices(num_clouds, num_points, keep_prob, device, generator=None, n_live=None):
    """Indices of pc_point_dropout (point_cloud_to.py:269-295) drawn on the device: for each of `num_clouds` clouds,
    int(num_points * keep_prob) DISTINCT point indices, a uniformly random subset (the same distribution as the reference's
    np.random.choice(replace=False), a different random stream), ascending.  int32 [num_clouds, n] for the `point_index`
    argument of pointcloud_project_fast / pointcloud_project_loss.

    Two 64-bit seed words come from torch's generator (`generator`, or the device's default one) and stay on the device;
    the choice itself is one kernel of this library (dpc_point_dropout_indices: hashed keys + radix select).  No host work,
    no upload, no sync, and safe inside HIP-graph capture: torch advances the generator at every replay, so every replay
    draws anew.  (torch.topk / sort are NOT used here: replayed from a graph they returned out-of-range indices at
    [128, 8000] on this ROCm build -- tests/test_gpu_parity.py::test_point_dropout_indices_in_a_replayed_graph.)

    `n_live` (int32 device tensor [1], e.g. DeviceSchedule.n_live): the rows keep their int(num_points * keep_prob) slots
    (the capacity) but only the first min(n_live, capacity) of each are filled, the count being read on the device -- a
    captured graph then follows the keep-probability schedule from replay to replay (hand the same tensor to the
    projection through its DeviceSchedule, which skips the unfilled slots)."""
    N = _native
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("dpc.render: point_dropout_indices draws on a GPU, got device %s" % device)
    keep = int(num_points * keep_prob)
    if not 0 <= keep <= num_points:
        raise ValueError("keep_prob %r leaves %d of %d points" % (keep_prob, keep, num_points))
    seed = torch.randint(-2 ** 62, 2 ** 62, (2,), dtype=torch.int64, device=device, generator=generator)
    out = torch.empty((num_clouds, keep), dtype=torch.int32, device=device)
    if n_live is not None:
        out.zero_()   # slots beyond the live count are never read by the kernels; zeros keep a debug range check quiet
    N.call(device, "dpc_point_dropout_indices_live", int(num_clouds), int(num_points), keep, N.ptr(n_live), N.ptr(seed),
           N.ptr(out))
    return out


# ------------------------------------------------------------------------------------------------------
# The caller's silhouette loss                       reference: dpc/models/model_pc_to.py:339-385, 410-440
# ------------------------------------------------------------------------------------------------------
def _refuse_full_size_masks(cfg, gt, n_pix, where):
    """cfg.pc_gauss_filter_gt with masks that are not at the silhouette's size yet: they have not been through smooth_gt."""
    if _get(cfg, "pc_gauss_filter_gt", False) and gt[0].numel() != n_pix:
        raise NotImplementedError("pc_gauss_filter_gt: true -- %s got full-size masks %s; it pools them but does not smooth "
                                  "them. Prepare them with dpc.render.smooth_gt(cfg, masks, size, 'masks', ...) and pass the "
                                  "[S,H,W,1] result (model_pc.py:398-404)" % (where, tuple(gt.shape)))


def silhouette_loss(pred, gt, num_candidates=1, valid_samples=None, cfg=None):
    """Projection loss of ModelPointCloud.add_proj_loss, fused with its gradient in one kernel.

    pred [S*K,H,W,1] candidate silhouettes; gt the masks [S,1,f*H,f*W] (or [S,f*H,f*W,1]), average-pooled f x f inside the
    kernel like the reference's AvgPool2d (model_pc_to.py:348-369, the same bits), or [S,H,W,1] already pooled;
    valid_samples [S] | None the per-sample weights w (:432-436).  K = 1: sum w^2 (gt-pred)^2 / S.  K > 1
    (proj_loss_pose_candidates): per sample the candidate with the smallest (unweighted) sum of squared differences wins
    and only winners contribute, w^2-weighted.  Returns (loss, winner [S] int32).
    cfg (optional): with cfg.pc_gauss_filter_gt, masks larger than the silhouettes are refused -- the kernel pools, it does
    not smooth; the smoothed masks come from smooth_gt(cfg, masks, size, "masks", ...) and arrive here as [S,H,W,1]."""
    if cfg is not None and gt.shape[0] and pred.shape[0]:
        _refuse_full_size_masks(cfg, gt, pred[0].numel(), "silhouette_loss")
    return SilhouetteLoss.apply(pred, gt, num_candidates, valid_samples)


# ------------------------------------------------------------------------------------------------------
# Depth supervision                                  reference: dpc/util/losses.py:113-136 (add_proj_depth_loss)
# ------------------------------------------------------------------------------------------------------
def _fused_parts(outputs):
    if not isinstance(outputs, ProjectionOutputs):
        raise TypeError("outputs must be what pointcloud_project_fast returned, got %s" % type(outputs).__name__)
    return outputs._fused


def project_depth(outputs):
    """Expected depth [B,H,W,1] of the projection `outputs` (what pointcloud_project_fast returned): the values of
    outputs["proj_depth"] (drc_depth_projection, dpc/util/drc.py:152-160, rows flipped like proj) from one column kernel on
    the fused node's grid instead of a smoothed grid plus the [D+1,B,H,W] probabilities; differentiable.  Outputs of the
    staged fallback (a Gaussian longer than the fused window) hand back their own proj_depth."""
    fused = _fused_parts(outputs)
    if fused is None:
        return outputs["proj_depth"]
    geom, grid_wh, s = fused
    return DepthMap.apply(grid_wh, s, geom)


def proj_depth_loss(cfg, outputs, depths, valid_samples=None, return_depth=False, gt_prepared=False):
    """add_proj_depth_loss (dpc/util/losses.py:113-136) without its weight: (1/2) sum_s w_s^2 sum_pix (g - depth)^2 / S.
    return_depth: (loss, depth [S,H,W,1] detached) -- the map the loss was formed from, written by the same launch.

    outputs: what pointcloud_project_fast returned for S clouds (one per sample); depths: inputs["depths"], [S,Hd,Wd,1],
    [S,1,Hd,Wd] or [S,Hd,Wd] with Hd = f*H, Wd = f*W for an integer f >= 1 -- g[s,y,x] = depths[s,f*y,f*x], the reference's
    tf.image.resize_images(..., NEAREST_NEIGHBOR), and g = cfg.max_depth where depths == cfg.max_dataset_depth when the two
    differ; valid_samples [S] | None: per-sample weights w, squared like silhouette_loss's (None, the reference: all ones).
    The caller multiplies by cfg.proj_depth_weight.  On the fused path the whole loss is two launches forward and one backward
    (csrc/dpc_depth.hip); outputs of the staged fallback get the same numbers from outputs["proj_depth"] with torch.
    gt_prepared: depths are what smooth_gt(cfg, depths, size, "depths", ...) returned, [S,H,W,1] -- read as they are, the
    max_dataset_depth remap already done there.  With cfg.pc_gauss_filter_gt and gt_prepared false the call is refused: the
    loss does not smooth, smooth_gt does."""
    if not gt_prepared:
        _refuse_unprepared_gt(cfg, "pc_gauss_filter_gt", "depths", "proj_depth_loss")
    fused = _fused_parts(outputs)
    if gt_prepared:
        _prepared_plane(outputs, depths, 1, "depths")
    S = outputs["proj"].shape[0]
    H, W = outputs["proj"].shape[1], outputs["proj"].shape[2]
    plane = _ops_plane(tuple(depths.shape))
    if plane is None:
        raise ValueError("depths must be [S,Hd,Wd,1], [S,1,Hd,Wd] or [S,Hd,Wd], got %s" % (tuple(depths.shape),))
    if depths.shape[0] != S:
        raise NotImplementedError("pose_predict_num_candidates: %d projections for %d depth maps -- the depth loss needs one "
                                  "cloud per sample (with K candidates the reference's shapes do not broadcast)"
                                  % (S, depths.shape[0]))
    Hd, Wd = plane
    if Hd < H or Wd < W or Hd % H or Wd % W or Hd // H != Wd // W:
        raise ValueError("depths %dx%d are not an integer multiple of the %dx%d projections" % (Hd, Wd, H, W))
    f = Hd // H
    max_depth = float(_get(cfg, "max_depth", 10.0))
    mdd = max_depth if gt_prepared else float(_get(cfg, "max_dataset_depth", max_depth))   # equal: no remap
    if fused is not None:
        geom, grid_wh, s = fused
        loss, depth = DepthLoss.apply(grid_wh, s, depths, f, mdd, valid_samples, geom, bool(return_depth))
        return (loss, depth) if return_depth else loss
    pred = outputs["proj_depth"].reshape(S, H, W)
    g = depths.reshape(S, Hd, Wd)[:, ::f, ::f].to(pred.dtype)
    if mdd != max_depth:
        g = torch.where(g == mdd, torch.full_like(g, max_depth), g)
    sq = ((g - pred) ** 2).sum((1, 2))
    if valid_samples is not None:
        sq = sq * valid_samples.to(sq.dtype) ** 2
    loss = 0.5 * sq.sum() / S
    return (loss, outputs["proj_depth"].detach()) if return_depth else loss


# ------------------------------------------------------------------------------------------------------
# Colour supervision          reference (TF-1 originals): dpc/util/point_cloud.py:98-134, 244-262, 275-277;
#                             dpc/util/drc.py:132-142; dpc/util/losses.py:69-90
# ------------------------------------------------------------------------------------------------------
def replicate_rgb(rgb, num_clouds, point_index=None):
    """Per-point colours [B/R,N,3] of shared point sets -> one row per cloud [B,n,3]: tf_repeat_0 over views and pose
    candidates, then the rgb half of pc_point_dropout -- cloud b keeps rgb[b // R][point_index[b]]
    (dpc/models/model_pc_to.py:254-258, 323-329).  Plain torch, differentiable; the renderer reads shared point sets in
    place, and so does the colour node under cfg.pc_rgb_deterministic (rgb_grids with point_index=); without the key it
    wants the replicated tensor."""
    S = rgb.shape[0]
    if S == 0 or num_clouds % S:
        raise ValueError("%d clouds cannot share %d colour sets: the number of clouds must be a multiple" % (num_clouds, S))
    if num_clouds != S:
        rgb = rgb.repeat_interleave(num_clouds // S, dim=0)
    if point_index is not None:
        if point_index.dim() != 2 or point_index.shape[0] != num_clouds:
            raise ValueError("point_index must be [%d, n], got %s" % (num_clouds, tuple(point_index.shape)))
        rgb = rgb.gather(1, point_index.long().unsqueeze(-1).expand(-1, -1, 3))
    return rgb


def _rgb_options(cfg):
    return (bool(_get(cfg, "pc_rgb_stop_points_gradient", False)), bool(_get(cfg, "pc_rgb_clip_after_conv", False)),
            bool(_get(cfg, "pc_rgb_divide_by_occupancies", False)), float(_get(cfg, "pc_rgb_divide_by_occupancies_epsilon", 0.01)))


def _rgb_grids(cfg, outputs, all_rgb, kernel, point_index=None):
    """(geom, voxels [B,D,H,W], smoothed colour grid [B,3,D,H,W], occupancies to divide by | None) of a projection."""
    stop, clip_after, divide, _ = _rgb_options(cfg)
    deterministic = bool(_get(cfg, "pc_rgb_deterministic", False))
    tr, vox = outputs["tr_pc"], outputs["voxels"]
    if deterministic:
        _ops_colour_sets(tr.shape, all_rgb.shape, point_index)   # per cloud, or colour sets read in place
    elif point_index is not None or tuple(all_rgb.shape) != tuple(tr.shape):
        raise ValueError("all_rgb must hold one colour per projected point, %s (replicate_rgb makes it from the decoder's "
                         "colours; colour sets and a point_index are read in place under pc_rgb_deterministic: true only), "
                         "got %s%s" % (tuple(tr.shape), tuple(all_rgb.shape), "" if point_index is None else " and a point_index"))
    B = tr.shape[0]
    geom = _geometry(cfg, kernel)
    if deterministic:                                                # point_cloud.py:98-134
        C = RgbSplatFixed.apply(tr, all_rgb, geom, stop, point_index)
    else:
        C = RgbSplat.apply(tr, all_rgb, geom, stop)
    if not clip_after:
        C = torch.clamp(C, 0.0, 1.0)                                 # :245-246
    if kernel is not None:
        C = Smooth.apply(C.reshape(B * 3, geom.D, geom.H, geom.W), geom).reshape(C.shape)   # convolve_rgb, :148-154
    div = None
    if divide:                                                       # :255-259: the RAW occupancies, gradient stopped
        with torch.no_grad():
            div = Splat.apply(tr.detach(), geom)
            if kernel is not None:
                div = Smooth.apply(div, geom)
    return geom, vox.reshape(B, geom.D, geom.H, geom.W), C, div


def _rgb_outputs(outputs):
    if not isinstance(outputs, ProjectionOutputs):
        raise TypeError("outputs must be what pointcloud_project_fast returned, got %s" % type(outputs).__name__)


def rgb_grids(cfg, outputs, all_rgb, kernel=None, point_index=None):
    """The grids every colour function starts from, made once: (geom, voxels [B,D,H,W], smoothed colour grid [B,3,D,H,W],
    occupancies to divide by | None) of the projection `outputs` and the colours all_rgb, as project_rgb describes them
    (splat, pre-clip, per-channel smoothing; the smoothed raw occupancies under pc_rgb_divide_by_occupancies).  Hand the
    result to project_rgb, proj_rgb_loss and drc_rgb_loss through `grids=`: they then share one colour splat and one set of
    smoothing passes (most of a colour node's time) and their gradients add up at the grids.
    point_index and the forms all_rgb may take: as in project_rgb."""
    _rgb_outputs(outputs)
    return _rgb_grids(cfg, outputs, all_rgb, kernel, point_index)


def project_rgb(cfg, outputs, all_rgb, kernel=None, grids=None, point_index=None):
    """The colour entries of the reference's output dict for the projection `outputs` (what pointcloud_project_fast
    returned, called with all_rgb=None): {"proj_rgb": [B,H,W,3], "voxels_rgb": [B,D,H,W,3]}.

    all_rgb [B,N,3]: one colour per projected point (rows like outputs["tr_pc"]; replicate_rgb).  The colours are splatted
    with the points' trilinear weights into the cells of the occupancy splat (dpc/util/point_cloud.py:98-134; no gradient
    from the weights to the points under pc_rgb_stop_points_gradient), clipped to [0,1] unless pc_rgb_clip_after_conv
    (:245-246), smoothed per channel with `kernel` (convolve_rgb, :148-154; None: no smoothing), divided by the smoothed raw
    occupancies + pc_rgb_divide_by_occupancies_epsilon under pc_rgb_divide_by_occupancies (:255-259), clipped under
    pc_rgb_clip_after_conv (:261-262), flipped along the image rows (:276) and integrated along every ray with the
    ray-termination probabilities of outputs["voxels"] over a white background (project_volume_rgb_integral,
    dpc/util/drc.py:132-142).  `kernel` must be the one the projection was made with.  Differentiable to all_rgb, to the
    points, pose, translation and focal length through outputs["tr_pc"], and to everything behind outputs["voxels"].
    By default the colour splat adds with fp32 atomics: results may differ in the last bits from run to run.

    cfg.pc_rgb_deterministic: true takes the bit-reproducible splat instead (64-bit fixed-point sums, RgbSplatFixed): the
    colour grid and everything computed from it are the same bits on every run and for every order of the points.  all_rgb
    may then also be the decoder's colour sets [B/R,N,3], read in place: cloud b takes rgb[b // R][point_index[b]] with
    point_index [B,n] (the dropout rows handed to the projection), or rgb[b // R] when N == n and there is no index -- what
    replicate_rgb would build, without building it; the gradient comes back in the sets' layout.  On this route colours must
    satisfy |c| <= 8: a larger, NaN or infinite colour turns every voxel of its cloud's colour grid into NaN (the other
    clouds are untouched).  Without the key, colour sets or a point_index raise ValueError.
    grids: what rgb_grids(cfg, outputs, all_rgb, kernel) returned, to share it with other colour functions (None: made here)."""
    _rgb_outputs(outputs)
    _, clip_after, _, div_eps = _rgb_options(cfg)
    geom, vox, C, div = _rgb_grids(cfg, outputs, all_rgb, kernel, point_index) if grids is None else grids
    proj_rgb = RgbMap.apply(vox, C, div, geom, div_eps, clip_after)
    Cf = C if div is None else C / (div.unsqueeze(1) + div_eps)
    if clip_after:
        Cf = torch.clamp(Cf, 0.0, 1.0)
    return {"proj_rgb": proj_rgb, "voxels_rgb": torch.flip(Cf.permute(0, 2, 3, 4, 1), [2])}


def _image_factor(outputs, images, what):
    """(planar, f) of images [S,Hi,Wi,3] or [S,3,Hi,Wi] against the projection's [S,H,W]: Hi = f*H, Wi = f*W, integer f >= 1."""
    S, H, W = outputs["proj"].shape[0], outputs["proj"].shape[1], outputs["proj"].shape[2]
    shape = tuple(images.shape)
    if len(shape) != 4 or (shape[3] != 3 and shape[1] != 3):
        raise ValueError("images must be [S,Hi,Wi,3] or [S,3,Hi,Wi], got %s" % (shape,))
    planar = shape[3] != 3
    Hi, Wi = (shape[2], shape[3]) if planar else (shape[1], shape[2])
    if shape[0] != S:
        raise NotImplementedError("pose_predict_num_candidates: %d projections for %d images -- the %s needs one "
                                  "cloud per sample (colour for K pose candidates is not implemented)" % (S, shape[0], what))
    if Hi < H or Wi < W or Hi % H or Wi % W or Hi // H != Wi // W:
        raise ValueError("images %dx%d are not an integer multiple of the %dx%d projections" % (Hi, Wi, H, W))
    f = Hi // H
    if f * H > 1024 or f * W > 1024:
        raise ValueError("images %dx%d: sides above 1024 are not supported" % (Hi, Wi))
    return planar, f


def proj_rgb_loss(cfg, outputs, all_rgb, images, kernel=None, valid_samples=None, return_rgb=False, grids=None,
                  point_index=None, gt_prepared=False):
    """add_proj_rgb_loss (dpc/util/losses.py:69-90) without its weight: (1/2) sum_s w_s^2 sum_{pix,c} (g - proj_rgb)^2 / S on
    the colour projection of project_rgb.  return_rgb: (loss, proj_rgb [S,H,W,3] detached) -- the image the loss was
    formed from, written by the same launch.

    outputs: what pointcloud_project_fast returned for S clouds (one per sample; fused or staged, both provide tr_pc and
    voxels); all_rgb [S,N,3]; images: inputs["images"], [S,Hi,Wi,3] or [S,3,Hi,Wi] with Hi = f*H, Wi = f*W for an integer
    f >= 1 -- g[s,y,x,c] = images[s,f*y,f*x,c]: the reference's tf.image.resize_images (bilinear, TF-1, no align_corners)
    maps output pixel y to source coordinate y * Hi / H = f*y, an integer, so it samples exactly there and this is the
    reference's value.  valid_samples [S] | None: per-sample weights w, squared like proj_depth_loss's (None, the reference:
    all ones).  The caller multiplies by cfg.proj_rgb_weight.  Splat and smoothing as in project_rgb; integral, squared
    error and their backward are one column kernel each way (csrc/dpc_rgb.hip).  grids, point_index and
    cfg.pc_rgb_deterministic (colour sets [S/R,N,3] read in place, |c| <= 8, a bit-reproducible loss): as in project_rgb.
    gt_prepared: images are what smooth_gt(cfg, images, size, "images", ...) returned, [S,H,W,3] -- read as they are.  With
    cfg.pc_gauss_filter_gt_rgb and gt_prepared false the call is refused: the loss does not smooth, smooth_gt does."""
    if not gt_prepared:
        _refuse_unprepared_gt(cfg, "pc_gauss_filter_gt_rgb", "images", "proj_rgb_loss")
    _rgb_outputs(outputs)
    if gt_prepared:
        _prepared_plane(outputs, images, 3, "images")
    planar, f = _image_factor(outputs, images, "colour loss")
    _, clip_after, _, div_eps = _rgb_options(cfg)
    geom, vox, C, div = _rgb_grids(cfg, outputs, all_rgb, kernel, point_index) if grids is None else grids
    loss, proj_rgb = RgbLoss.apply(vox, C, div, images, f, planar, valid_samples, geom, div_eps, clip_after)
    return (loss, proj_rgb) if return_rgb else loss


# ------------------------------------------------------------------------------------------------------
# Ray-consistency (DRC) losses         reference (TF-1 originals): dpc/util/losses.py:23-66, 93-110
# ------------------------------------------------------------------------------------------------------
def _check_drc_grid(cfg):
    vz = int(_get(cfg, "vox_size_z", -1))
    if vz != -1 and vz != int(cfg.vox_size):
        raise NotImplementedError("vox_size_z: %d with vox_size %d -- the reference's ray potentials tile the ground truth "
                                  "cfg.vox_size times along the ray and do not broadcast against %d probabilities "
                                  "(dpc/util/losses.py:25, 35)" % (vz, int(cfg.vox_size), vz + 1))


def drc_loss(cfg, outputs, masks, valid_samples=None, gt_prepared=False):
    """add_drc_loss (dpc/util/losses.py:23-29, 49-66) without its weight: sum_s w_s^2 sum_rays ((1 - g) sum_{k<D} p_k + g p_D) / S,
    the ray-consistency cost of the masks under the ray-termination probabilities p of outputs["drc_probs"] -- a ray that
    ends in a voxel pays 1 - g, one that escapes pays g.  No 1/2 and no square.

    outputs: what pointcloud_project_fast returned for S clouds (one per sample); masks [S,1,Hm,Wm], [S,Hm,Wm,1] or [S,Hm,Wm]
    with Hm = f*H, Wm = f*W for an integer f >= 1 -- g[s,y,x] = masks[s,f*y,f*x], where the reference's
    tf.image.resize_images (bilinear, TF-1, no align_corners) samples for an integer factor (proj_rgb_loss explains).
    The reference's caller hands over the masks add_proj_loss pooled (model_pc_to.py:354-366, 396-397): pool them first for
    its numbers (f = 1).  valid_samples [S] | None: per-sample weights w, squared like the other losses'.  The caller
    multiplies by cfg.drc_weight.  On the fused path the loss is two launches forward and one backward on the fused node's
    grid (csrc/dpc_drc_loss.hip), a node on (grid_wh, scaling_factor); outputs of the staged fallback get the same numbers
    from outputs["drc_probs"] with torch.
    gt_prepared: masks are what smooth_gt(cfg, masks, size, "masks", ...) returned, [S,H,W,1] -- the tensor add_proj_loss
    stored back into inputs['masks'] -- read as they are.  With cfg.pc_gauss_filter_gt and gt_prepared false the call is
    refused: the loss does not smooth, smooth_gt does."""
    if not gt_prepared:
        _refuse_unprepared_gt(cfg, "pc_gauss_filter_gt", "masks", "drc_loss")
    _check_drc_grid(cfg)
    fused = _fused_parts(outputs)
    if gt_prepared:
        _prepared_plane(outputs, masks, 1, "masks")
    S, H, W = outputs["proj"].shape[0], outputs["proj"].shape[1], outputs["proj"].shape[2]
    plane = _ops_plane(tuple(masks.shape))
    if plane is None:
        raise ValueError("masks must be [S,1,Hm,Wm], [S,Hm,Wm,1] or [S,Hm,Wm], got %s" % (tuple(masks.shape),))
    if masks.shape[0] != S:
        raise NotImplementedError("pose_predict_num_candidates: %d projections for %d masks -- the drc loss needs one cloud "
                                  "per sample (with K candidates the reference's shapes do not broadcast)" % (S, masks.shape[0]))
    Hm, Wm = plane
    if Hm < H or Wm < W or Hm % H or Wm % W or Hm // H != Wm // W:
        raise ValueError("masks %dx%d are not an integer multiple of the %dx%d projections" % (Hm, Wm, H, W))
    f = Hm // H
    if f * H > 1024 or f * W > 1024:
        raise ValueError("masks %dx%d: sides above 1024 are not supported" % (Hm, Wm))
    if fused is not None:
        geom, grid_wh, s = fused
        return DrcLoss.apply(grid_wh, s, masks, f, valid_samples, geom)
    p = outputs["drc_probs"][..., 0]                                   # [D+1,S,H,W], rows in image order
    g = masks.reshape(S, Hm, Wm)[:, ::f, ::f].to(p.dtype)
    cost = ((1.0 - g) * p[:-1].sum(0) + g * p[-1]).sum((1, 2))
    if valid_samples is not None:
        cost = cost * valid_samples.to(cost.dtype) ** 2
    return cost.sum() / S


def drc_rgb_loss(cfg, outputs, all_rgb, images, kernel=None, valid_samples=None, grids=None, point_index=None):
    """add_drc_rgb_loss (dpc/util/losses.py:32-46, 93-110) without its weight: sum_s w_s^2 sum_rays sum_k p_k psi_k / S with
    psi_k = sum_c (g_c - voxels_rgb_{k,c})^2 the squared distance of the colour of voxel k on the ray from the image's pixel,
    psi_D = sum_c (g_c - 1)^2 for the white background, and p the ray-termination probabilities of outputs["voxels"].

    outputs, all_rgb, images, kernel, valid_samples and the options read from cfg are proj_rgb_loss's (voxels_rgb is
    project_rgb's: division by the occupancies, clip after the convolution); images are read at (f*y, f*x).  The reference
    defines this loss and its weight key (drc_rgb_weight) but never calls it from get_loss; the caller multiplies by the
    weight.  A node on (voxels, colour grid): one column kernel each way (csrc/dpc_drc_loss.hip), nothing of the size of
    [D+1,B,H,W] or [B,D,H,W,3] is built.  grids: as in project_rgb -- shared with proj_rgb_loss, the two losses cost one
    splat and one set of smoothing passes.  point_index and cfg.pc_rgb_deterministic: as in project_rgb."""
    if _get(cfg, "pc_gauss_filter_gt_rgb", False):
        raise NotImplementedError("pc_gauss_filter_gt_rgb: true -- smoothing of the ground-truth images is not implemented "
                                  "(gauss_smoothen_image, dpc/util/losses.py:78-83)")
    _check_drc_grid(cfg)
    _rgb_outputs(outputs)
    planar, f = _image_factor(outputs, images, "drc colour loss")
    _, clip_after, _, div_eps = _rgb_options(cfg)
    geom, vox, C, div = _rgb_grids(cfg, outputs, all_rgb, kernel, point_index) if grids is None else grids
    return DrcRgbLoss.apply(vox, C, div, images, f, planar, valid_samples, geom, div_eps, clip_after)


# ------------------------------------------------------------------------------------------------------
# Smoothed ground truth (pc_gauss_filter_gt, pc_gauss_filter_gt_rgb, pc_gauss_filter_gt_switch_off)
# reference (TF-1 originals): dpc/util/gauss_kernel.py:14-24; dpc/models/model_pc.py:398-404; dpc/util/losses.py:78-83, 128-129
# ------------------------------------------------------------------------------------------------------
_GT_KINDS = {"masks": (_native.DPC_GT_RESIZE_MEAN, "pc_gauss_filter_gt"), "images": (_native.DPC_GT_RESIZE_SAMPLE, "pc_gauss_filter_gt_rgb"),
             "depths": (_native.DPC_GT_RESIZE_SAMPLE, "pc_gauss_filter_gt")}


def _smooth_gt_planes(gt, channels, planar, source, size, mode, taps=None, dev_taps=None, ntaps=None, remap=None):
    """[S,H,W,C] fp32 from ground truth in either layout: the device node, or on CPU tensors the same rule with torch ops."""
    if gt.is_cuda:
        return _ops_gt_smooth(gt, channels, planar, source, size, mode, taps, dev_taps, ntaps, remap)
    if dev_taps is not None:
        raise RuntimeError("dpc.render.smooth_gt: device taps with ground truth on %s" % gt.device)
    (Hs, Ws), (H, W), C = source, size, channels
    S = gt.shape[0]
    g = gt.detach().to(torch.float32)
    g = g.reshape(S, C, Hs, Ws) if planar else g.reshape(S, Hs, Ws, C).permute(0, 3, 1, 2)
    if remap is not None and remap[0] != remap[1]:
        g = torch.where(g == remap[0], torch.full_like(g, remap[1]), g)
    f = Hs // H
    if f > 1:
        g = torch.nn.functional.avg_pool2d(g, f) if mode == _native.DPC_GT_RESIZE_MEAN else g[:, :, ::f, ::f]
    w = torch.as_tensor(np.ascontiguousarray(taps, dtype=np.float32).reshape(-1))
    n = w.numel()
    if n != 1 or float(w[0]) != 1.0:   # one tap of 1.0: the resized bits as they are
        g = torch.nn.functional.conv2d(g.contiguous(), w.reshape(1, 1, 1, n).repeat(C, 1, 1, 1), padding=(0, n // 2), groups=C)
        g = torch.nn.functional.conv2d(g, w.reshape(1, 1, n, 1).repeat(C, 1, 1, 1), padding=(n // 2, 0), groups=C)
    return g.permute(0, 2, 3, 1).contiguous()


def gauss_smoothen_image(cfg, img, sigma_rel):
    """gauss_smoothen_image of the TF-1 original (dpc/util/gauss_kernel.py:14-24): img [S,H,W,C] (C = 1 or 3) -> [S,H,W,C],
    every channel convolved with gauss_kernel_1d(cfg.pc_gauss_kernel_size, sigma_rel) along the rows and then along the
    columns, zero padding ("SAME").  One launch (csrc/dpc_gt_smooth.hip); fp32; no gradient."""
    shape = tuple(img.shape)
    if len(shape) != 4 or shape[3] not in (1, 3):
        raise ValueError("img must be [S,H,W,1] or [S,H,W,3], got %s" % (shape,))
    taps = gauss_kernel_1d(int(cfg.pc_gauss_kernel_size), sigma_rel).numpy()
    return _smooth_gt_planes(img, shape[3], False, shape[1:3], shape[1:3], _native.DPC_GT_RESIZE_SAMPLE, taps)


def smooth_gt(cfg, gt, size, kind, sigma_rel=None, kernel=None, schedule=None):
    """The ground truth of one loss, resized to the projection's size and smoothed with the voxels' Gaussian, as ONE node:
    what cfg.pc_gauss_filter_gt (masks, depths) and cfg.pc_gauss_filter_gt_rgb (images) ask for in the TF-1 original
    (dpc/models/model_pc.py:398-404; dpc/util/losses.py:78-83, 128-129).  Returns [S,H,W,C] fp32, the layout the reference has
    after its permute: hand it to silhouette_loss / pointcloud_project_loss as already pooled masks, to proj_depth_loss,
    proj_rgb_loss and drc_loss with gt_prepared=True.

    size: the projection's (H, W), or an int.  kind and the layouts it takes (those of the loss it feeds):
      "masks"   [S,1,Hm,Wm], [S,Hm,Wm,1] or [S,Hm,Wm]; resized by the f x f mean of nn.AvgPool2d(f) (silhouette_loss)
      "images"  [S,Hi,Wi,3] or [S,3,Hi,Wi]; g[y,x] = images[f*y, f*x] (proj_rgb_loss)
      "depths"  [S,Hd,Wd,1], [S,1,Hd,Wd] or [S,Hd,Wd]; cfg.max_dataset_depth -> cfg.max_depth first where they differ, then
                g[y,x] = depths[f*y, f*x] (proj_depth_loss)
    with f = Hm / H = Wm / W an integer >= 1 and source sides <= 1024.  The blur is gauss_smoothen_image's: rows, then
    columns, zeros outside the plane -- so depth maps darken at the border, as in the reference.
    The taps come from exactly one of: sigma_rel (gauss_kernel_1d(cfg.pc_gauss_kernel_size, sigma_rel), on the host); kernel
    (the x/y taps of a smoothing_kernel(...) list); schedule (a DeviceSchedule or DeviceTaps: its taps_xy are read from device
    memory when the node runs, so a captured graph follows sigma).
    cfg.pc_gauss_filter_gt_switch_off with sigma_rel < 1.0: the resized ground truth unchanged, for masks and images (depth has
    no switch-off in the reference).  The switch needs sigma_rel: with kernel= or schedule= the taps are applied as they are,
    and a caller that honours the switch puts the identity kernel there (DeviceTaps; multiplying finite values by exactly 1
    and 0 reproduces the resized bits).  No gradient: ground truth needs none.  CPU tensors: the same rule with torch ops."""
    if kind not in _GT_KINDS:
        raise ValueError("kind must be 'masks', 'images' or 'depths', got %r" % (kind,))
    if sum(v is not None for v in (sigma_rel, kernel, schedule)) != 1:
        raise ValueError("smooth_gt takes its taps from exactly one of sigma_rel, kernel and schedule")
    mode, _ = _GT_KINDS[kind]
    H, W = (int(size), int(size)) if isinstance(size, (int, np.integer)) else (int(size[0]), int(size[1]))
    shape = tuple(gt.shape)
    if kind == "images":
        if len(shape) != 4 or (shape[3] != 3 and shape[1] != 3):
            raise ValueError("images must be [S,Hi,Wi,3] or [S,3,Hi,Wi], got %s" % (shape,))
        planar, C = shape[3] != 3, 3
        Hs, Ws = (shape[2], shape[3]) if planar else (shape[1], shape[2])
    else:
        plane = _ops_plane(shape)
        if plane is None:
            raise ValueError("%s must be [S,1,Hm,Wm], [S,Hm,Wm,1] or [S,Hm,Wm], got %s" % (kind, shape))
        (Hs, Ws), planar, C = plane, True, 1
    if H < 1 or W < 1 or Hs < H or Ws < W or Hs % H or Ws % W or Hs // H != Ws // W:
        raise ValueError("%s %dx%d are not an integer multiple of the %dx%d projections" % (kind, Hs, Ws, H, W))
    if Hs > 1024 or Ws > 1024:
        raise ValueError("%s %dx%d: sides above 1024 are not supported" % (kind, Hs, Ws))
    if shape[0] == 0:
        return torch.zeros((0, H, W, C), dtype=torch.float32, device=gt.device)
    remap = None
    if kind == "depths":
        max_depth = float(_get(cfg, "max_depth", 10.0))
        remap = (float(_get(cfg, "max_dataset_depth", max_depth)), max_depth)
    taps = dev_taps = ntaps = None
    if schedule is not None:
        dev_taps, ntaps = schedule.taps_xy, int(schedule.sizes[0])
    elif kernel is not None:
        taps = _kernel_taps(cfg, kernel)[0]
    else:
        taps = gauss_kernel_1d(int(cfg.pc_gauss_kernel_size), sigma_rel).numpy()
        if kind != "depths" and _get(cfg, "pc_gauss_filter_gt_switch_off", False) and sigma_rel < 1.0:
            taps = np.ones(1, dtype=np.float32)   # tf.where(tf.less(sigma_rel, 1.0), gt, smoothed)
    return _smooth_gt_planes(gt, C, planar, (Hs, Ws), (H, W), mode, taps, dev_taps, ntaps, remap)


def _refuse_unprepared_gt(cfg, key, what, where):
    if _get(cfg, key, False):
        raise NotImplementedError("%s: true -- %s takes the smoothed ground truth %s from dpc.render.smooth_gt, with "
                                  "gt_prepared=True; it does not smooth inside the loss (gauss_smoothen_image, %s)"
                                  % (key, where, what, "dpc/util/losses.py:78-83, 128-129; dpc/models/model_pc.py:398-404"))


def _prepared_plane(outputs, gt, channels, what):
    """Ground truth from smooth_gt against the projection: [S,H,W,C] exactly."""
    S, H, W = outputs["proj"].shape[0], outputs["proj"].shape[1], outputs["proj"].shape[2]
    if tuple(gt.shape) != (S, H, W, channels):
        raise ValueError("gt_prepared: %s must be what smooth_gt returned for this projection, [%d,%d,%d,%d], got %s"
                         % (what, S, H, W, channels, tuple(gt.shape)))


# ------------------------------------------------------------------------------------------------------
# Schedules read by the caller                       reference: dpc/models/model_pc_to.py:59-87
# ------------------------------------------------------------------------------------------------------
def get_smooth_sigma(cfg, global_step):
    """sigma_rel(step), linear from pc_relative_sigma to pc_relative_sigma_end (model_pc_to.py:59-63)."""
    return cfg.pc_relative_sigma + global_step / cfg.max_number_of_steps * (cfg.pc_relative_sigma_end - cfg.pc_relative_sigma)


def get_dropout_prob(cfg, global_step):
    """Point keep-probability schedule (model_pc_to.py:68-87)."""
    if not cfg.pc_point_dropout_scheduled:
        return cfg.pc_point_dropout
    if cfg.pc_point_dropout_exponential_schedule:
        raise NotImplementedError("pc_point_dropout_exponential_schedule: true calls torch.log on floats in the reference")
    k0 = cfg.pc_point_dropout
    slope = (1.0 - k0) / (cfg.pc_point_dropout_end_step - cfg.pc_point_dropout_start_step)
    keep = slope * (global_step / cfg.max_number_of_steps) + (k0 - slope * cfg.pc_point_dropout_start_step)
    return max(min(keep, 1.0), k0)


# ------------------------------------------------------------------------------------------------------
# Evaluation side: nearest target point / Chamfer      reference: dpc/util/point_cloud_distance.py:25-40,
#                                           dpc/run/eval_chamfer_to.py:24-44, 119-123
# ------------------------------------------------------------------------------------------------------
def point_cloud_distance(Vs, Vt):
    """For each point of Vs [Ns,3] the closest point of Vt [Nt,3] (point_cloud_distance.py:25-40).

    Returns (proj [Ns,3] = Vt[idx], minDist [Ns], idx [Ns] int64) like the reference; fp32 or fp64 after the inputs.
    Nothing of size Ns x Nt is materialised.  When Vs or Vt requires grad, minDist and proj carry gradient as the
    reference's do under autograd (minDist through dpc_nearest_batched_bwd as a one-pair call, proj through torch's
    indexing), with the same values as without; where a source point coincides with its nearest target the reference's
    gradient is NaN and this one is exactly zero (include/dpc_render.h)."""
    dev = _native.require_device(Vs, Vt)
    if Vs.dim() != 2 or Vt.dim() != 2 or Vs.shape[1] != 3 or Vt.shape[1] != 3:
        raise ValueError("point_cloud_distance expects [Ns,3] and [Nt,3], got %s and %s" % (tuple(Vs.shape), tuple(Vt.shape)))
    dtype = torch.float64 if torch.float64 in (Vs.dtype, Vt.dtype) else torch.float32
    vs, vt = Vs.detach().to(dtype).contiguous(), Vt.detach().to(dtype).contiguous()
    ns, nt = vs.shape[0], vt.shape[0]
    if nt == 0 and ns > 0:
        raise IndexError("point_cloud_distance: empty target cloud (argmin of an empty sequence)")
    if torch.is_grad_enabled() and (Vs.requires_grad or Vt.requires_grad):
        vt = Vt.to(dtype)
        _, dist, idx = nearest_batched(torch.cat([vt, Vs.to(dtype)]), [[nt, ns, 0, nt]], return_distances=True)
        return vt[idx], dist, idx
    is64 = int(dtype == torch.float64)
    proj = torch.empty((ns, 3), dtype=dtype, device=dev)
    dist = torch.empty((ns,), dtype=dtype, device=dev)
    idx = torch.empty((ns,), dtype=torch.int64, device=dev)
    ws = torch.empty((max(_native.lib().dpc_nearest_workspace_bytes(ns, nt, is64), 16),), dtype=torch.uint8, device=dev)
    _native.call(dev, "dpc_point_cloud_distance", _native.ptr(vs), _native.ptr(vt), ns, nt, is64, _native.ptr(proj),
                 _native.ptr(dist), _native.ptr(idx), _native.ptr(ws))
    return proj, dist, idx


def compute_distance(cfg, source_np, target_np, device=None):
    """eval_chamfer_to.py:24-44: numpy in, (min_dist, idx) numpy out (both float64 arrays, like the reference's
    np.concatenate onto float64 zeros).  The reference walks the source in cfg.pc_eval_chamfer_num_parts pieces to
    bound its [Ns,Nt,3] temporary; nothing of that size exists here, so the cloud goes through in one call."""
    device = torch.device("cuda") if device is None else device
    src = torch.from_numpy(np.ascontiguousarray(source_np)).to(device)
    tgt = torch.from_numpy(np.ascontiguousarray(target_np)).to(device)
    _, dist, idx = point_cloud_distance(src, tgt)
    return dist.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.float64)


def chamfer_distances(pred, gt):
    """The two directed means the evaluation reports per view (eval_chamfer_to.py:119-123):
    (mean_i min_j |pred_i - gt_j|, mean_j min_i |gt_j - pred_i|) as a float64 tensor [2] on the inputs' device."""
    p2g = point_cloud_distance(pred, gt)[1]
    g2p = point_cloud_distance(gt, pred)[1]
    return torch.stack([p2g.double().mean(), g2p.double().mean()])
