"""ctypes binding of libdpc_render.so (C ABI declared in include/dpc_render.h).

There is no CPU fallback: if the library is missing, or a tensor does not live on a HIP device, the
call raises.  The library is built in-tree by `make -C pytorch-unsup-pc_amd/csrc` (or
`python __graft_entry__.py`).
"""
import ctypes
import os

import torch

_CSRC = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "csrc"))
# DPC_RENDER_LIB points timing experiments at a variant build of the same library (tools/build_variant.sh); there is no
# other implementation to fall back to either way
LIB_PATH = os.environ.get("DPC_RENDER_LIB") or os.path.join(_CSRC, "libdpc_render.so")

ABI_VERSION = 15
DPC_MAX_TAPS = 63
DPC_MAX_POINTS = (1 << 20) - 1
DPC_SMALL_COLS = 12
COL_DQ, COL_DS, COL_DT, COL_DF = 0, 4, 5, 8
DPC_ERR_NULL = -1
DPC_ERR_SHAPE = -2
DPC_ERR_TAPS = -3
DPC_ERR_LDS = -4
DPC_STATUS_BAD_INDEX = 1
DPC_STATUS_VOXEL_TOO_SMALL = 2
DPC_STATUS_KEY_OVERFLOW = 4
DPC_STATUS_NONFINITE = 8
DPC_STATUS_DENSIFY_ORDER = 16
DPC_STATUS_NEAR = 32
DPC_STATUS_EMD_NOT_CONVERGED = 64
DPC_EMD_MAX_POINTS = 2048
DPC_FPS_MAX_POINTS = 16384
DPC_VOXEL_MAX_SIDE = 128
DPC_VOXEL_EDT_NONE = 2 ** 31 - 1
DPC_VOXEL_EDT_MAX_THRESHOLDS = 8
DPC_MESH_FILL_NONE, DPC_MESH_FILL_CARVE, DPC_MESH_FILL_PARITY = 0, 1, 2
DPC_PM_BLOCK, DPC_PM_FACE_TILE, DPC_PM_CHUNK_TILES = 256, 128, 8
DPC_WINDING_FRAC_BITS = 40
DPC_RAY_LDS_BYTES = 10240
DPC_KNN_MAX_K, DPC_KNN_TILE = 64, 512
DPC_GAUSS_NORM_NONE, DPC_GAUSS_NORM_ANALYTICAL, DPC_GAUSS_NORM_PER_POINT = 0, 1, 2
DPC_GAUSS_MAX_SIDE = 64
DPC_GT_RESIZE_MEAN, DPC_GT_RESIZE_SAMPLE = 0, 1
DPC_MESH_NEAR = 1e-3
DPC_MESH_AMBIENT, DPC_MESH_DIFFUSE = 0.25, 0.75


def knn_block(k):
    """DPC_KNN_BLOCK(k) of the header: the queries a workgroup of dpc_knn_batched holds."""
    return 256 if k <= 16 else 128 if k <= 32 else 64


class DpcParams(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("N", ctypes.c_int32), ("D", ctypes.c_int32), ("H", ctypes.c_int32),
                ("W", ctypes.c_int32), ("taps_xy", ctypes.c_int32), ("taps_z", ctypes.c_int32),
                ("camera_distance", ctypes.c_float), ("focal_length", ctypes.c_float),
                ("clip_val", ctypes.c_float), ("max_depth", ctypes.c_float), ("point_replicas", ctypes.c_int32),
                ("N_src", ctypes.c_int32), ("point_index", ctypes.c_void_p), ("status", ctypes.c_void_p),
                ("n_live", ctypes.c_void_p), ("dev_taps_xy", ctypes.c_void_p), ("dev_taps_z", ctypes.c_void_p)]


# (name, restype, argtypes) of every symbol include/dpc_render.h declares (tests/test_abi_and_host.py checks the header
# against SYMBOLS); argtypes None: the function takes no argument
_i, _i64, _d, _sz = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_size_t
_vp, _pp = ctypes.c_void_p, ctypes.POINTER(DpcParams)
_FUNCTIONS = (
    ("dpc_abi_version", _i, None),
    ("dpc_strerror", ctypes.c_char_p, [_i]),
    ("dpc_mask_words_per_plane", _sz, [_pp]),
    ("dpc_cells_bytes", _sz, [_pp]),
    ("dpc_workspace_bytes", _sz, [_pp]),
    ("dpc_check_grid", _i, [_pp, _i]),
    ("dpc_locate", _i, [_pp] + [_vp] * 7),
    ("dpc_project_fwd", _i, [_pp] + [_vp] * 16),
    ("dpc_project_bwd", _i, [_pp] + [_vp] * 17),
    # ABI 15: (gt, gt_factor, weights) in every fused-loss call
    ("dpc_project_loss_fwd", _i, [_pp] + [_vp] * 8 + [_i, _vp, _i] + [_vp] * 12 + [ctypes.POINTER(_i), _vp]),
    ("dpc_project_loss_bwd", _i, [_pp] + [_vp] * 13 + [_i, _vp, _i] + [_vp] * 2 + [_i] + [_vp] * 4),
    ("dpc_transform_fwd", _i, [_pp] + [_vp] * 6),
    ("dpc_transform_bwd", _i, [_pp] + [_vp] * 8),
    ("dpc_splat_fwd", _i, [_pp, _vp, _i, _vp, _vp, _vp]),
    ("dpc_splat_bwd", _i, [_pp, _vp, _i, _vp, _vp, _vp]),
    ("dpc_smooth", _i, [_pp, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    ("dpc_drc_fwd", _i, [_pp] + [_vp] * 5),
    ("dpc_drc_bwd", _i, [_pp] + [_vp] * 6),
    ("dpc_silhouette_loss", _i, [_vp, _i, _vp, _vp] + [_i] * 4 + [_vp, _vp, _vp, _vp]),
    ("dpc_gauss_voxels_fwd", _i, [_pp, _vp, _d, _i, _vp, _vp, _vp]),
    ("dpc_gauss_voxels_bwd", _i, [_pp, _vp, _d, _i, _vp, _vp, _vp, _vp]),
    ("dpc_gt_smooth", _i, [_vp] + [_i] * 8 + [ctypes.c_float] * 2 + [_vp, _vp, _i, _vp, _vp]),
    ("dpc_depth_workspace_bytes", _sz, [_pp]),
    ("dpc_depth_loss_fwd", _i, [_pp] + [_vp] * 4 + [_i, ctypes.c_float] + [_vp] * 5),
    ("dpc_depth_loss_bwd", _i, [_pp] + [_vp] * 4 + [_i, ctypes.c_float] + [_vp] * 7),
    ("dpc_rgb_splat_fwd", _i, [_pp] + [_vp] * 4),
    ("dpc_rgb_splat_bwd", _i, [_pp] + [_vp] * 6),
    ("dpc_rgb_loss_fwd", _i, [_pp] + [_vp] * 3 + [ctypes.c_float, _i, _vp, _i, _i] + [_vp] * 5),
    ("dpc_rgb_loss_bwd", _i, [_pp] + [_vp] * 3 + [ctypes.c_float, _i, _vp, _i, _i] + [_vp] * 7),
    ("dpc_rgb_splat_fixed_workspace_bytes", _sz, [_pp, _i]),
    ("dpc_rgb_splat_fixed_fwd", _i, [_pp, _vp, _vp, _i, _vp, _vp, _vp]),
    ("dpc_rgb_splat_fixed_bwd", _i, [_pp, _vp, _vp, _i] + [_vp] * 5),
    ("dpc_drc_workspace_bytes", _sz, [_pp]),
    ("dpc_drc_loss_fwd", _i, [_pp] + [_vp] * 4 + [_i] + [_vp] * 4),
    ("dpc_drc_loss_bwd", _i, [_pp] + [_vp] * 4 + [_i] + [_vp] * 6),
    ("dpc_drc_rgb_loss_fwd", _i, [_pp] + [_vp] * 3 + [ctypes.c_float, _i, _vp, _i, _i] + [_vp] * 4),
    ("dpc_drc_rgb_loss_bwd", _i, [_pp] + [_vp] * 3 + [ctypes.c_float, _i, _vp, _i, _i] + [_vp] * 5),
    ("dpc_point_dropout_indices", _i, [_i, _i, _i, _vp, _vp, _vp]),
    ("dpc_point_dropout_indices_live", _i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    ("dpc_schedule_update", _i, [_vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    ("dpc_taps_bucket", _i, [_vp, _i]),
    ("dpc_project_loss_step", _i, [_pp] + [_vp] * 8 + [_i, _vp, _i] + [_vp] * 15),
    ("dpc_nearest_workspace_bytes", _sz, [_i, _i, _i]),
    ("dpc_point_cloud_distance", _i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    ("dpc_icp_workspace_bytes", _sz, [_i, _vp, _vp]),
    ("dpc_icp_point_to_point", _i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _d, _i, _d, _d] + [_vp] * 6),
    ("dpc_chamfer_workspace_bytes", _sz, [_i, _vp, _i]),
    ("dpc_nearest_batched", _i, [_vp, _i, _i, _vp, _vp, _i] + [_vp] * 5),
    ("dpc_chamfer_bwd_workspace_bytes", _sz, [_i, _vp, _i]),
    ("dpc_nearest_batched_bwd", _i, [_vp, _i, _i, _vp, _vp, _i] + [_vp] * 4 + [_i] + [_vp] * 3),
    ("dpc_chamfer_pair_means", _i, [_vp, _i, _vp, _vp, _i] + [_vp] * 3),
    ("dpc_emd_lds_bytes", _sz, [_i]),
    ("dpc_emd_fwd", _i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _i, _d, _i] + [_vp] * 6),
    ("dpc_emd_bwd", _i, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _i] + [_vp] * 7),
    ("dpc_fps", _i, [_vp, _i, _i, _vp, _vp, _i] + [_vp] * 4),
    ("dpc_voxelise", _i, [_vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    ("dpc_voxel_threshold", _i, [_vp, _i, _i, _i, _i, _i, _d, _i, _vp, _vp]),
    ("dpc_voxel_unpack", _i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    ("dpc_voxel_stats", _i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    ("dpc_voxel_count", _i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    ("dpc_voxel2pc", _i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    ("dpc_voxelise_meshes", _i, [_vp, _i, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    ("dpc_voxel_carve", _i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    ("dpc_voxel_edt", _i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    ("dpc_voxel_shell", _i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    ("dpc_voxel_edt_stats", _i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp]),
    ("dpc_surface_workspace_bytes", _sz, [_vp, _i, _i]),
    ("dpc_surface_count", _i, [_vp, _i, _i, _vp, _vp, _i] + [_vp] * 5),
    ("dpc_surface_extract", _i, [_vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i] + [_vp] * 5),
    ("dpc_point_mesh_workspace_bytes", _sz, [_i]),
    ("dpc_point_mesh_distance", _i, [_vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]),
    ("dpc_point_mesh_closest_workspace_bytes", _sz, [_vp, _i]),
    ("dpc_point_mesh_closest", _i, [_vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _i] + [_vp] * 8),
    ("dpc_mesh_winding_workspace_bytes", _sz, [_vp, _i]),
    ("dpc_mesh_winding", _i, [_vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _i] + [_vp] * 5),
    ("dpc_mesh_winding_voxels_workspace_bytes", _sz, [_vp, _i, _i, _i, _i]),
    ("dpc_mesh_winding_voxels", _i, [_vp, _i, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i64] + [_vp] * 4),
    ("dpc_ray_mesh_workspace_bytes", _sz, [_vp, _i]),
    ("dpc_ray_mesh_intersect", _i, [_vp, _vp, _i, _i, _vp, _i, _i, _vp, _i, _vp, _vp, _i, _d, _d, _i] + [_vp] * 8),
    ("dpc_knn_batched", _i, [_vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    ("dpc_pca_normals", _i, [_vp, _i, _i, _vp, _vp, _i, _i] + [_vp] * 6),
    ("dpc_downsample_workspace_bytes", _sz, [_i, _i]),
    ("dpc_voxel_downsample", _i, [_vp, _i, _i, _vp, _vp, _i, _d] + [_vp] * 6),
    ("dpc_densify_workspace_bytes", _sz, [_i, _i64, _i64, _i64, _i]),
    ("dpc_densify", _i, [_vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp] + [_i] * 4 + [_vp] * 5),
    ("dpc_render_points", _i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _d, _d] + [_vp] * 4),
    ("dpc_render_meshes_workspace_bytes", _sz, [_vp, _i, _vp, _i]),
    ("dpc_render_meshes", _i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i] + [_vp] * 6),
    ("dpc_render_meshes_shaded_workspace_bytes", _sz, [_vp, _i, _vp, _i]),
    ("dpc_render_meshes_shaded", _i, [_vp, _i, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _i64, _vp, _vp, _i,
                                      _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i] + [_vp] * 6),
    ("dpc_profile_enable", _i, [_i]),
    ("dpc_profile_disable", _i, None),
    ("dpc_profile_count", _i, None),
    ("dpc_profile_get", _i, [_i, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_float)]),
    ("dpc_profile_get_id", _i, [_i, ctypes.c_char_p, _i]),
    ("dpc_profile_pair_overhead", _i, [_vp, _i, ctypes.POINTER(ctypes.c_float)]),
)
SYMBOLS = tuple(name for name, _, _ in _FUNCTIONS)


class DpcError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        super().__init__("%s failed: %s (code %d)" % (where, strerror(code), code))


_lib = None


def lib():
    """The loaded library; raises (loudly) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "dpc.render: %s is missing -- the HIP extension has not been built. Run `make -C %s` "
                "(needs /opt/rocm/bin/hipcc) or `python -c 'import __graft_entry__ as g; g.build()'`. "
                "There is no CPU fallback." % (LIB_PATH, _CSRC))
        L = ctypes.CDLL(LIB_PATH)
        for name, restype, argtypes in _FUNCTIONS:
            fn = getattr(L, name)
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
        if L.dpc_abi_version() != ABI_VERSION:
            raise RuntimeError("dpc.render: libdpc_render.so ABI %d, expected %d -- rebuild it (make -C %s)"
                               % (L.dpc_abi_version(), ABI_VERSION, _CSRC))
        _lib = L
    return _lib


def strerror(code):
    return lib().dpc_strerror(code).decode()


def check(code, where):
    if code != 0:
        raise DpcError(code, where)


def ptr(t):
    """Address of a tensor as a plain int (None -> NULL): the argtypes of the bindings turn it into a void*."""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream(dev):
    """torch's current HIP stream of `dev` as an address (the raw getter skips building a Stream object per call)."""
    if _raw_stream is not None:
        return _raw_stream(dev.index if dev.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(dev).cuda_stream


def stream_ptr(device):
    """stream() for a device given as a torch.device or a string."""
    return stream(torch.device(device))


class on:
    """`with torch.cuda.device(dev)` only when `dev` is not the current device already (the guard costs ~10 us of host time
    per call; a training process sits on its one device)."""

    __slots__ = ("guard",)

    def __init__(self, dev):
        self.guard = None if (dev.index is None or dev.index == torch.cuda.current_device()) else torch.cuda.device(dev)

    def __enter__(self):
        if self.guard is not None:
            self.guard.__enter__()

    def __exit__(self, *exc):
        if self.guard is not None:
            return self.guard.__exit__(*exc)
        return False


def call(dev, entry, *args):
    """One entry point of the library on `dev` and its current stream (every entry's last argument); raises DpcError on a
    return code.  The only way the package invokes an entry that takes a stream: the work goes to the current stream of
    the tensors' device and no return code is dropped."""
    with on(dev):
        rc = getattr(lib(), entry)(*args, stream(dev))
    if rc != 0:
        raise DpcError(rc, entry)


def require_device(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("dpc.render runs on MI355X only: got a %s tensor; move inputs to a HIP device "
                               "(there is no CPU path in this package)" % t.device)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("dpc.render: tensors on different devices (%s vs %s)" % (dev, t.device))
    return dev


def event_pair_overhead_ms(device, pairs=200):
    """What an empty event pair reads on the current stream (the floor in every profile_kernels figure)."""
    ms = ctypes.c_float()
    torch.cuda.synchronize(device)
    check(lib().dpc_profile_pair_overhead(stream_ptr(device), pairs, ctypes.byref(ms)), "dpc_profile_pair_overhead")
    return ms.value


def profile_kernels(fn, device, capacity=4096):
    """Run fn() with the library's per-kernel event timing on; returns {kernel_name: [ms, ...]}."""
    L = lib()
    check(L.dpc_profile_enable(capacity), "dpc_profile_enable")
    try:
        fn()
        torch.cuda.synchronize(device)
    finally:
        L.dpc_profile_disable()
    out = {}
    name, ms = ctypes.c_char_p(), ctypes.c_float()
    for i in range(L.dpc_profile_count()):
        check(L.dpc_profile_get(i, ctypes.byref(name), ctypes.byref(ms)), "dpc_profile_get")
        out.setdefault(name.value.decode(), []).append(ms.value)
    return out


def launched_instantiations(fn, device, capacity=4096):
    """Run fn() with the launch record on; returns the set of kernel template instantiations it launched, named like the
    demangled device symbols ("k_gather_hw<64, 8, 3>", "k_zcol_fwd_dyn")."""
    L = lib()
    check(L.dpc_profile_enable(capacity), "dpc_profile_enable")
    try:
        fn()
        torch.cuda.synchronize(device)
    finally:
        L.dpc_profile_disable()
    count = L.dpc_profile_count()
    if count >= capacity:
        raise RuntimeError("launched_instantiations: more than %d launches, the record is incomplete" % capacity)
    buf = ctypes.create_string_buffer(128)
    out = set()
    for i in range(count):
        check(L.dpc_profile_get_id(i, buf, len(buf)), "dpc_profile_get_id")
        out.add(buf.value.decode())
    return out
