"""Voxel-grid downsampling of ground-truth clouds on the GPU (densify/downsample_gt.py:47-57, open3d.voxel_down_sample).

The reference reads each dense model, calls open3d's VoxelDownSample and writes the result.  Here a whole group of
models goes into one dpc_voxel_downsample call (csrc/dpc_downsample.hip): the same fp64 keys and the same per-voxel sums
in input order, so every output point equals open3d's bit for bit.  Voxels come out in ascending (kx, ky, kz) order
rather than open3d's hash-map order (include/dpc_render.h states the semantics).

    voxel_down_sample  the thin wrapper over the C ABI: clouds in, [m_i,3] float64 device tensors out
    downsample_split   downsample_gt.py's file loop, batched: names, a loader and an optional writer

Reading and writing .mat files stays with the caller (load_dense, save), as everywhere in this package.
"""
import math
import numbers

import numpy as np
import torch

from . import _batch, _native, _split


def _voxel_size(voxel_size):
    if isinstance(voxel_size, bool) or not isinstance(voxel_size, numbers.Real):
        raise ValueError("voxel_down_sample: voxel_size must be a real number, got %r" % (voxel_size,))
    vs = float(voxel_size)
    if not math.isfinite(vs) or vs <= 0.0:
        raise ValueError("voxel_down_sample: voxel_size must be finite and > 0 (open3d refuses voxel_size <= 0), got %r"
                         % (voxel_size,))
    return vs


def _cloud(x, i):
    return _batch.cloud(x, "voxel_down_sample: cloud %d" % i, cast=None)


def _downsample_packed(clouds, vs):
    """One native call.  Returns (voxels [V,3] float64 on the device, counts [C] int64, offsets [C] int64) with cloud c's
    voxels at rows offsets[c] .. offsets[c] + counts[c]."""
    C = len(clouds)
    counts = np.array([len(c) for c in clouds], dtype=np.int64)
    M = int(counts.sum())
    if M > _batch.INT32_MAX - 1:
        raise ValueError("voxel_down_sample: more than 2^31 - 2 points in one call")
    desc = _batch.table(np.stack([np.cumsum(counts) - counts, counts], axis=1), 2,
                        "voxel_down_sample: more than 2^31 - 2 points in one call")
    L = _native.lib()
    host_desc = desc.ctypes.data
    _batch.dry_run(L.dpc_voxel_downsample(None, M, 0, None, host_desc, C, vs, None, None, None, None, None, None),
                   "voxel_down_sample: refused by dpc_voxel_downsample (voxel_size %r, %d points)" % (vs, M))
    dev = _batch.device("dpc.render voxel downsampling", clouds)
    dtype = _batch.widest(clouds)
    pts, _ = _batch.pack(clouds, dev, dtype)
    out = torch.empty((max(M, 1), 3), dtype=torch.float64, device=dev)
    info = torch.zeros((1 + 2 * C,), dtype=torch.int32, device=dev)  # status, out_count [C], out_offset [C]
    desc_d = _batch.on_device(desc, dev)
    ws = _batch.workspace(L.dpc_downsample_workspace_bytes(C, M), dev)
    _native.call(dev, "dpc_voxel_downsample", _native.ptr(pts), M, int(dtype == torch.float64), _native.ptr(desc_d), host_desc,
                 C, vs, _native.ptr(out), _native.ptr(info[1:1 + C]), _native.ptr(info[1 + C:]), _native.ptr(info[:1]),
                 _native.ptr(ws))
    info = info.cpu().numpy().astype(np.int64)  # the call's one synchronisation
    _batch.raise_status(int(info[0]), [
        (_native.DPC_STATUS_NONFINITE, lambda: "voxel_down_sample: cloud %d holds a NaN or inf coordinate"
         % next(i for i, c in enumerate(clouds) if not bool(torch.isfinite(c).all()))),
        (_native.DPC_STATUS_VOXEL_TOO_SMALL, "voxel_down_sample: voxel_size %r is too small for a cloud's extent (open3d: "
         "voxel_size * 2147483647 < the padded bounding box's largest side)" % vs),
        (_native.DPC_STATUS_KEY_OVERFLOW, "voxel_down_sample: the batch's voxel keys need more than 64 bits at voxel_size "
         "%r (%d clouds); pass fewer clouds per call or a larger voxel" % (vs, C))])
    counts, offsets = info[1:1 + C], info[1 + C:]
    V = int(counts.sum())
    return out[:V].clone(), counts, offsets


def voxel_down_sample(clouds, voxel_size):
    """open3d.voxel_down_sample(pcd, voxel_size) for every cloud, in one call and one synchronisation.

    clouds: a list of [n_i,3] float32 / float64 arrays or tensors, or a single [n,3] cloud.  Returns a list of [m_i,3]
    float64 tensors on the device (a single tensor for a single cloud): each voxel's points averaged in fp64, summed one
    at a time in input order, voxels in ascending (kx, ky, kz) order.  ValueError, before anything touches a device, for a
    voxel_size that is not finite and > 0 or a cloud that is not [n,3] float; after the call for NaN or inf coordinates,
    open3d's "voxel_size is too small" rule, or a batch whose voxel keys need more than 64 bits."""
    vs = _voxel_size(voxel_size)
    single = isinstance(clouds, (torch.Tensor, np.ndarray))
    items = [_cloud(c, i) for i, c in enumerate([clouds] if single else list(clouds))]
    if not items:
        return []
    voxels, counts, offsets = _downsample_packed(items, vs)
    res = [voxels[int(o):int(o) + int(n)] for o, n in zip(offsets, counts)]
    return res[0] if single else res


def downsample_split(model_names, load_dense, voxel_size=0.01, save=None, clouds_per_call=256):
    """downsample_gt.py's loop (densify/downsample_gt.py:38-57) over model_names, clouds_per_call models per native call.

    load_dense(name) -> [n,3] dense cloud, or None to skip the model (scipy.io.loadmat(path)["points"], say);
    save(name, points) is called with each [m,3] float64 result (scipy.io.savemat(path, {"points": points}), say).
    Returns {name: [m,3] float64 numpy}.  The result does not depend on clouds_per_call."""
    vs = _voxel_size(voxel_size)
    step = int(clouds_per_call)
    if step < 1:
        raise ValueError("downsample_split: clouds_per_call must be >= 1")
    result = {}

    def load(name, i):
        dense = load_dense(name)
        return None if dense is None else _cloud(dense, i)

    for batch in _split.batches(model_names, load, step):
        voxels, counts, offsets = _downsample_packed([cloud for _, cloud in batch], vs)
        host = voxels.cpu().numpy()
        for (name, _), o, n in zip(batch, offsets, counts):
            pts = host[int(o):int(o) + int(n)]
            result[name] = pts
            if save is not None:
                save(name, pts)
    return result
