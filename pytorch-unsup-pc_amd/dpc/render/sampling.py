"""Farthest-point sampling of point clouds, batched on the GPU.

Farthest-point sampling (FPS) starts from one point of a cloud and repeatedly takes the point farthest from everything
taken so far.  It is the usual way to bring clouds of unequal size to the common size the Earth Mover's Distance needs
(dpc/render/emd.py): deterministic, and it keeps the cloud's coverage where a uniform draw leaves holes and clumps.  All
clouds of a call go into one dpc_fps call (csrc/dpc_fps.hip: one workgroup per cloud, the cloud held on chip for all its
rounds).

    farthest_point_sample  indices (and the squared covering radii) of the samples, on the device

The distance expression, the tie rule and the outputs are in include/dpc_render.h (dpc_fps).
"""
import numpy as np
import torch

from . import _batch, _native
from ._ops import status_word

_WHAT = "dpc.render farthest-point sampling"
_FN = "farthest_point_sample"
MAX_POINTS = _native.DPC_FPS_MAX_POINTS


def _per_cloud(value, C, name, default=None):
    """value (None, an integer, or one integer per cloud) as a list of C Python ints."""
    if value is None:
        value = default
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    arr = np.asarray(value)
    if arr.dtype == object or not (np.issubdtype(arr.dtype, np.integer) or (arr.dtype.kind == "f" and (arr == np.floor(arr)).all())):
        raise ValueError("%s: %s must be an integer or one integer per cloud, got %r" % (_FN, name, value))
    if arr.ndim == 0:
        return [int(arr)] * C
    if arr.ndim != 1 or len(arr) != C:
        raise ValueError("%s: %s has %s entries for %d clouds" % (_FN, name, arr.shape, C))
    return [int(v) for v in arr]


def _check(clouds, num_samples, first):
    """The argument checks of a call, before anything touches a device: (cloud list, samples, firsts, host table, whether
    the result is one [B,m] tensor).  Every refusal the native entry point makes is made here first with the cloud's
    index in the message; the entry point's own dry run follows."""
    as_tensor = isinstance(clouds, torch.Tensor)
    if as_tensor:
        if clouds.dim() != 3:
            raise ValueError("%s: a tensor of clouds must be [B,n,3], got %s" % (_FN, tuple(clouds.shape)))
        clouds = clouds.unbind(0)
    C_list = [_batch.cloud(c, "%s: clouds[%d]" % (_FN, i)) for i, c in enumerate(clouds)]
    C = len(C_list)
    samples = _per_cloud(num_samples, C, "num_samples")
    firsts = _per_cloud(first, C, "first", 0)
    for i, (c, m, f) in enumerate(zip(C_list, samples, firsts)):
        n = len(c)
        if n == 0:
            raise ValueError("%s: clouds[%d] is empty (n = 0)" % (_FN, i))
        if n > MAX_POINTS:
            raise ValueError("%s: clouds[%d] has %d points, the limit is DPC_FPS_MAX_POINTS = %d (a cloud is held on chip by "
                             "one workgroup)" % (_FN, i, n, MAX_POINTS))
        if not 1 <= m <= n:
            raise ValueError("%s: clouds[%d] has %d points, num_samples = %d is outside [1, %d]" % (_FN, i, n, m, n))
        if not 0 <= f < n:
            raise ValueError("%s: clouds[%d] has %d points, first = %d is outside [0, %d)" % (_FN, i, n, f, n))
    counts = [len(c) for c in C_list]
    start, out = np.cumsum([0] + counts), np.cumsum([0] + samples)
    if start[-1] > _batch.INT32_MAX:
        raise ValueError("%s: more than 2^31 - 1 points in one call" % _FN)
    desc = _batch.table([(start[i], counts[i], firsts[i], out[i], samples[i]) for i in range(C)], 5,
                        "%s: cloud table entries must fit int32" % _FN)
    rc = _native.lib().dpc_fps(None, int(start[-1]), 0, None, desc.ctypes.data, C, None, None, None, None)
    _batch.dry_run(rc, "%s: dpc_fps refused the cloud table" % _FN)
    return C_list, samples, desc, as_tensor and len(set(samples)) <= 1


def _sample(clouds, num_samples, first, status=None):
    """farthest_point_sample with the status word to report into (None: the package's): (indices, radius2, one tensor?)."""
    C_list, samples, desc, stacked = _check(clouds, num_samples, first)
    _batch.refuse_cpu(clouds)
    dev = _batch.device(_WHAT, C_list)
    total_out = int(sum(samples))
    indices = torch.empty((total_out,), dtype=torch.int32, device=dev)
    radius2 = torch.empty((total_out,), dtype=torch.float64, device=dev)
    if C_list:
        dtype = _batch.widest(C_list)    # one fp64 cloud makes the whole call fp64 without changing an index
        pts, _ = _batch.pack(C_list, dev, dtype)
        desc_d = _batch.on_device(desc, dev)
        status = status_word(dev) if status is None else status
        _native.call(dev, "dpc_fps", _native.ptr(pts), int(pts.shape[0]), int(dtype == torch.float64), _native.ptr(desc_d),
                     desc.ctypes.data, len(C_list), _native.ptr(indices), _native.ptr(radius2), _native.ptr(status))
    if stacked:
        m = samples[0] if samples else 0
        return indices.view(len(C_list), m), radius2.view(len(C_list), m)
    return list(indices.split(samples)), list(radius2.split(samples))


def farthest_point_sample(clouds, num_samples, first=None, return_radius=False):
    """Farthest-point sampling of every cloud: int32 indices of num_samples of its points, on the device.  The first is
    point `first`; each later one is the point farthest from all taken before it (squared distance in fp64 whatever the
    input dtype, ties to the lowest index).  With return_radius: (indices, radius2), radius2 float64 in the same shape:
    radius2[k] is the squared distance from sample k to the nearest earlier sample, +inf for k = 0, non-increasing from
    k = 1 on; radius2[k] is also the squared covering radius of the first k samples.

    clouds: a [B,n,3] tensor, or a list of [n_i,3] tensors or arrays, 1 <= n_i <= DPC_FPS_MAX_POINTS (16384).
    num_samples: an int, or one per cloud, in [1, n_i].  first: None (point 0), an int, or one per cloud, in [0, n_i).
    Returns a [B,m] tensor for tensor input with a single m, otherwise a list of [m_i] tensors.  Indices are into each
    cloud's own rows, so cloud[idx.long()] stays differentiable through torch's indexing; the sampling itself has no
    gradient.

    Results are bit-identical from run to run, do not depend on which clouds share a call, and an fp32 cloud gives the
    indices of the same values stored as fp64 (include/dpc_render.h, dpc_fps).  No host synchronisation.  A cloud with a
    NaN or infinite coordinate has indices -1 and radius2 NaN, and sets DPC_STATUS_NONFINITE in the device status word,
    which check_status() returns; the other clouds are unaffected.  ValueError, before anything is launched and naming
    the cloud, for a shape that is not [n,3], an empty cloud, more than DPC_FPS_MAX_POINTS points, num_samples outside
    [1, n] and first outside [0, n); CPU tensors are refused."""
    indices, radius2 = _sample(clouds, num_samples, first)
    return (indices, radius2) if return_radius else indices
