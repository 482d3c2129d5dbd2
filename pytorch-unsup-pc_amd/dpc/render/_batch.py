"""Ragged-batch plumbing shared by the evaluation pipelines (alignment, chamfer, downsample, densify, emd, sampling, voxels,
meshvoxels, pointmesh, visualise, meshviews).

Each packs its items (clouds, pairs of clouds, meshes) into one buffer in the widest dtype among them, describes them in a
host int32 table that also goes to the device, asks the library's own argument checks before anything touches a device (a
dry run with NULL device pointers), allocates the workspace the library asks for, and turns the status bits of a job into
exceptions.

What a whole split needs on top of one such call lives next door in _split.py: the checks and the walk over groups of
models that the *_of_split functions share, and the walk over a split by model name.
"""
import numpy as np
import torch

from . import _native

INT32_MAX = np.iinfo(np.int32).max


def device(what, *groups):
    """The device of the first HIP tensor in groups (iterables of anything), else the current HIP device."""
    for g in groups:
        for x in g:
            if isinstance(x, torch.Tensor) and x.is_cuda:
                return x.device
    if not torch.cuda.is_available():
        raise RuntimeError("%s runs on MI355X only: no HIP device (there is no CPU path)" % what)
    return torch.device("cuda", torch.cuda.current_device())


def cloud(x, what, cast=torch.float32):
    """x (a tensor, or an array wrapped without a copy) as a detached [n,3] tensor; ValueError naming it as `what`
    otherwise.  A cloud that is not float32 / float64 is converted to `cast`, or refused when cast is None."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("%s must be [n,3], got %s" % (what, tuple(t.shape)))
    if t.dtype not in (torch.float32, torch.float64):
        if cast is None:
            raise ValueError("%s must be float32 or float64, got %s" % (what, t.dtype))
        t = t.to(cast)
    return t.detach()


def refuse_cpu(*groups):
    """Arrays are copied to the device; a CPU tensor is refused, as everywhere in the package.  groups: clouds arguments
    as the caller gave them, each a tensor or a list of tensors and arrays (one device per group)."""
    for group in groups:
        _native.require_device(*[c for c in ([group] if isinstance(group, torch.Tensor) else group)
                                 if isinstance(c, torch.Tensor)])


def widest(tensors):
    """float64 when one of the tensors is, else float32: the kernels compute in fp64 and fp32 widens exactly, so one fp64
    item makes the whole call fp64 without changing a result."""
    return torch.float64 if any(t.dtype == torch.float64 for t in tensors) else torch.float32


def pack(clouds, dev, dtype):
    """The clouds ([n_i,3] float32 / float64 tensors, at least one float64 when dtype is) in one contiguous
    [sum n_i, 3] tensor of dtype on dev, and the start of each.  Host clouds are joined by numpy (torch.cat of large host
    tensors took twice as long end to end) and copied once."""
    if any(c.is_cuda for c in clouds):
        packed = torch.cat([c.to(device=dev, dtype=dtype) for c in clouds])
    else:
        packed = torch.from_numpy(np.concatenate([c.numpy() for c in clouds])).to(device=dev, dtype=dtype)
    return packed.contiguous(), np.cumsum([0] + [len(c) for c in clouds])


def table(rows, width, message):
    """rows (an integer array, or a list of row tuples) as a C-contiguous [n, width] int32 host table;
    ValueError(message) when an entry does not fit int32."""
    desc = np.asarray(rows).reshape(-1, width)
    if desc.size and (desc.min() < np.iinfo(np.int32).min or desc.max() > INT32_MAX):
        raise ValueError(message)
    return np.ascontiguousarray(desc, dtype=np.int32)


def on_device(desc, dev):
    """The device copy of a host table; the entry points take both (the host one as desc.ctypes.data)."""
    return torch.from_numpy(desc).to(dev)


def dry_run(rc, message, exc=ValueError):
    """rc: what an entry point returned for the real host table and sizes with NULL for every device pointer; its
    checks run before anything touches a device.  Raises exc(message) when it refused them (DPC_ERR_SHAPE)."""
    if rc == _native.DPC_ERR_SHAPE:
        raise exc(message)


def workspace(nbytes, dev):
    """The workspace a *_workspace_bytes query asked for (at least 16 bytes, so the pointer is never NULL)."""
    return torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)


def raise_status(status, messages, exc=ValueError):
    """Raises exc for the first (DPC_STATUS_* bit, message) of `messages` whose bit is set in status; a message may be
    a callable, called only then."""
    for bit, message in messages:
        if status & bit:
            raise exc(message() if callable(message) else message)
