"""torch.autograd.Function wrappers over the C ABI: tensors in, tensors out, hand-written backward.

PyTorch is plumbing here (device memory, the current HIP stream, the autograd tape); every kernel is in
csrc/.  All work is enqueued on torch's current stream without synchronising, so a whole
forward+backward can be captured in a HIP graph.
"""
import ctypes

import numpy as np
import torch

from . import _native as N


class Geometry:
    """Per-call constants: grid, camera, tap weights (host side)."""

    __slots__ = ("D", "H", "W", "kxy", "kz", "camera_distance", "focal_length", "clip_val", "max_depth", "schedule",
                 "_params", "_kptrs")

    def __init__(self, D, H, W, kxy=None, kz=None, camera_distance=2.0, focal_length=1.875, clip_val=1e-5,
                 max_depth=10.0, schedule=None):
        """schedule: a DeviceSchedule (below) whose device-resident tap values / live-point count the kernels read at run
        time instead of this object's host arrays -- for captured HIP graphs that follow a sigma / dropout schedule."""
        self.schedule = schedule
        self.D, self.H, self.W = int(D), int(H), int(W)
        self.kxy = None if kxy is None else np.ascontiguousarray(kxy, dtype=np.float32).reshape(-1)
        self.kz = None if kz is None else np.ascontiguousarray(kz, dtype=np.float32).reshape(-1)
        if self.kxy is not None and self.kz is None:
            raise ValueError("an x/y kernel needs its z kernel (a z kernel alone is the D pass on a grid that has been through W and H)")
        for k in (self.kxy, self.kz):
            if k is not None and (k.size % 2 == 0 or k.size > N.DPC_MAX_TAPS):
                raise ValueError("smoothing kernels must have odd length <= %d, got %d" % (N.DPC_MAX_TAPS, k.size))
        self.camera_distance, self.focal_length = float(camera_distance), float(focal_length)
        self.clip_val, self.max_depth = float(clip_val), float(max_depth)
        self._params = {}     # (B, Npts, replicas) -> Sized DpcParams of the calls without a point_index
        self._kptrs = (None if self.kxy is None else self.kxy.ctypes.data, None if self.kz is None else self.kz.ctypes.data)

    def sized(self, B, Npts, point_replicas=1, point_index=None, n_src=0):
        """The DpcParams block of a call together with the buffer sizes the library derives from it (three native calls),
        as a `Sized`; cached per call shape when there is no per-call pointer in it (no point_index)."""
        if point_index is not None:
            return Sized(self.params(B, Npts, point_replicas, point_index, n_src))
        key = (B, Npts, point_replicas, n_src)
        hit = self._params.get(key)
        if hit is None:
            if len(self._params) >= 32:
                self._params.clear()
            hit = self._params[key] = Sized(self.params(B, Npts, point_replicas, None, n_src))
        return hit

    def params(self, B, Npts, point_replicas=1, point_index=None, n_src=0):
        """point_index: int32 device tensor [B,Npts] (kept alive by the caller for the duration of the call) selecting
        every cloud's points out of a stored set of n_src points."""
        sch = self.schedule
        dev = None if point_index is None else point_index.device
        return N.DpcParams(int(B), int(Npts), self.D, self.H, self.W,
                           0 if self.kxy is None else self.kxy.size, 0 if self.kz is None else self.kz.size,
                           self.camera_distance, self.focal_length, self.clip_val, self.max_depth, int(point_replicas),
                           int(n_src), None if point_index is None else point_index.data_ptr(),
                           None if dev is None or dev.type != "cuda" else status_word(dev).data_ptr(),
                           None if sch is None or sch.n_live is None else sch.n_live.data_ptr(),
                           None if sch is None or self.kxy is None else sch.taps_xy.data_ptr(),
                           None if sch is None or self.kz is None else sch.taps_z.data_ptr())

    def kern_ptrs(self):
        """Host addresses of the tap arrays (plain ints / None: the argtypes of the bindings take them as void*)."""
        return self._kptrs


class Sized:
    """A DpcParams block, a reference to it for the calls, and the sizes of the buffers a call with it needs."""

    __slots__ = ("P", "ref", "wpp", "cells_bytes", "ws_bytes", "bwd_rc")

    def __init__(self, P):
        L = N.lib()
        self.P, self.ref = P, ctypes.byref(P)
        self.wpp = L.dpc_mask_words_per_plane(self.ref)
        self.cells_bytes = max(L.dpc_cells_bytes(self.ref), 1)
        self.ws_bytes = max(L.dpc_workspace_bytes(self.ref), 1)
        self.bwd_rc = L.dpc_check_grid(self.ref, 1)   # 0, or why a backward could not follow a forward of this shape

    def require_backward(self, where):
        """A call whose inputs require gradients is refused BEFORE anything is launched when its backward could not run (grids
        wider than the backward's LDS tile): a forward that succeeds and a backward that then raises is the worse surprise."""
        if self.bwd_rc != 0:
            raise N.DpcError(self.bwd_rc, where + " (the inputs require gradients and the backward of this grid could not run)")


_status = {}


def status_word(device):
    """The int32 status word of `device` that every call with a point_index hands to the kernels (DpcParams.status): the
    DPC_STATUS_* bits are OR-ed into it on the device; read (and cleared) by dpc.render.check_status at a point where the
    caller synchronises anyway."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    w = _status.get(device)
    if w is None:
        w = _status[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return w


class DeviceSchedule:
    """Per-step schedule values in DEVICE memory, so that a captured HIP graph follows them from replay to replay
    (dpc/models/model_pc_to.py:59-87, 171-179, 254-258: sigma_rel(step) and the dropout keep-probability are recomputed every
    step; a graph freezes kernel arguments, not memory).  taps_xy / taps_z hold the Gaussian's current values, n_live the
    current number of kept points per cloud.  update() is one tiny launch on the current stream (the values travel as its
    arguments) -- enqueue it in front of a replay.  `buckets` remembers the compiled tap windows the graph was captured
    for: fits() says whether new values still fit them."""

    def __init__(self, device, kxy, kz, n_live=None, capacity=None):
        kxy = np.ascontiguousarray(kxy, dtype=np.float32).reshape(-1)
        kz = np.ascontiguousarray(kz, dtype=np.float32).reshape(-1)
        self.device = torch.device(device)
        self.taps_xy = torch.zeros(N.DPC_MAX_TAPS, dtype=torch.float32, device=device)
        self.taps_z = torch.zeros(N.DPC_MAX_TAPS, dtype=torch.float32, device=device)
        self.n_live = None if n_live is None else torch.zeros(1, dtype=torch.int32, device=device)
        self.capacity = capacity
        self.sizes = (kxy.size, kz.size)
        self.buckets = (taps_bucket(kxy), taps_bucket(kz))
        self.update(kxy, kz, n_live)

    def fits(self, kxy, kz, n_live=None):
        kxy = np.ascontiguousarray(kxy, dtype=np.float32).reshape(-1)
        kz = np.ascontiguousarray(kz, dtype=np.float32).reshape(-1)
        if (kxy.size, kz.size) != self.sizes:
            return False
        bx, bz = taps_bucket(kxy), taps_bucket(kz)
        if bx < 0 or bz < 0 or bx > self.buckets[0] or bz > self.buckets[1]:
            return False
        return n_live is None or self.capacity is None or n_live <= self.capacity

    def tight(self, kxy, kz, n_live=None):
        """fits(), and a graph captured for the new values would be no cheaper (same tap windows, capacity not twice the
        live count)."""
        if not self.fits(kxy, kz, n_live):
            return False
        kxy = np.ascontiguousarray(kxy, dtype=np.float32).reshape(-1)
        kz = np.ascontiguousarray(kz, dtype=np.float32).reshape(-1)
        same = (taps_bucket(kxy), taps_bucket(kz)) == self.buckets
        return same and (n_live is None or self.capacity is None or 2 * n_live > self.capacity or self.capacity <= 512)

    def update(self, kxy, kz, n_live=None):
        kxy = np.ascontiguousarray(kxy, dtype=np.float32).reshape(-1)
        kz = np.ascontiguousarray(kz, dtype=np.float32).reshape(-1)
        if (kxy.size, kz.size) != self.sizes:
            raise ValueError("the schedule was built for kernels of %s taps, got %s" % (self.sizes, (kxy.size, kz.size)))
        if not self.fits(kxy, kz, n_live):
            # the kernels that read these values were compiled / captured for the tap windows `buckets` and rows of `capacity`
            # slots: taps outside the window would be dropped silently, points beyond the rows never read
            raise ValueError("schedule values do not fit what the schedule was built for: tap windows %s (needed %s), capacity %s "
                             "(n_live %s) -- build a new DeviceSchedule (and capture again)"
                             % (self.buckets, (taps_bucket(kxy), taps_bucket(kz)), self.capacity, n_live))
        N.call(self.device, "dpc_schedule_update", kxy.ctypes.data, kxy.size, kz.ctypes.data, kz.size,
               0 if n_live is None else int(n_live), N.ptr(self.taps_xy), N.ptr(self.taps_z), N.ptr(self.n_live))


class DeviceTaps:
    """One 1-D kernel in DEVICE memory for dpc.render.smooth_gt(schedule=...): the part of a DeviceSchedule the ground-truth
    node reads (`taps_xy`, `sizes`), with no compiled tap window to fit -- the node takes any values of the same length.
    A captured training step keeps one of these for the ground truth next to the projection's DeviceSchedule, so that
    cfg.pc_gauss_filter_gt_switch_off can put the identity kernel there while sigma_rel < 1 without touching the taps the
    projection reads.  update() is one tiny launch on the current stream; enqueue it in front of a replay."""

    def __init__(self, device, kxy):
        kxy = np.ascontiguousarray(kxy, dtype=np.float32).reshape(-1)
        if kxy.size % 2 == 0 or kxy.size > N.DPC_MAX_TAPS:
            raise ValueError("smoothing kernels must have odd length <= %d, got %d" % (N.DPC_MAX_TAPS, kxy.size))
        self.device = torch.device(device)
        self.taps_xy = torch.zeros(N.DPC_MAX_TAPS, dtype=torch.float32, device=device)
        self.sizes = (kxy.size, 0)
        self.update(kxy)

    def update(self, kxy):
        kxy = np.ascontiguousarray(kxy, dtype=np.float32).reshape(-1)
        if kxy.size != self.sizes[0]:
            raise ValueError("the tap buffer was built for a kernel of %d taps, got %d" % (self.sizes[0], kxy.size))
        N.call(self.device, "dpc_schedule_update", kxy.ctypes.data, kxy.size, None, 0, 0, N.ptr(self.taps_xy), None, None)


def gt_smooth(gt, channels, planar, source, size, mode, taps=None, dev_taps=None, ntaps=None, remap=None):
    """dpc_gt_smooth (csrc/dpc_gt_smooth.hip): gt, S samples of `channels` channels of source = (Hs, Ws) = (f*H, f*W) values
    ([S,C,Hs,Ws] when planar, else [S,Hs,Ws,C]; fp32 after conversion), size (H, W) -> [S,H,W,C] fp32: remap (remap = (from, to) | None),
    resize by f (mode DPC_GT_RESIZE_MEAN / _SAMPLE), two-pass zero-padded blur.  Taps: a host array `taps`, or `dev_taps`
    (a device tensor read by the kernel at run time) with its length `ntaps`.  One launch, no gradient."""
    dev = N.require_device(gt, dev_taps)
    (Hs, Ws), (H, W) = (int(v) for v in source), (int(v) for v in size)
    g32 = _f32(gt)
    S, C = g32.shape[0], int(channels)
    if S * C * Hs * Ws != g32.numel():
        raise ValueError("ground truth %s does not hold %d x %d planes of %dx%d" % (tuple(gt.shape), S, C, Hs, Ws))
    host = None
    if dev_taps is None:
        host = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        ntaps = host.size
    elif dev_taps.dtype is not torch.float32 or dev_taps.numel() < int(ntaps):
        raise ValueError("dev_taps must hold %d fp32 values" % int(ntaps))
    lo, hi = (0.0, 0.0) if remap is None else (float(remap[0]), float(remap[1]))
    out = torch.empty((S, H, W, C), dtype=torch.float32, device=dev)
    N.call(dev, "dpc_gt_smooth", N.ptr(g32), S, C, Hs, Ws, int(bool(planar)), H, W, int(mode), lo, hi,
          None if host is None else host.ctypes.data, N.ptr(dev_taps), int(ntaps), N.ptr(out))
    return out


def taps_bucket(k):
    """Compiled tap-window radius a 1-D kernel needs in the fused kernels (-1: beyond them)."""
    k = np.ascontiguousarray(k, dtype=np.float32).reshape(-1)
    return N.lib().dpc_taps_bucket(k.ctypes.data, k.size)


def _f32(t):
    if t is None:
        return None
    if t.dtype is torch.float32 and t.is_contiguous():
        return t.detach()
    return t.detach().to(torch.float32).contiguous()


def _replicas(pc, q):
    """Clouds per point set: pc [S,N,3] shared by consecutive groups of B/S rows of q [B,4] (tf_repeat_0 order)."""
    B, S = q.shape[0], pc.shape[0]
    if S == B:
        return 1
    if S == 0 or B % S:
        raise ValueError("%d poses cannot share %d point sets: the number of clouds must be a multiple" % (B, S))
    return B // S


def _index32(point_index, pc, q):
    """Per-cloud point selection [B,n] -> contiguous int32 on the inputs' device (None passes through)."""
    if point_index is None:
        return None
    if point_index.dim() != 2 or point_index.shape[0] != q.shape[0]:
        raise ValueError("point_index must be [%d, n] (one row of point indices per cloud), got %s"
                         % (q.shape[0], tuple(point_index.shape)))
    if point_index.device != pc.device:
        raise RuntimeError("point_index lives on %s, the points on %s" % (point_index.device, pc.device))
    return point_index.detach().to(torch.int32).contiguous()


def _plane(shape):
    """(rows, cols) of a stack of single-channel images: [n,1,h,w] (NCHW, the reference's inputs["masks"]), [n,h,w,1] (its
    permuted masks and silhouettes) or [n,h,w]; None for any other layout."""
    if len(shape) == 4 and shape[3] == 1:
        return shape[1], shape[2]
    if len(shape) == 4 and shape[1] == 1:
        return shape[2], shape[3]
    if len(shape) == 3:
        return shape[1], shape[2]
    return None


def mask_factor(gt, S, H, W):
    """Pooling factor f of the ground truth of the fused loss (add_proj_loss, model_pc_to.py:346-354): 1 when `gt` holds
    S x H x W values (masks already pooled to the silhouette size, any [S, ...] layout), otherwise f = Hm / H = Wm / W for
    masks [S,1,Hm,Wm] or [S,Hm,Wm,1] -- the kernels pool them like nn.AvgPool2d(f), bit for bit.  Checked on the host:
    ValueError for a mask side below the silhouette's (the reference asserts) or not an integer multiple of it."""
    shape = tuple(gt.shape)
    if not shape or shape[0] != S:
        raise ValueError("gt must hold the masks of %d samples ([%d,1,Hm,Wm] or [%d,Hm,Wm,1]), got %s" % (S, S, S, shape))
    if gt.numel() == S * H * W:
        return 1
    plane = _plane(shape)
    if plane is None:
        raise ValueError("gt must be masks [%d,1,Hm,Wm] or [%d,Hm,Wm,1], got %s" % (S, S, shape))
    Hm, Wm = plane
    if Hm < H or Wm < W:
        raise ValueError("GT size should not be smaller than the prediction size: masks %dx%d, silhouettes %dx%d"
                         % (Hm, Wm, H, W))
    if Hm % H or Wm % W or Hm // H != Wm // W:
        raise ValueError("masks %dx%d are not an integer multiple of the %dx%d silhouettes (AvgPool2d(gt_size // pred_size))"
                         % (Hm, Wm, H, W))
    f = Hm // H
    if f * H > 1024 or f * W > 1024:
        raise ValueError("masks %dx%d: sides above 1024 are not supported" % (Hm, Wm))
    return f


def _weights32(weights, S):
    """Per-sample loss weights (the reference's inputs["valid_samples"]) -> contiguous fp32 [S]; None passes through."""
    if weights is None:
        return None
    if tuple(weights.shape) != (S,):
        raise ValueError("valid_samples must be [%d] (one weight per sample), got %s" % (S, tuple(weights.shape)))
    return _f32(weights)


def _meta(t):
    """(dtype, shape) of an input -- kept on ctx instead of the tensor itself (no reference cycles)."""
    return None if t is None else (t.dtype, tuple(t.shape))


def _small(dsmall, col, width, B):
    """Dense [B,width] view of one gradient block of the small-gradient buffer (contiguous: autograd takes it
    without cloning)."""
    return dsmall.as_strided((B, width), (width, 1), col * B)   # one op instead of a slice and a view


def _like_input(grad, meta):
    """Gradients arrive in the input's dtype and shape, like autograd's would."""
    if grad is None or meta is None:
        return None
    if grad.dtype is meta[0] and tuple(grad.shape) == meta[1]:
        return grad
    return grad.to(meta[0]).reshape(meta[1])


def _zero_grads(metas, dev):
    """Backward of an empty batch (no clouds on this rank): zeros in every input's own dtype and shape."""
    return tuple(None if m is None else torch.zeros(m[1], dtype=m[0], device=dev) for m in metas)


def _pose_grads(metas, has, dpc, dsmall, B, nones):
    """What the backward of a node with inputs (pc, q, t, f[, s], ...) returns: d pc and the blocks of the small-gradient
    buffer, each like its input (`metas`); `has`: which of t, f[, s] were given; then `nones` Nones for the other arguments."""
    grads = [_like_input(dpc, metas[0]), _like_input(_small(dsmall, N.COL_DQ, 4, B), metas[1])]
    for meta, present, (col, width) in zip(metas[2:], has, ((N.COL_DT, 3), (N.COL_DF, 1), (N.COL_DS, 1))):
        grads.append(_like_input(_small(dsmall, col, width, B), meta) if present else None)
    return tuple(grads) + (None,) * nones


def _new_cells(P, dev):
    return torch.empty((max(N.lib().dpc_cells_bytes(ctypes.byref(P)), 1),), dtype=torch.uint8, device=dev)


def decode_cells(cells, B, Npts, D):
    """Test helper: binned point records -> (code [B,N] int32, frac [B,N,3] float32, pts [B,N,3] float32) in
    original point order; also checks each chunk's z sort and bin offsets."""
    nblk = (Npts + 255) // 256
    chunk = 256 * 32 + ((2 * (D + 2) + 15) // 16) * 16
    raw = cells.cpu().numpy().reshape(B, nblk, chunk)
    code = np.full((B, Npts), -2, dtype=np.int32)
    frac = np.zeros((B, Npts, 3), dtype=np.float32)
    pts = np.zeros((B, Npts, 3), dtype=np.float32)
    for b in range(B):
        for k in range(nblk):
            n = min(256, Npts - 256 * k)
            rec = raw[b, k, :256 * 16].view(np.int32).reshape(256, 4)[:n]
            aux = raw[b, k, 256 * 16:256 * 32].view(np.int32).reshape(256, 4)[:n]
            perm = aux[:, 3]
            offs = raw[b, k, 256 * 32:256 * 32 + 2 * (D + 2)].view(np.uint16)
            assert offs[D + 1] == n and np.all(np.diff(offs.astype(np.int64)) >= 0)
            bins = np.where(rec[:, 0] < 0, D, rec[:, 0] >> 20)
            assert np.array_equal(np.sort(bins), bins), "records are not sorted by z bin"
            assert np.array_equal(np.searchsorted(bins, np.arange(D + 2)), offs), "bin offsets do not match the records"
            code[b, perm] = rec[:, 0]
            frac[b, perm] = rec[:, 1:].view(np.float32)
            pts[b, perm] = aux[:, :3].view(np.float32)
    assert (code != -2).all(), "some points are missing from the bins"
    return code, frac, pts


def locate_points(pc, q, t, f, geom):
    """First launch of the fused forward alone: (tr_pc [B,N,3] fp32, cells [B,N,4] int32 point records)."""
    dev = N.require_device(pc, q, t, f)
    pc32, q32, t32, f32 = _f32(pc), _f32(q), _f32(t), _f32(f)
    B, Npts = pc32.shape[0], pc32.shape[1]
    P = geom.params(B, Npts)
    tr = torch.empty_like(pc32)
    cells = _new_cells(P, dev)
    N.call(dev, "dpc_locate", ctypes.byref(P), N.ptr(pc32), N.ptr(q32), N.ptr(t32), N.ptr(f32), N.ptr(tr), N.ptr(cells))
    return tr, cells


# ------------------------------------------------------------------------------------------------------
# Fused hot path
# ------------------------------------------------------------------------------------------------------
class ProjectFused(torch.autograd.Function):
    """pointcloud_project_fast as three launches forward, two backward (csrc/dpc_entry.hip and the kernel files it names).

    forward(pc [B,N,3], q [B,4], t [B,3]|None, f [B,1]|None, s [B,1]|None, geom) -> proj [B,H,W,1], grid_wh [B,D,H,W]
    Saved for backward: the binned point records, the grid after clamp + W/H passes, the clamp mask and the per-ray
    transmittance.  grid_wh (the grid after clamp and the W, H passes) is a differentiable output too: the other entries
    of the reference's output dict are derived from it on demand (D pass, scale/clamp, DRC probabilities) and their
    gradients come back through here, added to the silhouette's -- the chain never runs a second time.
    """

    @staticmethod
    def forward(ctx, pc, q, t, f, s, geom, point_index=None, want_grad=False):
        dev = N.require_device(pc, q, t, f, s)
        pc32, q32, t32, f32, s32 = _f32(pc), _f32(q), _f32(t), _f32(f), _f32(s)
        idx = _index32(point_index, pc32, q32)
        B, reps = q32.shape[0], _replicas(pc32, q32)
        Npts = pc32.shape[1] if idx is None else idx.shape[1]
        Z = geom.sized(B, Npts, reps, idx, pc32.shape[1])
        # grad mode is always off INSIDE forward(): the caller passes what it saw outside
        if want_grad and B > 0 and any(x is not None and x.requires_grad for x in (pc, q, t, f, s)):
            Z.require_backward("dpc_project_fwd")
        grid_wh = torch.empty((B, geom.D, geom.H, geom.W), dtype=torch.float32, device=dev)
        mask = torch.empty((B, geom.D, Z.wpp), dtype=torch.int64, device=dev)
        cells = torch.empty((Z.cells_bytes,), dtype=torch.uint8, device=dev)
        proj = torch.empty((B, geom.H, geom.W, 1), dtype=torch.float32, device=dev)
        trans = torch.empty((B, geom.H, geom.W), dtype=torch.float32, device=dev)
        kxy, kz = geom.kern_ptrs()
        N.call(dev, "dpc_project_fwd", Z.ref, N.ptr(pc32), N.ptr(q32), N.ptr(t32), N.ptr(f32), N.ptr(s32), kxy, kz,
               None, N.ptr(cells), None, N.ptr(grid_wh), None, N.ptr(mask), N.ptr(proj), N.ptr(trans))
        ctx.geom = geom
        ctx.inputs = tuple(_meta(x) for x in (pc, q, t, f, s))
        empty = pc32.new_empty(0)
        ctx.save_for_backward(pc32, q32, t32 if t32 is not None else empty, f32 if f32 is not None else empty,
                              s32 if s32 is not None else empty, grid_wh, mask, cells, trans)
        ctx.has = (t is not None, f is not None, s is not None)
        ctx.npts, ctx.indexed = Npts, idx is not None
        ctx.set_materialize_grads(False)
        return proj, grid_wh

    @staticmethod
    def backward(ctx, dproj, dgrid):
        if dproj is None and dgrid is None:
            return None, None, None, None, None, None, None, None
        pc32, q32, t32, f32, s32, grid_wh, mask, cells, trans = ctx.saved_tensors
        has_t, has_f, has_s = ctx.has
        t32 = t32 if has_t else None
        f32 = f32 if has_f else None
        s32 = s32 if has_s else None
        geom = ctx.geom
        dev = pc32.device
        B, reps = q32.shape[0], _replicas(pc32, q32)
        Z = geom.sized(B, ctx.npts, reps, cells if ctx.indexed else None, pc32.shape[1])  # the backward reads the source
        # index out of the binned records; any non-NULL pointer says "dpc is per stored set, accumulate"
        dproj32 = torch.zeros((B, geom.H, geom.W), dtype=torch.float32, device=dev) if dproj is None else _f32(dproj)
        dgrid32 = _f32(dgrid)
        dpc = torch.zeros_like(pc32) if (reps > 1 or ctx.indexed) else torch.empty_like(pc32)  # clouds add into a shared gradient
        dsmall = torch.empty((N.DPC_SMALL_COLS * B,), dtype=torch.float32, device=dev)
        ws = torch.empty((Z.ws_bytes,), dtype=torch.uint8, device=dev)
        kxy, kz = geom.kern_ptrs()
        N.call(dev, "dpc_project_bwd", Z.ref, N.ptr(pc32), N.ptr(q32), N.ptr(t32), N.ptr(f32), N.ptr(s32), kxy, kz,
               N.ptr(cells), N.ptr(grid_wh), N.ptr(mask), N.ptr(trans), N.ptr(dproj32), N.ptr(dgrid32),
               N.ptr(dpc), N.ptr(dsmall), N.ptr(ws))
        return _pose_grads(ctx.inputs, ctx.has, dpc, dsmall, B, 3)


class ProjectLossFused(torch.autograd.Function):
    """pointcloud_project_fast + the caller's silhouette loss (add_proj_loss / proj_loss_pose_candidates) in one
    autograd node.  With one pose candidate per sample and gradients required, the forward's ray-march kernel also runs
    the column half of the backward (DRC backward + adjoint D pass, for dloss = 1), so the whole step is 3 launches
    forward + 1 backward; otherwise 3 (+ finalize) forward + 2 backward.  The silhouette gradient is never
    materialised; losing pose candidates skip their backward.

    forward(pc, q, t, f, s, gt, geom, K, point_index, want_grad, weights) -> (loss [], proj [B,H,W,1], winner [S] int32)
    gt: masks [S,1,f*H,f*W] or [S,f*H,f*W,1] (pooled f x f inside the kernels, mask_factor), or [S,H,W,1] already pooled;
    weights: [S] | None, the reference's valid_samples (loss = sum_s w_s^2 min_k sse / S).  gt and weights get no gradient.
    """

    @staticmethod
    def forward(ctx, pc, q, t, f, s, gt, geom, num_candidates, point_index=None, want_grad=True, weights=None):
        # shapes of the ground truth and the weights first: refused before anything touches the device
        B, K = q.shape[0], int(num_candidates)
        if K < 1 or B % K:
            raise ValueError("%d clouds is not a multiple of %d pose candidates" % (B, K))
        S = B // K
        if gt.dim() == 0 or gt.shape[0] != S:
            raise ValueError("gt must be [%d,%d,%d,1] (masks pooled to the silhouette size) or masks [%d,1,f*%d,f*%d], got %s"
                             % (S, geom.H, geom.W, S, geom.H, geom.W, tuple(gt.shape)))
        gf = mask_factor(gt, S, geom.H, geom.W)
        if weights is not None and tuple(weights.shape) != (S,):
            raise ValueError("valid_samples must be [%d] (one weight per sample), got %s" % (S, tuple(weights.shape)))
        dev = N.require_device(pc, q, t, f, s, gt, weights)
        pc32, q32, t32, f32, s32, gt32 = _f32(pc), _f32(q), _f32(t), _f32(f), _f32(s), _f32(gt)
        w32 = _weights32(weights, S)
        idx = _index32(point_index, pc32, q32)
        reps = _replicas(pc32, q32)
        Npts = pc32.shape[1] if idx is None else idx.shape[1]
        if B == 0:   # an empty shard (more ranks than samples): nothing to launch, loss 0, zero gradients
            ctx.empty, ctx.dev = True, dev
            ctx.inputs = tuple(_meta(x) for x in (pc, q, t, f, s))
            ctx.set_materialize_grads(False)
            proj = torch.zeros((0, geom.H, geom.W, 1), dtype=torch.float32, device=dev)
            winner = torch.zeros((0,), dtype=torch.int32, device=dev)
            ctx.mark_non_differentiable(proj, winner)
            return torch.zeros((), dtype=torch.float32, device=dev), proj, winner
        ctx.empty = False
        Z = geom.sized(B, Npts, reps, idx, pc32.shape[1])
        f32e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        grid_wh, proj, trans = f32e(B, geom.D, geom.H, geom.W), f32e(B, geom.H, geom.W, 1), f32e(B, geom.H, geom.W)
        sse, loss = f32e(B), torch.empty((), dtype=torch.float32, device=dev)
        sse_tiles = f32e(B, (geom.H * geom.W + 255) // 256)   # per-tile partials of the unfused ray march (fixed-order sum)
        mask = torch.empty((B, geom.D, Z.wpp), dtype=torch.int64, device=dev)
        winner = torch.empty((S,), dtype=torch.int32, device=dev)
        cells = torch.empty((Z.cells_bytes,), dtype=torch.uint8, device=dev)
        # backward buffers handed to the forward so it can run the column half of the backward right away -- only when a
        # backward can follow (grad mode is always off INSIDE forward(): the caller passes what it saw outside)
        want_grad = want_grad and any(x is not None and x.requires_grad for x in (pc, q, t, f, s))
        if want_grad:
            Z.require_backward("dpc_project_loss_fwd")
        ws = dsmall = None
        if want_grad and K == 1:
            ws = torch.empty((Z.ws_bytes,), dtype=torch.uint8, device=dev)
            dsmall = f32e(N.DPC_SMALL_COLS * B)
        fused = ctypes.c_int(0)
        kxy, kz = geom.kern_ptrs()
        N.call(dev, "dpc_project_loss_fwd", Z.ref, N.ptr(pc32), N.ptr(q32), N.ptr(t32), N.ptr(f32), N.ptr(s32), kxy, kz,
               N.ptr(gt32), gf, N.ptr(w32), K, None, N.ptr(cells), N.ptr(grid_wh), N.ptr(mask), N.ptr(proj),
               N.ptr(trans), N.ptr(sse), N.ptr(sse_tiles), N.ptr(loss), N.ptr(winner), N.ptr(ws), N.ptr(dsmall),
               ctypes.byref(fused))
        ctx.geom, ctx.K, ctx.fused, ctx.gf, ctx.weighted = geom, K, bool(fused.value), gf, w32 is not None
        ctx.inputs = tuple(_meta(x) for x in (pc, q, t, f, s))
        empty = pc32.new_empty(0)
        ctx.save_for_backward(pc32, q32, t32 if t32 is not None else empty, f32 if f32 is not None else empty,
                              s32 if s32 is not None else empty, gt32, grid_wh, mask, cells, proj, trans, winner,
                              ws if ctx.fused else empty, dsmall if ctx.fused else empty, w32 if w32 is not None else empty)
        ctx.has = (t is not None, f is not None, s is not None)
        ctx.npts, ctx.indexed = Npts, idx is not None
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(proj, winner)
        return loss, proj, winner

    @staticmethod
    def backward(ctx, dloss, _dproj, _dwinner):
        if dloss is None:
            return (None,) * 11
        if ctx.empty:
            return _zero_grads(ctx.inputs, ctx.dev) + (None,) * 6
        pc32, q32, t32, f32, s32, gt32, grid_wh, mask, cells, proj, trans, winner, ws, dsmall, w32 = ctx.saved_tensors
        w32 = w32 if ctx.weighted else None
        has_t, has_f, has_s = ctx.has
        t32, f32, s32 = (t32 if has_t else None), (f32 if has_f else None), (s32 if has_s else None)
        geom, dev = ctx.geom, pc32.device
        B, reps = q32.shape[0], _replicas(pc32, q32)
        Z = geom.sized(B, ctx.npts, reps, cells if ctx.indexed else None, pc32.shape[1])  # see ProjectFused.backward
        dl = dloss.detach().to(torch.float32).reshape(())
        dpc = torch.zeros_like(pc32) if (reps > 1 or ctx.indexed) else torch.empty_like(pc32)  # clouds add into a shared gradient
        # a FRESH block for dq / ds / dt / df on every call: k_gather_hw writes (never accumulates) them, and a block kept
        # across calls would alias the .grad tensors autograd took over from an earlier backward through this same forward
        out_small = torch.empty((N.DPC_SMALL_COLS * B,), dtype=torch.float32, device=dev)
        if not ctx.fused:
            ws = torch.empty((Z.ws_bytes,), dtype=torch.uint8, device=dev)
        kxy, kz = geom.kern_ptrs()
        N.call(dev, "dpc_project_loss_bwd", Z.ref, N.ptr(pc32), N.ptr(q32), N.ptr(t32), N.ptr(f32), N.ptr(s32), kxy, kz,
               N.ptr(cells), N.ptr(grid_wh), N.ptr(mask), N.ptr(proj), N.ptr(trans), N.ptr(gt32),
               ctx.gf, N.ptr(w32), ctx.K, N.ptr(winner), N.ptr(dl), int(ctx.fused), N.ptr(dpc), N.ptr(out_small), N.ptr(ws))
        return _pose_grads(ctx.inputs, ctx.has, dpc, out_small, B, 6)


class ProjectLossStep:
    """One training step's worth of the renderer -- pointcloud_project_loss and its backward -- as a PLAN: every buffer is
    allocated once and a call is ONE native call that enqueues the kernels on torch's current stream
    (dpc_project_loss_step, include/dpc_render.h: four launches with one pose candidate per sample, six with K).  What a loop
    uses instead of capturing the autograd path into a HIP graph: the same kernels and bits, no Python between the
    launches, and on MI355X 2-3 us per step faster than the replayed graph.  Gradients land in the plan's static tensors.

        plan = ProjectLossStep(geom, B, N, device)           # geom: dpc.render._geometry(cfg, kernel)
        loss = plan.run(pc, q, s, gt)                         # fp32 contiguous device tensors [B/R,N,3], [B,4], [B,1]|None, [B/K,H,W,1]
        loss = plan.run(pc, q, s, masks, valid_samples=w)     # or the raw masks [B/K,1,f*H,f*W] (pooled in the kernels) and
                                                              # per-sample weights [B/K] (loss = sum_s w_s^2 min_k sse / S)
        plan.dpc, plan.dq, plan.ds (plan.dt, plan.df)         # d loss / d input, overwritten by every run; plan.proj, plan.winner

    num_candidates = K pose candidates per sample (min-of-K loss); point_replicas = R clouds share a point set (pc is
    [B/R,N,3], the gradient [B/R,N,3] summed over the replicas)."""

    def __init__(self, geom, B, Npts, device, num_candidates=1, point_replicas=1):
        L = N.lib()
        self.geom, self.B, self.N, self.device = geom, int(B), int(Npts), torch.device(device)
        self.K, self.R = int(num_candidates), int(point_replicas)
        if self.K < 1 or self.B % self.K or self.R < 1 or self.B % self.R:
            raise ValueError("%d clouds: not a multiple of %d candidates / %d replicas" % (self.B, self.K, self.R))
        dev = self.device
        self.P = geom.params(self.B, self.N, self.R)
        P = self.P
        f32e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        wpp = L.dpc_mask_words_per_plane(ctypes.byref(P))
        self.cells = _new_cells(P, dev)
        self.grid_wh = f32e(self.B, geom.D, geom.H, geom.W)
        self.mask = torch.empty((self.B, geom.D, wpp), dtype=torch.int64, device=dev)
        self.proj, self.trans, self.sse = f32e(self.B, geom.H, geom.W, 1), f32e(self.B, geom.H, geom.W), f32e(self.B)
        self.sse_tiles = f32e(self.B, (geom.H * geom.W + 255) // 256)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.winner = torch.empty((self.B // self.K,), dtype=torch.int32, device=dev)
        self.ws = torch.empty((max(L.dpc_workspace_bytes(ctypes.byref(P)), 1),), dtype=torch.uint8, device=dev)
        self.fwd_dsmall, self.dsmall = f32e(N.DPC_SMALL_COLS * self.B), f32e(N.DPC_SMALL_COLS * self.B)
        self.dpc = torch.zeros((self.B // self.R, self.N, 3), dtype=torch.float32, device=dev)
        self.dq, self.ds = _small(self.dsmall, N.COL_DQ, 4, self.B), _small(self.dsmall, N.COL_DS, 1, self.B)
        self.dt, self.df = _small(self.dsmall, N.COL_DT, 3, self.B), _small(self.dsmall, N.COL_DF, 1, self.B)
        self._kxy, self._kz = geom.kern_ptrs()
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        self._fixed = (vp(self.cells), vp(self.grid_wh), vp(self.mask), vp(self.proj), vp(self.trans), vp(self.sse),
                       vp(self.sse_tiles), vp(self.loss), vp(self.winner), vp(self.ws), vp(self.fwd_dsmall))
        self._tail = (vp(self.dpc), vp(self.dsmall))
        self._fn = L.dpc_project_loss_step
        self._pref = ctypes.byref(self.P)

    @staticmethod
    def _arg(t, shape, name):
        if t is None:
            return None
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape or not t.is_cuda:
            raise ValueError("%s must be a contiguous float32 device tensor of shape %s, got %s %s"
                             % (name, shape, t.dtype, tuple(t.shape)))
        return ctypes.c_void_p(t.data_ptr())

    def bind(self, pc, q, s, gt, t=None, f=None, dloss=None, valid_samples=None):
        """Fix the input tensors (static buffers that are refilled in place): run() without arguments then skips the
        per-call checks and pointer conversions.  gt: [B/K,H,W,1] pooled masks, or the masks [B/K,1,f*H,f*W] /
        [B/K,f*H,f*W,1] themselves (the pooling factor f is fixed here); valid_samples: [B/K] weights | None."""
        B, g, S = self.B, self.geom, self.B // self.K
        gf = 1
        if gt is not None and gt.numel() != S * g.H * g.W:
            gf = mask_factor(gt, S, g.H, g.W)
            gptr = self._arg(gt, tuple(gt.shape), "gt")
        else:
            gptr = self._arg(gt, (S, g.H, g.W, 1), "gt")
        self._bound = (self._pref, self._arg(pc, (B // self.R, self.N, 3), "pc"), self._arg(q, (B, 4), "q"),
                       self._arg(t, (B, 3), "t"), self._arg(f, (B, 1), "f"), self._arg(s, (B, 1), "s"), self._kxy, self._kz,
                       gptr, gf, self._arg(valid_samples, (S,), "valid_samples"), self.K) + self._fixed \
            + (None if dloss is None else ctypes.c_void_p(dloss.data_ptr()),) + self._tail
        self.gt_factor = gf
        self._keep = (pc, q, s, gt, t, f, dloss, valid_samples)
        return self

    def run(self, pc=None, q=None, s=None, gt=None, t=None, f=None, dloss=None, valid_samples=None):
        """Enqueue forward + backward on torch's current stream; returns the loss tensor (static, no sync)."""
        if pc is not None:
            self.bind(pc, q, s, gt, t, f, dloss, valid_samples)
        if self.R > 1:
            self.dpc.zero_()    # the replicas ADD into the shared gradient (include/dpc_render.h, point_replicas)
        rc = self._fn(*self._bound, ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))
        if rc != 0:
            N.check(rc, "dpc_project_loss_step")
        return self.loss


# ------------------------------------------------------------------------------------------------------
# Stage-level functions (one per reference function)
# ------------------------------------------------------------------------------------------------------
class Transform(torch.autograd.Function):
    """pc_perspective_transform, quaternion branch."""

    @staticmethod
    def forward(ctx, pc, q, t, f, geom):
        dev = N.require_device(pc, q, t, f)
        pc32, q32, t32, f32 = _f32(pc), _f32(q), _f32(t), _f32(f)
        P = geom.params(pc32.shape[0], pc32.shape[1])
        out = torch.empty_like(pc32)
        N.call(dev, "dpc_transform_fwd", ctypes.byref(P), N.ptr(pc32), N.ptr(q32), N.ptr(t32), N.ptr(f32), N.ptr(out))
        ctx.geom, ctx.inputs, ctx.saved = geom, tuple(_meta(x) for x in (pc, q, t, f)), (pc32, q32, t32, f32)
        return out

    @staticmethod
    def backward(ctx, dout):
        pc32, q32, t32, f32 = ctx.saved
        dev = pc32.device
        P = ctx.geom.params(pc32.shape[0], pc32.shape[1])
        dout32 = dout.detach().to(torch.float32).contiguous()
        dpc = torch.empty_like(pc32)
        dsmall = torch.empty((N.DPC_SMALL_COLS * pc32.shape[0],), dtype=torch.float32, device=dev)
        N.call(dev, "dpc_transform_bwd", ctypes.byref(P), N.ptr(pc32), N.ptr(q32), N.ptr(t32), N.ptr(f32),
               N.ptr(dout32), N.ptr(dpc), N.ptr(dsmall))
        return _pose_grads(ctx.inputs, (True, True), dpc, dsmall, pc32.shape[0], 1)


class Splat(torch.autograd.Function):
    """pointcloud2voxels3d_fast: tr [B,N,3] (z,y,x) -> voxels [B,D,H,W]."""

    @staticmethod
    def forward(ctx, tr, geom):
        dev = N.require_device(tr)
        is64 = tr.dtype == torch.float64  # the reference's direct callers pass fp64 coordinates; keep them
        trc = tr.detach().contiguous() if is64 else _f32(tr)
        P = geom.params(trc.shape[0], trc.shape[1])
        vox = torch.empty((trc.shape[0], geom.D, geom.H, geom.W), dtype=torch.float32, device=dev)
        cells = _new_cells(P, dev)
        N.call(dev, "dpc_splat_fwd", ctypes.byref(P), N.ptr(trc), int(is64), N.ptr(cells), N.ptr(vox))
        ctx.geom, ctx.tr, ctx.trc, ctx.is64 = geom, _meta(tr), trc, is64
        return vox

    @staticmethod
    def backward(ctx, dvox):
        trc = ctx.trc
        dev = trc.device
        P = ctx.geom.params(trc.shape[0], trc.shape[1])
        dvox32 = dvox.detach().to(torch.float32).contiguous()
        dtr = torch.empty(trc.shape, dtype=torch.float32, device=dev)
        N.call(dev, "dpc_splat_bwd", ctypes.byref(P), N.ptr(trc), int(ctx.is64), N.ptr(dvox32), N.ptr(dtr))
        return _like_input(dtr, ctx.tr), None


def _smooth_call(x32, geom, transpose):
    """geom.kxy None: the D pass alone."""
    dev = x32.device
    B = x32.shape[0]
    P = geom.params(B, 0)
    out, tmp = torch.empty_like(x32), torch.empty_like(x32)
    kxy, kz = geom.kern_ptrs()
    N.call(dev, "dpc_smooth", ctypes.byref(P), kxy, kz, int(transpose), N.ptr(x32), N.ptr(out), N.ptr(tmp))
    return out


class Smooth(torch.autograd.Function):
    """smoothen_voxels3d on a [B,D,H,W] (or [B,1,D,H,W]) grid; the backward is the adjoint correlation."""

    @staticmethod
    def forward(ctx, vox, geom):
        N.require_device(vox)
        ctx.geom, ctx.vox = geom, _meta(vox)
        return _smooth_call(_f32(vox).reshape(-1, geom.D, geom.H, geom.W), geom, False).reshape(vox.shape)

    @staticmethod
    def backward(ctx, dout):
        geom = ctx.geom
        d32 = dout.detach().to(torch.float32).contiguous().reshape(-1, geom.D, geom.H, geom.W)
        return _like_input(_smooth_call(d32, geom, True), ctx.vox), None


class Drc(torch.autograd.Function):
    """drc_projection + drc_depth_projection: vox [B,D,H,W] -> proj [B,H,W], probs [D+1,B,H,W], depth [B,H,W]
    (no flips; the caller applies the reference's flips)."""

    @staticmethod
    def forward(ctx, vox, geom):
        dev = N.require_device(vox)
        vox32 = _f32(vox)
        B = vox32.shape[0]
        P = geom.params(B, 0)
        proj = torch.empty((B, geom.H, geom.W), dtype=torch.float32, device=dev)
        probs = torch.empty((geom.D + 1, B, geom.H, geom.W), dtype=torch.float32, device=dev)
        depth = torch.empty((B, geom.H, geom.W), dtype=torch.float32, device=dev)
        N.call(dev, "dpc_drc_fwd", ctypes.byref(P), N.ptr(vox32), N.ptr(proj), N.ptr(probs), N.ptr(depth))
        ctx.geom, ctx.vox, ctx.vox32 = geom, _meta(vox), vox32
        ctx.set_materialize_grads(False)  # unused outputs arrive as None, not as zero-filled [D+1,B,H,W] tensors
        return proj, probs, depth

    @staticmethod
    def backward(ctx, dproj, dprobs, ddepth):
        vox32 = ctx.vox32
        dev = vox32.device
        P = ctx.geom.params(vox32.shape[0], 0)
        c = lambda g: None if g is None else g.detach().to(torch.float32).contiguous()
        dproj, dprobs, ddepth = c(dproj), c(dprobs), c(ddepth)
        dvox = torch.empty_like(vox32)
        N.call(dev, "dpc_drc_bwd", ctypes.byref(P), N.ptr(vox32), N.ptr(dproj), N.ptr(dprobs), N.ptr(ddepth), N.ptr(dvox))
        return _like_input(dvox, ctx.vox), None


class GaussVoxels(torch.autograd.Function):
    """pointcloud2voxels of the TF-1 original (dpc/util/point_cloud.py:17-57), the exact Gaussian occupancy: tr [B,N,3]
    (z,y,x) -> voxels [B,G,G,G] with axes following components 0, 1, 2.  sigma is a launch argument (a Python float);
    normalise one of N.DPC_GAUSS_NORM_*.  The sums before the clip are kept for the backward's pass-through set."""

    @staticmethod
    def forward(ctx, tr, G, sigma, normalise):
        dev = N.require_device(tr)
        tr32 = _f32(tr)
        if tr32.dim() != 3 or tr32.shape[2] != 3:
            raise ValueError("transformed points must be [B,N,3], got %s" % (tuple(tr.shape),))
        B, Npts = tr32.shape[0], tr32.shape[1]
        geom = Geometry(G, G, G)
        P = geom.params(B, Npts)
        vox = torch.empty((B, G, G, G), dtype=torch.float32, device=dev)
        raw = torch.empty_like(vox) if ctx.needs_input_grad[0] else None
        N.call(dev, "dpc_gauss_voxels_fwd", ctypes.byref(P), N.ptr(tr32), float(sigma), int(normalise), N.ptr(raw), N.ptr(vox))
        ctx.geom, ctx.tr, ctx.tr32, ctx.raw, ctx.sigma, ctx.normalise = geom, _meta(tr), tr32, raw, float(sigma), int(normalise)
        return vox

    @staticmethod
    def backward(ctx, dvox):
        tr32 = ctx.tr32
        dev = tr32.device
        P = ctx.geom.params(tr32.shape[0], tr32.shape[1])
        dvox32 = dvox.detach().to(torch.float32).contiguous()
        dtr = torch.empty(tr32.shape, dtype=torch.float32, device=dev)
        N.call(dev, "dpc_gauss_voxels_bwd", ctypes.byref(P), N.ptr(tr32), ctx.sigma, ctx.normalise, N.ptr(ctx.raw), N.ptr(dvox32),
               N.ptr(dtr))
        return _like_input(dtr, ctx.tr), None, None, None


class SilhouetteLoss(torch.autograd.Function):
    """add_proj_loss / proj_loss_pose_candidates fused with its gradient (one launch, gradient precomputed in
    the forward; backward scales it by the incoming scalar).  gt: pooled masks (as many values per sample as pred has per
    silhouette) or the masks at f times pred's [H,W] (pooled f x f in the kernel); weights [S] | None."""

    @staticmethod
    def forward(ctx, pred, gt, num_candidates, weights=None):
        S = gt.shape[0]
        K = int(num_candidates)
        if pred.shape[0] != S * K:
            raise ValueError("pred has %d silhouettes, expected %d samples x %d candidates" % (pred.shape[0], S, K))
        n_pix = pred[0].numel() if S else 1
        H, W, gf = 1, n_pix, 1     # f = 1: any layout of n_pix values per sample, read as they are
        if S and gt[0].numel() != n_pix:
            plane = _plane(tuple(pred.shape))
            if plane is None or plane[0] * plane[1] != n_pix:
                raise ValueError("gt and pred silhouettes differ in size: %s vs %s" % (tuple(gt.shape), tuple(pred.shape)))
            H, W = plane
            gf = mask_factor(gt, S, H, W)
        if weights is not None and tuple(weights.shape) != (S,):
            raise ValueError("valid_samples must be [%d] (one weight per sample), got %s" % (S, tuple(weights.shape)))
        dev = N.require_device(pred, gt, weights)
        p32, g32 = _f32(pred), _f32(gt)
        w32 = _weights32(weights, S)
        part = torch.empty((S,), dtype=torch.float32, device=dev)
        winner = torch.empty((S,), dtype=torch.int32, device=dev)
        dpred = torch.empty_like(p32)
        N.call(dev, "dpc_silhouette_loss", N.ptr(g32), gf, N.ptr(w32), N.ptr(p32), S, K, H, W, N.ptr(part), N.ptr(winner),
               N.ptr(dpred))
        ctx.dpred, ctx.meta = dpred, _meta(pred)
        ctx.mark_non_differentiable(winner)
        return part.sum(), winner

    @staticmethod
    def backward(ctx, dloss, _dwinner):
        return _like_input(ctx.dpred * dloss, ctx.meta), None, None, None


# ------------------------------------------------------------------------------------------------------
# Expected depth and its loss from grid_wh (csrc/dpc_depth.hip)      reference: dpc/util/losses.py:113-136
# ------------------------------------------------------------------------------------------------------
_depth_ws = {}   # (device, stream, bytes) -> workspace whose tickets are zero between launches


def _depth_workspace(dev, nbytes):
    """Workspace of dpc_depth_loss_bwd.  Its first bytes are the tickets of the in-launch ds reduction: zero on entry, left
    zero by the kernel -- so the buffer is zeroed ONCE, when it is made, and kept per device and stream (launches of one
    stream run one after the other; another stream gets a buffer of its own).  While a HIP graph is being captured the buffer
    is not kept: it comes from the graph's pool and its zero fill is part of the graph."""
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), N.stream(dev), nbytes)
    ws = _depth_ws.get(key)
    if ws is None:
        if len(_depth_ws) >= 16:
            _depth_ws.clear()
        ws = _depth_ws[key] = torch.zeros((nbytes,), dtype=torch.uint8, device=dev)
    return ws


def _loss_targets(x32, gt, weights, f, geom, what, rgb=False):
    """Ground truth [S,f*H,f*W] ([.., 3] values per sample when rgb) and weights [S] | None of a loss on the B = S clouds of
    x32, as fp32: (gt32, w32)."""
    N.require_device(x32, gt, weights)
    B, gt32 = x32.shape[0], _f32(gt)
    if gt32.numel() != B * f * geom.H * f * geom.W * (3 if rgb else 1):
        raise ValueError("%s must hold %d x %d x %d%s values, got %s"
                         % (what, B, f * geom.H, f * geom.W, " x 3" if rgb else "", tuple(gt.shape)))
    return gt32, _weights32(weights, B)


def _loss_buffers(B, geom, dev):
    """(per-tile partial sums [B, ray tiles], scalar loss) of a column kernel and its one-block finalize."""
    return (torch.empty((B, (geom.H * geom.W + 255) // 256), dtype=torch.float32, device=dev),
            torch.empty((), dtype=torch.float32, device=dev))


def _column_backward(ctx, entry, ws_entry, extra, *grads):
    """One launch: d grid_wh (overwritten) and d s from the gradients arriving at the node's outputs (`grads`, None = absent).
    `extra`: the entry's scalars between gt_factor and the weights; `ws_entry` sizes its workspace."""
    grid_wh, s32, gt32, w32 = ctx.saved
    geom, dev, B = ctx.geom, grid_wh.device, grid_wh.shape[0]
    Z = geom.sized(B, 0)
    dgrid = torch.empty_like(grid_wh)
    ds = None if s32 is None else torch.empty((B,), dtype=torch.float32, device=dev)
    with N.on(dev):
        ws = _depth_workspace(dev, max(getattr(N.lib(), ws_entry)(Z.ref), 16))
    N.call(dev, entry, Z.ref, N.ptr(grid_wh), N.ptr(s32), geom.kern_ptrs()[1], N.ptr(gt32), ctx.gt_factor, *extra, N.ptr(w32),
          *[N.ptr(_f32(g)) for g in grads], N.ptr(dgrid), N.ptr(ds), N.ptr(ws))
    return _like_input(dgrid, ctx.metas[0]), _like_input(ds, ctx.metas[1])


def _depth_backward(ctx, dloss, ddepth):
    return _column_backward(ctx, "dpc_depth_loss_bwd", "dpc_depth_workspace_bytes", (ctx.max_dataset_depth,), dloss, ddepth)


def _depth_inputs(grid_wh, s, geom):
    dev = N.require_device(grid_wh, s)
    g32, s32 = _f32(grid_wh), _f32(s)
    if tuple(g32.shape[1:]) != (geom.D, geom.H, geom.W):
        raise ValueError("grid_wh must be [B,%d,%d,%d], got %s" % (geom.D, geom.H, geom.W, tuple(g32.shape)))
    if s32 is not None and s32.numel() != g32.shape[0]:
        raise ValueError("scaling_factor must hold one value per cloud (%d), got %s" % (g32.shape[0], tuple(s32.shape)))
    return dev, g32, s32


class DepthMap(torch.autograd.Function):
    """drc_depth_projection of the fused path: grid_wh [B,D,H,W] (ProjectFused's second output), s [B,1] | None ->
    expected depth [B,H,W,1], rows flipped like proj.  One launch forward, one backward."""

    @staticmethod
    def forward(ctx, grid_wh, s, geom):
        dev, g32, s32 = _depth_inputs(grid_wh, s, geom)
        B = g32.shape[0]
        depth = torch.empty((B, geom.H, geom.W, 1), dtype=torch.float32, device=dev)
        N.call(dev, "dpc_depth_loss_fwd", geom.sized(B, 0).ref, N.ptr(g32), N.ptr(s32), geom.kern_ptrs()[1], None, 1, 0.0, None,
              N.ptr(depth), None, None)
        ctx.geom, ctx.saved, ctx.metas = geom, (g32, s32, None, None), (_meta(grid_wh), _meta(s))
        ctx.gt_factor, ctx.max_dataset_depth = 1, 0.0
        return depth

    @staticmethod
    def backward(ctx, ddepth):
        return _depth_backward(ctx, None, ddepth) + (None,)


class DepthLoss(torch.autograd.Function):
    """add_proj_depth_loss on the fused path: grid_wh [B,D,H,W], s [B,1] | None, gt [S,f*H,f*W] depth maps (S = B),
    weights [S] | None -> (1/2) sum_s w_s^2 sum (g - depth)^2 / S with g the f-fold nearest-neighbour subsample of gt and
    max_dataset_depth replaced by max_depth.  Two launches forward (column kernel, one-block finalize), one backward."""

    @staticmethod
    def forward(ctx, grid_wh, s, gt, gt_factor, max_dataset_depth, weights, geom, want_depth=False):
        """Returns (loss, depth): depth [B,H,W,1] written by the same launch when want_depth (detached: differentiate
        DepthMap for a gradient through the map itself), else None."""
        dev, g32, s32 = _depth_inputs(grid_wh, s, geom)
        B, f = g32.shape[0], int(gt_factor)
        gt32, w32 = _loss_targets(g32, gt, weights, f, geom, "depths")
        tiles, loss = _loss_buffers(B, geom, dev)
        depth = torch.empty((B, geom.H, geom.W, 1), dtype=torch.float32, device=dev) if want_depth else None
        N.call(dev, "dpc_depth_loss_fwd", geom.sized(B, 0).ref, N.ptr(g32), N.ptr(s32), geom.kern_ptrs()[1], N.ptr(gt32), f,
              float(max_dataset_depth), N.ptr(w32), N.ptr(depth), N.ptr(tiles), N.ptr(loss))
        ctx.geom, ctx.saved, ctx.metas = geom, (g32, s32, gt32, w32), (_meta(grid_wh), _meta(s))
        ctx.gt_factor, ctx.max_dataset_depth = f, float(max_dataset_depth)
        if depth is not None:
            ctx.mark_non_differentiable(depth)
        return loss, depth

    @staticmethod
    def backward(ctx, dloss, _ddepth):
        return _depth_backward(ctx, dloss, None) + (None,) * 6


# ------------------------------------------------------------------------------------------------------
# Colour: splat (csrc/dpc_rgb_splat.hip), projection and loss (csrc/dpc_rgb.hip)
# reference (TF-1 originals): dpc/util/point_cloud.py:98-134, 244-262, 275-277; dpc/util/drc.py:132-142; dpc/util/losses.py:69-90
# ------------------------------------------------------------------------------------------------------
def _splat_forward(ctx, entry, tr, rgb, Z, geom, stop, n_set=(), ws=()):
    """Forward of a colour splat, the grid [B,3,D,H,W]; n_set / ws: the fixed-point entry's own arguments, as tuples."""
    tr32, rgb32 = _f32(tr), _f32(rgb)
    out = torch.empty((tr32.shape[0], 3, geom.D, geom.H, geom.W), dtype=torch.float32, device=tr32.device)
    N.call(tr32.device, entry, Z.ref, N.ptr(tr32), N.ptr(rgb32), *n_set, N.ptr(out), *ws)
    ctx.Z, ctx.saved, ctx.metas, ctx.stop = Z, (tr32, rgb32), (_meta(tr), _meta(rgb)), bool(stop)
    return out


def _splat_backward(ctx, entry, dC, n_set=(), ws=()):
    """Backward of a colour splat: (d tr | None, d rgb) in the inputs' dtypes and shapes."""
    tr32, rgb32 = ctx.saved
    dC32 = _f32(dC)
    drgb = torch.empty_like(rgb32)
    dtr = torch.empty_like(tr32) if (ctx.needs_input_grad[0] and not ctx.stop) else None
    N.call(tr32.device, entry, ctx.Z.ref, N.ptr(tr32), N.ptr(rgb32), *n_set, N.ptr(dC32), N.ptr(drgb), N.ptr(dtr), *ws)
    return _like_input(dtr, ctx.metas[0]), _like_input(drgb, ctx.metas[1])


class RgbSplat(torch.autograd.Function):
    """The rgb half of pointcloud2voxels3d_fast: tr [B,N,3] (z,y,x), rgb [B,N,3] -> colour grid [B,3,D,H,W] (planar), the
    points' trilinear weights times their colours, in the cells of the occupancy splat.  fp32 atomics: the grid is not
    bit-reproducible from run to run.  stop_points_gradient (pc_rgb_stop_points_gradient): no gradient to tr."""

    @staticmethod
    def forward(ctx, tr, rgb, geom, stop_points_gradient=False):
        N.require_device(tr, rgb)
        if tr.dim() != 3 or tr.shape[2] != 3 or tuple(rgb.shape) != tuple(tr.shape):
            raise ValueError("rgb must hold one colour per point, [B,N,3] like the points %s, got %s"
                             % (tuple(tr.shape), tuple(rgb.shape)))
        return _splat_forward(ctx, "dpc_rgb_splat_fwd", tr, rgb, geom.sized(tr.shape[0], tr.shape[1]), geom, stop_points_gradient)

    @staticmethod
    def backward(ctx, dC):
        return _splat_backward(ctx, "dpc_rgb_splat_bwd", dC) + (None, None)


def colour_sets(tr_shape, rgb_shape, point_index=None):
    """Layout check of colours that are read through the shared-set convention (RgbSplatFixed): tr [B,n,3], colours
    [B/R,N,3], point_index [B,n] | None (then N == n).  Returns R.  Host only: shapes in, ValueError out."""
    tr_shape, rgb_shape = tuple(tr_shape), tuple(rgb_shape)
    if len(tr_shape) != 3 or tr_shape[2] != 3:
        raise ValueError("the transformed points must be [B,n,3], got %s" % (tr_shape,))
    B, n = tr_shape[0], tr_shape[1]
    if point_index is not None and tuple(point_index.shape) != (B, n):
        raise ValueError("point_index must be [%d, %d] (one colour index per projected point), got %s"
                         % (B, n, tuple(point_index.shape)))
    sets = len(rgb_shape) == 3 and rgb_shape[2] == 3 and (rgb_shape[0] == B or (rgb_shape[0] > 0 and B % rgb_shape[0] == 0))
    if sets and point_index is None:
        sets = rgb_shape[1] == n
    elif sets:
        sets = rgb_shape[1] >= 1 or B == 0
    if not sets:
        raise ValueError("all_rgb must hold one colour per projected point, %s, or colour sets [B/R,N,3] shared by R consecutive "
                         "clouds each (N = %d, or any N >= 1 with a point_index [%d,%d]), got %s"
                         % (tr_shape, n, B, n, rgb_shape))
    return 1 if rgb_shape[0] == B else B // rgb_shape[0]


class RgbSplatFixed(torch.autograd.Function):
    """RgbSplat with a bit-reproducible sum, reading shared colour sets in place: tr [B,n,3] (z,y,x), rgb [B/R,N,3] ->
    colour grid [B,3,D,H,W] (planar).  The colour of point i of cloud b is rgb[b // R][point_index[b, i]] (point_index
    [B,n] | None: N == n and the index is i) -- what replicate_rgb would materialise.  Every contribution is k_rgb_splat's
    fp32 product, rounded once to 64-bit fixed point (2^-40) and added as an integer: the grid is the same bits on every
    run and for every order of the points.  Colours must satisfy |c| <= 8; a larger, NaN or infinite colour makes every voxel
    of its cloud NaN (other clouds are untouched).  Backward: d(tr) per cloud (none under stop_points_gradient), d(rgb) in
    the sets' own layout, summed in fixed point where clouds share a set; a contribution with no fixed-point value (NaN,
    Inf, magnitude >= 2^20) makes that set's gradient NaN.  Workspaces come from torch's allocator."""

    @staticmethod
    def forward(ctx, tr, rgb, geom, stop_points_gradient=False, point_index=None):
        reps = colour_sets(tr.shape, rgb.shape, point_index)
        dev = N.require_device(tr, rgb, point_index)
        ctx.idx = idx = None if point_index is None else point_index.detach().to(torch.int32).contiguous()   # Z points at it
        ctx.shared, n_set = reps > 1 or idx is not None, rgb.shape[1]
        Z = geom.sized(tr.shape[0], tr.shape[1], reps, idx, n_set if idx is not None else 0)
        ws = torch.empty((max(N.lib().dpc_rgb_splat_fixed_workspace_bytes(Z.ref, n_set), 16),), dtype=torch.uint8, device=dev)
        return _splat_forward(ctx, "dpc_rgb_splat_fixed_fwd", tr, rgb, Z, geom, stop_points_gradient, (n_set,), (N.ptr(ws),))

    @staticmethod
    def backward(ctx, dC):
        sets, n_set = ctx.saved[1].shape[:2]
        ws = None
        if ctx.shared:   # the sets' 64-bit sums and poison words (include/dpc_render.h)
            ws = torch.empty(((24 * sets * n_set + 4 * sets + 255) // 256 * 256 + 16,), dtype=torch.uint8, device=dC.device)
        return _splat_backward(ctx, "dpc_rgb_splat_fixed_bwd", dC, (n_set,), (N.ptr(ws),)) + (None,) * 3


def _rgb_inputs(vox, C, div, geom):
    dev = N.require_device(vox, C, div)
    v32, c32, d32 = _f32(vox), _f32(C), _f32(div)
    B = v32.shape[0]
    if tuple(v32.shape) != (B, geom.D, geom.H, geom.W):
        raise ValueError("voxels must be [B,%d,%d,%d], got %s" % (geom.D, geom.H, geom.W, tuple(vox.shape)))
    if tuple(c32.shape) != (B, 3, geom.D, geom.H, geom.W):
        raise ValueError("the colour grid must be [%d,3,%d,%d,%d], got %s" % (B, geom.D, geom.H, geom.W, tuple(C.shape)))
    if d32 is not None and tuple(d32.shape) != tuple(v32.shape):
        raise ValueError("the occupancies to divide by must be %s, got %s" % (tuple(v32.shape), tuple(div.shape)))
    return dev, v32, c32, d32


def _rgb_options(ctx, div_eps, clip_after, gt_factor, gt_planar):
    """The colour entries' scalars as the bindings take them, kept on ctx for the backward: (div_eps, clip_after)."""
    ctx.div_eps, ctx.clip_after = float(div_eps), int(bool(clip_after))
    ctx.gt_factor, ctx.gt_planar = int(gt_factor), int(bool(gt_planar))
    return ctx.div_eps, ctx.clip_after


def _rgb_loss_forward(ctx, entry, with_proj, vox, C, div, gt, gt_factor, gt_planar, weights, geom, div_eps, clip_after):
    """Forward of a loss on the renderer's grids against images (column kernel, one-block finalize): (loss, proj_rgb [B,H,W,3] |
    None), proj_rgb where the entry writes one (with_proj)."""
    dev, v32, c32, d32 = _rgb_inputs(vox, C, div, geom)
    B = v32.shape[0]
    eps, clip = _rgb_options(ctx, div_eps, clip_after, gt_factor, gt_planar)
    gt32, w32 = _loss_targets(v32, gt, weights, ctx.gt_factor, geom, "images", rgb=True)
    if B == 0:   # an empty shard: nothing to launch (empty tensors have no address to hand over), the loss of nothing is 0
        ctx.empty, ctx.dev, ctx.saved, ctx.metas = True, dev, (None,) * 6, (_meta(vox), _meta(C))
        return (torch.zeros((), dtype=torch.float32, device=dev),
                torch.zeros((0, geom.H, geom.W, 3), dtype=torch.float32, device=dev) if with_proj else None)
    ctx.empty = False
    tiles, loss = _loss_buffers(B, geom, dev)
    proj = torch.empty((B, geom.H, geom.W, 3), dtype=torch.float32, device=dev) if with_proj else None
    N.call(dev, entry, geom.sized(B, 0).ref, N.ptr(v32), N.ptr(c32), N.ptr(d32), eps, clip, N.ptr(gt32), ctx.gt_factor, ctx.gt_planar,
          N.ptr(w32), *([N.ptr(proj)] if with_proj else []), N.ptr(tiles), N.ptr(loss))
    ctx.geom, ctx.saved, ctx.metas = geom, (v32, c32, d32, gt32, w32, proj), (_meta(vox), _meta(C))
    return loss, proj


def _rgb_backward(ctx, entry, *grads):
    """One launch: d voxels and d colour grid (both overwritten).  `grads`: what the entry takes between the weights and the
    outputs -- the saved image where it needs one, the gradients arriving at the node's outputs (None = absent)."""
    if getattr(ctx, "empty", False):
        return _zero_grads(ctx.metas, ctx.dev)
    v32, c32, d32, gt32, w32, _ = ctx.saved
    geom, dev = ctx.geom, v32.device
    dvox, dC = torch.empty_like(v32), torch.empty_like(c32)
    N.call(dev, entry, geom.sized(v32.shape[0], 0).ref, N.ptr(v32), N.ptr(c32), N.ptr(d32), ctx.div_eps, ctx.clip_after, N.ptr(gt32),
          ctx.gt_factor, ctx.gt_planar, N.ptr(w32), *[N.ptr(_f32(g)) for g in grads], N.ptr(dvox), N.ptr(dC))
    return _like_input(dvox, ctx.metas[0]), _like_input(dC, ctx.metas[1])


class RgbMap(torch.autograd.Function):
    """project_volume_rgb_integral on the renderer's grids: voxels [B,D,H,W], colour grid [B,3,D,H,W] (after the
    Gaussian), div [B,D,H,W] | None (smoothed raw occupancies to divide by, a constant) -> proj_rgb [B,H,W,3], rows flipped
    like proj, white background.  One launch forward, one backward."""

    @staticmethod
    def forward(ctx, vox, C, div, geom, div_eps=0.01, clip_after=False):
        dev, v32, c32, d32 = _rgb_inputs(vox, C, div, geom)
        B = v32.shape[0]
        eps, clip = _rgb_options(ctx, div_eps, clip_after, 1, 0)
        proj = torch.empty((B, geom.H, geom.W, 3), dtype=torch.float32, device=dev)
        N.call(dev, "dpc_rgb_loss_fwd", geom.sized(B, 0).ref, N.ptr(v32), N.ptr(c32), N.ptr(d32), eps, clip, None, 1, 0, None, N.ptr(proj),
              None, None)
        ctx.geom, ctx.saved, ctx.metas = geom, (v32, c32, d32, None, None, None), (_meta(vox), _meta(C))
        return proj

    @staticmethod
    def backward(ctx, dproj):
        return _rgb_backward(ctx, "dpc_rgb_loss_bwd", None, None, dproj) + (None,) * 4


class RgbLoss(torch.autograd.Function):
    """add_proj_rgb_loss on the renderer's grids: (1/2) sum_s w_s^2 sum (g - proj_rgb)^2 / S with g the images sampled at
    (f*y, f*x).  gt [S,f*H,f*W,3], or [S,3,f*H,f*W] when gt_planar; weights [S] | None.  Returns (loss, proj_rgb [B,H,W,3]
    detached: differentiate RgbMap for a gradient through the image itself).  Two launches forward (column kernel,
    one-block finalize), one backward."""

    @staticmethod
    def forward(ctx, vox, C, div, gt, gt_factor, gt_planar, weights, geom, div_eps=0.01, clip_after=False):
        loss, proj = _rgb_loss_forward(ctx, "dpc_rgb_loss_fwd", True, vox, C, div, gt, gt_factor, gt_planar, weights, geom,
                                       div_eps, clip_after)
        ctx.mark_non_differentiable(proj)
        return loss, proj

    @staticmethod
    def backward(ctx, dloss, _dproj):
        return _rgb_backward(ctx, "dpc_rgb_loss_bwd", ctx.saved[5], dloss, None) + (None,) * 8


# ------------------------------------------------------------------------------------------------------
# Ray-consistency (DRC) mask and colour losses (csrc/dpc_drc_loss.hip)
# reference (TF-1 originals): dpc/util/losses.py:23-66, 93-110 on dpc/util/drc.py:48-106
# ------------------------------------------------------------------------------------------------------
class DrcLoss(torch.autograd.Function):
    """add_drc_loss on the fused path: grid_wh [B,D,H,W], s [B,1] | None, gt [S,f*H,f*W] masks (S = B), weights [S] | None ->
    sum_s w_s^2 sum_rays ((1 - g) sum_{k<D} p_k + g p_D) / S with g the mask at (f*row, f*col).  Two launches forward (column
    kernel, one-block finalize), one backward; the backward's workspace is the depth loss's (same contract, kept per stream)."""

    @staticmethod
    def forward(ctx, grid_wh, s, gt, gt_factor, weights, geom):
        dev, g32, s32 = _depth_inputs(grid_wh, s, geom)
        B, f = g32.shape[0], int(gt_factor)
        gt32, w32 = _loss_targets(g32, gt, weights, f, geom, "masks")
        tiles, loss = _loss_buffers(B, geom, dev)
        N.call(dev, "dpc_drc_loss_fwd", geom.sized(B, 0).ref, N.ptr(g32), N.ptr(s32), geom.kern_ptrs()[1], N.ptr(gt32), f, N.ptr(w32),
              N.ptr(tiles), N.ptr(loss))
        ctx.geom, ctx.saved, ctx.metas, ctx.gt_factor = geom, (g32, s32, gt32, w32), (_meta(grid_wh), _meta(s)), f
        return loss

    @staticmethod
    def backward(ctx, dloss):
        return _column_backward(ctx, "dpc_drc_loss_bwd", "dpc_drc_workspace_bytes", (), dloss) + (None,) * 4


class DrcRgbLoss(torch.autograd.Function):
    """add_drc_rgb_loss on the renderer's grids: sum_s w_s^2 sum_rays sum_k p_k psi_k / S, psi_k the squared distance of the
    voxel's colour (the background's white) from the image at (f*row, f*col).  Inputs as RgbLoss's.  Two launches forward
    (column kernel, one-block finalize), one backward."""

    @staticmethod
    def forward(ctx, vox, C, div, gt, gt_factor, gt_planar, weights, geom, div_eps=0.01, clip_after=False):
        return _rgb_loss_forward(ctx, "dpc_drc_rgb_loss_fwd", False, vox, C, div, gt, gt_factor, gt_planar, weights, geom,
                                 div_eps, clip_after)[0]

    @staticmethod
    def backward(ctx, dloss):
        return _rgb_backward(ctx, "dpc_drc_rgb_loss_bwd", dloss) + (None,) * 8
