"""Rendering predicted point clouds to shaded images on the GPU, in place of the reference's Blender step.

The reference renders a cloud by writing it to a temporary file and starting one Blender 2.79b process (Cycles, 500
samples) that places a small sphere at every point (dpc/render/render_point_cloud.py, render_point_cloud_blender.py;
render_point_cloud_runner.py does it once per model of a split).  Here the clouds of a whole batch are ray-traced in one
dpc_render_points call (csrc/dpc_raster.hip), in fp64, with the reference's camera and point geometry and a simple shading
of our own; include/dpc_render.h states the semantics and the deliberate deviations.

    camera_frame         obj_centened_camera_pos + the TRACK_TO constraint: host fp64 (C, r, u, f)
    render_point_clouds  a ragged batch of clouds -> [P,S,S,3] images on the device
    render_point_cloud   the reference's render_point_cloud(point_cloud, cfg) -> numpy uint8 [S,S,3]
    render_split         render_point_cloud_runner.py's loop for a list of model names
    write_png            8-bit RGB PNG with zlib and struct only
    write_png_rgba, write_png_gray16, read_png_any   the training views' render_N.png (RGBA8) and depth_N.png (16-bit grey)
"""
import numbers
import struct
import zlib

import numpy as np
import torch

from . import _batch, _native, _split

POINT_SIZE = 0.01      # DEFAULT_SIZE x the unit UV-sphere prototype (render_point_cloud_blender.py:137, :196)
SENSOR_MM = 32.0       # sensor_height (render_point_cloud_blender.py:86)
TRAIN_LENS_MM = 60.0   # like_train_data's lens (render_point_cloud_blender.py:85)
GREY = 0.5             # the prototype material (render_point_cloud_blender.py:95-97)
REST_SCALE = 0.75      # load_data: the points outside every colored subset (render_point_cloud_blender.py:145)


def camera_frame(azimuth, elevation, dist):
    """The camera of setup_camera (render_point_cloud_blender.py:33-60) as host fp64 (C, r, u, f), each a [3] array.

    obj_centened_camera_pos gives (x, y, z) = (d cos az cos el, d sin az cos el, d sin el) with deg / 180 * pi; the camera
    sits at C = (y, x, z).  TRACK_NEGATIVE_Z / UP_Y on the origin: f = -C / |C|, r = normalise(f x e_z), u = r x f.
    ValueError for dist <= 0 or a non-finite argument, and at elevation +-90 deg, where |f x e_z| < 1e-12 leaves no
    frame."""
    az, el, d = float(azimuth), float(elevation), float(dist)
    if not (np.isfinite(az) and np.isfinite(el) and np.isfinite(d)) or d <= 0.0:
        raise ValueError("camera_frame: azimuth %r, elevation %r, dist %r: need finite values and dist > 0"
                         % (azimuth, elevation, dist))
    phi, theta = el / 180 * np.pi, az / 180 * np.pi
    x = d * np.cos(theta) * np.cos(phi)
    y = d * np.sin(theta) * np.cos(phi)
    z = d * np.sin(phi)
    C = np.array([y, x, z], dtype=np.float64)
    nC = np.sqrt((C[0] * C[0] + C[1] * C[1]) + C[2] * C[2])
    f = -C / nC
    fz = np.array([f[1], -f[0], 0.0])  # f x e_z
    n = np.sqrt((fz[0] * fz[0] + fz[1] * fz[1]) + fz[2] * fz[2])
    if n < 1e-12:
        raise ValueError("camera_frame: elevation %r deg looks straight down or up: TRACK_TO has no frame there" % elevation)
    r = fz / n
    u = np.array([r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0]])
    return C, r, u, f


def _per_cloud(value, P, what):
    """A scalar or one value per cloud -> a list of P floats."""
    if isinstance(value, (numbers.Real, np.floating, np.integer)) or (np.ndim(value) == 0):
        return [float(value)] * P
    vals = [float(v) for v in np.asarray(value, dtype=np.float64).reshape(-1)]
    if len(vals) != P:
        raise ValueError("render_point_clouds: %s has %d values for %d clouds" % (what, len(vals), P))
    return vals


def _extra(values, clouds, P, width, what):
    """Optional per-point values (a list of None or [n] / [n,3] arrays per cloud) -> list of host/device tensors or None."""
    if values is None:
        return None
    if len(values) != P:
        raise ValueError("render_point_clouds: %s has %d entries for %d clouds" % (what, len(values), P))
    out = []
    for i, (v, c) in enumerate(zip(values, clouds)):
        if v is None:
            out.append(None)
            continue
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
        t = t.detach()
        shape = (len(c), 3) if width == 3 else (len(c),)
        if tuple(t.shape) != shape:
            raise ValueError("render_point_clouds: cloud %d: %s must be %s, got %s" % (i, what, shape, tuple(t.shape)))
        out.append(t)
    return out


def _packed_extra(values, clouds, dev, dtype, fill):
    """The per-cloud values (None: `fill` for every point) packed in cloud order on dev."""
    parts = [torch.from_numpy(np.broadcast_to(fill, (len(c),) + fill.shape).copy()) if v is None else v.cpu()
             for v, c in zip(values, clouds)]
    return torch.cat([x.to(dtype) for x in parts]).to(dev).contiguous()


def render_point_clouds(clouds, azimuth=140.0, elevation=15.0, dist=2.0, image_size=256, supersample=3, point_size=POINT_SIZE,
                        lens_mm=TRAIN_LENS_MM, colors=None, radii=None, dtype=torch.uint8, return_ids=False):
    """Render P prediction-frame clouds ([n_i,3] float32 / float64 tensors or arrays; n_i may be 0) in one call.

    azimuth, elevation (degrees) and dist are scalars or one value per cloud (vis_azimuth, vis_elevation, vis_dist);
    image_size S (render_image_size), supersample ss (ss x ss samples per pixel), point_size the sphere radius, lens_mm
    the focal length on a 32 mm sensor (60: like_train_data).  colors: None, or per cloud None or [n,3] albedos (float32);
    radii: None, or per cloud None or [n] radii (float64).  Returns [P,S,S,3] on the device: uint8 (dtype=torch.uint8,
    floor(255 clip(v, 0, 1) + 0.5) of the float32 image) or the float32 image (dtype=torch.float32); with return_ids also
    the [P,S ss,S ss] int32 index of the point each sample shows (-1: background).  ValueError naming the cloud for a
    non-finite coordinate, colour or radius; ValueError before anything touches a device for bad arguments."""
    if dtype not in (torch.uint8, torch.float32):
        raise ValueError("render_point_clouds: dtype must be torch.uint8 or torch.float32, got %s" % (dtype,))
    cl = [_batch.cloud(c, "render_point_clouds: cloud %d" % i) for i, c in enumerate(clouds)]
    P = len(cl)
    S, ss = int(image_size), int(supersample)
    az, el, d = (_per_cloud(v, P, w) for v, w in ((azimuth, "azimuth"), (elevation, "elevation"), (dist, "dist")))
    cols = _extra(colors, cl, P, 3, "colors")
    rads = _extra(radii, cl, P, 1, "radii")
    F = float(lens_mm) / SENSOR_MM * S if S > 0 else 1.0
    frames = np.zeros((P, 12), dtype=np.float64)
    for p in range(P):
        try:
            frames[p] = np.concatenate(camera_frame(az[p], el[p], d[p]))
        except ValueError as exc:
            raise ValueError("render_point_clouds: cloud %d: %s" % (p, exc)) from exc
    counts = [len(c) for c in cl]
    starts = np.cumsum([0] + counts)[:-1]
    table = _batch.table(np.stack([starts, counts], axis=1) if P else np.zeros((0, 2)), 2,
                         "render_point_clouds: more than 2^31 - 1 points in one call")
    n = int(sum(counts))
    L = _native.lib()
    host_table = table.ctypes.data
    _batch.dry_run(L.dpc_render_points(None, None, None, n, None, host_table, P, None, S, ss, F, float(point_size), None,
                                       None, None, None),
                   "render_point_clouds: refused by dpc_render_points (%d clouds of %d points, image_size %d, supersample "
                   "%d, focal %r px, point_size %r): need 1 <= image_size <= 4096, 1 <= supersample <= 4, a positive "
                   "focal length and point size" % (P, n, S, ss, F, point_size))
    dev = _batch.device("dpc.render point-cloud rendering", cl)
    scene = None
    if n:
        pts, _ = _batch.pack(cl, dev, torch.float64)
        scene = torch.stack([pts[:, 2], -pts[:, 0], pts[:, 1]], dim=1).contiguous()  # (p2, -p0, p1): exact
    col_t = None if cols is None or n == 0 else _packed_extra(cols, cl, dev, torch.float32, np.full(3, GREY, np.float32))
    rad_t = None if rads is None or n == 0 else _packed_extra(rads, cl, dev, torch.float64, np.float64(point_size))
    image = torch.empty((P, S, S, 3), dtype=torch.float32, device=dev)
    ids = torch.empty((P, S * ss, S * ss), dtype=torch.int32, device=dev) if return_ids else None
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    if P:
        table_d = _batch.on_device(table, dev)
        frames_d = torch.from_numpy(frames).to(dev)
        _native.call(dev, "dpc_render_points", _native.ptr(scene), _native.ptr(col_t), _native.ptr(rad_t), n, _native.ptr(table_d),
                     host_table, P, _native.ptr(frames_d), S, ss, F, float(point_size), _native.ptr(image), _native.ptr(ids),
                     _native.ptr(status))
        _batch.raise_status(int(status.item()), [(_native.DPC_STATUS_NONFINITE, lambda: _nonfinite_message(cl, cols, rads))])
    out = image if dtype == torch.float32 else to_uint8(image)
    return (out, ids) if return_ids else out


def _nonfinite_message(clouds, cols, rads):
    for i, c in enumerate(clouds):
        parts = [c.double()]
        if cols is not None and cols[i] is not None:
            parts.append(cols[i].double().to(c.device))
        if rads is not None and rads[i] is not None:
            r = rads[i].double().to(c.device)
            parts.append(torch.where(r > 0, r, torch.full_like(r, float("nan"))))
        if any(not bool(torch.isfinite(x).all()) for x in parts):
            return "render_point_clouds: cloud %d holds a NaN or infinite coordinate, colour or radius, or a radius <= 0" % i
    return "render_point_clouds: a cloud holds a NaN or infinite coordinate, colour or radius"


def to_uint8(image):
    """floor(255 clip(v, 0, 1) + 0.5) of a float32 image, in fp64 torch ops."""
    v = image.double().clamp(0.0, 1.0)
    return torch.floor(v * 255.0 + 0.5).to(torch.uint8)


def _cfg_get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def render_point_cloud(point_cloud, cfg, supersample=3):
    """The reference's render_point_cloud(point_cloud, cfg) (dpc/render/render_point_cloud.py:19-53): cfg a dict (as the
    notebooks pass it) or an attribute object with vis_azimuth, vis_elevation, vis_dist and render_image_size
    (render_cycles_samples is accepted and ignored: no path tracer here).  The cloud is reshaped to [-1,3] like the
    reference's np.reshape(point_cloud, (1, -1, 3)) and rendered like_train_data (60 mm lens).  Returns numpy uint8
    [S,S,3] (the reference returns Blender's PNG as read by imageio, RGBA)."""
    pc = point_cloud.detach() if isinstance(point_cloud, torch.Tensor) else np.asarray(point_cloud)
    pc = pc.reshape(-1, 3)
    img = render_point_clouds([pc], _cfg_get(cfg, "vis_azimuth"), _cfg_get(cfg, "vis_elevation"), _cfg_get(cfg, "vis_dist"),
                              int(_cfg_get(cfg, "render_image_size")), supersample=supersample, lens_mm=TRAIN_LENS_MM)
    return img[0].cpu().numpy()


def _subset_cloud(model, subsets):
    """load_data's colored subsets (render_point_cloud_blender.py:139-147): the points in no subset, grey at 0.75 x the
    size, then subset i's points in colour i at full size.  Returns (points, colors, radius scale)."""
    idx, colors = subsets
    idx = np.asarray(idx, dtype=bool)
    colors = np.asarray(colors, dtype=np.float32).reshape(-1, 3)
    if idx.ndim != 2 or idx.shape[1] != len(model) or len(colors) < idx.shape[0]:
        raise ValueError("render_split: colored_subsets must be (indices [k,%d] bool, colors [k,3]), got %s and %s"
                         % (len(model), idx.shape, colors.shape))
    rest = np.logical_not(np.any(idx, axis=0))
    pts = [model[rest]] + [model[idx[i]] for i in range(idx.shape[0])]
    cols = [np.full((int(rest.sum()), 3), GREY, np.float32)] + [np.repeat(colors[i:i + 1], int(idx[i].sum()), 0)
                                                                 for i in range(idx.shape[0])]
    scale = [np.full(int(rest.sum()), REST_SCALE)] + [np.ones(int(idx[i].sum())) for i in range(idx.shape[0])]
    return np.concatenate(pts), np.concatenate(cols), np.concatenate(scale)


def render_split(model_names, load_points, save=None, view=0, colored_subsets=None, models_per_call=256, **camera):
    """render_point_cloud_runner.py's loop over model_names, models_per_call clouds per dpc_render_points call.

    load_points(name) -> [V,N,3] (a prediction file's "points"), or None to skip the model; view `view` is rendered (the
    script's vis_idx = 0).  save(name, image_u8) is called per model (write_png, say).  colored_subsets = (indices [k,N]
    bool, colors [k,3]) restates load_data's subsets.  **camera goes to render_point_clouds (azimuth, elevation, dist,
    image_size, supersample, point_size, lens_mm).  Returns {name: uint8 [S,S,3] numpy image}; the images do not depend
    on models_per_call."""
    step = _split.checked_step("render_split", models_per_call)
    size = float(camera.pop("point_size", POINT_SIZE))
    result = {}

    def load(name, i):
        """(cloud, colours | None, radii | None) of the model's view."""
        pcs = load_points(name)
        if pcs is None:
            return None
        pcs = np.asarray(pcs.detach().cpu() if isinstance(pcs, torch.Tensor) else pcs)
        if pcs.ndim == 2:
            pcs = pcs[None]
        if pcs.ndim != 3 or pcs.shape[2] != 3 or not 0 <= view < pcs.shape[0]:
            raise ValueError("render_split: model %r: points must be [V,N,3] with view %d, got %s" % (name, view, pcs.shape))
        if colored_subsets is None:
            return pcs[view], None, None
        model, c, scale = _subset_cloud(pcs[view], colored_subsets)
        return model, c, scale * size

    for batch in _split.batches(model_names, load, step):
        clouds, cols, rads = ([item[k] for _, item in batch] for k in range(3))
        imgs = render_point_clouds(clouds, colors=cols if colored_subsets is not None else None,
                                   radii=rads if colored_subsets is not None else None, point_size=size, **camera)
        for (name, _), img in zip(batch, imgs.cpu().numpy()):
            result[name] = img
            if save is not None:
                save(name, img)
    return result


def write_png(path, image_u8):
    """An 8-bit RGB PNG of a [H,W,3] uint8 image (zlib and struct only)."""
    img = np.ascontiguousarray(image_u8.detach().cpu().numpy() if isinstance(image_u8, torch.Tensor) else image_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("write_png: need a [H,W,3] uint8 image, got %s %s" % (img.dtype, img.shape))
    h, w = img.shape[:2]

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    raw = b"".join(b"\x00" + img[i].tobytes() for i in range(h))  # filter type 0 on every row
    data = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
    with open(path, "wb") as fh:
        fh.write(data)


def read_png(path):
    """The [H,W,3] uint8 image of a PNG that write_png wrote (8-bit RGB, filter 0 rows)."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("read_png: %s is not a PNG" % path)
    pos, idat, w, h = 8, b"", 0, 0
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            if (depth, ctype) != (8, 2):
                raise ValueError("read_png: %s is not 8-bit RGB" % path)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    if (rows[:, 0] != 0).any():
        raise ValueError("read_png: %s uses PNG row filters" % path)
    return rows[:, 1:].reshape(h, w, 3).copy()


_PNG_KINDS = {(8, 6): (np.dtype(np.uint8), 4), (16, 0): (np.dtype(">u2"), 1), (8, 2): (np.dtype(np.uint8), 3)}


def _write_png_rows(path, rows, w, h, depth, ctype):
    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    raw = b"".join(b"\x00" + rows[i].tobytes() for i in range(h))  # filter type 0 on every row
    data = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
    with open(path, "wb") as fh:
        fh.write(data)


def write_png_rgba(path, image_u8):
    """An 8-bit RGBA PNG (straight alpha) of a [H,W,4] uint8 image: render_N.png of the training views."""
    img = np.ascontiguousarray(image_u8.detach().cpu().numpy() if isinstance(image_u8, torch.Tensor) else image_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 4:
        raise ValueError("write_png_rgba: need a [H,W,4] uint8 image, got %s %s" % (img.dtype, img.shape))
    _write_png_rows(path, img, img.shape[1], img.shape[0], 8, 6)


def write_png_gray16(path, image_u16):
    """A 16-bit greyscale PNG of a [H,W] uint16 image (big-endian samples): depth_N.png of the training views."""
    img = np.ascontiguousarray(image_u16.detach().cpu().numpy() if isinstance(image_u16, torch.Tensor) else image_u16)
    if img.dtype != np.uint16 or img.ndim != 2:
        raise ValueError("write_png_gray16: need a [H,W] uint16 image, got %s %s" % (img.dtype, img.shape))
    _write_png_rows(path, img.astype(">u2"), img.shape[1], img.shape[0], 16, 0)


def read_png_any(path):
    """The image of a PNG that write_png, write_png_rgba or write_png_gray16 wrote (filter 0 rows): [H,W,3] or [H,W,4]
    uint8, or [H,W] uint16."""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("read_png_any: %s is not a PNG" % path)
    pos, idat, w, h, kind = 8, b"", 0, 0, None
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            kind = _PNG_KINDS.get((depth, ctype))
            if kind is None:
                raise ValueError("read_png_any: %s is not 8-bit RGB / RGBA or 16-bit grey" % path)
        elif tag == b"IDAT":
            idat += body
        pos += 12 + n
    dtype, channels = kind
    stride = w * channels * dtype.itemsize
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + stride)
    if (rows[:, 0] != 0).any():
        raise ValueError("read_png_any: %s uses PNG row filters" % path)
    px = np.ascontiguousarray(rows[:, 1:]).view(dtype).reshape((h, w, channels) if channels > 1 else (h, w))
    return px.astype(np.uint16 if dtype.itemsize == 2 else np.uint8)
