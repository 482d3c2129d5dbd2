"""Training views from ShapeNet meshes on the GPU, in place of the reference's downloaded Blender renders.

The reference trains on <synth_set>-renders.tar.gz (data/download_train_data.sh): per model render_N.png (RGBA),
camera_N.mat and depth_N.png, which dpc/run/create_data_torch.py packs into <model>_features.p.  Here the views of a
whole group of models are rasterised in one dpc_render_meshes call (csrc/dpc_mesh_raster.hip), in fp64, with the camera
the reference's own projection expects (pc_perspective_transform's quaternion branch); include/dpc_render.h states the
semantics and the deliberate deviations from Blender's image.  Scenes that carry the models' textures and vertex
normals (load_obj_scene_shaded) go through dpc_render_meshes_shaded, which differs in the colour of a covered sample only.

    load_obj_scene          .obj (+ .mtl diffuse colours) -> V, F, material, Kd, names; every polygon, fan-triangulated
    load_obj_scene_shaded   the same, and vt, vn and the map_Kd images: a ShadedScene whose first five fields are those
    sample_camera_positions random camera positions in Blender's Z-up frame (the ranges are an assumption)
    view_rotation           cam_pos -> the 3 x 3 rotation of quaternion_from_campos(cam_pos), host fp64
    view_transform          the renderer's host transform of points: (d, v, u) of pc_perspective_transform
    render_mesh_views       scenes x camera positions -> rgba [W,S,S,4] uint8, depth [W,S,S] uint16 on the device
    camera_extrinsic        the 4 x 4 `extrinsic` of camera_N.mat for a camera position
    features_of_views       the dict create_record pickles (image, mask, name, extrinsic, cam_pos, depth)
    render_training_views   the loop over a split with caller-supplied I/O

Reading .obj files stays on the host; writing PNG / .mat / pickle files stays with the caller (tools/render_train_data.py).
"""
import collections
import os

import numpy as np
import torch

from . import _batch, _native, _split
from .alignment import as_rotation_matrix, quaternion_from_campos
from .densify import MeshError
from .visualise import read_png_any

DEFAULT_KD = 0.5           # the grey of a face without a usable material
WORKSPACE_LIMIT = 4 << 30  # bytes of dpc_render_meshes workspace per job (a single model may need more)
MAX_DEPTH = 10.0           # depth_N.png spans [0, 10] over 16 bits (create_data_torch.py:66-70)


# ------------------------------------------------------------------------------------------------------
# reading meshes
# ------------------------------------------------------------------------------------------------------
def _read_mtl(path):
    """{material name: Kd (r, g, b)} of a .mtl file; materials without a Kd line are left out."""
    out, name = {}, None
    with open(path) as fh:
        for text in fh:
            fields = text.split()
            if not fields:
                continue
            if fields[0] == "newmtl":
                name = " ".join(fields[1:])
            elif fields[0] == "Kd" and name is not None and len(fields) >= 4:
                out[name] = [float(x) for x in fields[1:4]]
    return out


def load_obj_scene(path):
    """An .obj file as (V [n,3] float64, F [f,3] int64, material [f] int64, Kd [k,3] float64, names [k]).

    Every face is kept and polygons are fan-triangulated ((0, i, i + 1)); only the vertex field of "v/vt/vn" is read.
    `usemtl` selects the material of the faces after it; the `mtllib` files, looked up next to the .obj, are read for Kd
    only.  Faces before any usemtl, a missing .mtl file and a material without Kd get one default grey (name "", Kd
    0.5), appended to the table when needed.  Kd values are clipped to [0, 1].  ValueError for a relative (<= 0) face
    index, as load_obj_mesh refuses them, IndexError for an index beyond the vertices or a face with fewer than three
    corners."""
    verts, faces, mats = [], [], []
    table, names, index = {}, [], {}
    here = os.path.dirname(os.path.abspath(path))
    current = None

    def material(name):
        key = name if name in table else None
        if key not in index:
            index[key] = len(names)
            names.append("" if key is None else key)
        return index[key]

    with open(path) as fh:
        for text in fh:
            fields = text.split()
            if not fields:
                continue
            tag = fields[0]
            if tag == "v":
                if len(fields) < 4:
                    raise IndexError("load_obj_scene: %s: a vertex line with %d coordinates" % (path, len(fields) - 1))
                verts.append([float(x) for x in fields[1:4]])
            elif tag == "f":
                if len(fields) < 4:
                    raise IndexError("load_obj_scene: %s: a face line with %d indices" % (path, len(fields) - 1))
                corners = [int(field.split("/", 1)[0]) - 1 for field in fields[1:]]
                if min(corners) < 0:
                    raise ValueError("load_obj_scene: %s: face index %d <= 0 (relative OBJ indices are refused)"
                                     % (path, min(corners) + 1))
                m = material(current)
                for i in range(1, len(corners) - 1):
                    faces.append((corners[0], corners[i], corners[i + 1]))
                    mats.append(m)
            elif tag == "usemtl":
                current = " ".join(fields[1:])
            elif tag == "mtllib":
                for name in fields[1:]:
                    lib = os.path.join(here, name)
                    if os.path.isfile(lib):
                        table.update(_read_mtl(lib))
    V = np.array(verts, dtype=np.float64).reshape(-1, 3)
    F = np.array(faces, dtype=np.int64).reshape(-1, 3)
    if len(F) and F.max() >= len(V):
        raise IndexError("load_obj_scene: %s: face index %d beyond the %d vertices" % (path, F.max() + 1, len(V)))
    Kd = np.array([[DEFAULT_KD] * 3 if n not in table else table[n] for n in names], dtype=np.float64).reshape(-1, 3)
    return V, F, np.array(mats, dtype=np.int64), np.clip(Kd, 0.0, 1.0), names


ShadedScene = collections.namedtuple("ShadedScene", "V F material Kd names uv face_uv normals face_vn mat_tex textures warnings")
ShadedScene.__doc__ = """load_obj_scene's five fields, then uv [n,2] float64, face_uv [f,3] int64 (-1: the corner has no vt),
normals [n,3] float64, face_vn [f,3] int64 (-1: no vn), mat_tex [k] int64 (the material's texture, -1: none), textures (a
list of [h,w,3] uint8 images, row 0 the top) and warnings (a list of strings: images that could not be used)."""


def _read_mtl_maps(path):
    """{material name: map_Kd file name} of a .mtl file: the last field of the line, backslashes as slashes."""
    out, name = {}, None
    with open(path) as fh:
        for text in fh:
            fields = text.split()
            if not fields:
                continue
            if fields[0] == "newmtl":
                name = " ".join(fields[1:])
            elif fields[0] == "map_Kd" and name is not None and len(fields) >= 2:
                out[name] = fields[-1].replace("\\", "/")
    return out


def _load_image(path):
    """The default image decoder: read_png_any for the PNGs it reads, else PIL when it is importable."""
    try:
        img = read_png_any(path)
        if img.ndim == 3 and img.dtype == np.uint8:
            return img
    except OSError:
        raise
    except Exception:  # not a PNG, or a PNG with row filters, palettes, interlacing: PIL's business
        pass
    try:
        from PIL import Image
    except ImportError:
        raise ValueError("not a PNG that read_png_any reads, and PIL is not installed") from None
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def load_obj_scene_shaded(path, load_image=None):
    """An .obj file as a ShadedScene: what load_obj_scene returns for it, and its texture coordinates, vertex normals
    and diffuse textures.

    Corners are read as v, v/vt, v//vn or v/vt/vn, and the fan triangulation carries each corner's vt and vn along; a
    corner without one gets -1 (such a face is rendered untextured, or flat-shaded).  A `vt` line gives (u, v) (a
    missing v is 0, a third value is ignored).  map_Kd of the `mtllib` files names a material's texture: the last field
    of the line with backslashes turned into slashes, looked up next to the .mtl; load_image(path) -> [h,w,3|4] uint8
    decodes it (alpha is dropped; the default reads PNGs with read_png_any and everything else with PIL when that is
    installed).  An image that is missing or cannot be decoded leaves its material untextured and adds a line to
    `warnings`; it is no error.  Images are shared between the materials that name the same file.  ValueError for a
    relative (<= 0) v, vt or vn index, IndexError for one beyond its array."""
    who = "load_obj_scene_shaded"
    verts, uvs, norms, faces, fts, fns, mats = [], [], [], [], [], [], []
    table, maps, names, index = {}, {}, [], {}
    here = os.path.dirname(os.path.abspath(path))
    current = None
    decode = _load_image if load_image is None else load_image

    def material(name):
        key = name if name in table else None
        if key not in index:
            index[key] = len(names)
            names.append("" if key is None else key)
        return index[key]

    def corner(field):
        parts = field.split("/")
        idx = [int(parts[0]), int(parts[1]) if len(parts) > 1 and parts[1] else None,
               int(parts[2]) if len(parts) > 2 and parts[2] else None]
        for what, k in zip(("face", "vt", "vn"), idx):
            if k is not None and k <= 0:
                raise ValueError("%s: %s: %s index %d <= 0 (relative OBJ indices are refused)" % (who, path, what, k))
        return tuple(-1 if k is None else k - 1 for k in idx)

    with open(path) as fh:
        for text in fh:
            fields = text.split()
            if not fields:
                continue
            tag = fields[0]
            if tag == "v":
                if len(fields) < 4:
                    raise IndexError("%s: %s: a vertex line with %d coordinates" % (who, path, len(fields) - 1))
                verts.append([float(x) for x in fields[1:4]])
            elif tag == "vt":
                if len(fields) < 2:
                    raise IndexError("%s: %s: a vt line without coordinates" % (who, path))
                uvs.append([float(fields[1]), float(fields[2]) if len(fields) > 2 else 0.0])
            elif tag == "vn":
                if len(fields) < 4:
                    raise IndexError("%s: %s: a vn line with %d coordinates" % (who, path, len(fields) - 1))
                norms.append([float(x) for x in fields[1:4]])
            elif tag == "f":
                if len(fields) < 4:
                    raise IndexError("%s: %s: a face line with %d indices" % (who, path, len(fields) - 1))
                corners = [corner(field) for field in fields[1:]]
                m = material(current)
                for i in range(1, len(corners) - 1):
                    tri = (corners[0], corners[i], corners[i + 1])
                    faces.append([c[0] for c in tri])
                    fts.append([c[1] for c in tri])
                    fns.append([c[2] for c in tri])
                    mats.append(m)
            elif tag == "usemtl":
                current = " ".join(fields[1:])
            elif tag == "mtllib":
                for name in fields[1:]:
                    lib = os.path.join(here, name)
                    if os.path.isfile(lib):
                        table.update(_read_mtl(lib))
                        folder = os.path.dirname(lib)
                        maps.update({k: os.path.join(folder, v) for k, v in _read_mtl_maps(lib).items()})
    V = np.array(verts, dtype=np.float64).reshape(-1, 3)
    UV = np.array(uvs, dtype=np.float64).reshape(-1, 2)
    VN = np.array(norms, dtype=np.float64).reshape(-1, 3)
    F, FT, FN = (np.array(a, dtype=np.int64).reshape(-1, 3) for a in (faces, fts, fns))
    for what, idx, arr in (("face", F, V), ("vt", FT, UV), ("vn", FN, VN)):
        if len(idx) and idx.max() >= len(arr):
            raise IndexError("%s: %s: %s index %d beyond the %d entries" % (who, path, what, idx.max() + 1, len(arr)))
    Kd = np.array([[DEFAULT_KD] * 3 if n not in table else table[n] for n in names], dtype=np.float64).reshape(-1, 3)
    textures, warnings, seen, mat_tex = [], [], {}, []
    for n in names:
        file = maps.get(n) if n in table else None
        if file is None:
            mat_tex.append(-1)
            continue
        if file not in seen:
            seen[file] = -1
            try:
                img = np.asarray(decode(file))
                if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4) or 0 in img.shape:
                    raise ValueError("the decoder returned %s %s, not [h,w,3|4] uint8" % (img.dtype, img.shape))
                seen[file] = len(textures)
                textures.append(np.ascontiguousarray(img[:, :, :3]))
            except Exception as exc:  # whatever a decoder raises: the material stays untextured
                warnings.append("%s: material %r: texture %s not used: %s" % (path, n, file, exc))
        mat_tex.append(seen[file])
    return ShadedScene(V, F, np.array(mats, dtype=np.int64), np.clip(Kd, 0.0, 1.0), names, UV, FT, VN, FN,
                       np.array(mat_tex, dtype=np.int64), textures, warnings)


# ------------------------------------------------------------------------------------------------------
# cameras
# ------------------------------------------------------------------------------------------------------
def sample_camera_positions(num_models, num_views, seed, azimuth_deg=(0.0, 360.0), elevation_deg=(-20.0, 40.0),
                            distance=2.0):
    """[num_models, num_views, 3] float64 camera positions in Blender's Z-up frame, (d cos el cos az, d cos el sin az,
    d sin el), azimuth and elevation uniform in their ranges (numpy default_rng(seed)), distance a scalar or a (lo, hi)
    range.

    ASSUMPTION: the distribution behind the released archive is not recorded in the reference; these defaults (all
    azimuths, elevations of -20 .. 40 degrees, distance 2) are ours.  The image does not depend on the distance: the
    projection normalises cam_pos and places the camera at cfg.camera_distance.  Elevations reaching +-90 degrees are
    refused: ypr_from_campos divides by sqrt(cx^2 + cy^2) there."""
    az, el = (tuple(float(x) for x in r) for r in (azimuth_deg, elevation_deg))
    dist = (float(distance),) * 2 if np.ndim(distance) == 0 else tuple(float(x) for x in distance)
    if len(az) != 2 or len(el) != 2 or len(dist) != 2 or not np.isfinite(az + el + dist).all():
        raise ValueError("sample_camera_positions: azimuth_deg, elevation_deg must be finite (lo, hi) pairs")
    if az[0] > az[1] or el[0] > el[1] or dist[0] > dist[1] or dist[0] <= 0.0:
        raise ValueError("sample_camera_positions: ranges must be ordered and distance > 0")
    if el[0] <= -90.0 or el[1] >= 90.0:
        raise ValueError("sample_camera_positions: elevation range %r reaches +-90 degrees, where the reference's "
                         "ypr_from_campos divides by zero" % (el,))
    M, V = int(num_models), int(num_views)
    if M < 0 or V < 0:
        raise ValueError("sample_camera_positions: num_models and num_views must be >= 0")
    rng = np.random.default_rng(seed)
    a = np.deg2rad(rng.uniform(az[0], az[1], (M, V)))
    e = np.deg2rad(rng.uniform(el[0], el[1], (M, V)))
    d = rng.uniform(dist[0], dist[1], (M, V))
    return np.stack([d * np.cos(e) * np.cos(a), d * np.cos(e) * np.sin(a), d * np.sin(e)], axis=-1)


def view_rotation(cam_pos):
    """The rotation R of q = quaternion_from_campos(cam_pos) (host fp64, [3,3]): quaternion_rotate(p, q) = R p.
    ValueError for a position on the vertical axis (elevation +-90 degrees) or a non-finite one."""
    c = np.asarray(cam_pos, dtype=np.float64).reshape(-1)
    if c.shape != (3,) or not np.isfinite(c).all() or not np.hypot(c[0], c[1]) > 0.0:
        raise ValueError("view_rotation: cam_pos %r must be three finite values off the vertical axis" % (cam_pos,))
    return as_rotation_matrix(quaternion_from_campos(c))


def view_transform(points, cam_pos, camera_distance=2.0, focal_length=1.875):
    """The renderer's host transform of [n,3] .obj-space points for one camera: (d, v, u) [n,3] with r = R p,
    d = r_0 + camera_distance, v = r_1 f / d, u = r_2 f / d.  pc_perspective_transform's quaternion branch returns
    (d - camera_distance, v, u)."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    R = view_rotation(cam_pos)
    r = np.stack([(R[k, 0] * P[:, 0] + R[k, 1] * P[:, 1]) + R[k, 2] * P[:, 2] for k in range(3)], axis=1)
    d = r[:, 0] + float(camera_distance)
    return np.stack([d, (r[:, 1] * float(focal_length)) / d, (r[:, 2] * float(focal_length)) / d], axis=1)


def camera_extrinsic(cam_pos, camera_distance=2.0):
    """The 4 x 4 `extrinsic` of camera_N.mat (float64): the matrix E that camera_from_blender (util/camera.py:15-35)
    rearranges into [[R, t], [0, 1]] with R = view_rotation(cam_pos) and t = (camera_distance, 0, 0), so that the matrix
    branch of pc_perspective_transform gives the quaternion branch's (d, f r_1, f r_2)."""
    R = view_rotation(cam_pos)
    E = np.zeros((4, 4), dtype=np.float64)
    E[2, 0], E[2, 2], E[2, 1] = -R[0, 0], R[0, 1], R[0, 2]
    E[1, 0], E[1, 2], E[1, 1] = R[1, 0], -R[1, 1], -R[1, 2]
    E[0, 0], E[0, 2], E[0, 1] = -R[2, 0], R[2, 1], R[2, 2]
    E[2, 3], E[1, 3], E[0, 3], E[3, 3] = float(camera_distance), 0.0, 0.0, 1.0
    return E


# ------------------------------------------------------------------------------------------------------
# rendering
# ------------------------------------------------------------------------------------------------------
def _cfg_get(cfg, key, default):
    if cfg is None:
        return default
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


_PLAIN_KD = np.array([[0.8, 0.8, 0.8]])   # the diffuse colour of a scene given as a bare (V, F) pair


def _scene(scene, i):
    """(V, F, material, Kd[, names]) -> host arrays (float64 [n,3], int32 [f,3], int32 [f], float64 [k,3]).  A bare
    (V, F) pair, as extract_surfaces returns it, is one material of _PLAIN_KD; device tensors are copied to the host."""
    if len(scene) == 2:
        scene = (scene[0], scene[1], np.zeros(len(scene[1]), dtype=np.int32), _PLAIN_KD)
    if len(scene) < 4:
        raise ValueError("render_mesh_views: scene %d must be (V, F, material, Kd[, names])" % i)
    V, F, mat, Kd = (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in scene[:4])
    V = np.ascontiguousarray(V.reshape(-1, 3) if V.size == 0 else V, dtype=np.float64)
    F = F.reshape(-1, 3) if F.size == 0 else F
    Kd = np.ascontiguousarray(Kd.reshape(-1, 3) if Kd.size == 0 else Kd, dtype=np.float64)
    mat = mat.reshape(-1)
    if V.ndim != 2 or V.shape[1] != 3 or F.ndim != 2 or F.shape[1] != 3 or Kd.ndim != 2 or Kd.shape[1] != 3:
        raise ValueError("render_mesh_views: scene %d: V, F and Kd must be [n,3], [f,3] and [k,3], got %s, %s, %s"
                         % (i, V.shape, F.shape, Kd.shape))
    if len(mat) != len(F):
        raise ValueError("render_mesh_views: scene %d: %d material ids for %d faces" % (i, len(mat), len(F)))
    for what, a in (("F", F), ("material", mat)):
        if a.size and (a.min() < np.iinfo(np.int32).min or a.max() > _batch.INT32_MAX):
            raise ValueError("render_mesh_views: scene %d: %s does not fit int32" % (i, what))
    if not (np.isfinite(Kd).all() and (Kd >= 0.0).all() and (Kd <= 1.0).all()):
        raise ValueError("render_mesh_views: scene %d: Kd must lie in [0, 1]" % i)
    return V, np.ascontiguousarray(F, dtype=np.int32), np.ascontiguousarray(mat, dtype=np.int32), Kd


def _is_shaded(scene):
    return hasattr(scene, "face_uv") and hasattr(scene, "face_vn")


def _attributes(scene, i, item):
    """The attributes of scene i (item = _scene(scene, i)) as host arrays (uv float64 [n,2], face_uv int32 [f,3], normals
    float64 [n,3], face_vn int32 [f,3], mat_tex int32 [k], textures [[h,w,3] uint8]); a plain tuple has none: every index
    -1."""
    f, k = len(item[1]), len(item[3])
    if not _is_shaded(scene):
        none = np.full((f, 3), -1, dtype=np.int32)
        return np.zeros((0, 2)), none, np.zeros((0, 3)), none, np.full(k, -1, dtype=np.int32), []
    uv, vn = np.asarray(scene.uv, dtype=np.float64), np.asarray(scene.normals, dtype=np.float64)
    uv, vn = uv.reshape(-1, 2) if uv.size == 0 else uv, vn.reshape(-1, 3) if vn.size == 0 else vn
    fuv, fvn, mt = (np.asarray(a) for a in (scene.face_uv, scene.face_vn, scene.mat_tex))
    fuv, fvn = fuv.reshape(-1, 3) if fuv.size == 0 else fuv, fvn.reshape(-1, 3) if fvn.size == 0 else fvn
    mt = mt.reshape(-1)
    if uv.ndim != 2 or uv.shape[1] != 2 or vn.ndim != 2 or vn.shape[1] != 3:
        raise ValueError("render_mesh_views: scene %d: uv and normals must be [n,2] and [n,3], got %s, %s"
                         % (i, uv.shape, vn.shape))
    if fuv.shape != (f, 3) or fvn.shape != (f, 3) or mt.shape != (k,):
        raise ValueError("render_mesh_views: scene %d: face_uv, face_vn and mat_tex must be [%d,3], [%d,3] and [%d], got "
                         "%s, %s, %s" % (i, f, f, k, fuv.shape, fvn.shape, mt.shape))
    for what, a in (("face_uv", fuv), ("face_vn", fvn), ("mat_tex", mt)):
        if a.dtype.kind not in "iu" or (a.size and (a.min() < np.iinfo(np.int32).min or a.max() > _batch.INT32_MAX)):
            raise ValueError("render_mesh_views: scene %d: %s must hold integers that fit int32" % (i, what))
    textures = []
    for t, img in enumerate(scene.textures):
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or 0 in img.shape:
            raise ValueError("render_mesh_views: scene %d: texture %d must be [h,w,3] uint8, got %s %s"
                             % (i, t, img.dtype, img.shape))
        textures.append(np.ascontiguousarray(img))
    c = lambda a, dt: np.ascontiguousarray(a, dtype=dt)
    return c(uv, np.float64), c(fuv, np.int32), c(vn, np.float64), c(fvn, np.int32), c(mt, np.int32), textures


def _tables(items, view_scene, attrs=None):
    """The mesh rows (6 int32, with attrs 12), the views' mesh indices and the totals; with attrs also the textures'
    (byte offset, width, height) rows, int64."""
    rows, tex, tot, to = [], [], [0] * 6, 0
    for k, (V, F, _, Kd) in enumerate(items):
        n = [len(V), len(F), len(Kd)]
        if attrs is not None:
            uv, _, vn, _, _, textures = attrs[k]
            n += [len(uv), len(vn), len(textures)]
            for img in textures:
                tex.append((to, img.shape[1], img.shape[0]))
                to += img.size
        rows.append([x for pair in zip(tot, n) for x in pair])
        tot = [a + b for a, b in zip(tot, n)] + tot[len(n):]
    width = 6 if attrs is None else 12
    meshes = _batch.table(rows if rows else np.zeros((0, width)), width,
                          "render_mesh_views: more than 2^31 - 1 vertices, faces, materials, uvs or normals in one call")
    views = _batch.table(np.asarray(view_scene, dtype=np.int64).reshape(-1, 1), 1, "render_mesh_views: bad scene index")
    if attrs is None:
        return meshes, views.reshape(-1), tuple(tot[:3])
    return meshes, views.reshape(-1), tuple(tot), np.ascontiguousarray(np.array(tex, dtype=np.int64).reshape(-1, 3)), to


def _workspace_bytes(meshes, views):
    L = _native.lib()
    return L.dpc_render_meshes_workspace_bytes(meshes.ctypes.data, len(meshes), views.ctypes.data, len(views))


def _status_message(items, view_scene, cams, S, bits, attrs=None, textures=True, smooth_normals=True):
    """Which scene a status bit came from, found on the host."""
    N = _native
    for i, (V, F, mat, Kd) in enumerate(items):
        if bits & N.DPC_STATUS_BAD_INDEX and len(F) and (F.min() < 0 or F.max() >= len(V) or mat.min() < 0
                                                         or mat.max() >= len(Kd)):
            return "render_mesh_views: scene %d has a face index outside its vertices or a material id outside its table" % i
        if bits & N.DPC_STATUS_NONFINITE and not np.isfinite(V).all():
            return "render_mesh_views: scene %d holds a NaN or infinite vertex coordinate" % i
        if attrs is None or not len(F):
            continue
        uv, fuv, vn, fvn, mt, tex = attrs[i]
        outside = lambda idx, n: idx.min() < -1 or idx.max() >= n
        if bits & N.DPC_STATUS_BAD_INDEX:
            if textures and (outside(fuv, len(uv)) or (len(mt) and outside(mt, len(tex)))):
                return ("render_mesh_views: scene %d has a texture coordinate index outside its uvs or a material's "
                        "texture index outside its textures" % i)
            if smooth_normals and outside(fvn, len(vn)):
                return "render_mesh_views: scene %d has a normal index outside its normals" % i
        if bits & N.DPC_STATUS_NONFINITE:
            used = lambda idx, a: a[idx[(idx >= 0) & (idx < len(a))]]
            if textures and not np.isfinite(used(fuv, uv)).all():
                return "render_mesh_views: scene %d holds a NaN or infinite texture coordinate" % i
            if smooth_normals and not np.isfinite(used(fvn, vn)).all():
                return "render_mesh_views: scene %d holds a NaN or infinite vertex normal" % i
    if bits & N.DPC_STATUS_BAD_INDEX:
        return "render_mesh_views: a face index or material id is out of range"
    if bits & N.DPC_STATUS_NONFINITE:
        return "render_mesh_views: a vertex or its projection is not finite"
    for w, s in enumerate(view_scene):
        V, F = items[s][0], items[s][1]
        R = cams[w, :9].reshape(3, 3)
        d = (R[0, 0] * V[:, 0] + R[0, 1] * V[:, 1]) + R[0, 2] * V[:, 2] + cams[w, 9]
        if len(F) and (d[np.unique(F)] <= N.DPC_MESH_NEAR).any():
            return ("render_mesh_views: view %d of scene %d: a face reaches the camera plane (depth <= %g); the model "
                    "must lie in front of the camera" % (w, s, N.DPC_MESH_NEAR))
    return "render_mesh_views: a face reaches the camera plane (depth <= %g)" % N.DPC_MESH_NEAR


def render_mesh_views(scenes, cam_pos, cfg=None, image_size=128, supersample=3, return_face_id=False, view_scene=None,
                      camera_distance=None, focal_length=None, textures=True, smooth_normals=True):
    """Render views of M scenes ((V, F, material, Kd[, names]) as load_obj_scene returns them) in one dpc_render_meshes call.

    A scene may also be a ShadedScene (load_obj_scene_shaded): its textured faces then take their colour from the
    texture and its faces with vertex normals are smooth-shaded (include/dpc_render.h, dpc_render_meshes_shaded), unless
    textures=False / smooth_normals=False switch that off for the call.  Both kinds may share a batch, which then goes
    through one dpc_render_meshes_shaded call; depth, face_id and alpha do not depend on the kind or the switches.  A
    batch of plain tuples, or one with both switches off, takes the dpc_render_meshes call.

    cam_pos: [M,V,3] (or a list of [v_i,3] per scene) camera positions in Blender's frame, views scene-major; or, with
    view_scene [W] (the scene of each view, in any order), [W,3].  camera_distance and focal_length come from cfg (a
    dict or attribute object; 2.0 and 1.875 when missing) as pc_perspective_transform reads them, unless given.
    Returns (rgba [W,S,S,4] uint8, depth [W,S,S] uint16) on the device, with return_face_id also face_id [W,S,S] int32:
    the face that gives the depth pixel (-1: background).  Each scene is stored once however many views it has.
    MeshError (a ValueError) naming the scene for a face index or material id out of range, a non-finite vertex or a
    face at the camera plane, and for a ShadedScene a uv, normal or texture index out of range or a non-finite uv or
    normal that a face names; ValueError before anything touches a device for bad arguments."""
    scenes = list(scenes)
    items = [_scene(s, i) for i, s in enumerate(scenes)]
    if (textures or smooth_normals) and any(_is_shaded(s) for s in scenes):
        attrs = [_attributes(s, i, items[i]) for i, s in enumerate(scenes)]
        return _render(items, attrs, cam_pos, cfg, image_size, supersample, return_face_id, view_scene, camera_distance,
                       focal_length, bool(textures), bool(smooth_normals))
    return _render(items, None, cam_pos, cfg, image_size, supersample, return_face_id, view_scene, camera_distance,
                   focal_length, True, True)


def _render(items, attrs, cam_pos, cfg, image_size, supersample, return_face_id, view_scene, camera_distance, focal_length,
            textures, smooth_normals):
    """render_mesh_views on checked scenes: attrs None is the dpc_render_meshes call, else dpc_render_meshes_shaded."""
    if view_scene is None:
        per = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in cam_pos]
        if len(per) != len(items):
            raise ValueError("render_mesh_views: cam_pos has %d entries for %d scenes" % (len(per), len(items)))
        view_scene = np.concatenate([np.full(len(c), i, dtype=np.int64) for i, c in enumerate(per)]) if per else []
        pos = np.concatenate(per) if per else np.zeros((0, 3))
    else:
        pos = np.asarray(cam_pos, dtype=np.float64).reshape(-1, 3)
    view_scene = np.asarray(view_scene, dtype=np.int64).reshape(-1)
    W = len(view_scene)
    if len(pos) != W:
        raise ValueError("render_mesh_views: %d camera positions for %d views" % (len(pos), W))
    if W and (view_scene.min() < 0 or view_scene.max() >= len(items)):
        raise ValueError("render_mesh_views: view_scene names a scene outside [0, %d)" % len(items))
    cd = float(_cfg_get(cfg, "camera_distance", 2.0) if camera_distance is None else camera_distance)
    fl = float(_cfg_get(cfg, "focal_length", 1.875) if focal_length is None else focal_length)
    if not (np.isfinite(cd) and np.isfinite(fl) and cd > 0.0 and fl > 0.0):
        raise ValueError("render_mesh_views: camera_distance %r and focal_length %r must be finite and > 0" % (cd, fl))
    cams = np.zeros((W, 11), dtype=np.float64)
    for w in range(W):
        try:
            cams[w, :9] = view_rotation(pos[w]).reshape(-1)
        except ValueError as exc:
            raise ValueError("render_mesh_views: view %d: %s" % (w, exc)) from exc
    cams[:, 9], cams[:, 10] = cd, fl
    S, ss = int(image_size), int(supersample)
    L = _native.lib()
    if attrs is not None:
        meshes, views, (nv, nf, nk, nu, nn, nt), tex, texel_bytes = _tables(items, view_scene, attrs)
        ht = tex.ctypes.data
    else:
        meshes, views, (nv, nf, nk) = _tables(items, view_scene)
    hm, hv = meshes.ctypes.data, views.ctypes.data
    if attrs is not None:
        rc = L.dpc_render_meshes_shaded(None, nv, None, None, nf, None, nk, None, nu, None, None, nn, None, None, None,
                                        texel_bytes, None, ht, nt, None, hm, len(meshes), None, hv, None, W, S, ss, None,
                                        None, None, None, None, None)
    else:
        rc = L.dpc_render_meshes(None, nv, None, None, nf, None, nk, None, hm, len(meshes), None, hv, None, W, S, ss,
                                 None, None, None, None, None, None)
    _batch.dry_run(rc, "render_mesh_views: refused by dpc_render_meshes (%d scenes, %d views, image_size %d, supersample %d): "
                   "need 1 <= image_size <= 1024, 1 <= supersample <= 4, at most 65535 views" % (len(items), W, S, ss))
    dev = _batch.device("dpc.render mesh rendering")
    rgba = torch.empty((W, S, S, 4), dtype=torch.uint8, device=dev)
    depth = torch.empty((W, S, S), dtype=torch.uint16, device=dev)
    face_id = torch.empty((W, S, S), dtype=torch.int32, device=dev) if return_face_id else None
    if W:
        cat = lambda k, dt, shape: torch.from_numpy(np.concatenate([it[k] for it in items]).astype(dt, copy=False)
                                                    .reshape(shape)).to(dev)
        verts, faces, mats, kd = cat(0, np.float64, (-1, 3)), cat(1, np.int32, (-1, 3)), cat(2, np.int32, (-1,)), \
            cat(3, np.float64, (-1, 3))
        meshes_d, views_d, cams_d = (torch.from_numpy(a).to(dev) for a in (meshes, views, cams))
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        N = _native
        geometry = (N.ptr(verts) if nv else None, nv, N.ptr(faces) if nf else None, N.ptr(mats) if nf else None, nf,
                    N.ptr(kd) if nk else None, nk)
        tail = (N.ptr(meshes_d), hm, len(meshes), N.ptr(views_d), hv, N.ptr(cams_d), W, S, ss, N.ptr(rgba), N.ptr(depth),
                N.ptr(face_id), N.ptr(status))
        if attrs is None:
            ws = _batch.workspace(_workspace_bytes(meshes, views), dev)
            N.call(dev, "dpc_render_meshes", *geometry, *tail, N.ptr(ws))
        else:
            # a switched-off group travels as NULL pointers: the library then reads none of it
            up = lambda arrays, dt, shape: torch.from_numpy(np.concatenate(arrays).astype(dt, copy=False).reshape(shape)).to(dev)
            uv_d = fuv_d = mt_d = tex_d = texels_d = vn_d = fvn_d = None
            if textures:
                uv_d, fuv_d, mt_d = up([a[0] for a in attrs], np.float64, (-1, 2)), up([a[1] for a in attrs], np.int32, (-1, 3)), \
                    up([a[4] for a in attrs], np.int32, (-1,))
                tex_d = torch.from_numpy(tex).to(dev)
                texels_d = up([img.reshape(-1) for a in attrs for img in a[5]] + [np.zeros(0, dtype=np.uint8)], np.uint8, (-1,))
            if smooth_normals:
                vn_d, fvn_d = up([a[2] for a in attrs], np.float64, (-1, 3)), up([a[3] for a in attrs], np.int32, (-1, 3))
            some = lambda t: N.ptr(t) if t is not None and t.numel() else None
            ws = _batch.workspace(L.dpc_render_meshes_shaded_workspace_bytes(hm, len(meshes), hv, len(views)), dev)
            N.call(dev, "dpc_render_meshes_shaded", *geometry, some(uv_d), nu, some(fuv_d), some(vn_d), nn, some(fvn_d),
                   some(mt_d), some(texels_d), texel_bytes, some(tex_d), ht, nt, *tail, N.ptr(ws))
        bits = int(status.item())
        if bits:
            raise MeshError(_status_message(items, view_scene, cams, S, bits, attrs, textures, smooth_normals))
    return (rgba, depth, face_id) if return_face_id else (rgba, depth)


# ------------------------------------------------------------------------------------------------------
# features                                               reference: dpc/run/create_data_torch.py:66-70, 102-162
# ------------------------------------------------------------------------------------------------------
def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def features_of_views(rgba, depth=None, cam_pos=None, extrinsic=None, name="", image_size=None, store_camera=True,
                      store_depth=True):
    """The dict create_record pickles as <model>_features.p for the V views of one model.

    rgba [V,S,S,4] uint8 (what imread returns for render_N.png): mask = alpha / 255; image = (rgb mask + 255 (1 - mask))
    / 255, the reference's white background, computed in float64 and stored as float32 like its `rgbs` array.  Keys:
    image [V,S,S,3] float32, mask [V,S,S,1] float32, name; with store_camera extrinsic [V,4,4] and cam_pos [V,3] float32;
    with store_depth depth [V,S,S,1] float32 from the uint16 depth [V,S,S] by loadDepth's arithmetic.  Only
    image_size == S (or None): the reference resizes with skimage otherwise, which is not reproduced here, so a
    different size raises ValueError: render at that size instead."""
    img = _host(rgba)
    if img.dtype != np.uint8 or img.ndim != 4 or img.shape[3] != 4 or img.shape[1] != img.shape[2]:
        raise ValueError("features_of_views: rgba must be [V,S,S,4] uint8, got %s %s" % (img.dtype, img.shape))
    V, S = img.shape[0], img.shape[1]
    if image_size is not None and int(image_size) != S:
        raise ValueError("features_of_views: image_size %d differs from the rendered %d; the reference's resize "
                         "(skimage) is not reproduced: render at image_size %d" % (image_size, S, image_size))
    rgbs = np.zeros((V, S, S, 3), dtype=np.float32)
    masks = np.zeros((V, S, S, 1), dtype=np.float32)
    for k in range(V):
        rgb = img[k][:, :, 0:3]
        mask = img[k][:, :, [3]]
        mask = mask / 255.0
        mask_fg = np.repeat(mask, 3, 2)
        mask_bg = 1.0 - mask_fg
        rgb = rgb * mask_fg + np.ones(rgb.shape) * 255.0 * mask_bg
        rgb = rgb / 255.0
        rgbs[k, :, :, :] = rgb
        masks[k, :, :, :] = mask
    feature = {"image": rgbs, "mask": masks, "name": name}
    if store_camera:
        if cam_pos is None or extrinsic is None:
            raise ValueError("features_of_views: store_camera needs cam_pos [V,3] and extrinsic [V,4,4]")
        cameras = np.zeros((V, 4, 4), dtype=np.float32)
        pos = np.zeros((V, 3), dtype=np.float32)
        cameras[:] = np.asarray(extrinsic, dtype=np.float64).reshape(V, 4, 4)
        pos[:] = np.asarray(cam_pos, dtype=np.float64).reshape(V, 3)
        feature["extrinsic"] = cameras
        feature["cam_pos"] = pos
    if store_depth:
        if depth is None:
            raise ValueError("features_of_views: store_depth needs depth [V,S,S] uint16")
        dm = _host(depth)
        if dm.dtype != np.uint16 or dm.shape != (V, S, S):
            raise ValueError("features_of_views: depth must be [%d,%d,%d] uint16, got %s %s" % (V, S, S, dm.dtype, dm.shape))
        depths = np.zeros((V, S, S, 1), dtype=np.float32)
        for k in range(V):
            d = dm[k].astype(np.float32)
            d = d * np.float32(MAX_DEPTH - 0) / np.float32(pow(2, 16) - 1) + np.float32(0)   # loadDepth
            d = (d - np.float32(0.0)) / np.float32(MAX_DEPTH)
            d = d * np.float32(MAX_DEPTH) + np.float32(0.0)   # the order-0 resize between these two lines keeps an equal size
            depths[k, :, :] = np.expand_dims(d, -1)
        feature["depth"] = depths
    return feature


# ------------------------------------------------------------------------------------------------------
# a split
# ------------------------------------------------------------------------------------------------------
def _checked(scene, i):
    """scene i with its arrays checked and converted: a plain 4-tuple, or a ShadedScene when it came as one."""
    item = _scene(scene, i)
    if not _is_shaded(scene):
        return item
    return ShadedScene(*item, list(getattr(scene, "names", None) or []), *_attributes(scene, i, item),
                       list(getattr(scene, "warnings", None) or []))


def _groups(items, view_counts, step, workspace_limit):
    """Consecutive index ranges of items, each at most `step` models and, unless it is one model, at most
    workspace_limit bytes of dpc_render_meshes workspace.  dpc_render_meshes_shaded asks for the same workspace (it
    fetches uvs, normals and texels where it shades and keeps nothing per view), so the estimate holds for both."""
    start, verts, faces = 0, 0, 0
    for k, it in enumerate(items):
        v, f = len(it[0]) * view_counts[k], len(it[1]) * view_counts[k]
        need = 16 * sum(view_counts[start:k + 1]) + 32 * (verts + v) + 8 * (faces + f) + 64
        if k > start and (k - start >= step or need > workspace_limit):
            yield start, k
            start, verts, faces = k, 0, 0
        verts, faces = verts + v, faces + f
    if start < len(items):
        yield start, len(items)


def _render_group(pairs, kwargs):
    """One render_mesh_views call for (scene, cameras [v,3]) pairs: per pair (rgba [v,S,S,4], depth [v,S,S]) on the host."""
    cams = [c for _, c in pairs]
    rgba, depth = render_mesh_views([scene for scene, _ in pairs], cams, **kwargs)
    rgba, depth = rgba.cpu().numpy(), depth.cpu().numpy()
    out, o = [], 0
    for c in cams:
        out.append((rgba[o:o + len(c)], depth[o:o + len(c)]))
        o += len(c)
    return out


def render_training_views(model_names, load_scene, cam_pos, save=None, models_per_call=64, errors=None, keep=True,
                          workspace_limit=WORKSPACE_LIMIT, **render):
    """The views of every model of a split, at most models_per_call models (and workspace_limit bytes of workspace) per
    dpc_render_meshes call.

    load_scene(name) -> (V, F, material, Kd[, names]) (load_obj_scene(path), say), or None to skip the model;
    cam_pos: {name: [V,3]}, a callable name -> [V,3], or an array [len(model_names),V,3]; save(name, rgba [V,S,S,4] uint8,
    depth [V,S,S] uint16, cam_pos [V,3]) is called per model with host arrays.  **render goes to render_mesh_views (cfg,
    image_size, supersample, camera_distance, focal_length, textures, smooth_normals; the last two matter for the
    ShadedScenes load_obj_scene_shaded returns).  Returns {name: (rgba, depth)}, or {} with keep=False.  The
    images do not depend on the batching.  A model whose loading or rendering fails raises an error that names it; with
    an `errors` dict it is recorded there (errors[name] = message) and skipped, and the other models go on."""
    step = _split.checked_step("render_training_views", models_per_call)
    model_names = list(model_names)
    if callable(cam_pos):
        cams_of = cam_pos
    elif isinstance(cam_pos, dict):
        cams_of = cam_pos.__getitem__
    else:
        arr = np.asarray(cam_pos, dtype=np.float64)
        if arr.ndim != 3 or arr.shape[0] != len(model_names) or arr.shape[2] != 3:
            raise ValueError("render_training_views: cam_pos must be [%d,V,3], got %s" % (len(model_names), arr.shape))
        lookup = {n: arr[i] for i, n in enumerate(model_names)}
        cams_of = lookup.__getitem__
    result = {}

    def load(name, i):
        scene = load_scene(name)
        if scene is None:
            return None
        item = _checked(scene, i)
        c = np.asarray(cams_of(name), dtype=np.float64).reshape(-1, 3)
        for p in c:
            view_rotation(p)
        return item, c

    for batch in _split.batches(model_names, load, step, errors, (ValueError, IndexError, KeyError, OSError)):
        names, pairs = [name for name, _ in batch], [pair for _, pair in batch]
        for a, b in _groups([scene for scene, _ in pairs], [len(c) for _, c in pairs], step, workspace_limit):
            done = _split.isolate(lambda group: _render_group(group, render), pairs[a:b], names[a:b], errors)
            for name, (_, c), res in zip(names[a:b], pairs[a:b], done):
                if res is None:
                    continue
                if keep:
                    result[name] = res
                if save is not None:
                    save(name, res[0], res[1], c)
    return result
