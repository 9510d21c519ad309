"""Headless voxel renderer: predicted label volumes -> images, ray-cast on the GPU (csrc/render.hip, one launch per batch).

The reference draws predictions with mayavi / open3d windows (scripts/visualization/kitti_vis_pred.py, NYU_vis_pred.py),
which need a display; the GPU nodes have none.  Here a view is 18 floats (`OccdRenderView`: an affine ray generator in
grid units), built from device calibration with torch ops (no host read-back), and the kernel walks one ray per pixel to
the first visible voxel.  Colours are integer arithmetic, so an image is exact once (voxel, face, fov) are known.

    views = [camera_view(cam_k, T_velo_2_cam, origin, 0.2), bev_view(dims, 2)]
    rgb = render_logits(ssc_logit, views, [(370, 1220), bev_size(dims, 2)])      # list of (B, h, w, 3) uint8
    write_png("frame.png", rgb[0][0])
"""
import math
import struct
import zlib

import numpy as np
import torch

from . import hip

SHADE = (160, 208, 256, 256)            # per face (x, y, z, started inside) over 256; csrc/render.hip shade_of()
BACKGROUND = (255, 255, 255)
ERROR_COLOURS = ((255, 160, 0), (220, 30, 30), (40, 90, 230))     # wrong class, false positive, false negative
ERR_WRONG, ERR_FALSE_POS, ERR_FALSE_NEG = 0, 1, 2                  # offsets into the last three palette rows
MODES = ("class", "error")

# SemanticKITTI: semantic-kitti.yaml color_map (stored there as BGR) of the 19 training classes, index 0 = empty
KITTI_COLOURS = (
    (0, 0, 0), (100, 150, 245), (100, 230, 245), (30, 60, 150), (80, 30, 180), (0, 0, 255), (255, 30, 30),
    (255, 40, 200), (150, 30, 90), (255, 0, 255), (255, 150, 255), (75, 0, 75), (175, 0, 75), (255, 200, 0),
    (255, 120, 50), (0, 175, 0), (135, 60, 0), (150, 240, 80), (255, 240, 150), (255, 0, 0))
# NYUv2: empty, ceiling, floor, wall, window, chair, bed, sofa, table, tvs, furniture, objects
NYU_COLOURS = (
    (0, 0, 0), (214, 38, 40), (43, 160, 43), (158, 216, 229), (114, 158, 206), (204, 204, 91), (255, 186, 119),
    (147, 102, 188), (30, 119, 181), (188, 188, 33), (255, 127, 12), (196, 175, 214))


def palette(dataset_or_n_classes):
    """-> (n_classes + 3, 3) uint8 CPU tensor: the class colours, then the three error colours.  "kitti" / 20: the
    SemanticKITTI colours; "NYU" / 12: a fixed table; any other class count: a deterministic generated table."""
    key = dataset_or_n_classes
    if key in ("kitti", 20):
        rows = list(KITTI_COLOURS)
    elif key in ("NYU", 12):
        rows = list(NYU_COLOURS)
    elif isinstance(key, int) and key >= 1:
        rows = [(0, 0, 0)]
        for i in range(1, key):                      # golden-ratio hue steps, two brightness levels
            h = (i * 0.61803398875) % 1.0
            s, v = 0.85, (1.0, 0.7)[i % 2]
            k = int(h * 6.0)
            f = h * 6.0 - k
            p, q, t = v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))
            r, g, b = ((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q))[k % 6]
            rows.append((int(r * 255), int(g * 255), int(b * 255)))
    else:
        raise ValueError("palette() takes 'kitti', 'NYU' or a class count, got %r" % (key,))
    return torch.tensor(rows + list(ERROR_COLOURS), dtype=torch.uint8)


# ------------------------------------------------------------------------------------------------------------- views
def _device(device):
    return torch.device(device) if device is not None else torch.device("cuda" if torch.cuda.is_available() else "cpu")


def camera_view(cam_k, T_velo_2_cam, vox_origin, voxel_size, flip=False, width=None):
    """Pinhole view of the camera itself: cam_k (..., 3, 3) and T_velo_2_cam (..., 4, 4) (world -> camera) tensors on
    any device, vox_origin (3 numbers or a (..., 3) tensor, metres) and the voxel size of the volume that will be
    rendered.  -> (..., 18) float32 on the calibration's device; t along a ray is camera depth in metres.  Pixel (u, v)
    is the pixel the package's projection rounds to (x fx / z + cx in [u - 1/2, u + 1/2)), so an overlay lines up with
    the FOV tables.  flip=True mirrors the image of `width` pixels (the loader's flip augmentation).  float64 inside;
    the rigid inverse is R^T, -R^T t (no matrix inversion, no host read-back)."""
    k = torch.as_tensor(cam_k).to(torch.float64)
    E = torch.as_tensor(T_velo_2_cam).to(device=k.device, dtype=torch.float64)
    Rt = E[..., :3, :3].transpose(-1, -2)
    centre = -(Rt @ E[..., :3, 3:4])[..., 0]                                   # camera centre in the world
    org = torch.as_tensor(vox_origin, dtype=torch.float64, device=k.device) if not torch.is_tensor(vox_origin) else \
        vox_origin.to(device=k.device, dtype=torch.float64)
    fx, fy, cx, cy = k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2]
    zero, one = torch.zeros_like(fx), torch.ones_like(fx)
    # direction in the camera frame of continuous pixel (x, y) = ((u + 1/2) - 1/2, (v + 1/2) - 1/2), z = 1
    d0 = torch.stack([(-0.5 - cx) / fx, (-0.5 - cy) / fy, one], -1)
    du = torch.stack([1.0 / fx, zero, zero], -1)
    dv = torch.stack([zero, 1.0 / fy, zero], -1)
    if flip:
        if width is None:
            raise ValueError("camera_view(flip=True) needs the image width")
        d0 = d0 + float(width) * du                                            # u' + 1/2 = W - (u + 1/2)
        du = -du
    rot = lambda d: (Rt @ d.unsqueeze(-1))[..., 0] / voxel_size
    o0 = (centre - org) / voxel_size
    z3 = torch.zeros_like(o0)
    o0, d0, du, dv = torch.broadcast_tensors(o0, rot(d0), rot(du), rot(dv))
    return torch.cat([o0, z3.expand_as(o0), z3.expand_as(o0), d0, du, dv], -1).to(torch.float32)


def bev_size(dims, pixels_per_voxel):
    """(H, W) of `bev_view`: x runs up the image, y to the left."""
    return int(dims[0]) * int(pixels_per_voxel), int(dims[1]) * int(pixels_per_voxel)


def bev_view(dims, pixels_per_voxel, device=None):
    """Orthographic view from above: pixel (u, v) looks down (-z) at x = X - (v + 1/2) / p, y = Y - (u + 1/2) / p
    (forward is up, left is left, as a driver sees the SemanticKITTI grid); t counts voxels from z = Z + 1.  -> (18,)."""
    X, Y, Z = (float(d) for d in dims)
    p = float(pixels_per_voxel)
    v = [X, Y, Z + 1.0, 0.0, -1.0 / p, 0.0, -1.0 / p, 0.0, 0.0, 0.0, 0.0, -1.0] + [0.0] * 6
    return torch.tensor(v, dtype=torch.float32, device=_device(device))


def oblique_view(dims, size, azimuth=-60.0, elevation=35.0, device=None):
    """Orthographic third-person view (what a viewer window opens with): the eye sits `elevation` degrees above the
    horizon at `azimuth` degrees from +x around the volume's centre, z is up in the image, and the volume's diagonal
    fills the smaller side of size = (H, W); t counts voxels.  -> (18,)."""
    H, W = int(size[0]), int(size[1])
    az, el = math.radians(azimuth), math.radians(elevation)
    f = (-math.cos(el) * math.cos(az), -math.cos(el) * math.sin(az), -math.sin(el))      # eye -> centre
    r = (-math.sin(az), math.cos(az), 0.0)                                                # image right (f x up, unit)
    up = (r[1] * f[2] - r[2] * f[1], r[2] * f[0] - r[0] * f[2], r[0] * f[1] - r[1] * f[0])  # r x f
    diag = math.sqrt(sum(float(d) ** 2 for d in dims))
    s = diag / min(H, W)                                                                  # voxels per pixel
    ou = [s * c for c in r]
    ov = [-s * c for c in up]
    o0 = [float(d) / 2 - diag * fc - (W / 2) * a - (H / 2) * b for d, fc, a, b in zip(dims, f, ou, ov)]
    return torch.tensor(o0 + ou + ov + list(f) + [0.0] * 6, dtype=torch.float32, device=_device(device))


# ------------------------------------------------------------------------------------------------------------ render
_palette_cache = {}


def _device_palette(pal, n_classes, device):
    if torch.is_tensor(pal):
        return pal.to(device=device, dtype=torch.uint8).contiguous()
    key = (pal if pal is not None else n_classes, str(device))
    t = _palette_cache.get(key)
    if t is None:                                # one host -> device copy per (palette, device), outside any capture
        t = _palette_cache[key] = palette(key[0]).to(device)
    return t


def _stack_views(views, B, device):
    if not torch.is_tensor(views):
        views = torch.stack([v.to(device).expand(B, 18) if v.dim() <= 2 else v for v in
                             (torch.as_tensor(v) for v in views)], 1)
    if views.dim() == 1:
        views = views[None]
    if views.dim() == 2:
        views = views[None].expand(B, -1, -1)
    if views.dim() != 3 or views.shape[0] != B or views.shape[2] != 18:
        raise ValueError("views must be (18,), (V, 18), (B, V, 18) or a list of (18,) / (B, 18) tensors")
    return views.to(device=device, dtype=torch.float32).contiguous()


def render_labels(labels, views, size, fov=None, target=None, mode="class", background=None, alpha=160, palette=None,
                  return_aux=False, n_classes=20):
    """Draw label volumes.  labels (B, X, Y, Z) (or (X, Y, Z)) on the GPU: uint8 / int16 / uint16 are read in place,
    wider integers are narrowed.  views: see `_stack_views`.  size: (H, W) for every view -> rgb (B, V, H, W, 3) uint8;
    or one (h, w) per view -> a list of V tensors (B, h, w, 3) rendered in the same launch.  fov: (B, X, Y, Z) bool mask,
    voxels outside are dimmed.  mode "error" colours against `target` (255 = ignored, transparent).  background
    (B, V, H, W, 3) uint8 + alpha (0..256): the voxels are blended over it.  palette: a name / class count for
    `palette()` or a (P, 3) uint8 tensor whose last three rows are the error colours (default: n_classes).
    return_aux: also hit (voxel index or -1), face, depth.  Capture-safe once the palette is on the device."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (MODES, mode))
    if mode == "error" and target is None:
        raise ValueError("mode='error' needs a target volume")
    narrow = lambda t: t if t.dtype in (torch.uint8, torch.int16, getattr(torch, "uint16", torch.int16)) else t.to(torch.int16)
    labels = narrow(labels[None] if labels.dim() == 3 else labels).contiguous()
    B = labels.shape[0]
    dev = labels.device
    if mode == "error":
        target = narrow(target[None] if target.dim() == 3 else target).to(dev).contiguous()
    else:
        target = None
    if fov is not None:
        fov = fov.to(dev).reshape(labels.shape).contiguous()
    views = _stack_views(views, B, dev)
    V = views.shape[1]
    per_view = not isinstance(size[0], int)
    sizes = [tuple(int(s) for s in hw) for hw in size] if per_view else None
    if per_view and len(sizes) != V:
        raise ValueError("%d sizes for %d views" % (len(sizes), V))
    H, W = (max(s[0] for s in sizes), max(s[1] for s in sizes)) if per_view else (int(size[0]), int(size[1]))
    out = hip.render_voxels(labels, views, (H, W), _device_palette(palette, n_classes, dev), target=target, fov=fov,
                            background=background, alpha=alpha, bg_colour=BACKGROUND, view_sizes=sizes, aux=return_aux)
    if not per_view:
        return out
    crop = lambda t: [t[:, i, :h, :w] for i, (h, w) in enumerate(sizes)]
    return tuple(crop(t) for t in out) if return_aux else crop(out)


def render_logits(ssc_logit, views, size, **kw):
    """`render_labels` of the arg-max of (B, C, X, Y, Z) logits; a channels-last view of wider rows (what the eval path
    returns) is consumed in place and only the uint16 volume is materialised."""
    kw.setdefault("n_classes", int(ssc_logit.shape[1]))
    return render_labels(hip.argmax_labels_u16(ssc_logit), views, size, **kw)


# --------------------------------------------------------------------------------------------------- the sequence map
MAP_BEV_SIDE = 2048


def render_map(volume, views, size, mode="class", background=None, alpha=160, palette=None, t_max=None, return_aux=False,
               skip=True):
    """Draw a sequence map (semantic_map.MapVolume) by ray-casting its bricks directly (csrc/map_render.hip, one launch).
    views: (18,), (V, 18) or a list of (18,) tensors in the volume's window voxel units (`map_camera_view`,
    `map_bev_view`, `map_oblique_view`).  size: (H, W) for every view -> rgb (V, H, W, 3) uint8; or one (h, w) per view
    -> a list of V tensors (h, w, 3) rendered in the same launch.  mode "error" colours the prediction against the
    ground-truth map and needs a volume built with `gt`.  background (V, H, W, 3) uint8 + alpha (0..256): the voxels are
    blended over it.  palette: as for `render_labels` (default: the volume's class count).  t_max: hits deeper than this
    (in the unit of the view's t: metres for a camera, voxels otherwise) are misses; None = no limit.  return_aux: also
    hit (row * 4096 + brick-local voxel, or -1; int64), face, depth.  The images are, bit for bit, what `render_labels`
    draws from the window's dense volume.  skip=False walks absent bricks voxel by voxel (the same images; for A/B runs)."""
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (MODES, mode))
    if mode == "error" and volume.target is None:
        raise ValueError("mode='error' needs a MapVolume built with a ground-truth map (gt)")
    dev = volume.labels.device
    views = _stack_views(views, 1, dev)[0].contiguous()
    V = views.shape[0]
    per_view = not isinstance(size[0], int)
    sizes = [tuple(int(s) for s in hw) for hw in size] if per_view else None
    if per_view and len(sizes) != V:
        raise ValueError("%d sizes for %d views" % (len(sizes), V))
    H, W = (max(s[0] for s in sizes), max(s[1] for s in sizes)) if per_view else (int(size[0]), int(size[1]))
    out = hip.map_render(volume.labels, volume.cells, views, (H, W), _device_palette(palette, volume.n_classes, dev),
                         target=volume.target if mode == "error" else None, background=background, alpha=alpha,
                         bg_colour=BACKGROUND, view_sizes=sizes, t_max=float("inf") if t_max is None else float(t_max),
                         skip=skip, aux=return_aux)
    if not per_view:
        return out
    crop = lambda t: [t[i, :h, :w] for i, (h, w) in enumerate(sizes)]
    return tuple(crop(t) for t in out) if return_aux else crop(out)


def map_camera_view(cam_k, T_velo_2_cam, pose, volume, flip=False, width=None):
    """The map seen through a frame's camera: cam_k (3, 3), T_velo_2_cam (4, 4) (sensor -> camera) and the frame's `pose`
    (4 x 4 sensor -> world, as fuse.read_kitti_poses returns) -> (18,) float32 in the volume's window voxel units, t =
    camera depth in metres.  Equals camera_view(cam_k, T_velo_2_cam @ rigid_inverse(pose), volume.origin_metres,
    volume.voxel_size), but composed in float64 relative to the window origin: the camera centre is formed as
    R_pose c + (t_pose - origin), so a pose kilometres from world zero keeps the float32 ray origins small."""
    k = torch.as_tensor(cam_k).to(torch.float64).cpu()
    E = torch.as_tensor(T_velo_2_cam).to(torch.float64).cpu()
    P = torch.as_tensor(np.asarray(pose, dtype=np.float64)) if not torch.is_tensor(pose) else pose.to(torch.float64).cpu()
    org = torch.as_tensor(np.asarray(volume.origin_metres, dtype=np.float64))
    R = P[:3, :3]
    world_2_cam = torch.eye(4, dtype=torch.float64)                    # world' -> camera, world' = world - window origin
    world_2_cam[:3, :3] = E[:3, :3] @ R.T
    world_2_cam[:3, 3] = E[:3, 3] - E[:3, :3] @ (R.T @ (P[:3, 3] - org))
    view = camera_view(k, world_2_cam, (0.0, 0.0, 0.0), volume.voxel_size, flip=flip, width=width)
    return view.to(volume.labels.device)


def map_bev_view(volume, max_side=MAP_BEV_SIDE):
    """Orthographic view from above over the whole window -> (view (18,), (h, w)): `bev_view` at the largest whole number
    of pixels per voxel whose image fits `max_side`.  Where the window is longer than `max_side` voxels, one pixel per n =
    ceil(side / max_side) voxels instead: the pixel draws the column under its centre and the n^2 - 1 others are not
    looked at -- point sampling, not an average; thin structures can drop out of such a picture."""
    X, Y = int(volume.dims[0]), int(volume.dims[1])
    side, max_side = max(X, Y), int(max_side)
    if max_side < 1:
        raise ValueError("max_side must be >= 1, got %r" % (max_side,))
    dev = volume.labels.device
    if side <= max_side:
        ppv = max_side // side
        return bev_view(volume.dims, ppv, device=dev), bev_size(volume.dims, ppv)
    n = -(-side // max_side)
    return bev_view(volume.dims, 1.0 / n, device=dev), (-(-X // n), -(-Y // n))


def map_oblique_view(volume, size, azimuth=-60.0, elevation=35.0):
    """`oblique_view` over the volume's window."""
    return oblique_view(volume.dims, size, azimuth, elevation, device=volume.labels.device)


MAP_VIEW_NAMES = ("bev", "oblique")


def map_standard_views(names, volume, bev_side=None):
    """The views the model hook and tools/map_sequence.py draw of a map -> ([(18,) tensors], [(h, w)])."""
    views, sizes = [], []
    for name in names:
        if name == "bev":
            view, size = map_bev_view(volume, MAP_BEV_SIDE if bev_side is None else bev_side)
        elif name == "oblique":
            view, size = map_oblique_view(volume, OBLIQUE_SIZE), OBLIQUE_SIZE
        else:
            raise ValueError("unknown map view %r (have %s)" % (name, MAP_VIEW_NAMES))
        views.append(view)
        sizes.append((int(size[0]), int(size[1])))
    return views, sizes


def write_map_pictures(volume, prefix, names, bev_side=None, palette=None):
    """<prefix>_{pred,gt,err}_{view}.png of a MapVolume (pred alone when it was built without gt) -> the paths.  The gt
    picture draws the volume with the target as labels."""
    views, sizes = map_standard_views(names, volume, bev_side)
    kinds = [("pred", volume, "class")]
    if volume.target is not None:
        kinds += [("gt", volume.target_volume(), "class"), ("err", volume, "error")]
    paths = []
    for kind, vol, mode in kinds:
        images = render_map(vol, views, sizes, mode=mode, palette=palette)
        for name, img in zip(names, images):
            paths.append(write_png("%s_%s_%s.png" % (prefix, kind, name), img))
    return paths


# --------------------------------------------------------------------------------------------------------------- png
def write_png(path, rgb):
    """(H, W, 3) or (H, W) uint8 array / tensor -> an 8-bit PNG (filter 0 on every row; zlib and struct only)."""
    a = rgb.detach().cpu().numpy() if torch.is_tensor(rgb) else np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png takes a non-empty uint8 (H, W, 3) or (H, W) image, got %s %s" % (a.shape, a.dtype))
    H, W = a.shape[:2]
    rows = np.zeros((H, 1 + W * (3 if a.ndim == 3 else 1)), dtype=np.uint8)
    rows[:, 1:] = a.reshape(H, -1)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) +
                chunk(b"IEND", b""))
    return path


# ------------------------------------------------------------------------------------------------- batch -> views
VIEW_NAMES = ("camera", "bev", "oblique")
OBLIQUE_SIZE = (480, 640)
BEV_SIDE = 512                              # the BEV gets the whole number of pixels per voxel that fits this side


def standard_views(names, dims, device, camera):
    """The views the model hook and tools/render_predictions.py draw -> ([(18,) or (B, 18) tensors], [(h, w)]).
    `camera()` -> (view, (h, w)) is called only when "camera" is among `names`."""
    views, sizes = [], []
    for name in names:
        if name == "camera":
            view, size = camera()
        elif name == "bev":
            ppv = max(1, BEV_SIDE // max(int(dims[0]), int(dims[1])))
            view, size = bev_view(dims, ppv, device=device), bev_size(dims, ppv)
        elif name == "oblique":
            view, size = oblique_view(dims, OBLIQUE_SIZE, device=device), OBLIQUE_SIZE
        else:
            raise ValueError("unknown render view %r (have %s)" % (name, VIEW_NAMES))
        views.append(view)
        sizes.append((int(size[0]), int(size[1])))
    return views, sizes


def batch_camera(batch, dataset, kitti_origin=None, device=None):
    """The left camera's calibration of a batch -> (cam_k (B, 3, 3), world -> camera (B, 4, 4) float64, origin).  kitti:
    `cam_k`, `T_velo_2_cam` (its float64 copy when present) and the dataset's voxel origin.  Any other dataset: `cam_k`,
    `cam_pose` (camera -> world, inverted here as a rigid transform) and `vox_origin` from the batch, or
    NotImplementedError naming what is missing."""
    def left(key, n):
        rows = [torch.as_tensor(t).reshape(-1, n, n)[0] for t in batch[key]]
        return torch.stack([r.to(device) if device is not None else r for r in rows]).to(torch.float64)
    if dataset == "kitti":
        return left("cam_k", 3), left("T_velo_2_cam_f64" if "T_velo_2_cam_f64" in batch else "T_velo_2_cam", 4), kitti_origin
    missing = [k for k in ("cam_k", "cam_pose", "vox_origin") if k not in batch]
    if missing:
        raise NotImplementedError("the 'camera' view of a %s batch needs %s in the batch (missing: %s); 'bev' and "
                                  "'oblique' need only the grid" % (dataset, "cam_k, cam_pose and vox_origin",
                                                                    ", ".join(missing)))
    pose = left("cam_pose", 4)
    Rt = pose[:, :3, :3].transpose(1, 2)
    E = torch.zeros_like(pose)
    E[:, :3, :3] = Rt
    E[:, :3, 3] = -(Rt @ pose[:, :3, 3:4])[..., 0]
    E[:, 3, 3] = 1.0
    vo = batch["vox_origin"]
    vo = torch.stack([torch.as_tensor(v) for v in vo]) if not torch.is_tensor(vo) else vo
    return left("cam_k", 3), E, vo.reshape(-1, 3).to(device=E.device, dtype=torch.float64)
