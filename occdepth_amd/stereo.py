"""Stereo depth targets from the batch's rectified image pair, matched on the GPU (csrc/stereo.hip).

The benched configuration (`trans_2d_to_3d="flosp_depth"`, `use_stereo_depth_gt=True`) supervises its depth
distribution with a per-frame `gt_depth` map that the reference loads from 16-bit PNGs (kitti_dataset.py:40-44,
:338-348) written by a stereo network it does not ship.  This module builds that map from what every batch already
holds -- the image pair and its calibration -- with a classical matcher:

    census 9 x 7  ->  Hamming cost  ->  semi-global matching over the four axis-aligned paths (P1, P2)
    ->  winner-take-all  ->  uniqueness, left-right and inner checks  ->  parabola sub-pixel fit  ->  depth = f B / d

Everything up to the sub-pixel fit is integer arithmetic; the full specification is the comment above `OccdStereoArgs`
in include/occdepth_amd.h and its executable form is the numpy restatement in tests/test_stereo.py, which the kernels
match bit for bit.  NOT built: diagonal paths, median or speckle filtering, an adaptive P2.

    depth = stereo_depth(batch_img, cam_k, cam_E, ida)           # (B, 1, H, W) float32, 0 = no measurement
    disp, (S, d0, flags) = sgm_disparity(gray_pair, 64, return_aux=True)

All functions take GPU tensors, launch on the current stream, read nothing back and allocate their workspace per call:
they are safe inside a captured step.
"""
import struct
import zlib

import numpy as np
import torch

from . import hip

IMAGENET_MEAN = (0.485, 0.456, 0.406)      # the loader's normalisation (kitti_dataset.py:64-68)
IMAGENET_STD = (0.229, 0.224, 0.225)
MAX_DISP = 192                             # f B ~ 382 px m on KITTI: 192 px reaches the 2 m near bound of the depth axis
P1, P2, UNIQUENESS = 10, 120, 95
FLAG_UNIQUE, FLAG_CONSISTENT, FLAG_INNER = 1, 2, 4
DEPTH_PNG_SCALE = 256.0                    # load_depth: metres = png / 256, 0 = invalid


def _on_gpu(t, name):
    """`t` itself when it is a GPU tensor; a clear error otherwise (there is no CPU path)."""
    if not torch.is_tensor(t):
        raise TypeError(f"{name} must be a torch tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is a CPU tensor: the stereo matcher runs on the GPU only (csrc/stereo.hip has no CPU "
                           "path); move the batch to the device first")
    return t


def gray_from_normalized(img, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """img (B, 2, 3, H, W) float32, normalised as the loader does ((u / 255 - mean) / std) -> (B, 2, H, W) uint8:
    u_c = clamp(rint((x_c std_c + mean_c) 255), 0, 255), g = (77 u_R + 150 u_G + 29 u_B + 128) >> 8."""
    img = _on_gpu(img, "img")
    if img.dim() != 5 or img.shape[1] != 2 or img.shape[2] != 3:
        raise ValueError("img must be (B, 2, 3, H, W): a stereo pair of RGB images, got %s" % (tuple(img.shape),))
    return hip.stereo_census(img=img.float().contiguous(), mean=mean, std=std)[0]


def _gray_on_gpu(gray):
    gray = _on_gpu(gray, "gray")
    if gray.dim() == 3:
        gray = gray[None]
    if gray.dim() != 4 or gray.shape[1] != 2 or gray.dtype != torch.uint8:
        raise ValueError("a gray pair must be uint8 (B, 2, H, W) or (2, H, W), got %s %s" % (tuple(gray.shape), gray.dtype))
    return gray.contiguous()


def census(gray):
    """gray (B, 2, H, W) uint8 -> (B, 2, H, W) int64: the 9 x 7 census words (bit k: neighbour k < centre)."""
    return hip.stereo_census(gray=_gray_on_gpu(gray))[1]


def _direction_mats(flipped, B, device):
    """`flipped` -> the (B, V, 4, 4) float32 matrices whose [b, 0, 0, 0] sign the kernels read, or None."""
    if flipped is None:
        return None
    f = torch.as_tensor(flipped)
    if f.dim() == 4:                                   # the batch's ida_mats themselves
        return f.to(device=device, dtype=torch.float32).contiguous()
    if f.dim() == 0:
        f = f.expand(B)
    if f.dim() != 1 or f.shape[0] != B:
        raise ValueError("flipped must be None, one flag, (B,) flags or (B, V, 4, 4) ida matrices, got %s" % (tuple(f.shape),))
    sign = 1.0 - 2.0 * f.to(device=device).to(torch.float32)          # device ops only: no host read
    return sign.reshape(B, 1, 1, 1).expand(B, 1, 4, 4).contiguous()


def _match(census_words, max_disp, flipped, p1, p2, uniqueness):
    B = int(census_words.shape[0])
    return hip.stereo_sgm(census_words, max_disp=max_disp, ida=_direction_mats(flipped, B, census_words.device),
                          p1=p1, p2=p2, uniqueness=uniqueness)


def sgm_disparity(gray_pair, max_disp=MAX_DISP, flipped=None, p1=P1, p2=P2, uniqueness=UNIQUENESS, return_aux=False):
    """gray_pair (B, 2, H, W) uint8 ([:, 0] the left image) -> disparity (B, H, W) float32, 0 where a pixel fails one of
    the three checks.  max_disp: a multiple of 64 in 64..256.  flipped: None, (B,) booleans or the batch's (B, V, 4, 4)
    ida matrices -- a flipped frame (both images mirrored by the loader) matches x + d instead of x - d.  return_aux: also
    (S (B, H, W, D) int16 summed path costs, d0 (B, H, W) int32 winners, flags (B, H, W) uint8: 1 unique | 2 consistent |
    4 inner)."""
    words = hip.stereo_census(gray=_gray_on_gpu(gray_pair))[1]
    S, d0, flags, disp = _match(words, max_disp, flipped, p1, p2, uniqueness)
    return (disp, (S, d0, flags)) if return_aux else disp


def _calibration(cam_k, cam_E, device):
    def stack(t, n, name):
        if isinstance(t, (list, tuple)):
            t = torch.stack([torch.as_tensor(e).to(device) for e in t])
        t = torch.as_tensor(t).to(device=device, dtype=torch.float64)
        if t.dim() == 3:
            t = t[None]
        if t.dim() != 4 or t.shape[1] < 2 or tuple(t.shape[2:]) != (n, n):
            raise ValueError("%s must be (B, V, %d, %d) with the two cameras of the pair as views 0 and 1, got %s"
                             % (name, n, n, tuple(t.shape)))
        return t.contiguous()
    return stack(cam_k, 3, "cam_k"), stack(cam_E, 4, "cam_E")


def stereo_depth(img_or_gray, cam_k, cam_E, ida=None, max_disp=MAX_DISP, p1=P1, p2=P2, uniqueness=UNIQUENESS,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The left camera's depth map of a rectified pair -> (B, 1, H, W) float32 metres, 0 = no measurement: the shape and
    conventions of the batch's `gt_depth` under use_stereo_depth_gt (`load_depth`).

    img_or_gray: (B, 2, 3, H, W) float images normalised with mean / std, or a (B, 2, H, W) uint8 gray pair.  cam_k
    (B, V, 3, 3) and cam_E (B, V, 4, 4) (world -> camera), tensors or per-sample lists: depth = fB / disparity with
    fB = float32(cam_k[b, 0, 0, 0] * |t_0 - t_1|), t_v the translation column of cam_E[b, v], computed in float64 on the
    device.  ASSUMES view 0 is the left camera of a rectified pair.  ida: the batch's (B, V, 4, 4) ida_mats (a frame with
    ida[b, 0, 0, 0] < 0 was mirrored by the loader) or None."""
    t = _on_gpu(img_or_gray, "img")
    if t.dtype == torch.uint8:
        gray = _gray_on_gpu(t)
        words = hip.stereo_census(gray=gray)[1]
    else:
        if t.dim() != 5 or t.shape[1] != 2 or t.shape[2] != 3:
            raise ValueError("img must be a (B, 2, 3, H, W) float stereo pair or a (B, 2, H, W) uint8 gray pair, got %s %s"
                             % (tuple(t.shape), t.dtype))
        words = hip.stereo_census(img=t.float().contiguous(), mean=mean, std=std)[1]
    B = int(words.shape[0])
    k, E = _calibration(cam_k, cam_E, words.device)
    if k.shape[0] != B or E.shape[0] != B or k.shape[1] != E.shape[1]:
        raise ValueError("calibration of %d / %d frames and %d / %d views for %d image pairs"
                         % (k.shape[0], E.shape[0], k.shape[1], E.shape[1], B))
    if ida is not None and isinstance(ida, (list, tuple)):
        ida = torch.stack([torch.as_tensor(m).to(words.device) for m in ida])
    disp = _match(words, max_disp, ida, p1, p2, uniqueness)[3]
    return hip.stereo_depth(disp, k, E).unsqueeze(1)


# ----------------------------------------------------------------------------------------------- host side: PNG files
def focal_baseline(cam_k, cam_E):
    """float32(f B) of a calibration on the host (numpy): cam_k (V, 3, 3), cam_E (V, 4, 4) -- the value the depth kernel
    computes on the device."""
    k = np.asarray(cam_k, dtype=np.float64)
    E = np.asarray(cam_E, dtype=np.float64)
    t = E[0, :3, 3] - E[1, :3, 3]
    return np.float32(k[0, 0, 0] * np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]))


def depth_to_png16(depth):
    """depth (H, W) float metres -> uint16 round(depth * 256), 0 = invalid (also for non-finite and negative values),
    clipped to 65535: what `load_depth` divides by 256."""
    d = np.asarray(depth, dtype=np.float64)
    q = np.rint(np.where(np.isfinite(d) & (d > 0), d, 0.0) * DEPTH_PNG_SCALE)
    return np.clip(q, 0, 65535).astype(np.uint16)


def write_png16(path, image):
    """(H, W) uint16 -> a 16-bit grayscale PNG (filter 0 on every row; zlib and struct only)."""
    a = np.asarray(image)
    if a.dtype != np.uint16 or a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png16 takes a non-empty uint16 (H, W) image, got %s %s" % (a.shape, a.dtype))
    H, W = a.shape
    rows = np.zeros((H, 1 + 2 * W), dtype=np.uint8)
    rows[:, 1:] = a.astype(">u2").view(np.uint8).reshape(H, 2 * W)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 16, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))
    return path
