"""Which voxels of a frame the camera could see (K34, csrc/visibility.hip), and the vote weights made from that.

A scene-completion network predicts the surfaces the camera saw with the free space in front of them, and whatever it
guessed behind them.  The sequence map (semantic_map.py) can weight a frame's vote by which of the two a voxel is:

    view, size = camera_rays(cam_k, T_velo_2_cam, vox_origin, 0.2, (370, 1220))
    visible = visible_voxels(labels, view, size)                      # (X, Y, Z) uint8 on the GPU, one launch pair
    weight = vote_weights(visible, fov_mask, w_visible=4, w_hidden=1)   # uint8, 0 outside the mask
    m.integrate(labels, pose, weight=weight)
    m.sample(pose, own=labels, own_weight=weight, exclude_self=True)

Visibility is pixel-centric: the camera's own pixel rays carve the volume, and a voxel is visible when some ray reaches
it before (or as) its first occupied voxel.  The voxel-centric rule (is the ray to the voxel's centre free?) hides nearly
all distant ground: at 40 m the ray to the centre of a road voxel enters the ground layer metres earlier.  The effect of
any weighting on mIoU is not measured (no checkpoint and no dataset where this was built).
"""
import math

import torch

from . import hip, render


def camera_rays(cam_k, T_velo_2_cam, vox_origin, voxel_size, image_hw, scale=1.0):
    """The pixel rays of the (left) camera as one view -> (view (..., 18) float32, (h, w)).  cam_k (..., 3, 3),
    T_velo_2_cam (..., 4, 4) and vox_origin as render.camera_view takes them; image_hw = (H, W) of the camera image.
    scale: rays per pixel along each image axis -- the same frustum cut into h = ceil(H scale), w = ceil(W scale) rays
    (pixel centres map to pixel centres: fx' = s fx, cx' = s (cx + 1/2) - 1/2).  1.0 is the camera itself."""
    s = float(scale)
    if not s > 0.0:
        raise ValueError("scale must be positive, got %r" % (scale,))
    H, W = int(image_hw[0]), int(image_hw[1])
    if H < 1 or W < 1:
        raise ValueError("image_hw must be (H, W) >= 1, got %r" % (image_hw,))
    k = torch.as_tensor(cam_k).to(torch.float64)
    if s != 1.0:
        k = k.clone()
        k[..., 0, 0] *= s
        k[..., 1, 1] *= s
        k[..., 0, 2] = s * (k[..., 0, 2] + 0.5) - 0.5
        k[..., 1, 2] = s * (k[..., 1, 2] + 0.5) - 0.5
    return render.camera_view(k, T_velo_2_cam, vox_origin, voxel_size), (int(math.ceil(H * s)), int(math.ceil(W * s)))


def visible_voxels(labels, view, size):
    """labels (X, Y, Z) on the GPU (uint8 / int16 / uint16 read in place, wider integers narrowed), view (18,), size =
    (h, w) -> (X, Y, Z) uint8: 1 where a pixel ray reaches the voxel, up to and including its first occupied voxel
    (0 < label < 255).  One fill and one ray launch (hip.frame_visibility); no host synchronisation."""
    if labels.dim() != 3:
        raise ValueError("visible_voxels takes one (X, Y, Z) label volume, got %r" % (tuple(labels.shape),))
    if labels.dtype not in (torch.uint8, torch.int16, getattr(torch, "uint16", torch.int16)):
        labels = labels.to(torch.int16)
    view = torch.as_tensor(view).reshape(-1)
    if view.numel() != 18:
        raise ValueError("visible_voxels takes one (18,) view, got %d numbers" % view.numel())
    view = view.to(device=labels.device, dtype=torch.float32).contiguous()
    return hip.frame_visibility(labels.contiguous(), view, size)


def check_weights(w_visible, w_hidden):
    """-> (w_visible, w_hidden) as ints: 0..255 each, w_visible >= 1 (the voxels the camera saw always vote)."""
    wv, wh = int(w_visible), int(w_hidden)
    if wv != w_visible or wh != w_hidden or not (1 <= wv <= 255 and 0 <= wh <= 255):
        raise ValueError("vote weights are integers with 1 <= w_visible <= 255 and 0 <= w_hidden <= 255, got %r, %r"
                         % (w_visible, w_hidden))
    return wv, wh


def vote_weights(visible, mask, w_visible, w_hidden):
    """visible (X, Y, Z) uint8 / bool, mask the frame's own (X Y Z) bool / uint8 table or None -> (X, Y, Z) uint8:
    w_visible where visible, w_hidden elsewhere, 0 outside the mask (what SemanticMap.integrate takes as `weight`)."""
    wv, wh = check_weights(w_visible, w_hidden)
    w = torch.where(visible != 0, torch.full_like(visible, wv, dtype=torch.uint8), torch.full_like(visible, wh, dtype=torch.uint8))
    if mask is not None:
        mask = torch.as_tensor(mask)
        if mask.numel() != visible.numel():
            raise ValueError("mask must hold X Y Z = %d entries, got %r" % (visible.numel(), tuple(mask.shape)))
        w = w * (mask.to(visible.device).reshape(visible.shape) != 0).to(torch.uint8)
    return w.contiguous()
