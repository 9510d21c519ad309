"""Depth-rendering loss (K36): the soft occupancy of `ssc_logit` is alpha-composited along the left camera's pixel rays into
an expected depth image, which is held to a metric depth map -- rendering supervision as in RenderOcc / SurroundOcc, the
training-side counterpart of the ray-wise metric (ray_metric.py).

    views = frame_views(cam_k, T_velo_2_cam, origin, 0.2, width=W, flip=ida[:, 0, 0, 0] < 0)     # (B, 18), no host read
    loss = RenderDepthLoss(stride=4, max_depth=51.2)(ssc_logit, gt_depth, views)
    depth, opacity = render_depth(ssc_logit, views, (H, W), stride=4)

With a = 1 - softmax(z)[0] per voxel, a ray visits voxels v_1 .. v_n at entry depths t_1 <= .. <= t_n (the renderer's walk,
ended at `max_depth`):  T_1 = 1, w_i = T_i a_i, T_{i+1} = T_i (1 - a_i),  d^ = sum w_i t_i + T_{n+1} t_end,  t_end =
min(slab exit, max_depth).  A ray is valid when it meets the grid and its measurement D is finite, 0 < D <= max_depth and
behind the grid's entry; its target is D_r = min(D, t_end) and its loss omega_r |d^ - D_r| with omega_r = 1 ("abs") or
1 / max(D_r, REL_FLOOR) ("rel");  L = sum / max(1, #valid).  There is no path-length weighting: a clipped corner counts like
a full crossing.  The specification is in include/occdepth_amd.h (K36); GPU float32 logits run on csrc/render_loss.hip
(`hip.render_*`; a missing library is an error), everything else -- CPU tensors, other dtypes -- on the torch formulation below, which
walks in float32 and composites in the logits' dtype under autograd.
"""
import torch

from .. import hip

REL_FLOOR = 0.25        # metres: bounds omega, and with it the kernels' fixed-point sums
Q24 = 16777216.0


# ------------------------------------------------------------------------------------------------------------- views
def frame_views(cam_k, T_velo_2_cam, vox_origin, voxel_size, width=None, flip=None):
    """One camera view per frame -> (B, 18) float32 on the calibration's device (render.camera_view; t = camera depth in
    metres).  flip: a (B,) bool DEVICE tensor (the loader's mirror flag, ida_mats[b, 0, 0, 0] < 0) -- mirrored frames get
    the mirrored view (d0 + W du, -du) of the image of `width` pixels, chosen with torch.where: no host read."""
    from .. import render
    plain = render.camera_view(cam_k, T_velo_2_cam, vox_origin, voxel_size)
    if flip is None:
        return plain
    if width is None:
        raise ValueError("frame_views(flip=...) needs the image width")
    mirrored = render.camera_view(cam_k, T_velo_2_cam, vox_origin, voxel_size, flip=True, width=width)
    return torch.where(flip.to(plain.device).reshape(-1, 1), mirrored, plain)


# ------------------------------------------------------------------------------------------- the torch formulation
def slab_rays(views, dims, image_hw, stride=1, offset=(0, 0), max_depth=hip.RENDER_LOSS_MAX_DEPTH):
    """Ray generation and slab test of csrc/render_loss.hip in float32, vectorised over the N = B h w rays (torch
    elementwise ops round once each, like the kernel's contract-off arithmetic; no host read).  views (B, 18) -> dict of
    t_entry, t_end (N,) f32, alive (N,) bool, shape (B, h, w), and the rays themselves (o, d, inv: three (N,) each)."""
    X, Y, Z = (int(d) for d in dims)
    h, w = hip.render_loss_rays(image_hw, stride, offset)
    g = views.detach().to(torch.float32)
    if g.dim() != 2 or g.shape[1] != 18:
        raise ValueError("views must be (B, 18), got %s" % (tuple(views.shape),))
    B, dev, f32 = g.shape[0], g.device, torch.float32
    s, ou, ov = int(stride), int(offset[0]), int(offset[1])
    fu = (ou + s * torch.arange(w, device=dev)).to(f32) + 0.5
    fv = (ov + s * torch.arange(h, device=dev)).to(f32) + 0.5
    fu = fu[None, None, :].expand(B, h, w).reshape(-1)
    fv = fv[None, :, None].expand(B, h, w).reshape(-1)
    g = g[:, None, :].expand(B, h * w, 18).reshape(-1, 18)
    o = [g[:, i] + fu * g[:, 3 + i] + fv * g[:, 6 + i] for i in range(3)]
    d = [g[:, 9 + i] + fu * g[:, 12 + i] + fv * g[:, 15 + i] for i in range(3)]
    N = fu.numel()
    inf = torch.full((N,), float("inf"), dtype=f32, device=dev)
    zero = torch.zeros(N, dtype=f32, device=dev)
    md = torch.full((N,), float(max_depth), dtype=f32, device=dev)
    alive = torch.ones(N, dtype=torch.bool, device=dev)
    for c in o + d:
        alive &= torch.isfinite(c)
    tn, tf = -inf, inf
    inv, ext = [], [float(X), float(Y), float(Z)]
    for i in range(3):
        nz = d[i] != 0
        r = torch.where(nz, 1.0 / torch.where(nz, d[i], inf), zero)
        inv.append(r)
        a, c = (0.0 - o[i]) * r, (ext[i] - o[i]) * r
        lo, hi = torch.minimum(a, c), torch.maximum(a, c)
        tn = torch.where(nz & (lo > tn), lo, tn)
        tf = torch.where(nz, torch.minimum(tf, hi), tf)
        alive &= nz | ((o[i] >= 0) & (o[i] < ext[i]))
    t = torch.where(tn > 0, tn, zero)
    alive &= tf >= t
    return {"t_entry": t, "t_end": torch.where(alive, torch.minimum(tf, md), md), "alive": alive, "shape": (B, h, w),
            "o": o, "d": d, "inv": inv}


def walk_rays(views, dims, image_hw, stride=1, offset=(0, 0), max_depth=hip.RENDER_LOSS_MAX_DEPTH):
    """`slab_rays` and the walk behind it -> its dict (without the rays) plus
      index (N, K) int64  voxel b S + (x Y + y) Z + z of step k (0 where the step does not exist)
      t     (N, K) f32    entry depth of step k
      step  (N, K) bool   the step exists."""
    X, Y, Z = (int(d) for d in dims)
    rays = slab_rays(views, dims, image_hw, stride, offset, max_depth)
    o, d, inv, alive, t = rays.pop("o"), rays.pop("d"), rays.pop("inv"), rays["alive"], rays["t_entry"]
    B, h, w = rays["shape"]
    N, dev, f32 = t.numel(), t.device, torch.float32
    ext = [float(X), float(Y), float(Z)]
    inf = torch.full((N,), float("inf"), dtype=f32, device=dev)
    zero = torch.zeros(N, dtype=f32, device=dev)
    md = torch.full((N,), float(max_depth), dtype=f32, device=dev)
    act = alive & (t < md)
    idx, sgn, m = [], [], []
    for i in range(3):
        first = torch.clamp(torch.floor(o[i] + d[i] * t), 0.0, ext[i] - 1.0)
        idx.append(torch.where(alive, first, zero).to(torch.int64))
        sgn.append((d[i] > 0).to(torch.int64) - (d[i] < 0).to(torch.int64))
    edge = lambda i: torch.where(sgn[i] != 0, ((idx[i] + (sgn[i] > 0)).to(f32) - o[i]) * inv[i], inf)
    m = [edge(i) for i in range(3)]
    lim = (X, Y, Z)
    frame = torch.arange(B, device=dev)[:, None].expand(B, h * w).reshape(-1) * (X * Y * Z)
    out_i, out_t, out_s = [], [], []
    for _ in range(X + Y + Z + 3):
        if not bool(act.any()):
            break
        vox = (idx[0] * Y + idx[1]) * Z + idx[2]
        out_i.append(torch.where(act, frame + vox, torch.zeros_like(vox)))
        out_t.append(t)
        out_s.append(act)
        ax = torch.where((m[0] <= m[1]) & (m[0] <= m[2]), 0, torch.where(m[1] <= m[2], 1, 2))
        mm = torch.where(ax == 0, m[0], torch.where(ax == 1, m[1], m[2]))
        act = act & (mm < md)
        for i in range(3):
            move = act & (ax == i)
            idx[i] = torch.where(move, idx[i] + sgn[i], idx[i])
            inside = (idx[i] >= 0) & (idx[i] < lim[i])
            act = act & (inside | ~move)
            idx[i] = idx[i].clamp(0, lim[i] - 1)
            m[i] = torch.where(move, edge(i), m[i])
        t = torch.where(act, mm, t)
    if not out_i:
        out_i, out_t, out_s = [torch.zeros(N, dtype=torch.int64, device=dev)], [zero], [torch.zeros_like(alive)]
    rays.update(index=torch.stack(out_i, 1), t=torch.stack(out_t, 1), step=torch.stack(out_s, 1))
    return rays


def opacity_of(logits):
    """a = 1 - softmax(logits, 1)[:, 0], formed as the sum of the other classes (no cancellation when p_0 -> 1)."""
    return torch.softmax(logits, 1)[:, 1:].sum(1).clamp(max=1.0)


def _composite(logits, walk):
    """-> (d^ (N,), rendered opacity (N,)) in the logits' dtype, differentiable."""
    dt = logits.dtype
    a = opacity_of(logits).reshape(-1)
    ag = a[walk["index"]] * walk["step"].to(dt)                    # a step that does not exist is transparent
    trans = torch.cumprod(1.0 - ag, 1)                             # T_{k+1}
    before = torch.cat([torch.ones_like(trans[:, :1]), trans[:, :-1]], 1)
    depth = (before * ag * walk["t"].to(dt)).sum(1) + trans[:, -1] * walk["t_end"].to(dt)
    return depth, 1.0 - trans[:, -1]


def _targets(walk, gt_depth, stride, offset, max_depth, norm, dt):
    """-> (valid (N,) bool, D_r (N,), omega (N,)) of the rays' pixels of gt_depth (B, 1, H, W) / (B, H, W)."""
    D = gt_depth[:, 0] if gt_depth.dim() == 4 else gt_depth
    D = D[:, int(offset[1])::int(stride), int(offset[0])::int(stride)].to(torch.float32).reshape(-1)
    valid = walk["alive"] & torch.isfinite(D) & (D > 0) & (D <= float(max_depth)) & (D > walk["t_entry"])
    Dr = torch.minimum(torch.where(valid, D, torch.ones_like(D)), walk["t_end"]).to(dt)
    omega = torch.ones_like(Dr) if norm == "abs" else 1.0 / Dr.clamp(min=REL_FLOOR)
    return valid, Dr, omega


def _check_norm(norm):
    if norm not in hip.RENDER_LOSS_NORMS:
        raise ValueError("norm must be 'abs' or 'rel', got %r" % (norm,))


def render_loss_torch(logits, gt_depth, views, stride=1, offset=(0, 0), max_depth=hip.RENDER_LOSS_MAX_DEPTH, norm="abs"):
    """The torch formulation: -> (loss, d^ (B, h, w), rendered opacity (B, h, w), #valid rays); differentiable in logits."""
    _check_norm(norm)
    H, W = gt_depth.shape[-2:]
    walk = walk_rays(views.to(logits.device), logits.shape[2:], (H, W), stride, offset, max_depth)
    depth, alpha = _composite(logits, walk)
    valid, Dr, omega = _targets(walk, gt_depth.to(logits.device), stride, offset, max_depth, norm, logits.dtype)
    n_valid = valid.sum()
    per_ray = omega * (depth - Dr).abs() * valid.to(logits.dtype)
    loss = per_ray.sum() / n_valid.clamp(min=1).to(logits.dtype)
    return loss, depth.reshape(walk["shape"]), alpha.reshape(walk["shape"]), n_valid


# ----------------------------------------------------------------------------------------------------- the HIP path
_hsum = {}


def _hsum_buffer(B, S, device):
    """H (B, S) int64: zeroed once here, left clean by every backward (occd_render_depth_bwd_voxels stores the zeros back)."""
    key = (int(B), int(S), str(device))
    buf = _hsum.get(key)
    if buf is None:
        buf = _hsum[key] = torch.zeros((B, S), dtype=torch.int64, device=device)
    return buf


class _RenderDepth(torch.autograd.Function):
    """Opacity pass, forward ray pass; backward ray pass, voxel pass (csrc/render_loss.hip).  The `_DepthBCE` pattern: the
    mean's divisor and the incoming gradient stay on the device (gscale), no host read, capture-safe."""

    @staticmethod
    def forward(ctx, logits, gt_depth, views, stride, offset, max_depth, norm):
        dims = tuple(logits.shape[2:])
        H, W = gt_depth.shape[-2:]
        opacity = hip.render_opacity(logits)
        depth, alpha, stats = hip.render_depth_fwd(opacity, views, dims, (H, W), stride, offset, max_depth, gt_depth, norm)
        st = stats.double()
        valid = st[1].clamp(min=1.0)
        ctx.save_for_backward(logits, gt_depth, views, opacity, depth, valid)
        ctx.geom = (dims, (int(H), int(W)), stride, offset, max_depth, norm)
        ctx.mark_non_differentiable(depth, alpha, stats)
        return (st[0] / (Q24 * valid)).float(), depth, alpha, stats

    @staticmethod
    def backward(ctx, g, *unused):
        logits, gt_depth, views, opacity, depth, valid = ctx.saved_tensors
        dims, image_hw, stride, offset, max_depth, norm = ctx.geom
        hsum = _hsum_buffer(opacity.shape[0], opacity.shape[1], opacity.device)
        hip.render_depth_bwd_rays(opacity, views, dims, image_hw, stride, offset, max_depth, gt_depth, norm, depth, hsum)
        gscale = (g.double() / valid).float().reshape(1)
        return hip.render_depth_bwd_voxels(logits, hsum, gscale), None, None, None, None, None, None


def _device_views(views, logits):
    v = views.to(device=logits.device, dtype=torch.float32)
    if v.dim() == 1:
        v = v[None].expand(logits.shape[0], 18)
    if v.dim() != 2 or v.shape[0] != logits.shape[0] or v.shape[1] != 18:
        raise ValueError("views must be (18,) or (B, 18) with B = %d, got %s" % (logits.shape[0], tuple(views.shape)))
    return v.contiguous()


def render_depth(logits, views, depth_hw, stride=1, offset=(0, 0), max_depth=hip.RENDER_LOSS_MAX_DEPTH):
    """A soft depth image of a prediction: logits (B, C, X, Y, Z), views (B, 18) / (18,), the camera image's (H, W) ->
    (depth, opacity), both (B, h, w) (`hip.render_loss_rays`): the expected depth d^ along every ray and the ray's
    accumulated opacity.  GPU float32 logits go through the kernels (no autograd graph: images only, usable under no_grad);
    anything else through the torch formulation (differentiable)."""
    if logits.dim() != 5:
        raise ValueError("logits must be (B, C, X, Y, Z), got %s" % (tuple(logits.shape),))
    views = _device_views(views, logits)
    if hip.render_loss_usable(logits):
        with torch.no_grad():
            depth, alpha, _ = hip.render_depth_fwd(hip.render_opacity(logits), views, logits.shape[2:], depth_hw, stride, offset,
                                                   max_depth)
        return depth, alpha
    walk = walk_rays(views, logits.shape[2:], depth_hw, stride, offset, max_depth)
    depth, alpha = _composite(logits, walk)
    return depth.reshape(walk["shape"]), alpha.reshape(walk["shape"])


class RenderDepthLoss:
    """loss = RenderDepthLoss(stride, max_depth, norm)(logits, gt_depth, views): logits (B, C, X, Y, Z) (class 0 empty),
    gt_depth (B, 1, H, W) / (B, H, W) float32 metres (0 = no measurement), views (B, 18).  After a call, `last` holds the
    detached (d^, rendered opacity, #valid rays) of that call."""

    def __init__(self, stride=4, max_depth=hip.RENDER_LOSS_MAX_DEPTH, norm="abs", offset=(0, 0)):
        _check_norm(norm)
        self.stride, self.offset, self.max_depth, self.norm = int(stride), (int(offset[0]), int(offset[1])), float(max_depth), norm
        if not 0.0 < self.max_depth <= hip.RENDER_LOSS_MAX_DEPTH:
            raise ValueError("max_depth must lie in (0, %g], got %r" % (hip.RENDER_LOSS_MAX_DEPTH, max_depth))
        hip.render_loss_rays((self.offset[1] + 1, self.offset[0] + 1), self.stride, self.offset)      # stride / offset checks
        self.last = None

    def __call__(self, logits, gt_depth, views):
        if logits.dim() != 5:
            raise ValueError("logits must be (B, C, X, Y, Z), got %s" % (tuple(logits.shape),))
        views = _device_views(views, logits)
        gt_depth = gt_depth.to(logits.device)
        if hip.render_loss_usable(logits, gt_depth):
            loss, depth, alpha, stats = _RenderDepth.apply(logits, gt_depth.float(), views, self.stride, self.offset,
                                                           self.max_depth, self.norm)
            self.last = (depth, alpha, stats[1])
            return loss
        loss, depth, alpha, n_valid = render_loss_torch(logits, gt_depth, views, self.stride, self.offset, self.max_depth, self.norm)
        self.last = (depth.detach(), alpha.detach(), n_valid)
        return loss

    def valid_rays(self, gt_depth, views, dims):
        """(valid (B, h, w) bool, D_r (B, h, w)) of a call's rays: what the val metrics are taken over (torch, small images)."""
        H, W = gt_depth.shape[-2:]
        walk = slab_rays(views, dims, (H, W), self.stride, self.offset, self.max_depth)
        valid, Dr, _ = _targets(walk, gt_depth, self.stride, self.offset, self.max_depth, "abs", torch.float32)
        return valid.reshape(walk["shape"]), Dr.reshape(walk["shape"])

