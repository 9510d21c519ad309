"""Cost of the depth-rendering loss (K36, csrc/render_loss.hip) on a config-2 frame: 256 x 256 x 32 voxels x 20 classes seen
through the 370 x 1220 KITTI camera, at strides 1, 2 and 4.  The scene is bench_visibility.py's synthetic street turned into
logits (6 on the labelled class plus unit noise); the depth map is the street's own rendered depth with 0.5 m of noise and
30 % of the pixels unmeasured.  It times

    opacity        occd_render_opacity (streaming, once per step whatever the stride)
    fwd            occd_render_depth_fwd          yardstick: K34 (occd_frame_visibility) on the same rays -- the same walk
                                                  with a byte load where this one gathers a float
    bwd rays       occd_render_depth_bwd_rays     yardstick: its own 8-byte integer atomics per second
    bwd voxels     occd_render_depth_bwd_voxels (streaming)
    torch          the package's torch formulation of the whole loss, forward + backward, at stride 4 (the A/B baseline; at
                   stride 1 its (rays, steps) tensors do not fit a sensible budget)

    python tools/bench_render_loss.py [--rounds 7] [--kernel-iters 50] [--out profiles/render_loss_ab.txt]

The training-step and forward-frame lines at the end of the committed profile are bench.py runs of the same session (fresh
processes of the parent commit and of this tree in turn), added by hand.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_map import C, DIMS, ORIGIN, VOXEL, interleaved  # noqa: E402
from bench_visibility import IMAGE_HW, street  # noqa: E402
from occdepth_amd import hip, render, visibility  # noqa: E402
from occdepth_amd.loss import render_loss as rl  # noqa: E402
from oracle import inputs  # noqa: E402

MAX_DEPTH = 54.0
EPS = 1e-3


def steps_per_ray(views, hw, stride, gt, dev):
    """Voxels visited per VALID ray, counted by the forward pass itself: with a constant opacity EPS the rendered opacity is
    1 - (1 - EPS)^n.  It is the number of atomics of a backward pass that skips nothing (zero terms and rays whose T reached
    an exact 0 do fewer)."""
    S = DIMS[0] * DIMS[1] * DIMS[2]
    op = torch.full((1, S), EPS, device=dev)
    _, alpha, stats = hip.render_depth_fwd(op, views, DIMS, hw, stride, (0, 0), MAX_DEPTH, gt, "abs")
    n = torch.round(torch.log1p(-alpha.double()) / math.log1p(-EPS))
    valid, _ = rl.RenderDepthLoss(stride=stride, max_depth=MAX_DEPTH).valid_rays(gt, views, DIMS)
    assert int(valid.sum()) == int(stats[1])
    return int(n[valid].sum()), int(valid.sum()), int(n.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=50, help="calls per window of the device-event timings")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "render_loss_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_loss.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    X, Y, Z = DIMS
    S = X * Y * Z
    H, W = IMAGE_HW
    labels = torch.from_numpy(street(DIMS)).to(dev)
    g = torch.Generator(device="cuda").manual_seed(0)
    lab = torch.where(labels == 255, torch.zeros_like(labels), labels).long()
    logits = torch.randn((1, C, X, Y, Z), device=dev, generator=g)
    logits.scatter_add_(1, lab[None, None], torch.full((1, 1, X, Y, Z), 6.0, device=dev))
    rows = torch.zeros((1, X, Y, Z, 24), device=dev)                        # the 3-D stack's channels-last rows, cs = 24
    rows[..., :C] = logits.permute(0, 2, 3, 4, 1)
    logits_cl = rows[..., :C].permute(0, 4, 1, 2, 3)
    k, E = torch.from_numpy(inputs.KITTI_K), torch.from_numpy(inputs.KITTI_TR)
    views = render.camera_view(k, E, ORIGIN, VOXEL).reshape(1, 18).to(dev).contiguous()
    palette = render.palette("kitti").to(dev)
    truth = hip.render_voxels(labels[None], views[:, None], IMAGE_HW, palette, aux=True)[3][0, 0]
    gt = torch.where(torch.isfinite(truth), truth + 0.5 * torch.randn(truth.shape, device=dev, generator=g), torch.zeros_like(truth))
    gt = torch.where(torch.rand(gt.shape, device=dev, generator=g) < 0.3, torch.zeros_like(gt), gt).clamp(min=0.0)[None, None].contiguous()

    opacity = hip.render_opacity(logits_cl)
    assert torch.equal(opacity, hip.render_opacity(logits))
    hsum = torch.zeros((1, S), dtype=torch.int64, device=dev)
    gscale = torch.full((1,), 1e-5, device=dev)
    lines = ["depth-rendering loss (K36), %d x %d x %d voxels x %d classes, the %d x %d KITTI camera, max_depth %.0f m;"
             % (X, Y, Z, C, H, W, MAX_DEPTH),
             "ms per call, median (min) over %d rounds of %d calls (device events; the variants alternate inside every round);"
             % (args.rounds, args.kernel_iters), "tools/bench_render_loss.py", ""]
    res = interleaved({"opacity_planes": lambda: hip.render_opacity(logits), "opacity_rows": lambda: hip.render_opacity(logits_cl)},
                      args.rounds, args.kernel_iters)
    gb = S * (4.0 * C + 4.0) / 1e9
    lines.append("occd_render_opacity          planes %8.4f (%.4f) ms = %.2f TB/s; channels-last rows (cs 24) %8.4f (%.4f) ms"
                 % (res["opacity_planes"] + (gb / res["opacity_planes"][0],) + res["opacity_rows"]))
    result = {"opacity_ms": round(res["opacity_rows"][0], 5), "strides": {}}
    for stride in (1, 2, 4):
        h, w = hip.render_loss_rays(IMAGE_HW, stride)
        depth, alpha, stats = hip.render_depth_fwd(opacity, views, DIMS, IMAGE_HW, stride, (0, 0), MAX_DEPTH, gt, "abs")
        vview, vsize = visibility.camera_rays(k, E, ORIGIN, VOXEL, IMAGE_HW, scale=1.0 / stride)
        vview = vview.to(dev).contiguous()

        def bwd_rays():
            hip.render_depth_bwd_rays(opacity, views, DIMS, IMAGE_HW, stride, (0, 0), MAX_DEPTH, gt, "abs", depth, hsum)

        def bwd_voxels():
            hip.render_depth_bwd_voxels(logits_cl, hsum, gscale)

        def bwd_both():
            bwd_rays()
            bwd_voxels()

        # `rays` alone keeps adding into H (the wrap of a 64-bit sum costs nothing and changes no address); `bwd` is the pair
        # as a step runs it, the voxel pass on the H the ray pass left
        res = interleaved({"fwd": lambda: hip.render_depth_fwd(opacity, views, DIMS, IMAGE_HW, stride, (0, 0), MAX_DEPTH, gt, "abs"),
                           "k34": lambda: hip.frame_visibility(labels, vview, vsize),
                           "bwd": bwd_both, "rays": bwd_rays}, args.rounds, args.kernel_iters)
        hsum.zero_()
        rays_ms = res["rays"][0]
        atomics, n_valid, visited = steps_per_ray(views, IMAGE_HW, stride, gt, dev)
        lines.append("stride %d: %d x %d = %d rays, %d valid (%.1f voxels visited per valid ray, %.1f per ray)"
                     % (stride, h, w, h * w, n_valid, atomics / max(1, n_valid), visited / (h * w)))
        lines.append("  occd_render_depth_fwd        %8.4f (%.4f) ms; K34 on the same rays %.4f (%.4f) ms: %.2fx"
                     % (res["fwd"] + res["k34"] + (res["fwd"][0] / res["k34"][0],)))
        lines.append("  occd_render_depth_bwd_rays   %8.4f (%.4f) ms; with occd_render_depth_bwd_voxels behind it %.4f (%.4f) ms:"
                     % (res["rays"] + res["bwd"]))
        lines.append("    at most %.2f M 8-byte integer atomics = %.1f MB: %.3f TB/s of added bytes, %.2f G atomics/s"
                     % (atomics / 1e6, atomics * 8 / 1e6, atomics * 8 / 1e9 / rays_ms, atomics / 1e6 / rays_ms))
        result["strides"][stride] = {"fwd_ms": round(res["fwd"][0], 5), "k34_ms": round(res["k34"][0], 5),
                                     "bwd_ms": round(res["bwd"][0], 5), "bwd_rays_ms": round(res["rays"][0], 5),
                                     "atomics": atomics, "valid": n_valid}
    # the whole loss, forward + backward, kernels against the torch formulation
    fn = rl.RenderDepthLoss(stride=4, max_depth=MAX_DEPTH)
    leaf = rows.clone().requires_grad_(True)

    def hip_loss():
        leaf.grad = None
        fn(leaf[..., :C].permute(0, 4, 1, 2, 3), gt, views).backward()

    def torch_loss():
        leaf.grad = None
        rl.render_loss_torch(leaf[..., :C].permute(0, 4, 1, 2, 3), gt, views, 4, (0, 0), MAX_DEPTH, "abs")[0].backward()

    whole = interleaved({"hip": hip_loss}, args.rounds, 10)["hip"]
    by_torch = interleaved({"torch": torch_loss}, 3, 1)["torch"]
    hip_loss()
    g_hip = leaf.grad.clone()
    l_hip = float(fn(leaf[..., :C].permute(0, 4, 1, 2, 3), gt, views))
    torch_loss()
    l_torch = float(rl.render_loss_torch(leaf[..., :C].permute(0, 4, 1, 2, 3), gt, views, 4, (0, 0), MAX_DEPTH, "abs")[0])
    diff = float((g_hip - leaf.grad).abs().max() / leaf.grad.abs().max())
    lines.append("")
    lines.append("the whole loss at stride 4, forward + backward through autograd (host enqueue included):")
    lines.append("  kernels %8.4f (%.4f) ms; torch formulation %8.2f (%.2f) ms (%.0fx); loss %.6f / %.6f, gradient max|delta| / max %.2e"
                 % (whole + by_torch + (by_torch[0] / whole[0], l_hip, l_torch, diff)))
    lines.append("")
    lines.append("the effect of the rendering loss on mIoU or RayIoU is not measured: no checkpoint and no dataset where this was run.")
    result.update(whole_ms=round(whole[0], 4), torch_ms=round(by_torch[0], 2))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
