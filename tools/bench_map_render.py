"""Cost of drawing the sequence map (render.render_map, K31 csrc/map_render.hip) on the map of tools/bench_map.py: a
200-frame straight drive at a 45 degree heading, 1 m per frame, 256 x 256 x 32 voxel frames.  Two label sets: bench_map's
(uniform classes, 10 % of the voxels 255 -- a solid block to every ray) and a scene (a ground slab, 2 % clutter above
it, the rest empty -- rays travel through present bricks before they hit).  It times, per view,

    BEV          the whole window from above at max_side 2048
    oblique      480 x 640
    camera       370 x 1220 through the left camera of frame 100, t_max 80 m (and without a limit)

and compares in the same session, the variants alternating inside every round:

    skip on / skip off     absent bricks left in one step, or walked voxel by voxel (flags bit 0)
    sparse / dense         occd_map_render against occd_render_voxels on the densified window (cropped by key_range until
                           it is below 2^31 voxels), whose images must be the same
    all of it against the forward frame, given --frame-ms

    python tools/bench_map_render.py [--frame-ms MS] [--rounds 7] [--iters 20] [--out profiles/map_render_ab.txt]

--frame-ms: the forward frame measured in the same session (1000 / the frames/s of bench.py --gpus 1 --steps 20
--warmup 5); without it the shares are left out.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import render, semantic_map as sm, synthetic  # noqa: E402
from tools.bench_map import C, DIMS, DRIVE_FRAMES, ORIGIN, VOXEL, pose, window_ms  # noqa: E402

CAMERA_FRAME, CAMERA_SIZE, T_MAX = 100, (370, 1220), 80.0
DENSE_LIMIT = 1 << 31


def interleaved(variants, rounds, iters):
    """{name: fn} -> {name: (median ms, min ms, max ms)}; every round runs each variant once, in turn."""
    for fn in variants.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            ms[name].append(window_ms(fn, iters))
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ms.items()}


def frame_labels(kind, dev):
    g = torch.Generator(device="cuda").manual_seed(0)
    if kind == "uniform":                                                 # tools/bench_map.py's
        labels = torch.randint(0, C, DIMS, device=dev, generator=g, dtype=torch.uint8)
        labels[torch.rand(DIMS, device=dev, generator=g) < 0.1] = 255
        return labels
    labels = torch.zeros(DIMS, dtype=torch.uint8, device=dev)            # a scene: ground, clutter, air
    labels[:, :, :8] = 9
    clutter = torch.rand(DIMS, device=dev, generator=g) < 0.02
    labels[clutter] = torch.randint(1, C, DIMS, device=dev, generator=g, dtype=torch.uint8)[clutter]
    return labels


def drive_volume(kind, dev):
    labels = frame_labels(kind, dev)
    m = sm.SemanticMap(C, VOXEL, ORIGIN, DIMS)
    for f in range(DRIVE_FRAMES):
        m.integrate(labels, pose(float(f)))
    vol = sm.MapVolume(m)
    key_range = None
    lo, hi = vol.key_min.copy(), vol.key_max.copy()
    while np.prod((hi - lo + 1) * 16, dtype=np.int64) >= DENSE_LIMIT:     # crop the longest axis about its middle
        a = int(np.argmax(hi - lo))
        q = (hi[a] - lo[a] + 1) // 4
        lo[a], hi[a] = lo[a] + q, hi[a] - q
        key_range = (lo.copy(), hi.copy())
    if key_range is not None:
        vol = sm.MapVolume(m, key_range=key_range)
    bricks = m.n_bricks
    m.release()
    return vol, bricks, key_range


def densified(vol):
    """The dense (16 Gx, 16 Gy, 16 Gz) uint8 volume of the window, absent bricks 255."""
    G = vol.grid
    dense = torch.full(G + (16, 16, 16), 255, dtype=torch.uint8, device=vol.labels.device)
    at = torch.from_numpy(vol.keys - vol.key_min).to(vol.labels.device)
    dense[at[:, 0], at[:, 1], at[:, 2]] = vol.labels.view(-1, 16, 16, 16)
    return dense.permute(0, 3, 1, 4, 2, 5).reshape(vol.dims).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="launches per window of the device-event timings")
    ap.add_argument("--frame-ms", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "map_render_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_render.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    share = (lambda ms: "  = %5.2f %% of the %.2f ms forward frame" % (100 * ms / args.frame_ms, args.frame_ms)) \
        if args.frame_ms else (lambda ms: "")
    lines = ["drawing the sequence map (occd_map_render, K31): the %d-frame straight drive of tools/bench_map.py, heading 45 degrees,"
             % DRIVE_FRAMES,
             "%d x %d x %d voxel frames x %d classes; ms per launch of one view, median (min .. max) over %d rounds of %d launches,"
             % (DIMS + (C, args.rounds, args.iters)),
             "device events, the variants of a view alternating inside every round; tools/bench_map_render.py", ""]
    result = {"frame_ms": args.frame_ms}
    cam_k, cam_E = torch.from_numpy(synthetic.KITTI_K), torch.from_numpy(synthetic.KITTI_TR)
    for kind in ("uniform", "scene"):
        vol, bricks, key_range = drive_volume(kind, dev)
        dense = densified(vol)
        pal = render.palette("kitti").to(dev)
        bev, bev_hw = render.map_bev_view(vol, 2048)
        views = {"bev": (bev, bev_hw, None),
                 "oblique": (render.map_oblique_view(vol, render.OBLIQUE_SIZE), render.OBLIQUE_SIZE, None),
                 "camera": (render.map_camera_view(cam_k, cam_E, pose(float(CAMERA_FRAME)), vol), CAMERA_SIZE, T_MAX)}
        occupied = float(((vol.labels > 0) & (vol.labels < 255)).float().mean())
        lines.append("%s labels: %d bricks in the map, %d rows (%.1f MB of labels), window %d x %d x %d bricks = %d cells, %.1f %% present,"
                     % ((kind, bricks, vol.n_rows, vol.n_rows * 4096 / 1e6) + vol.grid + (vol.cells.numel(),
                        100.0 * float((vol.cells >= 0).float().mean()))))
        lines.append("  %.1f %% of the voxels of the rows occupied; dense window %d x %d x %d = %.0f MB%s"
                     % ((100 * occupied,) + vol.dims + (dense.numel() / 1e6, "" if key_range is None else
                        ", cropped to the keys %s .. %s" % (key_range[0].tolist(), key_range[1].tolist()))))
        result[kind] = {"rows": vol.n_rows, "cells": vol.cells.numel(), "dense_MB": round(dense.numel() / 1e6, 1)}
        for name, (view, hw, t_max) in views.items():
            v1 = view[None].contiguous()
            variants = {"skip": lambda: render.render_map(vol, v1, hw, palette=pal, t_max=t_max),
                        "no_skip": lambda: render.render_map(vol, v1, hw, palette=pal, t_max=t_max, skip=False)}
            if t_max is not None:
                variants["skip_no_limit"] = lambda: render.render_map(vol, v1, hw, palette=pal)
            variants["dense"] = lambda: render.render_labels(dense, v1, hw, palette=pal)
            sparse = render.render_map(vol, v1, hw, palette=pal, return_aux=True)
            flat = render.render_map(vol, v1, hw, palette=pal, skip=False, return_aux=True)
            thick = render.render_labels(dense, v1, hw, palette=pal, return_aux=True)
            same = bool(torch.equal(sparse[0][0], thick[0][0, 0]) and torch.equal(sparse[2][0], thick[2][0, 0])
                        and torch.equal(sparse[3][0].view(torch.int32), thick[3][0, 0].view(torch.int32))
                        and all(torch.equal(a, b) for a, b in zip(sparse, flat)))
            hits = float((sparse[1] >= 0).float().mean())
            got = interleaved(variants, args.rounds, args.iters)
            lines.append("  %-8s %4d x %-4d  %5.1f %% of the pixels hit%s; images, faces and depth bits equal (skip, no skip, dense): %s"
                         % (name, hw[0], hw[1], 100 * hits, "" if t_max is None else " (no limit)", same))
            label = {"skip": "sparse, skip on" + ("" if t_max is None else ", t_max %g m" % t_max),
                     "no_skip": "sparse, skip off" + ("" if t_max is None else ", t_max %g m" % t_max),
                     "skip_no_limit": "sparse, skip on, no limit", "dense": "dense occd_render_voxels"}
            for key, ms in got.items():
                ratio = "" if key == "skip" else "  %.2fx skip on" % (ms[0] / got["skip"][0])
                lines.append("    %-32s %8.3f (%.3f .. %.3f) ms%s%s" % ((label[key],) + ms + (ratio, share(ms[0]))))
            result[kind][name] = {k: round(v[0], 4) for k, v in got.items()}
            result[kind][name]["same"] = same
        lines.append("")
        del dense, vol
    lines.append("no real sequence was drawn: no dataset and no checkpoint where this was run.  The effect on any score is nil by")
    lines.append("construction: drawing reads the maps and changes nothing.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
