"""Time occd_render_voxels (render.render_labels) on a config-2 frame: a 256 x 256 x 32 uint16 label volume to the
1220 x 370 camera view, to a 512 x 512 BEV, and to both in one launch.  Device events after warm-up, many launches per
window.  Two volumes: a synthetic street scene (ground, walls, clutter) and an EMPTY volume, the worst case, in which
every ray walks the whole grid.  Prints one JSON line; set it beside the forward time bench.py reports for the same frame.

    python tools/bench_render.py [--iters 200] [--warmup 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import hip, render  # noqa: E402
from oracle import inputs  # noqa: E402

DIMS, ORIGIN, VOXEL = (256, 256, 32), (0.0, -25.6, -2.0), 0.2
CAMERA_HW, BEV_PPV = (370, 1220), 2


def street(dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    vol = torch.zeros(DIMS, dtype=torch.int16)
    vol[:, :, :9] = 9                                           # road surface below the sensor
    vol[:, :96, 9:20] = 13                                      # building fronts on both sides
    vol[:, 160:, 9:24] = 15
    clutter = torch.rand(DIMS, generator=g) < 0.01
    vol[clutter] = torch.randint(1, 20, (int(clutter.sum()),), generator=g).to(torch.int16)
    vol[:12, 116:140, 9:] = 0                                   # free space around the camera
    return vol[None].contiguous().to(dev)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda")
    cam = render.camera_view(torch.from_numpy(inputs.KITTI_K), torch.from_numpy(inputs.KITTI_TR), ORIGIN, VOXEL).to(dev)
    bev = render.bev_view(DIMS, BEV_PPV, device=dev)
    bev_hw = render.bev_size(DIMS, BEV_PPV)
    out = {"volume": "256x256x32 uint16, B=1", "camera": "%dx%d" % CAMERA_HW[::-1], "bev": "%dx%d" % bev_hw[::-1], "ms": {}}
    for name, vol in (("street", street(dev)), ("empty", torch.zeros((1,) + DIMS, dtype=torch.int16, device=dev))):
        cases = {"camera": ([cam], [CAMERA_HW]), "bev": ([bev], [bev_hw]), "both": ([cam, bev], [CAMERA_HW, bev_hw])}
        row = {}
        pal = render.palette("kitti").to(dev)
        for case, (views, sizes) in cases.items():
            stacked = torch.stack(views)[None].contiguous()
            canvas = (max(s[0] for s in sizes), max(s[1] for s in sizes))
            row[case] = round(timed(lambda: hip.render_voxels(vol, stacked, canvas, pal, view_sizes=sizes), args.iters,
                                    args.warmup), 4)
        with hip.profile() as prof:
            imgs, hit, _, _ = render.render_labels(vol, [cam, bev], [CAMERA_HW, bev_hw], palette="kitti", return_aux=True)
        row["hit_share"] = [round(float((h >= 0).float().mean()), 3) for h in hit]
        row["profiled_both_aux"] = {k: {"ms": round(v["ms"], 4), "bytes": v["bytes"]} for k, v in prof.rows.items()}
        out["ms"][name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
