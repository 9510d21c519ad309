"""Time the three training-target builders (occdepth_amd/targets.py) at config 2: B=1, stereo (V=2), 256 x 256 x 32,
1220 x 370, frustum_size 8 (F=64), 20 classes.  Device events after warm-up; prints one JSON line with the time per
builder and per sample, and the bytes each writes over its time.

    python tools/bench_targets.py [--iters 50] [--warmup 10]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -d out -- python tools/bench_targets.py` (separately).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import targets  # noqa: E402
from oracle import inputs  # noqa: E402


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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    target = torch.randint(0, 20, (1, 256, 256, 32), generator=g, dtype=torch.uint8)
    target[torch.rand(target.shape, generator=g) < 0.6] = 0
    target[torch.rand(target.shape, generator=g) < 0.2] = 255
    target = target.to(dev)
    tr2 = inputs.KITTI_TR.copy()
    tr2[0, 3] = -0.54
    E = torch.from_numpy(np.stack([inputs.KITTI_TR, tr2]))[None].to(dev)
    K = torch.from_numpy(np.stack([inputs.KITTI_K, inputs.KITTI_K]))[None].to(dev)
    geo = dict(vox_origin=(0.0, -25.6, -2.0), voxel_size=0.2, img_wh=(1220, 370), frustum_size=8, n_classes=20)
    t18 = targets.downsample_label(target, 8)
    res = {
        "frustum_targets": (timed(lambda: targets.frustum_targets(E, K, target, **geo), args.iters, args.warmup),
                            64 * target.numel() + 64 * 20 * 4 + target.numel()),
        "downsample_label": (timed(lambda: targets.downsample_label(target, 8), args.iters, args.warmup),
                             target.numel() + t18.numel()),
        "cp_mega_matrix": (timed(lambda: targets.cp_mega_matrix(t18), args.iters, args.warmup), 4 * 4096 * 512 + t18.numel()),
    }
    out = {k: {"ms": round(ms, 4), "bytes": b, "GB_per_s": round(b / (ms * 1e-3) / 1e9, 1)} for k, (ms, b) in res.items()}
    out["per_sample_ms"] = round(sum(ms for ms, _ in res.values()), 4)
    out["config"] = "B=1 V=2 256x256x32 1220x370 F=64 C=20"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
