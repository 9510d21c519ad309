"""Time occd_vox2pix (hip.vox2pix: the reference dataset's voxel -> pixel tables, built on the GPU) at config 2: B=1,
stereo (V=2), 1220 x 370, at the project scale (128 x 128 x 16, 0.4 m) and, for reference, the output-scale grid
(256 x 256 x 32, 0.2 m).  Device events after warm-up.  Next to it the CPU time of oracle.inputs.vox2pix on the same
grids -- a NUMPY PROXY of the loader's work: the reference runs a numba kernel, and numba is not available to time it.
Also the bytes per sample the collate no longer carries when the loader's vox2pix is stubbed
(targets.defer_dataset_projection).  Prints one JSON line.

    python tools/bench_vox2pix.py [--iters 200] [--warmup 20] [--cpu-reps 3]

Per-kernel times: run it under `rocprofv3 --kernel-trace --stats -d out -- python tools/bench_vox2pix.py` (separately).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import hip  # noqa: E402
from oracle import inputs  # noqa: E402

GRIDS = {"project_scale_2": (0.4, (128, 128, 16)), "output_scale_1": (0.2, (256, 256, 32))}
ORIGIN, IMG_WH, SCENE = (0.0, -25.6, -2.0), (1220, 370), (51.2, 51.2, 6.4)


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
    ap.add_argument("--cpu-reps", type=int, default=3)
    args = ap.parse_args()
    dev = "cuda"
    tr2 = inputs.KITTI_TR.copy()
    tr2[0, 3] = -0.54
    E_np = np.stack([inputs.KITTI_TR, tr2])
    E = torch.from_numpy(E_np)[None].to(dev).contiguous()
    K = torch.from_numpy(np.stack([inputs.KITTI_K, inputs.KITTI_K]))[None].to(dev).contiguous()
    ida = torch.eye(4).repeat(1, 2, 1, 1).to(dev).contiguous()
    ida[0, 1, 0, 0] = -1.0                               # one flipped view: the flip is part of the timed work
    out = {"config": "B=1 V=2 1220x370, KITTI calibration", "grids": {}}
    shipped = 0
    for name, (vs, dims) in GRIDS.items():
        n = dims[0] * dims[1] * dims[2]
        ms = timed(lambda: hip.vox2pix(E, K, ida, ORIGIN, vs, dims, IMG_WH), args.iters, args.warmup)
        written = 2 * n * 17                             # (px, py) int64 + one fov byte per voxel and view
        t = []
        for _ in range(args.cpu_reps):
            t0 = time.perf_counter()
            for v in range(2):
                inputs.vox2pix(E_np[v], inputs.KITTI_K, ORIGIN, vs, IMG_WH[0], IMG_WH[1], SCENE, 0)
            t.append(time.perf_counter() - t0)
        # what the reference's collate ships per sample for this scale: projected_pix (V, N, 1, 2) int64 + fov_mask
        # (V, N, 1) bool (collate.py:20-23, 36-37; pix_z is not collated)
        carried = 2 * n * (16 + 1)
        shipped += carried
        out["grids"][name] = {"dims": list(dims), "voxel_m": vs, "gpu_ms": round(ms, 4), "bytes_written": written,
                              "GB_per_s": round(written / (ms * 1e-3) / 1e9, 1),
                              "cpu_numpy_proxy_ms": round(1e3 * min(t), 1), "collate_bytes_per_sample": carried}
    out["collate_bytes_per_sample_saved"] = shipped
    print(json.dumps(out))


if __name__ == "__main__":
    main()
