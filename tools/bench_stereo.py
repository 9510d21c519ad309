"""Time the stereo matcher (occdepth_amd/stereo.py, csrc/stereo.hip) on one KITTI-sized frame: 370 x 1220, D = 192, B = 1.
Total time of `stereo_depth` from a normalised float image pair (device events after warm-up, many calls per window) and
the time of each kernel (the library's launch-time profiler, in a pass of its own), with the bytes each kernel moves as
computed from the shapes.  Prints one JSON line; set it beside the training step's time (tools/bench_train.py).

    python tools/bench_stereo.py [--iters 50] [--warmup 5] [--max-disp 192] [--hw 370 1220]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import hip, stereo, synthetic  # noqa: E402


def textured_pair(H, W, shift, dev):
    """A normalised float pair: smoothed noise, the right image shifted by `shift` pixels (a fronto-parallel wall)."""
    g = torch.Generator().manual_seed(0)
    tex = torch.rand(1, 1, H, W + shift, generator=g)
    tex = torch.nn.functional.avg_pool2d(tex, 3, 1, 1)
    u = ((tex - tex.min()) / (tex.max() - tex.min()) * 255.0).round()
    left, right = u[0, 0, :, :W], u[0, 0, :, shift:]            # right[x] = left[x + shift]: disparity `shift`
    rgb = torch.stack([left, right])[:, None].expand(2, 3, H, W) / 255.0
    mean = torch.tensor(stereo.IMAGENET_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(stereo.IMAGENET_STD).view(1, 3, 1, 1)
    return ((rgb - mean) / std)[None].contiguous().to(dev)


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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-disp", type=int, default=stereo.MAX_DISP)
    ap.add_argument("--hw", type=int, nargs=2, default=(370, 1220))
    args = ap.parse_args()
    dev = torch.device("cuda")
    H, W = args.hw
    D = args.max_disp
    img = textured_pair(H, W, 20, dev)
    frame = synthetic.to_device(synthetic.kitti_frame(batch=1, img_hw=(8, 16)), dev)
    k, E = torch.stack(frame["cam_k"]), torch.stack(frame["T_velo_2_cam_f64"])
    run = lambda: stereo.stereo_depth(img, k, E, max_disp=D)
    depth = run()
    gray = stereo.gray_from_normalized(img)
    out = {"frame": "%dx%d, D=%d, B=1" % (W, H, D),
           "valid_share": round(float((depth > 0).float().mean()), 3),
           "median_disparity_of_valid": round(float(stereo.sgm_disparity(gray, D)[depth[:, 0] > 0].median()), 2),
           "stereo_depth_ms": round(timed(run, args.iters, args.warmup), 4),
           "sgm_from_gray_ms": round(timed(lambda: stereo.sgm_disparity(gray, D), args.iters, args.warmup), 4)}
    with hip.profile() as prof:
        for _ in range(args.iters):
            run()
        torch.cuda.synchronize()
    out["kernels"] = {name: {"ms": round(r["ms"] / max(r["launches"], 1), 4), "MB": round(r["bytes"] / max(r["launches"], 1) / 1e6, 1),
                             "GB_per_s": round(r["bytes"] / max(r["ms"], 1e-9) / 1e6, 1)}
                      for name, r in prof.rows.items() if name.startswith("stereo_")}
    out["kernel_sum_ms"] = round(sum(v["ms"] for v in out["kernels"].values()), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
