"""Cost of the RayIoU pass (occd_ray_metric, K35) on a config-2 frame: 256 x 256 x 32 voxels x 20 classes, the default
direction fan of ray_metric.lidar_directions (64 beams x 900 azimuths = 57600 rays per origin).  The target is the synthetic
street of tools/bench_visibility.py (2 % of the voxels 255); the prediction is the target rolled one voxel along x with
255 -> 0 and 20 % of the occupied labels redrawn.  It times, alternating inside every round,

    tiled, K = 1       the default ray order (8 x 8 beam x azimuth blocks: a wave holds neighbouring rays), the sensor origin
    beam-major, K = 1  the same rays with tile=None: the A/B of the ray order
    tiled, K = 8       eight origins along a straight drive (ray_metric.trajectory_origins, 5 m apart)
    beam-major, K = 8

by device events over windows of back-to-back calls and by the library's own event pair around every launch, and checks
that both orders give the same counters.

    python tools/bench_ray_metric.py [--frame-ms MS] [--rounds 7] [--kernel-iters 100] [--out profiles/ray_metric_ab.txt]

--frame-ms: the forward frame measured in the same session (1000 / the frames/s of bench.py --gpus 1 --steps 20
--warmup 5); without it the shares are left out.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_map import C, DIMS, ORIGIN, VOXEL, interleaved  # noqa: E402
from bench_map_sample import per_launch_ms  # noqa: E402
from bench_visibility import street  # noqa: E402
from occdepth_amd import hip, ray_metric  # noqa: E402

THRESHOLDS_M = (1.0, 2.0, 4.0)
ORIGINS, ORIGIN_STEP_M = 8, 5.0


def prediction(target, seed=1):
    rng = np.random.RandomState(seed)
    p = np.roll(target, 1, axis=0)
    p[p == 255] = 0
    redraw = (p > 0) & (rng.rand(*p.shape) < 0.2)
    p[redraw] = rng.randint(1, C, size=int(redraw.sum()))
    return p


def drive_origins():
    poses = {f: np.eye(4) for f in range(ORIGINS)}
    for f in poses:
        poses[f] = poses[f].copy()
        poses[f][0, 3] = ORIGIN_STEP_M * f
    return ray_metric.trajectory_origins(poses, 0, ORIGINS, 1, ORIGIN, VOXEL, DIMS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=100, help="calls per window of the device-event timings")
    ap.add_argument("--frame-ms", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "ray_metric_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ray_metric.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    X, Y, Z = DIMS
    share = (lambda ms: "  = %.2f %% of the %.2f ms forward frame" % (100 * ms / args.frame_ms, args.frame_ms)) \
        if args.frame_ms else (lambda ms: "")
    street_np = street(DIMS)
    target = torch.from_numpy(street_np)[None].to(dev)
    pred = torch.from_numpy(prediction(street_np))[None].to(dev)
    dirs = {"tiled": ray_metric.lidar_directions().to(dev), "beam-major": ray_metric.lidar_directions(tile=None).to(dev)}
    N = int(dirs["tiled"].shape[0])
    origins = {1: ray_metric.sensor_origin(ORIGIN, VOXEL).reshape(1, 1, 3).to(dev), ORIGINS: drive_origins()[None].to(dev)}
    assert tuple(origins[ORIGINS].shape) == (1, ORIGINS, 3)
    thr = [float(np.float32(t / VOXEL)) for t in THRESHOLDS_M]
    size = hip.ray_metric_size(C, len(thr))
    scratch = torch.zeros(size, dtype=torch.int64, device=dev)

    def call(order, K, counts=scratch):
        return hip.ray_metric(pred, target, origins[K], dirs[order], counts, thr, C)

    counts = {}
    for K in origins:
        for order in dirs:
            counts[order, K] = call(order, K, torch.zeros(size, dtype=torch.int64, device=dev)).cpu()
    same = all(torch.equal(counts["tiled", K], counts["beam-major", K]) for K in origins)
    variants = {(order, K): (lambda order=order, K=K: call(order, K)) for K in origins for order in dirs}
    res = interleaved(variants, args.rounds, args.kernel_iters)
    alone = {key: per_launch_ms(fn, "ray_metric", args.kernel_iters) for key, fn in variants.items()}

    volume_bytes = 2.0 * X * Y * Z                                           # both volumes once, one byte per label
    lines = ["RayIoU pass (K35 occd_ray_metric), %d x %d x %d voxels x %d classes, %d rays per origin (64 beams x 900 azimuths), thresholds %s m;"
             % (X, Y, Z, C, N, "/".join("%g" % t for t in THRESHOLDS_M)),
             "ms per call, median (min) over %d rounds of %d calls (device events; the variants alternate inside every round);"
             % (args.rounds, args.kernel_iters), "tools/bench_ray_metric.py", ""]
    m = ray_metric.RayMetrics(C, VOXEL, dirs["tiled"])
    for K in origins:
        s = m.reset().merge_(counts["tiled", K]).get_stats()
        lines.append("scene, K = %d: a synthetic street; of %d rays %d valid, %d dropped on unknown voxels, %d valid rays miss the prediction; "
                     "RayIoU of the synthetic pair %.4f (a property of the scene, not of any model)"
                     % (K, s["rays"], s["valid"], s["unknown"], s["pred_miss"], s["RayIoU"]))
    lines.append("both ray orders give the same counters: %s" % same)
    lines.append("")
    for K in origins:
        rays = float(K * N)
        least = volume_bytes + 12.0 * N + 12.0 * K
        for order in dirs:
            ms, lo = res[order, K]
            lines.append("K = %d, %-10s %8.4f (%.4f) ms  %7.2f Grays/s  least traffic %.2f MB -> %6.1f GB/s%s"
                         % (K, order, ms, lo, rays / ms * 1e-6, least * 1e-6, least / ms * 1e-6, share(ms)))
            lines.append("   by the library's own event pair (no host enqueue in it), mean of %d: %.4f ms" % (args.kernel_iters, alone[order, K]))
        lines.append("   tiled / beam-major: %.2fx (events), %.2fx (event pair)"
                     % (res["tiled", K][0] / res["beam-major", K][0], alone["tiled", K] / alone["beam-major", K]))
    lines.append("")
    lines.append("least traffic = both label volumes once + the directions + the origins; the rays re-read the volumes from the caches,")
    lines.append("so GB/s over the least traffic is far below what the memory system moves: the pass is bound by the dependent")
    lines.append("gather-and-step chain of each ray, not by HBM.  Two separate walks (a SEPARATE variant) were not built or measured.")
    lines.append("no RayIoU of a trained model is measured: no checkpoint and no dataset where this was run.")
    result = {"ms": {"%s_k%d" % key: round(v[0], 5) for key, v in res.items()},
              "launch_ms": {"%s_k%d" % key: round(v, 5) for key, v in alone.items()}, "same_counters": same,
              "rays_per_origin": N, "frame_ms": args.frame_ms}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
