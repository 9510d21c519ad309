"""Cost of the distance-tolerant scores (occd_dist_metric, K37) on a config-2 frame: 256 x 256 x 32 voxels x 20 classes,
max_d2 = 1024 (window 32 along every axis).  The target is the synthetic street of tools/bench_visibility.py (2 % of the
voxels 255); the prediction is the target rolled one voxel along x with 255 -> 0 and 20 % of the occupied labels redrawn
(tools/bench_ray_metric.py).  It times, alternating inside every round,

    fused        DistanceMetrics.add_batch: the x pass feeds the counters, D is never written (the default)
    unfused      hip.edt_sq of both volumes for all 20 slots (D written out, 2 x 20 uint16 volumes), then the counting with
                 torch operators (one bincount per side and slot): the A/B of feeding the counters from the last pass

by device events over windows of back-to-back calls, splits the fused call by axis pass with the library's own event pairs,
and computes the same counters once without the kernel -- scipy.ndimage.distance_transform_edt on the host where scipy
imports, else torch min-plus over shifted copies on the GPU -- to report its time and that the counters are equal.

    python tools/bench_dist_metric.py [--frame-ms MS] [--rounds 7] [--iters 10] [--out profiles/dist_metric_ab.txt]

--frame-ms: the forward frame measured in the same session (1000 / the frames/s of bench.py --gpus 1 --steps 20
--warmup 5); without it the shares are left out.  --parent-frame-ms / --parent-frame-spread: the same of the parent
commit, copied into the report.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_map import C, DIMS, VOXEL, interleaved  # noqa: E402
from bench_ray_metric import prediction  # noqa: E402
from bench_visibility import street  # noqa: E402
from occdepth_amd import dist_metric, hip  # noqa: E402

MAX_D2 = 1024


def unfused(pred, target, counts, scratch, out):
    """The counters from hip.edt_sq and torch operators: D of every slot is written out and read back."""
    T = MAX_D2
    query = target != 255
    slots = list(range(C))
    for side, (members, seeds) in enumerate(((pred, target), (target, pred))):
        D = hip.edt_sq(seeds, slots, C, T, out=out, scratch=scratch).to(torch.int64) & 0xFFFF
        for s in slots:
            sel = query & (((members >= 1) & (members < C)) if s == 0 else (members == s))
            counts[side, s] += torch.bincount(D[:, s][sel], minlength=T + 2)
    return counts


def scipy_counts(pred, target):
    """Host: one exact transform per side and slot -> counters, or None without scipy."""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    T = MAX_D2
    counts = np.zeros((2, C, T + 2), dtype=np.int64)
    query = target != 255
    for side, (members, seeds) in enumerate(((pred, target), (target, pred))):
        for s in range(C):
            sel = query & dist_metric.seeds_of(members, s, C)
            if not sel.any():
                continue
            seed = dist_metric.seeds_of(seeds, s, C)
            if seed.any():
                d = np.minimum(np.rint(ndimage.distance_transform_edt(~seed) ** 2), T + 1).astype(np.int64)
            else:
                d = np.full(seed.shape, T + 1, dtype=np.int64)
            counts[side, s] = np.bincount(d[sel], minlength=T + 2)
    return counts.reshape(-1)


def torch_counts(pred, target):
    """GPU, torch operators only: min-plus over shifted copies, pass by pass."""
    T = MAX_D2
    r = int(np.floor(np.sqrt(T)))
    counts = torch.zeros((2, C, T + 2), dtype=torch.int64, device=pred.device)
    query = target != 255
    for side, (members, seeds) in enumerate(((pred, target), (target, pred))):
        for s in range(C):
            slot = (lambda v: (v >= 1) & (v < C)) if s == 0 else (lambda v, s=s: v == s)
            g = torch.where(slot(seeds), 0, T + 1).to(torch.int32)
            for axis in (2, 1, 0):
                out = g.clone()
                n = g.shape[axis]
                for k in range(1, min(r, n - 1) + 1):
                    lo, hi = g.narrow(axis, 0, n - k), g.narrow(axis, k, n - k)
                    torch.minimum(out.narrow(axis, 0, n - k), hi + k * k, out=out.narrow(axis, 0, n - k))
                    torch.minimum(out.narrow(axis, k, n - k), lo + k * k, out=out.narrow(axis, k, n - k))
                g = out.clamp_(max=T + 1)
            counts[side, s] = torch.bincount(g[query & slot(members)].to(torch.int64), minlength=T + 2)
    return counts.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="calls per window of the device-event timings")
    ap.add_argument("--frame-ms", type=float, default=None)
    ap.add_argument("--parent-frame-ms", type=float, nargs="*", default=None, help="the parent commit's forward frame, run by run")
    ap.add_argument("--this-frame-ms", type=float, nargs="*", default=None, help="this commit's forward frame (switch off), run by run")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "dist_metric_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dist_metric.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    X, Y, Z = DIMS
    T = MAX_D2
    share = (lambda ms: "  = %.2f %% of the %.2f ms forward frame" % (100 * ms / args.frame_ms, args.frame_ms)) \
        if args.frame_ms else (lambda ms: "")
    street_np = street(DIMS)
    pred_np = prediction(street_np)
    target = torch.from_numpy(street_np)[None].to(dev)
    pred = torch.from_numpy(pred_np)[None].to(dev)

    metric = dist_metric.DistanceMetrics(C, VOXEL, max_d2=T)
    metric.add_batch(pred, target)
    fused_counts = metric.counts().cpu().numpy().copy()
    stats = metric.get_stats()
    out = torch.empty((1, C) + DIMS, dtype=torch.int16, device=dev)
    scratch = torch.empty(hip.edt_scratch_bytes(1, C, DIMS), dtype=torch.uint8, device=dev)
    loose = torch.zeros((2, C, T + 2), dtype=torch.int64, device=dev)
    unfused_counts = unfused(pred, target, loose, scratch, out).cpu().numpy().reshape(-1).copy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    other = scipy_counts(pred_np[None], street_np[None])
    other_name = "scipy.ndimage.distance_transform_edt on the host (one call per side and slot that has a query)"
    if other is None:
        other = torch_counts(pred[0], target[0]).cpu().numpy()
        other_name = "torch min-plus over shifted copies on the GPU (scipy does not import here)"
    torch.cuda.synchronize()
    other_ms = (time.perf_counter() - t0) * 1e3

    variants = {"fused": lambda: metric.add_batch(pred, target),
                "unfused": lambda: unfused(pred, target, loose, scratch, out)}
    res = interleaved(variants, args.rounds, args.iters)
    metric.add_batch(pred, target)
    torch.cuda.synchronize()
    with hip.profile() as prof:
        for _ in range(args.iters):
            metric.add_batch(pred, target)
    rows = {tag: prof.rows[tag]["ms"] / args.iters for tag in ("dist_metric", "dist_metric_z", "dist_metric_y", "dist_metric_x")}

    groups = -(-2 * C // hip.EDT_CHUNK)
    lines = ["distance-tolerant scores (K37 occd_dist_metric), %d x %d x %d voxels x %d classes, max_d2 = %d (window %d), 2 x %d "
             "transforms per frame in %d groups of %d;" % (X, Y, Z, C, T, int(np.sqrt(T)), C, groups, hip.EDT_CHUNK),
             "ms per call, median (min) over %d rounds of %d calls (device events; the variants alternate inside every round);"
             % (args.rounds, args.iters), "tools/bench_dist_metric.py", "",
             "scene: a synthetic street and its copy shifted one voxel along x with 20 %% of the labels redrawn; %d predicted and %d "
             "true occupied query voxels; F_geo@0.2/0.4/0.8 m = %s, CD_geo = %.3f m (properties of the scene, not of any model)"
             % (stats["queries"][0, 0], stats["queries"][1, 0], "/".join("%.3f" % v for v in stats["F_geo"]), stats["CD_geo"]), ""]
    ms, lo = res["fused"]
    lines.append("add_batch, fused (the x pass feeds the counters)       %8.3f (%.3f) ms%s" % (ms, lo, share(ms)))
    lines.append("   by the library's own event pairs, mean of %d calls: whole call %.3f ms = z sweeps %.3f + y pass %.3f + x pass with "
                 "counting %.3f (+ gaps between the %d launches)"
                 % (args.iters, rows["dist_metric"], rows["dist_metric_z"], rows["dist_metric_y"], rows["dist_metric_x"], 3 * groups))
    ms_u, lo_u = res["unfused"]
    lines.append("unfused (edt_sq writes D of 2 x %d slots, torch counts)  %8.3f (%.3f) ms%s   fused / unfused: %.2fx"
                 % (C, ms_u, lo_u, share(ms_u), ms / ms_u))
    lines.append("   counters equal to the fused call's: %s" % bool(np.array_equal(unfused_counts, fused_counts)))
    lines.append("designs: the windowed min-plus (packed 16-bit pairs, 8 rows per thread) is the only kernel form built; the lower-envelope")
    lines.append("   (parabola) form was not built or measured.  The x pass of the fused call skips tiles without a query of the slot, so")
    lines.append("   its time depends on the scene; the z and y passes do not.")
    lines.append("scratch: %d bytes (%.1f MiB) held by DistanceMetrics, whatever the batch size; counters: %d bytes"
                 % (metric.scratch_bytes(), metric.scratch_bytes() / 2 ** 20, 8 * metric.size))
    lines.append("without the kernel: %s: %.0f ms (one run, wall clock); counters equal to the kernel's: %s"
                 % (other_name, other_ms, bool(np.array_equal(other, fused_counts))))
    lines.append("")
    if args.parent_frame_ms and args.this_frame_ms:
        p, t = sorted(args.parent_frame_ms), sorted(args.this_frame_ms)
        lines.append("forward frame (bench.py --gpus 1 --steps 20 --warmup 5), same machine, same session, ms per run:")
        lines.append("   parent commit:            %s   (spread %.3f .. %.3f)" % (" ".join("%.3f" % v for v in args.parent_frame_ms), p[0], p[-1]))
        lines.append("   this commit, switch off:  %s   (spread %.3f .. %.3f)" % (" ".join("%.3f" % v for v in args.this_frame_ms), t[0], t[-1]))
        lines.append("   median inside the parent's own spread: %s" % bool(p[0] <= float(np.median(t)) <= p[-1]))
    lines.append("no score of a trained model is measured: no checkpoint and no dataset where this was run.")
    result = {"ms": {k: round(v[0], 4) for k, v in res.items()}, "split_ms": {k: round(v, 4) for k, v in rows.items()},
              "other_ms": round(other_ms, 1), "equal_unfused": bool(np.array_equal(unfused_counts, fused_counts)),
              "equal_other": bool(np.array_equal(other, fused_counts)), "scratch_bytes": metric.scratch_bytes(),
              "frame_ms": args.frame_ms}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
