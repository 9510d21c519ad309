"""Time the raw-label decode (targets.kitti_labels, occd_kitti_labels) at the SemanticKITTI size, 256 x 256 x 32, for
B = 1 and B = 4: the decode alone (with and without the occluded mask) and decode + 1:8 downsample + relation matrix --
everything `OccDepth.step` adds for a batch that carries raw voxel files.  Device events after warm-up.  Next to it the CPU
time of the preprocessing pass for one frame, restated in numpy (remap + mask, then the per-block loop of
_downsample_label): the reference itself is not available where this runs; tests/golden/make_golden_raw_labels.py
--time-full times the reference's own functions.  Prints one JSON line.

    python tools/bench_kitti_labels.py [--iters 200] [--warmup 20] [--cpu-reps 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import targets  # noqa: E402

SCENE = (256, 256, 32)


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


def synthetic(rng, frames):
    n = SCENE[0] * SCENE[1] * SCENE[2]
    keys = np.asarray([raw for raw, _ in targets.KITTI_LEARNING_MAP], dtype=np.uint16)
    raw = rng.choice(keys, size=(frames, n))
    raw[rng.random((frames, n)) < 0.6] = 0
    return raw, np.packbits(rng.random((frames, n)) < 0.1, axis=1), np.packbits(rng.random((frames, n)) < 0.4, axis=1)


def cpu_pass(raw, invalid_bits, lut):
    """One frame of the preprocessing pass in numpy: -> (seconds of remap + mask, seconds of the 1:8 block loop)."""
    t0 = time.perf_counter()
    label = lut[raw].astype(np.float32)
    label[np.unpackbits(invalid_bits) == 1] = 255
    label = label.reshape(SCENE)
    t1 = time.perf_counter()
    out = np.zeros(tuple(s // 8 for s in SCENE), dtype=np.uint8)
    for x in range(out.shape[0]):
        for y in range(out.shape[1]):
            for z in range(out.shape[2]):
                block = label[8 * x:8 * x + 8, 8 * y:8 * y + 8, 8 * z:8 * z + 8].astype(np.int32).reshape(-1)
                n0, n255 = int((block == 0).sum()), int((block == 255).sum())
                if n0 + n255 > 0.95 * 512:
                    out[x, y, z] = 0 if n0 > n255 else 255
                else:
                    out[x, y, z] = np.argmax(np.bincount(block[(block > 0) & (block < 255)]))
    return t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=1)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    n = SCENE[0] * SCENE[1] * SCENE[2]
    out = {"scene": list(SCENE), "gpu": {}}
    for frames in (1, 4):
        raw_np, inv_np, occ_np = synthetic(rng, frames)
        raw, inv, occ = (torch.from_numpy(a).cuda() for a in (raw_np, inv_np, occ_np))

        def chain():
            return targets.cp_mega_matrix(targets.downsample_label(targets.kitti_labels(raw, inv, scene_size=SCENE), 8))

        ms = timed(lambda: targets.kitti_labels(raw, inv, scene_size=SCENE), args.iters, args.warmup)
        ms_occ = timed(lambda: targets.kitti_labels(raw, inv, occ, scene_size=SCENE), args.iters, args.warmup)
        ms_chain = timed(chain, args.iters, args.warmup)
        moved, moved_occ = frames * n * (2 + 0.125 + 1), frames * n * (2 + 0.25 + 2)
        out["gpu"][f"B={frames}"] = {"decode_ms": round(ms, 4), "decode_GB_per_s": round(moved / ms / 1e6, 1),
                                     "decode_with_occluded_ms": round(ms_occ, 4),
                                     "decode_with_occluded_GB_per_s": round(moved_occ / ms_occ / 1e6, 1),
                                     "decode_downsample_relation_ms": round(ms_chain, 4)}
    raw_np, inv_np, _ = synthetic(rng, 1)
    lut = targets.kitti_remap_lut()
    reps = [cpu_pass(raw_np[0], inv_np[0], lut) for _ in range(max(args.cpu_reps, 1))]
    out["cpu_numpy_per_frame"] = {"remap_mask_ms": round(1e3 * min(r[0] for r in reps), 1),
                                  "downsample_label_ms": round(1e3 * min(r[1] for r in reps), 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
