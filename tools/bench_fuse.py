"""Cost of temporal fusion (occdepth_amd/fuse.py) on a config-2 frame: 256 x 256 x 32 voxels x 20 classes, windows 2, 4
and 8.  Synthetic randn * 3 logits and synthetic driving poses (1 m forward, 1.5 degrees of yaw and a slight drift per
key frame).  For every window it times, with device events after warm-up,

    store      occd_fuse_store of one frame, from (C, S) planes and from channels-last rows, at row pitch 20 and 32
    fuse       occd_fuse_frames, one launch, at both pitches (labels + n_obs; no probability output)
    torch ops  the same computation on the same GPU with torch operators: softmax of the current frame, index
               arithmetic, index_select per source, accumulate, argmax

The variants alternate inside every round (one process, one device); the file holds the median and the minimum over the
rounds.  Achieved bytes/s of the fuse launch = its minimal traffic (K rows of 20 floats read, 2 bytes written per voxel)
over the median time.  The torch-ops figure is the baseline: no earlier commit has this step.

    python tools/bench_fuse.py [--rounds 7] [--iters 10] [--out profiles/fuse_ab.txt]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import fuse, hip  # noqa: E402

DIMS, C, ORIGIN, VOXEL = (256, 256, 32), 20, (0.0, -25.6, -2.0), 0.2
WINDOWS, PITCHES = (2, 4, 8), (20, 32)
FRAME_MS = 14.7            # the forward frame of the README (bench.py, config 2)


def pose(n):
    a = np.deg2rad(1.5 * n)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = (1.0 * n, 0.02 * n * n, 0.0)
    return T


def window_ms(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def interleaved(variants, rounds, iters):
    """{name: fn} -> {name: (median ms, min ms)}; every round runs each variant once, in turn."""
    for fn in variants.values():           # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            ms[name].append(window_ms(fn, iters))
    return {name: (statistics.median(v), min(v)) for name, v in ms.items()}


def torch_store(logits):
    return torch.softmax(logits.reshape(C, -1), 0).t().contiguous()


def torch_fuse(rows, affines, weights, centres):
    """rows[k]: (S, C); affines (K, 12) float32 on the device; centres (S, 3).  -> labels, n_obs."""
    X, Y, Z = DIMS
    acc = torch.zeros_like(rows[0])
    n = torch.zeros(rows[0].shape[0], dtype=torch.uint8, device=acc.device)
    for k, r in enumerate(rows):
        g = affines[k]
        s = centres @ g[:9].reshape(3, 3).t() + g[9:]
        idx = torch.floor(s).to(torch.int64)
        ok = (idx[:, 0] >= 0) & (idx[:, 0] < X) & (idx[:, 1] >= 0) & (idx[:, 1] < Y) & (idx[:, 2] >= 0) & (idx[:, 2] < Z)
        flat = ((idx[:, 0].clamp(0, X - 1) * Y + idx[:, 1].clamp(0, Y - 1)) * Z + idx[:, 2].clamp(0, Z - 1))
        acc += torch.index_select(r, 0, flat) * (ok.to(acc.dtype) * weights[k]).unsqueeze(1)
        n += ok.to(torch.uint8)
    return acc.argmax(1).to(torch.uint8), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "fuse_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fuse.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    X, Y, Z = DIMS
    S = X * Y * Z
    K_max = max(WINDOWS)
    g = torch.Generator(device="cuda").manual_seed(0)
    planes = torch.randn((C,) + DIMS, device=dev, generator=g) * 3
    buf = torch.zeros(DIMS + (24,), device=dev)
    buf[..., :C] = planes.permute(1, 2, 3, 0)
    cl = buf[..., :C].permute(3, 0, 1, 2)                     # the eval path's channels-last view
    rows = {p: torch.empty((K_max, S, p), device=dev) for p in PITCHES}
    for k in range(K_max):                                    # K different frames in the ring
        frame = torch.randn((C,) + DIMS, device=dev, generator=g) * 3
        for p in PITCHES:
            hip.fuse_store(frame, rows[p][k])
        del frame
    poses = [pose(K_max - 1 - k) for k in range(K_max)]       # source k is k key frames back
    affines = [fuse.IDENTITY] + [fuse.grid_affine(poses[k], poses[0], ORIGIN, VOXEL) for k in range(1, K_max)]
    aff_dev = torch.from_numpy(np.stack(affines)).to(dev)
    i, j, l = torch.meshgrid(torch.arange(X, device=dev), torch.arange(Y, device=dev), torch.arange(Z, device=dev), indexing="ij")
    centres = torch.stack([i, j, l], -1).reshape(-1, 3).float() + 0.5
    del i, j, l

    lines = ["temporal fusion, %d x %d x %d voxels x %d classes, float32; ms per call, median (min) over %d rounds of %d calls,"
             % (X, Y, Z, C, args.rounds, args.iters), "variants alternating inside every round; tools/bench_fuse.py", ""]
    store = interleaved({
        "planes_p20": lambda: hip.fuse_store(planes, rows[20][0]), "planes_p32": lambda: hip.fuse_store(planes, rows[32][0]),
        "rows_p20": lambda: hip.fuse_store(cl, rows[20][0]), "rows_p32": lambda: hip.fuse_store(cl, rows[32][0]),
        # the rows kernel's predecessor: one thread per row, scalar loads (kept for rows that are not 16-byte pieces)
        "rows_p20_softmax_channels": lambda: hip.load().occd_softmax_channels(
            buf.data_ptr(), rows[20][0].data_ptr(), S, 24, 0, 20, 0, C, 0, torch.cuda.current_stream().cuda_stream),
        "torch_softmax_rows": lambda: torch_store(planes)}, args.rounds, args.iters)
    lines.append("store pass (one frame; reads %.0f MB of logits, writes %.0f MB of rows at pitch 20, %.0f MB at pitch 32)"
                 % (S * C * 4 / 1e6, S * 20 * 4 / 1e6, S * 32 * 4 / 1e6))
    for name, (med, mn) in store.items():
        lines.append("  %-26s %8.3f (%.3f) ms" % (name, med, mn))
    lines.append("")
    result = {"store_ms": {k: round(v[0], 4) for k, v in store.items()}, "windows": {}}
    for K in WINDOWS:
        w = [1.0] * K
        ref = hip.fuse_frames([rows[20][k] for k in range(K)], affines[:K], w, DIMS, C)
        tl, tn = torch_fuse([rows[20][k] for k in range(K)], aff_dev, w, centres)
        agree = float((tl == ref[0].reshape(-1)).float().mean()), float((tn == ref[1].reshape(-1)).float().mean())
        p32 = hip.fuse_frames([rows[32][k] for k in range(K)], affines[:K], w, DIMS, C)
        same = bool(torch.equal(p32[0], ref[0]) and torch.equal(p32[1], ref[1]))
        del ref, tl, tn, p32
        got = interleaved({
            "fuse_p20": lambda: hip.fuse_frames([rows[20][k] for k in range(K)], affines[:K], w, DIMS, C),
            "fuse_p32": lambda: hip.fuse_frames([rows[32][k] for k in range(K)], affines[:K], w, DIMS, C),
            "torch_fuse": lambda: torch_fuse([rows[20][k] for k in range(K)], aff_dev, w, centres)}, args.rounds, args.iters)
        minimal = S * (K * C * 4 + 2)
        lines.append("window %d: minimal traffic %.0f MB (K rows of %d floats read + 2 bytes written per voxel)" % (K, minimal / 1e6, C))
        for name, (med, mn) in got.items():
            extra = "  %6.2f TB/s of minimal traffic" % (minimal / (med * 1e-3) / 1e12) if name != "torch_fuse" else ""
            lines.append("  %-12s %8.3f (%.3f) ms%s" % (name, med, mn, extra))
        kernels = store["rows_p20"][0] + got["fuse_p20"][0]
        ops = store["torch_softmax_rows"][0] + got["torch_fuse"][0]
        lines.append("  per frame, store (channels-last, pitch 20) + fuse: %.3f ms = %.1f %% of the %.1f ms forward frame;"
                     % (kernels, 100 * kernels / FRAME_MS, FRAME_MS))
        lines.append("  torch ops, softmax + fuse: %.3f ms (%.1fx)" % (ops, ops / kernels))
        lines.append("  labels equal to the torch-ops result on %.4f %% of the voxels, n_obs on %.4f %%; pitch 32 = pitch 20: %s"
                     % (100 * agree[0], 100 * agree[1], same))
        lines.append("")
        result["windows"][K] = {"fuse_ms": {k: round(v[0], 4) for k, v in got.items()}, "per_frame_ms": round(kernels, 4),
                                "torch_ops_ms": round(ops, 4), "fuse_p20_TBps": round(minimal / (got["fuse_p20"][0] * 1e-3) / 1e12, 3)}
    lines.append("pitch: see fuse_p20 against fuse_p32 and the store rows above; the package default is pitch = classes rounded up to 4.")
    lines.append("the torch-ops version rounds every product and sum on its own (the kernel fuses multiply-adds), so a voxel at a")
    lines.append("rounding boundary can differ; the kernel is held to a float64 restatement by tests/test_fuse_gpu.py, not to it.")
    lines.append("every window re-uses the same buffers back to back: of the store pass's 336 MB a part can stay in the 256 MB")
    lines.append("Infinity Cache, which a frame's single call does not have; the fuse launch at window 8 streams 1.3 GB.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
