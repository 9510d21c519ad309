"""Cost of the sequence-level semantic map (occdepth_amd/semantic_map.py) on a config-2 frame: 256 x 256 x 32 voxels x 20
classes at a 45 degree heading.  Synthetic labels (uniform classes, 10 % of the voxels 255).  It times

    integrate    one frame into a map that already knows its bricks: the host side (brick selection, directory, table;
                 wall clock) and the kernel (device events) separately, and the whole call back to back
    torch ops    the same votes on the same GPU with torch operators from the same table: int32 index arithmetic, a
                 label gather and index_put_(accumulate=True) into an int32 pool (the baseline: no earlier commit has
                 this step)
    extraction   extract() and brick_labels() of every brick, for the map of a 200-frame straight drive, 1 m per frame

and writes the map's memory per frame of new ground.  Achieved bytes/s of the integrate kernel = its minimal traffic (the
vote row of every voting voxel read and written once, the frame's labels read once) over the median time.

    python tools/bench_map.py [--frame-ms MS] [--rounds 7] [--iters 10] [--out profiles/map_ab.txt]

--frame-ms: the forward frame measured in the same session (1000 / the frames/s of bench.py --gpus 1 --steps 20
--warmup 5); without it the shares are left out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from occdepth_amd import hip, semantic_map as sm  # noqa: E402

DIMS, C, ORIGIN, VOXEL = (256, 256, 32), 20, (0.0, -25.6, -2.0), 0.2
HEADING = 45.0
DRIVE_FRAMES = 200


def pose(metres):
    a = np.deg2rad(HEADING)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = (metres * np.cos(a), metres * np.sin(a), 0.0)
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
    for fn in variants.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            ms[name].append(window_ms(fn, iters))
    return {name: (statistics.median(v), min(v)) for name, v in ms.items()}


def wall_ms(fn, rounds, iters):
    """Host wall clock per call, median (min) over the rounds; the device is idle before every round."""
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            fn()
        ms.append((time.perf_counter() - t) * 1e3 / iters)
    return statistics.median(ms), min(ms)


def torch_votes(pool32, table, local, labels):
    """The votes of one frame with torch operators: pool32 (capacity, 4096, pitch) int32, table (n, 16) int32 on the
    device, local (4096, 3) int32, labels (S,) uint8."""
    X, Y, Z = DIMS
    A = table[:, 4:13].reshape(-1, 3, 3)
    gq = (A[:, None, :, :] * local[None, :, None, :]).sum(-1) + table[:, None, 13:16]             # (n, 4096, 3) int32
    idx = gq >> 16
    ok = (idx[..., 0] >= 0) & (idx[..., 0] < X) & (idx[..., 1] >= 0) & (idx[..., 1] < Y) & (idx[..., 2] >= 0) & (idx[..., 2] < Z)
    flat = ((idx[..., 0].clamp(0, X - 1) * Y + idx[..., 1].clamp(0, Y - 1)) * Z + idx[..., 2].clamp(0, Z - 1)).long()
    lab = labels[flat].long()
    ok &= lab < C
    rows = table[:, 0].long()[:, None] * 4096 + torch.arange(4096, device=table.device)[None]
    where = (rows * pool32.shape[2] + lab)[ok]
    pool32.view(-1).index_put_((where,), torch.ones_like(where, dtype=torch.int32), accumulate=True)
    return pool32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="calls per window of the host-side timings")
    ap.add_argument("--kernel-iters", type=int, default=200, help="calls per window of the device-event timings")
    ap.add_argument("--frame-ms", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "map_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_map.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    X, Y, Z = DIMS
    S = X * Y * Z
    g = torch.Generator(device="cuda").manual_seed(0)
    labels = torch.randint(0, C, DIMS, device=dev, generator=g, dtype=torch.uint8)
    labels[torch.rand(DIMS, device=dev, generator=g) < 0.1] = 255

    m = sm.SemanticMap(C, VOXEL, ORIGIN, DIMS)
    m.integrate(labels, pose(0.0))
    voting = int((m.votes.view(torch.int16).to(torch.int32) & 0xFFFF).sum())
    table = m.frame_table(pose(0.0), dev)
    n = len(table)
    dev_table, host_table = m.upload(table, dev)
    minimal = voting * m.pitch * 2 * 2 + S
    share = (lambda ms: "  = %.2f %% of the %.2f ms forward frame" % (100 * ms / args.frame_ms, args.frame_ms)) \
        if args.frame_ms else (lambda ms: "")

    lines = ["semantic map, %d x %d x %d voxels x %d classes, heading %g degrees; ms per call, median (min) over %d rounds of %d calls"
             % (X, Y, Z, C, HEADING, args.rounds, args.iters),
             "(host wall clock) or %d calls (device events; the two device variants alternate inside every round); tools/bench_map.py"
             % args.kernel_iters, ""]
    lines.append("one frame: %d bricks selected for %d bricks' worth of volume, %d voting voxels of %d, %d bytes per brick (pitch %d)"
                 % (n, S // 4096, voting, S, m.brick_bytes, m.pitch))
    host = wall_ms(lambda: m.frame_table(pose(0.0), dev), args.rounds, args.iters)
    upload = wall_ms(lambda: m.upload(table, dev), args.rounds, args.iters)
    whole = wall_ms(lambda: m.integrate(labels, pose(0.0)), args.rounds, args.iters)
    pool32 = torch.zeros((m.capacity, 4096, m.pitch), dtype=torch.int32, device=dev)
    local = torch.from_numpy(np.stack(np.meshgrid(*(np.arange(16),) * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.int32)).to(dev)
    flat_labels = labels.reshape(-1)
    # the torch-ops votes equal the kernel's on a fresh pool
    fresh = sm.SemanticMap(C, VOXEL, ORIGIN, DIMS)
    fresh.integrate(labels, pose(0.0))
    torch_votes(pool32, dev_table, local, flat_labels)
    same = bool(torch.equal(pool32[:fresh.capacity].to(torch.int16).reshape(fresh.votes.shape), fresh.votes))
    pool32.zero_()
    del fresh
    got = interleaved({
        "integrate_kernel": lambda: hip.map_integrate(m.pool(), dev_table, labels, DIMS, C, table_host=host_table),
        "torch_ops": lambda: torch_votes(pool32, dev_table, local, flat_labels)}, args.rounds, args.kernel_iters)
    k_ms, t_ms = got["integrate_kernel"][0], got["torch_ops"][0]
    lines.append("integrate, known bricks:")
    lines.append("  host: selection + directory + table   %8.3f (%.3f) ms wall%s" % (host + (share(host[0]),)))
    lines.append("  host: pinned copy of the table        %8.3f (%.3f) ms wall" % upload)
    lines.append("  kernel occd_map_integrate             %8.3f (%.3f) ms%s" % (got["integrate_kernel"] + (share(k_ms),)))
    lines.append("    minimal traffic %.0f MB (the %d-byte vote row of every voting voxel read and written, %d MB of labels read):"
                 " %.2f TB/s" % (minimal / 1e6, m.pitch * 2, S // 1000000, minimal / (k_ms * 1e-3) / 1e12))
    lines.append("    (back-to-back calls re-use the same %.0f MB of counters, which fit the 256 MB Infinity Cache; see the rotating"
                 % (n * m.brick_bytes / 1e6))
    lines.append("    launches of the drive below for counters that come from HBM)")
    lines.append("  integrate(), whole call, back to back %8.3f (%.3f) ms wall per frame%s" % (whole + (share(whole[0]),)))
    lines.append("  torch ops (int32 pool, index_put_)    %8.3f (%.3f) ms (%.1fx the kernel)%s; votes equal to the kernel's: %s"
                 % (got["torch_ops"] + (t_ms / k_ms, share(t_ms), same)))
    if host[0] + upload[0] > k_ms:
        lines.append("  the host side costs more than the kernel (%.1fx): the frame's cost is Python and numpy, not the GPU.  Caching the"
                     % ((host[0] + upload[0]) / k_ms))
        lines.append("  candidate lattice per frame and keeping the directory as a sorted int64 array (np.searchsorted) or a device hash")
        lines.append("  would remove most of it; not tuned here.")
    lines.append("")
    del pool32

    # a straight drive
    drive = sm.SemanticMap(C, VOXEL, ORIGIN, DIMS)
    drive.integrate(labels, pose(0.0))
    first = drive.n_bricks
    torch.cuda.synchronize()
    t = time.perf_counter()
    for f in range(1, DRIVE_FRAMES):
        drive.integrate(labels, pose(float(f)))
    torch.cuda.synchronize()
    drive_ms = (time.perf_counter() - t) * 1e3 / (DRIVE_FRAMES - 1)
    per_frame = (drive.n_bricks - first) * drive.brick_bytes / (DRIVE_FRAMES - 1)
    keys = drive.brick_keys()
    # the kernel on counters that are not in the Infinity Cache: four disjoint stretches of the drive in turn (4 x the pool of
    # one frame), every brick known
    spots = [drive.upload(drive.frame_table(pose(d), dev), dev) for d in (0.0, 60.0, 120.0, 180.0)]
    assert drive.n_bricks == len(keys)
    turn = [0]

    def rotating():
        t_dev, t_host = spots[turn[0] % len(spots)]
        turn[0] += 1
        hip.map_integrate(drive.pool(), t_dev, labels, DIMS, C, table_host=t_host)
    rot = interleaved({"rotating": rotating}, args.rounds, args.kernel_iters)["rotating"]
    ex = wall_ms(lambda: (drive.extract(min_obs=1), torch.cuda.synchronize()), args.rounds, 5)
    bl = wall_ms(lambda: (drive.brick_labels(keys), torch.cuda.synchronize()), args.rounds, 5)
    tab = wall_ms(lambda: drive._key_table(keys), args.rounds, 5)
    n_kept = len(drive.extract(min_obs=1)[1])
    lines.append("straight drive, %d frames, 1 m per frame: %d bricks (%d after the first frame), %.0f MB of counters in use, pool %.0f MB"
                 " after %d (re)allocations" % (DRIVE_FRAMES, drive.n_bricks, first, drive.n_bricks * drive.brick_bytes / 1e6,
                                                 drive.nbytes / 1e6, drive.grown))
    lines.append("  %.2f MB of map per frame (= per metre) of new ground; integrate() with new bricks and pool growth %.3f ms wall per frame"
                 % (per_frame / 1e6, drive_ms))
    lines.append("  occd_map_integrate over four disjoint stretches in turn (%.0f MB of counters between two visits of a brick):"
                 % (sum(len(t[1]) for t in spots) * drive.brick_bytes / 1e6))
    lines.append("                                   %8.3f (%.3f) ms, %.2f TB/s of the minimal traffic%s"
                 % (rot + (minimal / (rot[0] * 1e-3) / 1e12, share(rot[0]))))
    lines.append("  extract(min_obs=1): %d voxels  %8.3f (%.3f) ms wall: host table, count + scan + write, synchronised"
                 % ((n_kept,) + ex))
    lines.append("  brick_labels(every brick)        %8.3f (%.3f) ms wall, host table and synchronise included" % bl)
    lines.append("  the host table of %d bricks alone %7.3f (%.3f) ms wall; the kernels read the %.0f MB of counters once (extract twice)"
                 % ((len(keys),) + tab + (drive.n_bricks * drive.brick_bytes / 1e6,)))
    lines.append("")
    lines.append("the effect of the map on any score is not measured: no checkpoint and no dataset where this was run.")
    result = {"bricks_per_frame": n, "host_ms": round(host[0], 4), "upload_ms": round(upload[0], 4), "kernel_ms": round(k_ms, 4),
              "integrate_wall_ms": round(whole[0], 4), "torch_ops_ms": round(t_ms, 4),
              "kernel_TBps": round(minimal / (k_ms * 1e-3) / 1e12, 3), "extract_ms": round(ex[0], 3),
              "brick_labels_ms": round(bl[0], 3), "kernel_rotating_ms": round(rot[0], 4), "drive_bricks": drive.n_bricks, "MB_per_frame": round(per_frame / 1e6, 3),
              "frame_ms": args.frame_ms}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
