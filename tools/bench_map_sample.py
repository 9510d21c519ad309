"""Cost of reading the sequence map back into a frame (SemanticMap.sample, occd_map_sample, K32) on a config-2 frame: 256 x
256 x 32 voxels x 20 classes at a 45 degree heading, in the map of the 200-frame straight drive of tools/bench_map.py
(synthetic labels, uniform classes, 10 % of the voxels 255).  It times

    sample       one frame in the middle of the drive: the host side (window, directory, table; wall clock), the pinned
                 copies, the kernel (device events) and the whole call back to back, separately
    integrate    the same frame voting into the same map (known bricks), kernel only, in the same rounds: both kernels
                 touch the same vote rows once
    torch ops    the same read-back on the same GPU with torch operators from the same table and directory: int32 index
                 arithmetic, an advanced-index gather from the pool, max / argmax and sum (the A/B baseline; it must give
                 the same labels)

and both kernels again over four disjoint stretches of the drive in turn, where the counters come from HBM and not from
the Infinity Cache.  Achieved bytes/s of the sample kernel = the bytes it must move (the vote row of every voxel read
once, the voxel's own label read, 3 bytes written, the directory and the table read) over the median time.

    python tools/bench_map_sample.py [--frame-ms MS] [--rounds 7] [--iters 10] [--out profiles/map_sample_ab.txt]

--frame-ms: the forward frame measured in the same session (1000 / the frames/s of bench.py --gpus 1 --steps 20
--warmup 5); without it the shares are left out.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_map import C, DIMS, DRIVE_FRAMES, HEADING, ORIGIN, VOXEL, interleaved, pose, wall_ms  # noqa: E402
from occdepth_amd import hip, semantic_map as sm  # noqa: E402


def frame_lattice(dims, device):
    """(X Y Z, 3) int32: the frame voxels in flat order, z fastest."""
    axes = [torch.arange(d, dtype=torch.int32, device=device) for d in dims]
    return torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)


def torch_sample(pool, table, cells, own, Bq, dq, lattice, n_classes, min_obs=1, keep_own=False):
    """occd_map_sample without exclude_self, with torch operators: pool (capacity, 4096, pitch) int16, table (n, 16) and
    cells (gx, gy, gz) int32 on the device, own (S,) uint8 / int16 or None, Bq (3, 3) and dq (3,) int32 device tensors,
    lattice (S, 3) int32 -> labels (S,) uint8, n_obs (S,) int16 holding uint16 bits."""
    wq = (lattice[:, None, :] * Bq[None]).sum(-1, dtype=torch.int32) + dq                          # (S, 3) int32, wrapping
    idx = wq >> 16
    cell, loc = idx >> 4, idx & 15
    inside = torch.ones(len(lattice), dtype=torch.bool, device=lattice.device)
    at = []
    for a in range(3):
        inside &= (cell[:, a] >= 0) & (cell[:, a] < cells.shape[a])
        at.append(cell[:, a].clamp(0, cells.shape[a] - 1).long())
    row = torch.where(inside, cells[at[0], at[1], at[2]], torch.full_like(at[0], -1, dtype=torch.int32))
    have = (row >= 0) & (row < len(table))
    slot = table[row.clamp(0, len(table) - 1).long(), 0].long()
    have &= (slot >= 0) & (slot < pool.shape[0])
    voxel = ((loc[:, 0] * 16 + loc[:, 1]) * 16 + loc[:, 2]).long()
    cnt = (pool[slot.clamp(0, pool.shape[0] - 1), voxel, :n_classes].to(torch.int32) & 0xFFFF) * have[:, None]
    n = cnt.sum(-1, dtype=torch.int32)
    best, label = cnt.max(-1)                                              # the first maximum: the lowest class on a tie
    wide = None if own is None else own.reshape(-1).to(torch.int32) & 0xFFFF
    if keep_own:
        mine = cnt.gather(1, wide.clamp(max=n_classes - 1).long()[:, None])[:, 0]
        label = torch.where((wide < n_classes) & (mine == best) & (best > 0), wide.long(), label)
    fallback = torch.full_like(label, 255) if wide is None else wide.clamp(max=255).long()
    labels = torch.where(n >= max(int(min_obs), 1), label, fallback).to(torch.uint8)
    return labels, n.clamp(max=65535).to(torch.int16)


def per_launch_ms(fn, tag, calls):
    """Device time of one launch, from the library's own event pair around every launch (hip.profile): unlike a window of
    back-to-back calls it does not include the host's enqueue time, which for kernels this short is the larger part."""
    fn()
    torch.cuda.synchronize()
    with hip.profile() as prof:
        for _ in range(calls):
            fn()
    row = prof.rows[tag]
    return row["ms"] / row["launches"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="calls per window of the host-side timings")
    ap.add_argument("--kernel-iters", type=int, default=100, help="calls per window of the device-event timings")
    ap.add_argument("--frame-ms", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "map_sample_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_sample.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    X, Y, Z = DIMS
    S = X * Y * Z
    g = torch.Generator(device="cuda").manual_seed(0)
    labels = torch.randint(0, C, DIMS, device=dev, generator=g, dtype=torch.uint8)
    labels[torch.rand(DIMS, device=dev, generator=g) < 0.1] = 255
    share = (lambda ms: "  = %.2f %% of the %.2f ms forward frame" % (100 * ms / args.frame_ms, args.frame_ms)) \
        if args.frame_ms else (lambda ms: "")

    drive = sm.SemanticMap(C, VOXEL, ORIGIN, DIMS)
    for f in range(DRIVE_FRAMES):
        drive.integrate(labels, pose(float(f)))
    torch.cuda.synchronize()
    mid = pose(100.0)
    cells, table, key_min = drive.frame_cells(mid, dev)
    Bq, dq = sm.sample_coefficients(mid, ORIGIN, VOXEL, key_min, DIMS)
    dev_table, host_table = drive.upload(table, dev)
    dev_cells, _ = drive.upload(cells, dev)
    int_table = drive.frame_table(mid, dev)                                # every brick known: nothing is admitted
    int_dev, int_host = drive.upload(int_table, dev)
    pool = drive.pool()

    def kernel(exclude_self=False, t=(dev_table, host_table, dev_cells, Bq, dq, cells.shape)):
        return hip.map_sample(pool, t[0], t[2], labels, DIMS, C, t[3], t[4], t[5], keep_own=True, exclude_self=exclude_self,
                              table_host=t[1])

    got = kernel()
    met = int((got[1] != 0).sum())
    lattice = frame_lattice(DIMS, dev)
    tBq, tdq = torch.from_numpy(Bq).to(dev), torch.from_numpy(dq).to(dev)
    want = torch_sample(pool, dev_table, dev_cells, labels, tBq, tdq, lattice, C, 1, True)
    same = bool(torch.equal(got[0].reshape(-1), want[0]) and torch.equal(got[1].reshape(-1), want[1]))
    changed = int((got[0] != labels).sum())
    minimal = S * (drive.pitch * 2 + 3 + 1) + cells.size * 4 + table.size * 4

    lines = ["map read-back, %d x %d x %d voxels x %d classes, heading %g degrees, frame 100 of the %d-frame drive (1 m per frame, %d bricks,"
             % (X, Y, Z, C, HEADING, DRIVE_FRAMES, drive.n_bricks),
             "%.0f MB of counters); ms per call, median (min) over %d rounds of %d calls (host wall clock) or %d calls (device events; the"
             % (drive.n_bricks * drive.brick_bytes / 1e6, args.rounds, args.iters, args.kernel_iters),
             "device variants alternate inside every round); tools/bench_map_sample.py", ""]
    lines.append("one frame: window %d x %d x %d bricks, %d of its bricks in the map (integrate selects %d), %d of %d voxels meet a vote,"
                 % (cells.shape + (len(table), len(int_table), met, S)))
    lines.append("  %d labels differ from the frame's own (keep_own, min_obs 1)" % changed)
    host = wall_ms(lambda: drive.frame_cells(mid, dev), args.rounds, args.iters)
    coef = wall_ms(lambda: sm.sample_coefficients(mid, ORIGIN, VOXEL, key_min, DIMS), args.rounds, args.iters)
    upload = wall_ms(lambda: (drive.upload(table, dev), drive.upload(cells, dev)), args.rounds, args.iters)
    whole = wall_ms(lambda: drive.sample(mid, own=labels, keep_own=True), args.rounds, args.iters)
    res = interleaved({
        "sample": kernel,
        "sample_exclude_self": lambda: kernel(True),
        "integrate": lambda: hip.map_integrate(pool, int_dev, labels, DIMS, C, table_host=int_host),
        "torch_ops": lambda: torch_sample(pool, dev_table, dev_cells, labels, tBq, tdq, lattice, C, 1, True)},
        args.rounds, args.kernel_iters)
    k_ms, i_ms, t_ms = res["sample"][0], res["integrate"][0], res["torch_ops"][0]
    lines.append("sample:")
    lines.append("  host: window + directory + table      %8.3f (%.3f) ms wall%s" % (host + (share(host[0]),)))
    lines.append("  host: coefficients                    %8.3f (%.3f) ms wall" % coef)
    lines.append("  host: pinned copies, table and cells  %8.3f (%.3f) ms wall" % upload)
    lines.append("  kernel occd_map_sample (keep_own)     %8.3f (%.3f) ms%s" % (res["sample"] + (share(k_ms),)))
    lines.append("    bytes it must move %.0f MB (the %d-byte vote row of every voxel, its own label, 3 bytes written, %d KB of directory"
                 % (minimal / 1e6, drive.pitch * 2, (cells.size + table.size) * 4 // 1000))
    lines.append("    and table): %.2f TB/s" % (minimal / (k_ms * 1e-3) / 1e12))
    lines.append("  kernel, exclude_self + keep_own       %8.3f (%.3f) ms" % res["sample_exclude_self"])
    lines.append("  kernel occd_map_integrate, same frame %8.3f (%.3f) ms: sample costs %.2fx" % (res["integrate"] + (k_ms / i_ms,)))
    lines.append("    (back-to-back calls re-use the same counters, which fit the 256 MB Infinity Cache; see the rotating launches below)")
    alone = {"sample": per_launch_ms(kernel, "map_sample", args.kernel_iters),
             "sample_exclude_self": per_launch_ms(lambda: kernel(True), "map_sample", args.kernel_iters),
             "integrate": per_launch_ms(lambda: hip.map_integrate(pool, int_dev, labels, DIMS, C, table_host=int_host), "map_integrate",
                                        args.kernel_iters)}
    lines.append("  one launch by its own event pair (no host enqueue in it), mean of %d: sample %.4f ms = %.2f TB/s, with exclude_self %.4f ms,"
                 % (args.kernel_iters, alone["sample"], minimal / (alone["sample"] * 1e-3) / 1e12, alone["sample_exclude_self"]))
    lines.append("    integrate %.4f ms: sample costs %.2fx" % (alone["integrate"], alone["sample"] / alone["integrate"]))
    lines.append("  sample(), whole call, back to back    %8.3f (%.3f) ms wall per frame%s" % (whole + (share(whole[0]),)))
    lines.append("  torch ops (gather, max, sum)          %8.3f (%.3f) ms (%.1fx the kernel)%s; labels and n_obs equal to the kernel's: %s"
                 % (res["torch_ops"] + (t_ms / k_ms, share(t_ms), same)))
    if host[0] + upload[0] > k_ms:
        lines.append("  the host side costs more than the kernel (%.1fx): the frame's cost is Python and numpy, as for integrate; not tuned here."
                     % ((host[0] + coef[0] + upload[0]) / k_ms))
    lines.append("")

    # counters that are not in the Infinity Cache: four disjoint stretches of the drive in turn
    spots = []
    for d in (20.0, 70.0, 120.0, 170.0):
        P = pose(d)
        c, t, kmin = drive.frame_cells(P, dev)
        b, q = sm.sample_coefficients(P, ORIGIN, VOXEL, kmin, DIMS)
        td, th = drive.upload(t, dev)
        spots.append(((td, th, drive.upload(c, dev)[0], b, q, c.shape), drive.upload(drive.frame_table(P, dev), dev)))
    turn = [0, 0]

    def rot_sample():
        turn[0] += 1
        kernel(False, spots[turn[0] % len(spots)][0])

    def rot_integrate():
        turn[1] += 1
        t_dev, t_host = spots[turn[1] % len(spots)][1]
        hip.map_integrate(pool, t_dev, labels, DIMS, C, table_host=t_host)
    rot = interleaved({"sample": rot_sample, "integrate": rot_integrate}, args.rounds, args.kernel_iters)
    lines.append("four disjoint stretches of the drive in turn (%.0f MB of counters between two visits of a brick, both kernels in every round):"
                 % (sum(len(s[0][1]) for s in spots) * drive.brick_bytes / 1e6))
    lines.append("  kernel occd_map_sample                %8.3f (%.3f) ms, %.2f TB/s of the bytes it must move%s"
                 % (rot["sample"] + (minimal / (rot["sample"][0] * 1e-3) / 1e12, share(rot["sample"][0]))))
    lines.append("  kernel occd_map_integrate             %8.3f (%.3f) ms: sample costs %.2fx"
                 % (rot["integrate"] + (rot["sample"][0] / rot["integrate"][0],)))
    rot_alone = (per_launch_ms(rot_sample, "map_sample", args.kernel_iters), per_launch_ms(rot_integrate, "map_integrate", args.kernel_iters))
    lines.append("  one launch by its own event pair: sample %.4f ms = %.2f TB/s, integrate %.4f ms: sample costs %.2fx"
                 % (rot_alone[0], minimal / (rot_alone[0] * 1e-3) / 1e12, rot_alone[1], rot_alone[0] / rot_alone[1]))
    lines.append("")
    lines.append("the effect of the read-back on any score is not measured: no checkpoint and no dataset where this was run.")
    result = {"window_bricks": int(cells.size), "bricks_in_map": int(len(table)), "host_ms": round(host[0], 4),
              "upload_ms": round(upload[0], 4), "kernel_ms": round(k_ms, 4), "kernel_exclude_self_ms": round(res["sample_exclude_self"][0], 4),
              "integrate_kernel_ms": round(i_ms, 4), "sample_wall_ms": round(whole[0], 4), "torch_ops_ms": round(t_ms, 4),
              "kernel_TBps": round(minimal / (k_ms * 1e-3) / 1e12, 3), "kernel_rotating_ms": round(rot["sample"][0], 4),
              "integrate_rotating_ms": round(rot["integrate"][0], 4), "same_as_torch": same, "launch_ms": {k: round(v, 5) for k, v in alone.items()},
              "launch_rotating_ms": [round(v, 5) for v in rot_alone], "frame_ms": args.frame_ms}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
