"""Cost of summing two sequence maps (SemanticMap.merge, occd_map_merge, K33), of keeping a map in a file and of the
exchange between ranks, on the map of the 200-frame straight drive of tools/bench_map.py (256 x 256 x 32 voxels x 20
classes at a 45 degree heading, synthetic labels).  It times

    merge        every brick of the drive's map added into a copy of it, and a 256-brick chunk (what the rank exchange
                 merges at a time; 16 disjoint chunks in turn, so the counters come from HBM), for every split of a brick
                 over workgroups the library offers; bytes/s over the traffic it must move (two reads and one write per
                 counter)
    copy         a device-to-device copy of the same bricks (one read, one write): the yardstick for a streaming kernel
    torch ops    the same sum with torch operators: index, int32 add, clamp, index_put (it must give the same bytes)
    save / load  SemanticMap.save and SemanticMap.load of that map, MB/s of file
    exchange     merge_over_ranks between two processes that share this GPU, through gloo: every rank maps every second
                 frame.  Time-sliced on one GPU and staged through host memory: not a stand-in for eight ranks over xGMI.

    python tools/bench_map_merge.py [--rounds 7] [--iters 20] [--frame-ms-parent A B C --frame-ms-this A B C]
                                    [--out profiles/map_merge_ab.txt]

--frame-ms-parent / --frame-ms-this: the forward frame (1000 / the frames/s of bench.py --gpus 1 --steps 20 --warmup 5) of
the parent commit and of this one, fresh processes run in turn in the same session; they are only reported.
"""
import argparse
import datetime
import json
import os
import socket
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_map import C, DIMS, DRIVE_FRAMES, HEADING, ORIGIN, VOXEL, interleaved, pose  # noqa: E402
from occdepth_amd import hip, semantic_map as sm  # noqa: E402

SPLITS = (1, 2, 4, 8)
CHUNK = 256


def drive_map(frames, device="cuda"):
    g = torch.Generator(device=device).manual_seed(0)
    labels = torch.randint(0, C, DIMS, device=device, generator=g, dtype=torch.uint8)
    labels[torch.rand(DIMS, device=device, generator=g) < 0.1] = 255
    m = sm.SemanticMap(C, VOXEL, ORIGIN, DIMS)
    for f in frames:
        m.integrate(labels, pose(float(f)))
    return m


def torch_merge(pool, src, slots, rows):
    total = (pool[slots].to(torch.int32) & 0xFFFF) + (src[rows].to(torch.int32) & 0xFFFF)
    pool[slots] = total.clamp(max=65535).to(torch.int16)


def rank_worker():
    """One rank of the exchange: RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment -> one JSON line."""
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    m = drive_map(range(rank, DRIVE_FRAMES, world))
    mine = len(m.occupied_keys())
    torch.cuda.synchronize()
    dist.barrier()
    t = time.perf_counter()
    sm.merge_over_ranks(m, chunk_bricks=CHUNK)
    torch.cuda.synchronize()
    dist.barrier()
    wall = time.perf_counter() - t
    print("EXCHANGE " + json.dumps({"rank": rank, "own_bricks": mine, "bricks": len(m.occupied_keys()), "wall_s": wall}), flush=True)
    dist.destroy_process_group()


def exchange(world=2, timeout=600):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank-worker"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True, env=dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                                                  MASTER_PORT=str(port))) for r in range(world)]
    rows = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=timeout)
            line = [l for l in out.splitlines() if l.startswith("EXCHANGE ")]
            if p.returncode != 0 or not line:
                raise SystemExit("a rank of the exchange failed:\n" + out[-3000:])
            rows.append(json.loads(line[-1][len("EXCHANGE "):]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frame-ms-parent", type=float, nargs="*", default=[])
    ap.add_argument("--frame-ms-this", type=float, nargs="*", default=[])
    ap.add_argument("--no-exchange", action="store_true")
    ap.add_argument("--rank-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "map_merge_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_map_merge.py measures on the GPU; there is none here")
    if args.rank_worker:
        return rank_worker()
    dev = torch.device("cuda")
    src_map = drive_map(range(DRIVE_FRAMES))
    dst_map = sm.SemanticMap(C, VOXEL, ORIGIN, DIMS).merge(src_map)
    n = src_map.n_bricks
    keys = src_map.brick_keys()
    table = np.stack([dst_map.slots(keys), src_map.slots(keys)], 1).astype(np.int32)
    pool, src = dst_map.pool(), src_map.pool()
    brick = src_map.brick_bytes

    # the same bytes from the kernel and from torch operators, on a copy
    a, b = pool.clone(), pool.clone()
    full_dev, full_host = dst_map.upload(table, dev)
    hip.map_merge(a, src, full_dev, table_host=full_host)
    t64 = torch.from_numpy(table.astype(np.int64)).to(dev)
    torch_merge(b, src, t64[:, 0], t64[:, 1])
    same = bool(torch.equal(a, b))
    del a, b

    def rotating(fn, count):
        state = [0]

        def run():
            state[0] += 1
            fn(state[0] % count)
        return run

    def chunk_variants(size, splits, others=True):
        """Merges of `size` bricks, the disjoint chunks of the map in turn, so that the counters come from HBM."""
        starts = range(0, n - size + 1, size)
        tabs = [dst_map.upload(table[s:s + size], dev) for s in starts]
        idx = [t64[s:s + size] for s in starts]
        out = {("split %d" % s if s else "default"): rotating(
            lambda i, s=s: hip.map_merge(pool, src, tabs[i][0], table_host=tabs[i][1], split=s), len(tabs)) for s in splits}
        if others:
            out["copy"] = rotating(lambda i: pool[i * size:(i + 1) * size].copy_(src[i * size:(i + 1) * size]), len(tabs))
            out["torch ops"] = rotating(lambda i: torch_merge(pool, src, idx[i][:, 0], idx[i][:, 1]), len(tabs))
        return out, len(tabs)

    big = {"split %d" % s: (lambda s=s: hip.map_merge(pool, src, full_dev, table_host=full_host, split=s)) for s in SPLITS}
    big["copy"] = lambda: pool[:n].copy_(src[:n])
    big["torch ops"] = lambda: torch_merge(pool, src, t64[:, 0], t64[:, 1])
    big["default"] = lambda: hip.map_merge(pool, src, full_dev, table_host=full_host)
    small, n_chunks = chunk_variants(CHUNK, SPLITS + (0,))
    res_big = interleaved(big, args.rounds, max(2, args.iters // 4))
    res_small = interleaved(small, args.rounds, args.iters)
    between = {size: interleaved(chunk_variants(size, (1, 8, 0), others=False)[0], args.rounds, args.iters) for size in (512, 1024, 2048)}

    lines = ["map merge, %d x %d x %d voxels x %d classes, heading %g degrees, the %d-frame drive: %d bricks, %.0f MB of counters per map;"
             % (DIMS + (C, HEADING, DRIVE_FRAMES, n, n * brick / 1e6)),
             "ms per call, median (min) over %d rounds (device events, the variants alternate inside every round); tools/bench_map_merge.py"
             % args.rounds, ""]
    for title, res, count in (("all %d bricks" % n, res_big, n), ("%d bricks, %d disjoint chunks in turn" % (CHUNK, n_chunks), res_small, CHUNK)):
        lines.append("%s (%.0f MB per operand):" % (title, count * brick / 1e6))
        for name, (med, low) in res.items():
            moved = (2 if name == "copy" else 3) * count * brick
            lines.append("  %-10s %8.4f (%.4f) ms  %6.2f TB/s over %d x the counters" % (name, med, low, moved / (med * 1e-3) / 1e12,
                                                                                      2 if name == "copy" else 3))
        lines.append("")
    lines.append("between the two sizes (disjoint chunks in turn), ms: " + "; ".join(
        "%d bricks: %s" % (size, ", ".join("%s %.4f" % (name, v[0]) for name, v in res.items())) for size, res in between.items()))
    lines.append("  default = what the library picks when the caller names no split")
    lines.append("")
    lines.append("kernel and torch operators leave the same bytes: %s" % same)
    lines.append("")

    # save / load
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "drive.occmap")
        torch.cuda.synchronize()
        t = time.perf_counter()
        src_map.save(path)
        save_s = time.perf_counter() - t
        size = os.path.getsize(path)
        t = time.perf_counter()
        back = sm.SemanticMap.load(path)
        torch.cuda.synchronize()
        load_s = time.perf_counter() - t
        slots = torch.from_numpy(src_map.slots(back.brick_keys()).astype(np.int64)).to(dev)
        round_trip = bool(torch.equal(back.pool()[:back.n_bricks], src.index_select(0, slots)))
        del back
    lines.append("save: %.0f MB of file in %.2f s = %.0f MB/s; load: %.2f s = %.0f MB/s (one run each, %d bricks per pinned buffer, the"
                 % (size / 1e6, save_s, size / 1e6 / save_s, load_s, size / 1e6 / load_s, src_map.chunk_bricks))
    lines.append("  file in the system's temporary directory); the loaded counters equal the saved ones: %s" % round_trip)
    lines.append("")
    result = {"bricks": n, "same_as_torch": same, "round_trip": round_trip, "save_MBps": round(size / 1e6 / save_s, 1),
              "load_MBps": round(size / 1e6 / load_s, 1),
              "all_ms": {k: round(v[0], 4) for k, v in res_big.items()}, "chunk_ms": {k: round(v[0], 4) for k, v in res_small.items()},
              "between_ms": {str(size): {k: round(v[0], 4) for k, v in res.items()} for size, res in between.items()}}

    if not args.no_exchange:
        del dst_map, pool
        torch.cuda.empty_cache()
        rows = exchange()
        lines.append("merge_over_ranks, two processes on this one GPU through gloo, every rank maps every second frame (%s occupied bricks),"
                     % " / ".join(str(r["own_bricks"]) for r in rows))
        lines.append("  %d bricks after the exchange, %d-brick chunks: %.2f s wall (the slower rank).  The two processes take turns on the GPU and"
                     % (rows[0]["bricks"], CHUNK, max(r["wall_s"] for r in rows)))
        lines.append("  every chunk goes device -> pinned host -> loopback TCP -> pinned host -> device: it says nothing about eight ranks over xGMI.")
        lines.append("")
        result["exchange_wall_s"] = round(max(r["wall_s"] for r in rows), 3)
    if args.frame_ms_parent and args.frame_ms_this:
        lines.append("forward frame, bench.py --gpus 1 --steps 20 --warmup 5, fresh processes in turn, ms: parent %s (median %.3f), this %s (median %.3f)"
                     % (" ".join("%.3f" % v for v in args.frame_ms_parent), statistics.median(args.frame_ms_parent),
                        " ".join("%.3f" % v for v in args.frame_ms_this), statistics.median(args.frame_ms_this)))
        lines.append("  the frame runs no new code.")
        lines.append("")
        result["frame_ms_parent"], result["frame_ms_this"] = args.frame_ms_parent, args.frame_ms_this
    lines.append("the effect of merged maps on any score is not measured: no checkpoint, no dataset and no multi-GPU node where this was run.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
