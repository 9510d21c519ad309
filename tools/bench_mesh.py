"""Cost of the surface mesh (occdepth_amd/mesh.py, K39) on the 200-frame straight drive of tools/bench_map.py and on one
256 x 256 x 32 frame.  Synthetic labels: a street-like scene (ground, blocks, free space above), so that the surface is a
surface and not noise.  It times, with device events,

    count, emit, sort, heads, weld    the stages of hip.mesh_faces on their own (the sort as ms per 8-bit pass)
    mesh_volume / mesh_labels         the whole call, wall clock, its two host synchronisations included
    torch operators                   the weld from the same corner keys: torch.unique(int64 keys, return_inverse) on the GPU
    numpy                             the same on the host (numpy.unique), the copy of the keys to the host not counted

checks the three welds equal, and on the frame also the whole mesh against the restatement of tests/test_mesh.py.

    python tools/bench_mesh.py [--rounds 5] [--iters 5] [--frame-ms "PARENT ...; THIS ..."] [--out profiles/mesh_ab.txt]

--frame-ms: a line about the forward frame of bench.py --gpus 1 --steps 20 --warmup 5 measured in the same session, copied
into the report.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from occdepth_amd import hip, mesh, render, semantic_map as sm  # noqa: E402
from tools.bench_map import C, DIMS, DRIVE_FRAMES, ORIGIN, VOXEL, pose  # noqa: E402


def street(dev):
    """(256, 256, 32) uint8: two ground layers, blocks of a few classes on a 32-voxel grid, 0 above, 255 in a far corner."""
    X, Y, Z = DIMS
    lab = torch.zeros(DIMS, dtype=torch.uint8, device=dev)
    lab[:, :, :2] = 9
    g = torch.Generator(device="cpu").manual_seed(0)
    for bx in range(0, X, 32):
        for by in range(0, Y, 32):
            w, d, h = (int(v) for v in torch.randint(4, 20, (3,), generator=g))
            lab[bx + 4:bx + 4 + w, by + 6:by + 6 + d, 2:2 + h] = int(torch.randint(1, C, (1,), generator=g))
    lab[200:, 200:, 20:] = 255
    return lab


def device_ms(fn, rounds, iters):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / iters)
    return statistics.median(ms), min(ms)


def wall_ms(fn, rounds):
    fn()
    ms = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), min(ms)


def stages(name, rows, cells, whole, args, lines):
    """Time the stages of hip.mesh_faces on (rows, cells); `whole`: the public call.  -> the result row."""
    grid = tuple(cells.shape)
    bits = sum(hip.mesh_key_bits(grid))
    counts, row_cell = hip.mesh_count(rows, cells)
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    offsets, F = (ends - counts).contiguous(), int(ends[-1])
    face_label, face_dir, keys_lo, keys_hi, refs = hip.mesh_emit(rows, cells, row_cell, offsets, F)
    wide = keys_lo.long() & 0xFFFFFFFF
    if keys_hi is not None:
        wide = wide | (keys_hi.long() << 32)
    copies = lambda: (keys_lo.clone(), None if keys_hi is None else keys_hi.clone(), refs.clone())
    s_lo, s_hi, s_refs = hip.mesh_sort_corners(*copies(), bits)
    marks = hip.mesh_heads(s_lo, s_hi, grid)
    ranks = torch.cumsum(marks, 0, dtype=torch.int32)
    V = int(ranks[-1])
    quads, vertices = hip.mesh_weld(s_lo, s_hi, s_refs, ranks, V, grid)

    t = {"count": device_ms(lambda: hip.mesh_count(rows, cells), args.rounds, args.iters),
         "emit": device_ms(lambda: hip.mesh_emit(rows, cells, row_cell, offsets, F), args.rounds, args.iters),
         "copies": device_ms(copies, args.rounds, args.iters),
         "copies+sort": device_ms(lambda: hip.mesh_sort_corners(*copies(), bits), args.rounds, args.iters),
         "heads": device_ms(lambda: hip.mesh_heads(s_lo, s_hi, grid), args.rounds, args.iters),
         "scan": device_ms(lambda: torch.cumsum(marks, 0, dtype=torch.int32), args.rounds, args.iters),
         "weld": device_ms(lambda: hip.mesh_weld(s_lo, s_hi, s_refs, ranks, V, grid), args.rounds, args.iters)}
    sort = t["copies+sort"][0] - t["copies"][0]
    passes = hip.sort_passes(0, min(bits, 32)) + (hip.sort_passes(0, bits - 32) if bits > 32 else 0)
    pair_bytes = 4 * F * 20.0                                                  # keys read twice, values once, both written once
    whole_ms = wall_ms(whole, args.rounds)

    # the same weld from torch operators and from numpy
    def torch_weld():
        uniq, inverse = torch.unique(wide, return_inverse=True)
        return uniq, inverse
    t_torch = device_ms(torch_weld, args.rounds, max(1, args.iters // 2))
    uniq, inverse = torch_weld()
    bz, by = hip.mesh_key_bits(grid)[2], hip.mesh_key_bits(grid)[1]
    t_vertices = torch.stack([uniq >> (by + bz), (uniq >> bz) & ((1 << by) - 1), uniq & ((1 << bz) - 1)], -1).to(torch.int32)
    same_torch = bool(torch.equal(t_vertices, vertices)) and bool(torch.equal(inverse.reshape(-1, 4).to(torch.int32), quads))
    host_keys = wide.cpu().numpy()
    np_ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        n_uniq, n_inverse = np.unique(host_keys, return_inverse=True)
        np_ms.append((time.perf_counter() - t0) * 1e3)
    same_numpy = np.array_equal(n_uniq, uniq.cpu().numpy()) and np.array_equal(n_inverse.reshape(-1, 4), quads.cpu().numpy())
    ours = sort + t["heads"][0] + t["scan"][0] + t["weld"][0]

    lines.append("%s: %d brick rows in a window of %d x %d x %d bricks, key of %d bits; F = %d faces, V = %d vertices, 4 F = %d corner references"
                 % ((name, int(rows.shape[0])) + grid + (bits, F, V, 4 * F)))
    lines.append("  occd_mesh_count (fill + invert the directory + count)  %8.4f (%.4f) ms" % t["count"])
    lines.append("  occd_mesh_emit                                         %8.4f (%.4f) ms" % t["emit"])
    lines.append("  sort on K38, %d passes over %d bits                      %8.4f ms (clones + sort %.4f less the clones %.4f) = %.4f ms a pass:"
                 % (passes, bits, sort, t["copies+sort"][0], t["copies"][0], sort / passes))
    lines.append("      %.2f TB/s against the %.3f GB a pass must move (profiles/lovasz_ab.txt records 1.80 TB/s for K38 at 41 M pairs)"
                 % (pair_bytes / (sort / passes * 1e-3) / 1e12, pair_bytes / 1e9))
    lines.append("  occd_mesh_heads                                        %8.4f (%.4f) ms" % t["heads"])
    lines.append("  torch.cumsum of the marks                              %8.4f (%.4f) ms" % t["scan"])
    lines.append("  occd_mesh_weld                                         %8.4f (%.4f) ms" % t["weld"])
    lines.append("  the whole call, wall clock, two host reads included    %8.3f (%.3f) ms" % whole_ms)
    lines.append("  the weld (sort + heads + scan + weld) %.3f ms; torch.unique(int64 keys, return_inverse) on the GPU %.3f (%.3f) ms (%.2fx),"
                 % (ours, t_torch[0], t_torch[1], t_torch[0] / ours))
    lines.append("      equal: %s; numpy.unique on the host %.0f ms (%.0fx), equal: %s" % (same_torch, min(np_ms), min(np_ms) / ours, same_numpy))
    m = mesh.Mesh(vertices, quads, face_label, face_dir, np.zeros(3), VOXEL)
    return m, {"F": F, "V": V, "count_ms": round(t["count"][0], 4), "emit_ms": round(t["emit"][0], 4), "sort_ms": round(sort, 4),
               "sort_pass_ms": round(sort / passes, 4), "heads_ms": round(t["heads"][0], 4), "weld_ms": round(t["weld"][0], 4),
               "whole_ms": round(whole_ms[0], 3), "torch_unique_ms": round(t_torch[0], 3), "numpy_unique_ms": round(min(np_ms), 1),
               "equal": bool(same_torch and same_numpy)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frame-ms", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    labels = street(dev)
    lines = ["surface mesh (K39), closed surface (cap_unknown = 1); ms, median (min) over %d rounds of %d calls (device events) or of one call"
             % (args.rounds, args.iters), "(wall clock); tools/bench_mesh.py", ""]
    result = {}

    # one frame
    rows, cells = mesh.brick_rows(labels)
    m, result["frame"] = stages("one frame, %d x %d x %d voxels" % DIMS, rows, cells, lambda: mesh.mesh_labels(labels, VOXEL, ORIGIN),
                                args, lines)
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_mesh import mesh_ref
        t0 = time.perf_counter()
        want = mesh_ref(rows.cpu().numpy(), cells.cpu().numpy())
        ref_s = time.perf_counter() - t0
        got = (m.vertices, m.quads, m.face_label, m.face_dir)
        same = all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
        lines.append("  the numpy restatement of tests/test_mesh.py on the host: %.2f s for the whole mesh, equal: %s" % (ref_s, same))
        result["frame"]["restatement_s"], result["frame"]["restatement_equal"] = round(ref_s, 2), bool(same)
    except ImportError as e:
        lines.append("  the numpy restatement was not run: %s" % e)
    import tempfile
    fd, path = tempfile.mkstemp(suffix=".ply")
    os.close(fd)
    colours = render.palette("kitti")
    t0 = time.perf_counter()
    mesh.write_mesh_ply(path, m, colours)
    w_s = time.perf_counter() - t0
    size = os.path.getsize(path)
    os.remove(path)
    lines.append("  write_mesh_ply: %.1f MB in %.3f s = %.0f MB/s (device -> host copies and the face records included)" % (size / 1e6, w_s, size / 1e6 / w_s))
    result["frame"]["ply_MBps"] = round(size / 1e6 / w_s, 1)
    lines.append("")

    # the drive
    drive = sm.SemanticMap(C, VOXEL, ORIGIN, DIMS)
    for f in range(DRIVE_FRAMES):
        drive.integrate(labels, pose(float(f)))
    t0 = time.perf_counter()
    volume = sm.MapVolume(drive, None, 1, drop_empty=False)
    torch.cuda.synchronize()
    vol_s = time.perf_counter() - t0
    _, result["drive"] = stages("straight drive, %d frames, 1 m per frame" % DRIVE_FRAMES, volume.labels, volume.cells,
                                lambda: mesh.mesh_volume(volume), args, lines)
    lines.append("  (building the MapVolume first, brick labels of every brick and the directory: %.2f s wall)" % vol_s)
    lines.append("")
    if args.frame_ms:
        lines.append("forward frame, bench.py --gpus 1 --steps 20 --warmup 5, fresh processes in turn, ms:")
        lines.append("  " + args.frame_ms)
        lines.append("  the frame runs no new code: with the switch off mesh.py is not imported.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
