"""Cost of the connected components (occdepth_amd/panoptic.py, K40, csrc/ccl.hip) on the synthetic street of
tools/bench_mesh.py: one 256 x 256 x 32 frame, B = 1, the SemanticKITTI things and stuff classes, both connectivities.
It times, from the library's per-launch device events (hip.profile),

    tile-local, seam, flatten          the stages of occd_ccl_segments, on the street, the prediction, a dense random volume
                                       and a solid block
    init + seam over every pair        the same with the tile-local pass switched off (OCCD_CCL_NO_TILE_PASS)
    roots, compact, filter             the other entry points
    overlaps                           marks, emit, the passes of the K38 sort, heads, rows (prediction = the street with 10 %
                                       of its voxels relabelled)

and, wall clock with their host reads, hip.ccl_compact, hip.ccl_overlaps and PanopticMetrics.add_batch as a whole; then the
same segments from scipy.ndimage.label on the host and from torch operators on the GPU (the voxel indices of a class
min-pooled over the 3 x 3 x 3 neighbourhood, or its six faces, until nothing changes), with a check that all three are equal.

    python tools/bench_ccl.py [--rounds 5] [--iters 5] [--frame-ms "PARENT ...; THIS ..."] [--out profiles/ccl_ab.txt]
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

from occdepth_amd import hip, panoptic as pan  # noqa: E402
from tools.bench_mesh import street, wall_ms  # noqa: E402

THINGS, STUFF = pan.KITTI_THINGS, pan.KITTI_STUFF


def stage_ms(fn, tags, rounds, iters):
    """{tag: median over the rounds of the device time of one launch group with that profile tag}, ms."""
    fn()
    torch.cuda.synchronize()
    seen = {t: [] for t in tags}
    for _ in range(rounds):
        with hip.profile() as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        for t in tags:
            row = prof.rows.get(t)
            if row is not None and row["launches"]:
                seen[t].append(row["ms"] / iters)
    return {t: (statistics.median(v) if v else float("nan")) for t, v in seen.items()}


def torch_segments(labels, things, connectivity):
    """The things segments from torch operators: per class, 1 + voxel index min-pooled over the neighbourhood until stable."""
    X, Y, Z = labels.shape
    index = torch.arange(1, X * Y * Z + 1, dtype=torch.float32, device=labels.device).reshape(1, 1, X, Y, Z)   # exact below 2^24
    big = torch.full_like(index, float(1 << 24))
    seg = torch.zeros((X, Y, Z), dtype=torch.int32, device=labels.device)
    pool = torch.nn.functional.max_pool3d
    rounds = 0
    for c in things:
        own = (labels == c).reshape(1, 1, X, Y, Z)
        if not bool(own.any()):
            continue
        val = torch.where(own, index, big)
        while True:
            for _ in range(8):                                          # one host read per eight rounds
                if connectivity == 26:
                    nxt = -pool(-val, 3, 1, 1)
                else:
                    nxt = torch.minimum(torch.minimum(-pool(-val, (3, 1, 1), 1, (1, 0, 0)), -pool(-val, (1, 3, 1), 1, (0, 1, 0))),
                                        -pool(-val, (1, 1, 3), 1, (0, 0, 1)))
                prev, val = val, torch.where(own, nxt, big)
                rounds += 1
            if torch.equal(prev, val):
                break
        seg = torch.where(own.reshape(X, Y, Z), val.reshape(X, Y, Z).to(torch.int32), seg)
    return seg, rounds


def scipy_segments(labels, things, connectivity):
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    out = np.zeros(labels.shape, dtype=np.int32)
    for c in things:
        comp, n = ndimage.label(labels == c, structure=structure)
        if n:
            flat = comp.reshape(-1)
            first = np.full(n + 1, flat.size, dtype=np.int64)
            np.minimum.at(first, flat, np.arange(flat.size))
            out = np.where(comp > 0, first[comp] + 1, out).astype(np.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frame-ms", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ccl_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ccl.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    target = street(dev).reshape((1, 256, 256, 32)).contiguous()
    g = torch.Generator(device="cpu").manual_seed(1)
    flip = (torch.rand(target.shape, generator=g) < 0.1).to(dev)
    pred = torch.where(flip, torch.randint(0, 20, target.shape, generator=g).to(torch.uint8).to(dev), target)
    pred = torch.where(pred == 255, torch.zeros_like(pred), pred).contiguous()
    # two volumes a street is not: three things classes at random in 95 % of the voxels (large tortuous components), and one
    # solid block of one class (the longest union-find chains): what the arrangement costs where it is worst
    dense = torch.where(torch.rand(target.shape, generator=g) < 0.95, torch.randint(1, 4, target.shape, generator=g),
                        torch.zeros(target.shape, dtype=torch.int64)).to(torch.uint8).to(dev).contiguous()
    solid = torch.ones_like(target)
    ws = hip.ccl_workspace(1, target.shape[1:], dev)
    lines = ["connected components (K40), one 256 x 256 x 32 frame of the synthetic street (prediction: 10 % of the voxels relabelled),"
             " SemanticKITTI things 1-8 / stuff 9-19;", "ms, median over %d rounds of %d calls: device events per launch group (hip.profile) "
             "or wall clock where a host read is part of the call; tools/bench_ccl.py" % (args.rounds, args.iters), ""]
    result = {}
    for connectivity in (26, 6):
        seg = {name: hip.ccl_segments(vol, THINGS, STUFF, connectivity, ws) for name, vol in (("target", target), ("prediction", pred))}
        comp = {name: hip.ccl_compact(seg[name], vol) for name, vol in (("target", target), ("prediction", pred))}
        lines.append("connectivity %d: %d segments in the street, %d in the prediction (largest %d / %d voxels)"
                     % (connectivity, int(comp["target"][1].sum()), int(comp["prediction"][1].sum()),
                        int(comp["target"][3][1].max()), int(comp["prediction"][3][1].max())))
        r = result[str(connectivity)] = {}
        for name, vol in (("street", target), ("prediction", pred), ("dense", dense), ("solid", solid)):
            t = stage_ms(lambda: hip.ccl_segments(vol, THINGS, STUFF, connectivity, ws, check=False),
                         ("ccl_tile", "ccl_seam", "ccl_flatten"), args.rounds, args.iters)
            u = stage_ms(lambda: hip.ccl_segments(vol, THINGS, STUFF, connectivity, ws, tile_pass=False, check=False),
                         ("ccl_init", "ccl_seam_all", "ccl_flatten"), args.rounds, args.iters)
            same = bool(torch.equal(hip.ccl_segments(vol, THINGS, STUFF, connectivity, ws, tile_pass=False),
                                    hip.ccl_segments(vol, THINGS, STUFF, connectivity, ws)))
            lines.append("  %-10s tile-local %.4f + seam %.4f + flatten %.4f = %.4f ms;  without the tile-local pass: init %.4f + seam over "
                         "every pair %.4f + flatten %.4f = %.4f ms (equal: %s)"
                         % (name, t["ccl_tile"], t["ccl_seam"], t["ccl_flatten"], sum(t.values()), u["ccl_init"], u["ccl_seam_all"],
                            u["ccl_flatten"], sum(u.values()), same))
            r[name] = {"tile_ms": round(t["ccl_tile"], 4), "seam_ms": round(t["ccl_seam"], 4), "flatten_ms": round(t["ccl_flatten"], 4),
                       "untiled_ms": round(sum(u.values()), 4), "untiled_equal": same}
        t = stage_ms(lambda: hip.ccl_compact(seg["prediction"], pred), ("ccl_roots", "ccl_compact"), args.rounds, args.iters)
        w = wall_ms(lambda: hip.ccl_compact(seg["prediction"], pred), args.rounds)
        lines.append("  compaction (prediction): roots %.4f + compact %.4f ms; hip.ccl_compact with the scans and its host read, wall %.3f (%.3f) ms"
                     % (t["ccl_roots"], t["ccl_compact"], w[0], w[1]))
        f = stage_ms(lambda: hip.ccl_filter(pred, THINGS, 5, connectivity, STUFF, ws, seg=seg["prediction"]), ("ccl_filter",), args.rounds, args.iters)
        lines.append("  filter (min_voxels 5, segments given): %.4f ms" % f["ccl_filter"])
        (g_ids, g_count, g_off, _), (p_ids, p_count, p_off, _) = comp["target"], comp["prediction"]
        overlaps = lambda: hip.ccl_overlaps(g_ids, g_count, g_off, p_ids, p_count, p_off, target)
        rows = overlaps()
        tags = ("ccl_pair_marks", "ccl_pair_emit", "sort_hist", "sort_scan", "sort_scatter", "ccl_pair_heads", "ccl_pair_rows")
        o = stage_ms(overlaps, tags, args.rounds, args.iters)
        w_o = wall_ms(overlaps, args.rounds)
        bits = int(g_count.sum()).bit_length() + int(p_count.sum()).bit_length()
        lines.append("  overlaps: %d pairs -> %d rows; marks %.4f, emit %.4f, sort over %d bits (%d passes) %.4f, heads %.4f, rows %.4f ms; "
                     "hip.ccl_overlaps with its scans and two host reads, wall %.3f (%.3f) ms"
                     % (int(rows[:, 2].sum()), rows.shape[0], o["ccl_pair_marks"], o["ccl_pair_emit"], bits, hip.sort_passes(0, bits),
                        o["sort_hist"] + o["sort_scan"] + o["sort_scatter"], o["ccl_pair_heads"], o["ccl_pair_rows"], w_o[0], w_o[1]))
        metric = pan.PanopticMetrics(20, THINGS, STUFF, connectivity)
        w_m = wall_ms(lambda: metric.add_batch(pred, target), args.rounds)
        lines.append("  PanopticMetrics.add_batch as a whole (components of both volumes, overlaps, matching on the host), wall %.3f (%.3f) ms"
                     % w_m)
        r.update({"compact_wall_ms": round(w[0], 3), "filter_ms": round(f["ccl_filter"], 4), "overlaps_wall_ms": round(w_o[0], 3),
                  "add_batch_wall_ms": round(w_m[0], 3)})
        # the same segments elsewhere (things only: the other two have no notion of stuff)
        ours = hip.ccl_segments(pred, THINGS, (), connectivity, ws)
        t_seg, n_rounds = torch_segments(pred[0], THINGS, connectivity)
        w_t = wall_ms(lambda: torch_segments(pred[0], THINGS, connectivity), 2)
        same_t = bool(torch.equal(t_seg, ours[0]))
        line = "  torch operators on the GPU (%d pooling rounds over %d classes): %.1f ms wall, equal: %s" % (n_rounds, len(THINGS), w_t[1], same_t)
        try:
            host = pred[0].cpu().numpy()
            t0 = time.perf_counter()
            s_seg = scipy_segments(host, THINGS, connectivity)
            s_ms = (time.perf_counter() - t0) * 1e3
            same_s = bool(np.array_equal(s_seg, ours[0].cpu().numpy()))
            line += "; scipy.ndimage.label on the host, brought into canonical form: %.0f ms, equal: %s" % (s_ms, same_s)
            r.update({"scipy_ms": round(s_ms, 1), "scipy_equal": same_s})
        except ImportError as e:
            line += "; scipy was not run: %s" % e
        lines.append(line)
        r.update({"torch_ms": round(w_t[1], 1), "torch_equal": same_t})
        lines.append("")
    if args.frame_ms:
        lines.append("forward frame, bench.py --gpus 1 --steps 20 --warmup 5, fresh processes in turn, ms:")
        lines.append("  " + args.frame_ms)
        lines.append("  the frame runs no new code: with the switch off panoptic.py is not imported.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
