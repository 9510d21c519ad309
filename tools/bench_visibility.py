"""Cost of the per-frame visibility pass (occd_frame_visibility, K34) and of weighted votes on a config-2 frame: 256 x 256 x
32 voxels x 20 classes seen through the 370 x 1220 KITTI camera.  A synthetic street (two layers of road, boxes of cars and
buildings, 2 % of the voxels 255).  It times

    K34            occd_frame_visibility (its fill kernel and its ray kernel), by device events and by the library's own
                   event pair around the call
    render         occd_render_voxels on the same volume and view: the same walk without the carve stores (it writes an
                   RGB image instead) -- the yardstick, in the same rounds
    torch ops      the same marked volume with torch operators: the walk as elementwise float32 tensor arithmetic over
                   all rays, one scatter per step (the A/B baseline; it must give the same bytes)
    weighted       occd_map_integrate_weighted / occd_map_sample_weighted against the unweighted kernels, the same frame
                   into the same bricks of a short drive's map, in the same rounds

    python tools/bench_visibility.py [--frame-ms MS] [--rounds 7] [--kernel-iters 100] [--out profiles/visibility_ab.txt]

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

from bench_map import C, DIMS, ORIGIN, VOXEL, interleaved, pose  # noqa: E402
from bench_map_sample import per_launch_ms  # noqa: E402
from occdepth_amd import hip, render, semantic_map as sm, visibility  # noqa: E402
from oracle import inputs  # noqa: E402

IMAGE_HW = (370, 1220)
W_VISIBLE, W_HIDDEN = 4, 1
MAP_FRAMES = 40


def street(dims, seed=0):
    """(X, Y, Z) uint8: road, a pavement step, boxes (cars, buildings), 2 % unknown; the camera's surroundings free."""
    X, Y, Z = dims
    rng = np.random.RandomState(seed)
    vol = np.zeros(dims, dtype=np.uint8)
    vol[:, :, :2] = 9                                                        # road: the camera stands 1.7 m above it
    vol[:, : Y // 2 - 30, 2] = 11
    vol[:, Y // 2 + 30:, 2] = 11
    for _ in range(60):
        sx, sy, sz = rng.randint(8, 40), rng.randint(8, 40), rng.randint(6, Z - 2)
        x, y = rng.randint(20, X - sx), rng.choice([rng.randint(0, Y // 2 - 30 - min(sy, Y // 2 - 31)), rng.randint(Y // 2 + 30, Y - sy)])
        vol[x:x + sx, y:y + sy, 2:2 + sz] = rng.randint(1, 20)
    for _ in range(25):                                                      # cars on the road
        x, y = rng.randint(15, X - 25), rng.randint(Y // 2 - 28, Y // 2 + 18)
        vol[x:x + 22, y:y + 9, 2:9] = 1
    vol[rng.rand(*dims) < 0.02] = 255
    vol[:12, Y // 2 - 6:Y // 2 + 6, 2:] = 0
    return vol


def torch_visibility(labels, view, size):
    """occd_frame_visibility with torch operators: labels (X, Y, Z) uint8 on the GPU, view (18,) float32 -> (X, Y, Z)
    uint8.  Every product and sum is its own float32 tensor operation (nothing contracts), one scatter per step, no host
    synchronisation: X + Y + Z + 3 steps for every ray."""
    X, Y, Z = labels.shape
    H, W = size
    dev = labels.device
    g = view
    fu = (torch.arange(W, device=dev, dtype=torch.float32) + 0.5)[None, :, None]
    fv = (torch.arange(H, device=dev, dtype=torch.float32) + 0.5)[:, None, None]
    o = ((g[0:3] + fu * g[3:6]) + fv * g[6:9]).reshape(-1, 3)
    d = ((g[9:12] + fu * g[12:15]) + fv * g[15:18]).reshape(-1, 3)
    dims = torch.tensor([X, Y, Z], device=dev, dtype=torch.float32)
    idims = torch.tensor([X, Y, Z], device=dev, dtype=torch.int64)
    inf = torch.tensor(float("inf"), device=dev)
    zero = torch.zeros((), device=dev)
    alive = torch.isfinite(o).all(1) & torch.isfinite(d).all(1)
    nz = d != 0
    inv = torch.where(nz, 1.0 / torch.where(nz, d, torch.ones_like(d)), torch.zeros_like(d))
    ta, tc = (0.0 - o) * inv, (dims - o) * inv
    lo, hi = torch.fmin(ta, tc), torch.fmax(ta, tc)
    tn = torch.where(nz, lo, -inf).max(1).values
    tf = torch.where(nz, hi, inf).min(1).values
    alive &= (nz | ((o >= 0) & (o < dims))).all(1)
    t = torch.where(tn > 0, tn, zero)
    alive &= tf >= t
    idx = torch.fmin(torch.fmax(torch.floor(o + d * t[:, None]), zero), dims - 1.0)
    idx = torch.where(torch.isfinite(idx), idx, torch.zeros_like(idx)).to(torch.int64)
    step = torch.sign(d).to(torch.int64)
    m = torch.where(step != 0, ((idx + (step > 0)).to(torch.float32) - o) * inv, inf)
    flat = labels.reshape(-1)
    S = X * Y * Z
    visible = torch.zeros(S + 1, dtype=torch.uint8, device=dev)             # one spare byte for the rays that are done
    one = torch.ones(len(o), dtype=torch.uint8, device=dev)
    rows = torch.arange(len(o), device=dev)
    for _ in range(X + Y + Z + 3):
        vox = (idx[:, 0] * Y + idx[:, 1]) * Z + idx[:, 2]
        visible.scatter_(0, torch.where(alive, vox, torch.full_like(vox, S)), one)
        lab = flat[vox]
        alive = alive & ~((lab > 0) & (lab < 255))
        ax = torch.where((m[:, 0] <= m[:, 1]) & (m[:, 0] <= m[:, 2]), 0, torch.where(m[:, 1] <= m[:, 2], 1, 2))
        mv = m[rows, ax]
        alive = alive & (mv < inf)
        moved = idx[rows, ax] + torch.where(alive, step[rows, ax], torch.zeros_like(ax))
        alive = alive & (moved >= 0) & (moved < idims[ax])
        idx[rows, ax] = torch.where(alive, moved, idx[rows, ax])
        m[rows, ax] = torch.where(alive, ((moved + (step[rows, ax] > 0)).to(torch.float32) - o[rows, ax]) * inv[rows, ax], m[rows, ax])
    return visible[:S].reshape(X, Y, Z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernel-iters", type=int, default=100, help="calls per window of the device-event timings")
    ap.add_argument("--frame-ms", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "visibility_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_visibility.py measures on the GPU; there is none here")
    dev = torch.device("cuda")
    X, Y, Z = DIMS
    S = X * Y * Z
    H, W = IMAGE_HW
    share = (lambda ms: "  = %.2f %% of the %.2f ms forward frame" % (100 * ms / args.frame_ms, args.frame_ms)) \
        if args.frame_ms else (lambda ms: "")
    labels = torch.from_numpy(street(DIMS)).to(dev)
    view, size = visibility.camera_rays(torch.from_numpy(inputs.KITTI_K), torch.from_numpy(inputs.KITTI_TR), ORIGIN, VOXEL, IMAGE_HW)
    view = view.to(dev).contiguous()
    palette = render.palette("kitti").to(dev)

    visible, hit = hip.frame_visibility(labels, view, size, return_hit=True)
    drawn = hip.render_voxels(labels[None], view[None, None], size, palette, aux=True)[1][0, 0]
    same_hit = bool(torch.equal(hit, drawn))
    by_torch = torch_visibility(labels, view, size)
    same_torch = bool(torch.equal(by_torch, visible))
    walked = int((hit >= 0).sum())
    occupied = (labels > 0) & (labels < 255)

    res = interleaved({"visibility": lambda: hip.frame_visibility(labels, view, size),
                       "render": lambda: hip.render_voxels(labels[None], view[None, None], size, palette)},
                      args.rounds, args.kernel_iters)
    torch_ms = interleaved({"torch_ops": lambda: torch_visibility(labels, view, size)}, 3, 1)["torch_ops"]
    alone = {"visibility": per_launch_ms(lambda: hip.frame_visibility(labels, view, size), "frame_visibility", args.kernel_iters),
             "render": per_launch_ms(lambda: hip.render_voxels(labels[None], view[None, None], size, palette), "render_voxels",
                                     args.kernel_iters)}
    v_ms, r_ms = res["visibility"][0], res["render"][0]

    lines = ["per-frame visibility (K34) and weighted votes, %d x %d x %d voxels x %d classes, the %d x %d KITTI camera (%d rays);"
             % (X, Y, Z, C, H, W, H * W),
             "ms per call, median (min) over %d rounds of %d calls (device events; the variants alternate inside every round);"
             % (args.rounds, args.kernel_iters), "tools/bench_visibility.py", ""]
    lines.append("scene: a synthetic street, %.1f %% of the voxels occupied; %d of %d rays end on a voxel; %.1f %% of the voxels are marked"
                 % (100 * float(occupied.float().mean()), walked, H * W, 100 * float(visible.float().mean())))
    lines.append("  visible: %.1f %% of the occupied voxels, %.1f %% of the free ones; hit equal to occd_render_voxels' hit: %s"
                 % (100 * float(visible[occupied].float().mean()), 100 * float(visible[~occupied].float().mean()), same_hit))
    lines.append("K34 occd_frame_visibility (fill + rays)  %8.4f (%.4f) ms%s" % (res["visibility"] + (share(v_ms),)))
    lines.append("occd_render_voxels, same volume and view %8.4f (%.4f) ms: K34 costs %.2fx the render pass" % (res["render"] + (v_ms / r_ms,)))
    lines.append("  by the library's own event pair (no host enqueue in it), mean of %d: K34 %.4f ms, render %.4f ms: %.2fx"
                 % (args.kernel_iters, alone["visibility"], alone["render"], alone["visibility"] / alone["render"]))
    lines.append("torch ops (the walk as tensor arithmetic)  %8.2f (%.2f) ms (%.0fx K34); the same bytes as the kernel: %s"
                 % (torch_ms + (torch_ms[0] / v_ms, same_torch)))
    lines.append("")

    # weighted against unweighted votes: the same frame into the same bricks of a short drive's map
    weight = visibility.vote_weights(visible, None, W_VISIBLE, W_HIDDEN)
    mask = weight != 0
    drive = sm.SemanticMap(C, VOXEL, ORIGIN, DIMS)
    for f in range(MAP_FRAMES):
        drive.integrate(labels, pose(float(f)), weight=weight)
    torch.cuda.synchronize()
    mid = pose(MAP_FRAMES / 2.0)
    int_dev, int_host = drive.upload(drive.frame_table(mid, dev), dev)
    cells, table, key_min = drive.frame_cells(mid, dev)
    Bq, dq = sm.sample_coefficients(mid, ORIGIN, VOXEL, key_min, DIMS)
    dev_table, host_table = drive.upload(table, dev)
    dev_cells, _ = drive.upload(cells, dev)
    pool = drive.pool()
    wres = interleaved({
        "integrate": lambda: hip.map_integrate(pool, int_dev, labels, DIMS, C, mask=mask, table_host=int_host),
        "integrate_weighted": lambda: hip.map_integrate_weighted(pool, int_dev, labels, DIMS, C, weight, table_host=int_host),
        "sample": lambda: hip.map_sample(pool, dev_table, dev_cells, labels, DIMS, C, Bq, dq, cells.shape, own_mask=mask,
                                         exclude_self=True, keep_own=True, table_host=host_table),
        "sample_weighted": lambda: hip.map_sample_weighted(pool, dev_table, dev_cells, labels, DIMS, C, Bq, dq, cells.shape,
                                                           own_weight=weight, exclude_self=True, keep_own=True, table_host=host_table)},
        args.rounds, args.kernel_iters)
    lines.append("weighted votes (w_visible %d, w_hidden %d) against the unweighted kernels with the same volume as a mask, frame %d of a"
                 % (W_VISIBLE, W_HIDDEN, MAP_FRAMES // 2))
    lines.append("%d-frame drive (1 m per frame, %d bricks, %.0f MB of counters):" % (MAP_FRAMES, drive.n_bricks, drive.n_bricks * drive.brick_bytes / 1e6))
    for name, base in (("integrate_weighted", "integrate"), ("sample_weighted", "sample")):
        lines.append("  occd_map_%-20s %8.4f (%.4f) ms, occd_map_%s %.4f (%.4f) ms: %.2fx%s"
                     % ((name,) + wres[name] + (base,) + wres[base] + (wres[name][0] / wres[base][0], share(wres[name][0]))))
    lines.append("  (sample: exclude_self + keep_own; back-to-back calls re-use counters that fit the Infinity Cache)")
    lines.append("")
    lines.append("the effect of occlusion-aware votes on mIoU is not measured: no checkpoint and no dataset where this was run.")
    result = {"visibility_ms": round(v_ms, 5), "render_ms": round(r_ms, 5), "ratio": round(v_ms / r_ms, 3),
              "launch_ms": {k: round(v, 5) for k, v in alone.items()}, "torch_ops_ms": round(torch_ms[0], 3),
              "same_as_torch": same_torch, "hit_same_as_render": same_hit, "visible_share": round(float(visible.float().mean()), 4),
              "weighted_ms": {k: round(v[0], 5) for k, v in wres.items()}, "frame_ms": args.frame_ms}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
