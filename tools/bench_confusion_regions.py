"""Time the SSC confusion pass by region (occd_ssc_confusion_regions) against what it replaces, at config 2's output
grid: B = 1, 256 x 256 x 32 voxels, C = 20, channels-last float32 logits (rows of 24 floats, the 3-D stack's layout).

    (a) hip.ssc_confusion                      one (C, C) matrix, the parent's pass (K7)
    (b) hip.ssc_confusion_regions              the six `kitti` regions (full, fov, 12.8m, 25.6m and the two FOV
                                               intersections), FOV computed in the kernel from the calibration
    (c) what a user did before                 hip.vox2pix at output scale, then per region a masked copy of the
                                               target (torch.where) and one hip.ssc_confusion

Two synthetic inputs: `scene` -- large coherent runs of (empty, empty) voxels, an unlabelled wedge and a thin occupied
layer, so that most waves agree on (target, prediction) as in a real sweep -- and `random`, independent classes per
voxel, the worst case for the wave aggregation (every wave is mixed).  Each variant is captured into a hipGraph of
`--launches` launches; after a warm-up the three graphs are replayed in turn for `--rounds` rounds between device events
and the median time per launch is reported.  The counts of (b) are checked against (a) and (c) before anything is timed.

    python tools/bench_confusion_regions.py [--launches 20] [--rounds 15] [--out profiles/confusion_regions.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from occdepth_amd import hip, train_graph  # noqa: E402
from occdepth_amd.loss.sscMetrics import metric_box  # noqa: E402
from oracle import inputs  # noqa: E402

DIMS, C, CS = (256, 256, 32), 20, 24
ORIGIN, VOX, IMG_WH = (0.0, -25.6, -2.0), 0.2, (1220, 370)


def make_inputs(kind, dev, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "random":
        target = torch.randint(0, C, (1,) + DIMS, generator=g).to(torch.uint8)
        target[torch.rand((1,) + DIMS, generator=g) < 0.1] = 255
        logits = torch.randn((1,) + DIMS + (C,), generator=g)
    else:
        target = torch.zeros((1,) + DIMS, dtype=torch.uint8)
        blocks = torch.randint(1, C, (1, DIMS[0] // 8, DIMS[1] // 8, 1), generator=g).to(torch.uint8)
        layer = blocks.repeat_interleave(8, 1).repeat_interleave(8, 2).expand(1, DIMS[0], DIMS[1], 4)
        target[..., 4:8] = layer                                        # a thin occupied layer, one class per 8 x 8 column
        x = torch.arange(DIMS[0]).view(1, -1, 1, 1)
        y = torch.arange(DIMS[1]).view(1, 1, -1, 1)
        target[((y - DIMS[1] // 2).abs() > x + 40).expand_as(target)] = 255      # an unlabelled wedge beside the sensor
        truth = torch.where(target == 255, torch.zeros_like(target), target).long()
        wrong = torch.rand((1,) + DIMS, generator=g) < 0.02             # isolated errors
        truth = torch.where(wrong, torch.randint(0, C, (1,) + DIMS, generator=g), truth)
        logits = 0.5 * torch.randn((1,) + DIMS + (C,), generator=g)
        logits.scatter_add_(-1, truth.unsqueeze(-1), torch.full((1,) + DIMS + (1,), 6.0))
    rows = torch.zeros((1,) + DIMS + (CS,))
    rows[..., :C] = logits
    rows = rows.to(dev)
    return rows[..., :C].permute(0, 4, 1, 2, 3), target.to(dev)


def box_member(box, dev):
    m = torch.zeros((1,) + DIMS, dtype=torch.bool, device=dev)
    m[:, box[0]:box[1], box[2]:box[3], box[4]:box[5]] = True
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "confusion_regions.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU; there is nothing to time without one"
    dev = "cuda"
    tr2 = inputs.KITTI_TR.copy()
    tr2[0, 3] = -0.54
    E = torch.from_numpy(np.stack([inputs.KITTI_TR, tr2]))[None].to(dev).contiguous()
    K = torch.from_numpy(np.stack([inputs.KITTI_K, inputs.KITTI_K]))[None].to(dev).contiguous()
    calib = (E, K, ORIGIN, VOX, IMG_WH, (0,))
    boxes = [metric_box((0.0, r, -r / 2, r / 2), ORIGIN, VOX, DIMS) for r in (12.8, 25.6)]
    regions = [(None, 0), (None, hip.NEED_FOV), (boxes[0], 0), (boxes[1], 0), (boxes[0], hip.NEED_FOV), (boxes[1], hip.NEED_FOV)]
    members = [None, None, box_member(boxes[0], dev), box_member(boxes[1], dev)]
    unl = torch.full((1,) + DIMS, 255, dtype=torch.uint8, device=dev)
    results, lines = {}, []
    for kind in ("scene", "random"):
        logits, target = make_inputs(kind, dev)
        assert hip._logit_layout(logits) == (DIMS[0] * DIMS[1] * DIMS[2] * CS, 1, CS)
        h_a = torch.zeros(C, C, dtype=torch.int64, device=dev)
        h_b = torch.zeros(6, C, C, dtype=torch.int64, device=dev)
        h_c = torch.zeros(6, C, C, dtype=torch.int64, device=dev)

        def run_a():
            hip.ssc_confusion(h_a, target, logits=logits)

        def run_b():
            hip.ssc_confusion_regions(h_b, target, regions, logits=logits, fov=calib)

        def run_c():
            fov = hip.vox2pix(E, K, None, ORIGIN, VOX, DIMS, IMG_WH)[1][:, 0, :, 0].view((1,) + DIMS)
            for r, m in enumerate([None, fov, members[2], members[3], members[2] & fov, members[3] & fov]):
                hip.ssc_confusion(h_c[r], target if m is None else torch.where(m, target, unl), logits=logits)

        for fn in (run_a, run_b, run_c):                  # eager once: the counts must agree before anything is timed
            fn()
        torch.cuda.synchronize()
        assert torch.equal(h_b[0], h_a) and torch.equal(h_b, h_c), "the region pass disagrees with the masked K7 passes"
        share = [float(h_b[r].sum()) / max(1.0, float(h_b[0].sum())) for r in range(6)]
        graphs = []
        for fn in (run_a, run_b, run_c):
            g = train_graph.new_graph()
            with torch.cuda.graph(g):
                for _ in range(args.launches):
                    fn()
            train_graph.seal_graph(g)
            graphs.append(g)
        for g in graphs * 3:                              # warm-up replays of every graph
            g.replay()
        torch.cuda.synchronize()
        times = [[], [], []]
        for _ in range(args.rounds):                      # a, b, c in turn: what disturbs one round disturbs all three
            for i, g in enumerate(graphs):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                g.replay()
                t1.record()
                t1.synchronize()
                times[i].append(1e3 * t0.elapsed_time(t1) / args.launches)
        med = [float(np.median(t)) for t in times]
        lo = [float(np.min(t)) for t in times]
        hi = [float(np.max(t)) for t in times]
        n = DIMS[0] * DIMS[1] * DIMS[2]
        bytes_a = n * (4.0 * CS + 1)                      # the rows as stored (24 floats) + the target byte
        results[kind] = {"a_us": round(med[0], 2), "b_us": round(med[1], 2), "c_us": round(med[2], 2),
                         "b_over_a": round(med[1] / med[0], 3), "c_over_b": round(med[2] / med[1], 2),
                         "a_GB_per_s": round(bytes_a / med[0] / 1e3, 1), "region_share_of_labelled": [round(s, 3) for s in share]}
        lines.append(f"[{kind}]  median of {args.rounds} rounds x {args.launches} launches per hipGraph replay, us per launch (min .. max)")
        for tag, i in (("(a) ssc_confusion, 1 matrix              ", 0), ("(b) ssc_confusion_regions, 6 regions, FOV in kernel", 1),
                       ("(c) vox2pix + 6 x (torch.where + ssc_confusion)    ", 2)):
            lines.append(f"  {tag} {med[i]:9.2f}   ({lo[i]:.2f} .. {hi[i]:.2f})")
        lines.append(f"  (b) / (a) = {med[1] / med[0]:.3f}   (expectation: <= 1.5)      (c) / (b) = {med[2] / med[1]:.2f}")
        lines.append(f"  (a) reads {bytes_a / 1e6:.1f} MB -> {bytes_a / med[0] / 1e3:.0f} GB/s;  labelled voxels per region / full: "
                     + " ".join(f"{s:.3f}" for s in share))
        del graphs
    head = [f"SSC confusion by region, B=1 {DIMS[0]}x{DIMS[1]}x{DIMS[2]} C={C} channels-last rows of {CS} floats, "
            f"{torch.cuda.get_device_name(0)}", "tools/bench_confusion_regions.py", ""]
    text = "\n".join(head + lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
