"""Time the clipped optimizer step on the parameter set of the config-2 model (the a100 yaml's geometry through
configs.kitti_a100; only the parameters are used, with random gradients), two arms alternating in one process:

    A  torch.nn.utils.clip_grad_norm_(params, c) + AdamW(fused=True, capturable=True).step()   (the parent's way)
    B  occdepth_amd.optim.clip_adamw_step(opt, c)                                              (csrc/optim.hip)

Each arm is timed twice: launched eagerly (device events around every repetition: the host's launch work is inside, and
both arms are host-bound there) and replayed from a captured hipGraph (device time alone -- how the fast training step runs
it).  After warm-up; medians, spread (min / max and the 10th / 90th percentile), the
number of kernel launches per step (torch profiler, one step per arm) and B's share of the bandwidth bound:
(28 + 4) bytes x parameters over the 8.0 TB/s HBM peak (a float4 copy reaches 6.29 TB/s).  The clip value is half the
gradients' norm, so the clip is active in both arms.  Needs a GPU and libocc_hip.so: there is no fall-back.

    python tools/bench_clip_adamw.py [--reps 60] [--warmup 10] [--out profiles/clip_adamw_bench.json]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from occdepth_amd import configs, hip, optim, train_graph  # noqa: E402

HBM_PEAK = 8.0e12


def parameter_shapes():
    from occdepth_amd.models.OccDepth import OccDepth
    cfg = configs.kitti_a100.clone()
    with contextlib.redirect_stdout(io.StringIO()):
        m = OccDepth(class_names=[str(i) for i in range(cfg.n_classes)], class_weights=torch.ones(cfg.n_classes),
                     class_weights_occ=torch.ones(2), full_scene_size=tuple(cfg.full_scene_size),
                     project_res=configs.PROJECT_RES, config=cfg)
    return [tuple(p.shape) for p in m.parameters() if p.requires_grad]


def make_arm(shapes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ps = [torch.nn.Parameter(0.05 * torch.randn(s, device="cuda", generator=g)) for s in shapes]
    for p in ps:
        p.grad = torch.randn(p.shape, device="cuda", generator=g)
    opt = train_graph.make_capturable(torch.optim.AdamW(ps, lr=2e-4, weight_decay=1e-4, fused=True))
    return ps, opt


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA
               and "memcpy" not in e.key.lower() and "memset" not in e.key.lower())


def spread(ms):
    q = statistics.quantiles(ms, n=10)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "p10_ms": round(q[0], 4), "p90_ms": round(q[-1], 4), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_adamw_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_adamw: needs a GPU (there is no CPU arm)")
    if args.reps < 50:
        raise SystemExit("bench_clip_adamw: at least 50 timed repetitions per arm")
    hip.load()
    shapes = parameter_shapes()
    n_params = sum(int(torch.Size(s).numel()) for s in shapes)
    ps_a, opt_a = make_arm(shapes, 0)
    ps_b, opt_b = make_arm(shapes, 0)
    clip = 0.5 * float(torch.nn.utils.get_total_norm([p.grad for p in ps_a]))
    saved = [p.grad.clone() for p in ps_a]                  # arm A rescales its gradients in place: restored untimed

    def arm_a():
        torch.nn.utils.clip_grad_norm_(ps_a, clip)
        opt_a.step()

    def arm_b():
        optim.clip_adamw_step(opt_b, clip)

    def restore():
        torch._foreach_copy_([p.grad for p in ps_a], saved)

    times = {"A": [], "B": []}
    for i in range(args.warmup + args.reps):
        for name, fn in (("A", arm_a), ("B", arm_b)):
            restore()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append(t0.elapsed_time(t1))
    restore()
    n_a, n_b = launches(arm_a), launches(arm_b)
    a, b = spread(times["A"]), spread(times["B"])
    # the same two arms replayed from captured graphs (A rescales its gradients on every replay: the timing does not care)
    graphs = {}
    for name, fn, opt in (("A", arm_a, opt_a), ("B", arm_b, opt_b)):
        optim.prepare_capture(opt)
        g = train_graph.new_graph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, capture_error_mode=train_graph.CAPTURE_MODE):
            fn()
        train_graph.seal_graph(g)
        graphs[name] = g
    keep = optim.live_tables(opt_b)                          # what graph B reads must outlive it
    gtimes = {"A": [], "B": []}
    for i in range(args.warmup + args.reps):
        for name in ("A", "B"):
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            graphs[name].replay()
            t1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                gtimes[name].append(t0.elapsed_time(t1))
    del keep
    ga, gb = spread(gtimes["A"]), spread(gtimes["B"])
    bound_ms = 1e3 * 32.0 * n_params / HBM_PEAK
    out = {"workload": "config-2 (configs.kitti_a100) parameter set, float32, random gradients, clip = norm / 2 (active)",
           "tensors": len(shapes), "parameters": n_params,
           "A_clip_grad_norm_plus_fused_adamw": dict(a, kernel_launches=n_a),
           "B_clip_adamw_step": dict(b, kernel_launches=n_b, chunk_descriptors=sum(max(1, -(-int(torch.Size(s).numel()) // hip.OPTIM_CHUNK)) for s in shapes)),
           "B_over_A": round(b["median_ms"] / a["median_ms"], 4),
           "graph_replay": {"A": ga, "B": gb, "B_over_A": round(gb["median_ms"] / ga["median_ms"], 4)},
           "bandwidth_bound": {"bytes": 32 * n_params, "hbm_peak_TB_s": HBM_PEAK / 1e12, "bound_ms": round(bound_ms, 4),
                               "B_graph_share_of_bound": round(bound_ms / gb["median_ms"], 4),
                               "B_graph_TB_s": round(32.0 * n_params / (gb["median_ms"] * 1e-3) / 1e12, 3),
                               "B_eager_share_of_bound": round(bound_ms / b["median_ms"], 4)},
           "timing": "device events around each repetition, arms alternating, warm-up "
                     f"{args.warmup}; eager figures include the host's launch work, graph_replay is device time"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
