"""dev: depthwise + SE-pooling kernel on the EfficientNet-B7 shapes of a config-2 frame (two views), both staging forms of
dwconv2d_kernel in one process (occd_dwconv2d_set_stage: 0 element-wise, 1 16-byte chunks), GB/s against the bytes it has to
move (read x, write y).  Per form: the best of three rounds of back-to-back launches and the spread of the three; the input
planes lie on the padded pitch of the expand GEMM's result, as in the frame (--dense: contiguous planes).

    python tools/bench_dw.py [--dense] [--eager] [--iters N]
"""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from occdepth_amd import hip

ap = argparse.ArgumentParser()
ap.add_argument("--dense", action="store_true")
ap.add_argument("--eager", action="store_true")
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()
lib = hip.load()


def rounds(fn, iters):
    """(best, worst) ms per launch of three rounds of `iters` back-to-back launches; the launches are captured into a graph
    once and replayed, as the frame is (--eager: enqueued one by one from Python, which costs ~15 us each and hides any
    kernel shorter than that)."""
    fn(); torch.cuda.synchronize(); ts = []
    graph = None
    if not args.eager:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(iters): fn()
        torch.cuda.current_stream().wait_stream(side)
        graph.replay(); torch.cuda.synchronize()
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if graph is not None:
            graph.replay()
        else:
            for _ in range(iters): fn()
        e1.record(); torch.cuda.synchronize(); ts.append(e0.elapsed_time(e1) / iters)
    return min(ts), max(ts)


# (C, H, W, k, stride, launches per frame): the dwconv2d_nchw rows of profiles/r06_frame_per_launch.txt
SHAPES = [(64, 185, 610, 3, 1, 1), (32, 185, 610, 3, 1, 3), (192, 185, 610, 3, 2, 1), (288, 93, 305, 3, 1, 6),
          (288, 93, 305, 5, 2, 1), (480, 47, 153, 5, 1, 6), (480, 47, 153, 3, 2, 1), (960, 24, 77, 3, 1, 9),
          (960, 24, 77, 5, 1, 1), (1344, 24, 77, 5, 1, 9), (1344, 24, 77, 5, 2, 1), (2304, 12, 39, 5, 1, 12),
          (2304, 12, 39, 3, 1, 1), (3840, 12, 39, 3, 1, 3)]
print("# us per launch: best of 3 rounds x %d launches (worst round in brackets); GB/s of the best round" % args.iters)
print("# forms: element-wise = occd_dwconv2d_set_stage(0); chunks = (2), one plane per workgroup; paired = (1), the default: chunks, planes")
print("#        of <= 128 items two to a workgroup (the same launch as `chunks` elsewhere)")
print("# %-32s %3s  %-17s %-17s %-17s %5s %5s %5s  %s" % ("launch", "n", "element-wise", "chunks", "paired", "GB/s", "GB/s", "GB/s", "verdict"))
NAMES = ("element-wise", "chunks", "paired")
tot = [0.0, 0.0, 0.0]
for C, H, W, k, s, n in SHAPES:
    if args.dense:
        x = torch.randn(2, C, H, W, device="cuda")
    else:
        x = hip.padded_rows((2, C, H * W), "cuda")
        x.copy_(torch.randn(2, C, H * W, device="cuda"))
        x = x.view(2, C, H, W)
    w = torch.randn(C, 1, k, k, device="cuda") * 0.2
    sc = torch.rand(C, device="cuda") + 0.5; sh = torch.randn(C, device="cuda") * 0.1
    res = []
    out = []
    for form in (0, 2, 1):
        old = lib.occd_dwconv2d_set_stage(form)
        try:
            res.append(rounds(lambda: hip.dwconv2d_same_pool(x, w, sc, sh, s, "swish"), args.iters))
            out.append(hip.dwconv2d_same_pool(x, w, sc, sh, s, "swish")[:2])
        finally:
            lib.occd_dwconv2d_set_stage(old)
    same = all(torch.equal(out[0][0], o[0]) and torch.equal(out[0][1], o[1]) for o in out[1:])
    Ho, Wo = -(-H // s), -(-W // s)
    by = 4.0 * 2 * C * (H * W + Ho * Wo)
    for i in range(3):
        tot[i] += n * res[i][0]
    # a form is ahead only beyond the spread: its WORST round against the BEST round of each other form
    ahead = [i for i in range(3) if all(res[i][1] < res[j][0] for j in range(3) if j != i)]
    verdict = NAMES[ahead[0]] if ahead else "inside the spread: " + " / ".join(
        NAMES[i] for i in range(3) if not any(res[j][1] < res[i][0] for j in range(3)))
    print("%-34s %3d  %6.1f [%6.1f]  %6.1f [%6.1f]  %6.1f [%6.1f]  %5.0f %5.0f %5.0f  %s%s" % (
        "%d k%d s%d @2x%dx%d" % (C, k, s, H, W), n, res[0][0] * 1e3, res[0][1] * 1e3, res[1][0] * 1e3, res[1][1] * 1e3,
        res[2][0] * 1e3, res[2][1] * 1e3, by / res[0][0] / 1e6, by / res[1][0] / 1e6, by / res[2][0] / 1e6, verdict,
        "" if same else "  BITS DIFFER"), flush=True)
print("family per frame: element-wise %.3f ms, chunks %.3f ms, paired %.3f ms" % tuple(tot))
