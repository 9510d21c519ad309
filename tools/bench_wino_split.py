"""K10 against K10h (the two-term fp16 split) on every fused-Winograd launch geometry of the config-2 frame (dev tool, GPU):

    python tools/bench_wino_split.py > profiles/wino_f16x2_ab.txt

N(0,1) data; warm-up launches, then the best of three rounds of back-to-back launches between stream events (as
bench.py::isolated_head).  `spread` is (worst - best) / best of the three rounds; K10h takes a geometry by default only where
it is faster by more than that (hip.wino_f16x2_wins)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from occdepth_amd import hip

# (cin, cout, H, W, residual, launches per frame): the wino_conv3x3 rows of profiles/r06_frame_per_launch.txt, batch 2
GEOMETRIES = [(80, 80, 370, 1220, False, 1), (160, 160, 185, 610, False, 1), (320, 320, 93, 305, False, 1),
              (128, 128, 47, 153, True, 6), (32, 160, 185, 610, True, 1), (48, 320, 93, 305, True, 1),
              (224, 1280, 24, 77, True, 1), (80, 640, 47, 153, True, 1), (64, 128, 47, 153, False, 1)]


def rounds(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return min(ts), (max(ts) - min(ts)) / min(ts)


def main():
    hip.load()
    torch.manual_seed(0)
    print(f"{'geometry':28s} {'workgroups':>10s} {'K10 ms':>9s} {'spread':>7s} {'K10h ms':>9s} {'spread':>7s} {'K10/K10h':>9s}  rule")
    tot = [0.0, 0.0, 0.0]
    for cin, cout, H, W, with_res, n in GEOMETRIES:
        x = torch.randn(2, cin, H, W, device="cuda")
        w = torch.randn(cout, cin, 3, 3, device="cuda") * 0.1
        sc, sh = torch.rand(cout, device="cuda") + 0.5, torch.randn(cout, device="cuda")
        res = torch.randn(2, cout, H, W, device="cuda") if with_res else None
        y = torch.empty(2, cout, H, W, device="cuda")
        ops = (hip.wino_pack_weights(w, sc), hip.wino_pack_weights_f16x2(w, sc))
        iters = max(5, min(50, int(20.0 / (1e-6 * cin * cout * H * W / 2e3 + 0.02))))
        (t32, s32), (t16, s16) = (rounds(lambda: hip.conv2d_3x3_fused(x, u, cout, sh, "leaky", res=res, res_first=True, out=y),
                                         iters) for u in ops)
        wgs = 2 * ((cout + 31) // 32) * ((((H + 1) // 2) * ((W + 1) // 2) + 127) // 128)
        wins = hip.wino_f16x2_wins(2, cin, cout, H, W)
        tot[0] += n * t32
        tot[1] += n * t16
        tot[2] += n * (t16 if wins else t32)
        print(f"{cin:4d}>{cout:<4d} @2x{H}x{W:<10d} {wgs:10d} {t32:9.4f} {100 * s32:6.1f}% {t16:9.4f} {100 * s16:6.1f}% "
              f"{t32 / t16:9.2f}  {'K10h' if wins else 'K10'}", flush=True)
    print(f"per frame (launch counts applied): K10 {tot[0]:.3f} ms, K10h {tot[1]:.3f} ms, by the rule {tot[2]:.3f} ms")


if __name__ == "__main__":
    main()
